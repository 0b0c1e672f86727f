"""Drop-in group-phase ``PPNetMultiScale`` (ScaleProtoSeg phase 2) on the MI355X kernels.

Mirrors segmentation/model/model_multiscale_group.py:82-519: same constructor, ``group_projection``
(ModuleList of bias-free Linear(n_k -> G)), ``last_layer_group``, ``group_class_identity``,
``compute_group`` (returns a list), ``state_dict`` keys (no ``last_layer``), simplex initialisation.

Fused form of the grouping head: every class's projection is a row block of ONE dense [G*K', P] matrix
(zeros outside the class's prototype columns), so ``cat_k(act[:, idx_k] @ W_k^T)`` is the kernel's head
contraction act @ Wd^T; ``exp`` and the ``last_layer_group`` product follow inside the same kernel (a second
split-bf16 MFMA on the unit tiles), and the backward forms dUnits in registers.  The reference instead gathers per
class with a host sync per class per forward (:297-301).
"""
from __future__ import annotations

import os
from typing import Any, List, Optional, Tuple

import torch
import torch.nn as nn

from ._cache import cached
from .functional import (MAX_FUSED_HEAD_ROWS, MAX_FUSED_TAIL_CLASSES, GroupTables, SpxError, cross_entropy_from_logits,
                         group_dense, group_exp, invalidate_pack_cache, proto_head_forward, wide_group_tail, wide_linear)
from .model_multiscale import _HeadOut, _PrototypeBankMixin, _build_add_on, _first_add_on_channels
from .msc import PackedMaps
from .utils import projection_simplex_sort, projection_simplex_sort_


class GroupRegTables:
    """Device tables of the weight-side regularisers (csrc/spx_reg.hip), cached with the GroupTables they extend:
    block_info int32 [J, 4] = (first flat weight element, n_j, first unit row, 0) and spans int32 [J, S, 2]."""

    def __init__(self, block_info, spans, nspans: int, G: int, S: int):
        self.block_info, self.spans, self.nspans, self.G, self.S = block_info, spans, int(nspans), int(G), int(S)


def group_scale_spans(prototype_class_identity: torch.Tensor, scale_num_prototypes, num_scales: int, num_groups: int):
    """(block_info [J, 4], spans [J, S, 2], number of non-empty spans) for the classes that own prototypes, in block order.
    The span of (class block j, scale s) is the range of j's local weight columns that ScaleMax takes its maximum over
    (segmentation/model/loss.py:366-390): the counts of j's prototypes inside scale_num_prototypes[s], laid end to end in
    scale order; a scale without any of j's prototypes has the empty span (c, c).  Pure host work."""
    ident = prototype_class_identity.detach().cpu()
    K = ident.shape[1]
    info, spans, nspans, off, u0 = [], [], 0, 0, 0
    for k in range(K):
        n = int(torch.count_nonzero(ident[:, k]))
        if n == 0:
            continue                                                       # loss.py:362-363
        prev, row = 0, []
        for s in range(num_scales):
            lo, hi = (int(v) for v in scale_num_prototypes[s])
            cnt = int(torch.count_nonzero(ident[lo:hi, k]))
            if cnt and prev + cnt > n:
                raise SpxError(f"class {k}: the scale ranges hold more of its prototypes ({prev + cnt}) than it owns ({n})")
            row.append((prev, prev + cnt))
            nspans += cnt > 0
            prev += cnt
        info.append((off, n, u0, 0))
        spans.append(row)
        off += num_groups * n
        u0 += num_groups
    return (torch.tensor(info, dtype=torch.int32).reshape(-1, 4), torch.tensor(spans, dtype=torch.int32).reshape(-1, num_scales, 2),
            nspans)


class PPNetMultiScale(_PrototypeBankMixin, nn.Module):
    """Group-phase module; the reference names it ``PPNetMultiScale`` in model_multiscale_group.py (:82), so
    ``from scaleprotoseg_amd.model_multiscale_group import PPNetMultiScale`` works as upstream.  The package exports it
    as ``PPNetMultiScaleGroup`` to keep it apart from the prototype-phase class."""

    def __init__(
        self,
        features: nn.Module,
        img_size: int,
        prototype_shape: Tuple[int, int, int, int],
        proto_layer_rf_info: List[float],
        num_classes: int,
        init_weights: bool = True,
        prototype_activation_function: str = "log",
        add_on_layers_type: str = "bottleneck",
        bottleneck_stride: Optional[int] = None,
        patch_classification: bool = False,
        num_scales: int = 4,
        scale_head_type: Optional[str] = None,
        num_groups: int = 3,
        incorrect_strength: float = -0.5,
        equiv_path: Optional[os.PathLike] = None,
        equiv_scale_weight: float = 0.25,
    ):
        super().__init__()
        self.img_size = img_size
        self.bottleneck_stride = bottleneck_stride
        self.patch_classification = patch_classification
        self.num_groups = num_groups
        self.incorrect_strength = incorrect_strength
        if equiv_path is not None:
            raise SpxError("equiv_path initialisation is deprecated in the reference (NOT USED) and not built")
        self._init_scale_head(scale_head_type, prototype_shape)
        self.prototype_activation_function = prototype_activation_function
        self._init_bank(prototype_shape, num_classes, num_scales)
        self.proto_layer_rf_info = proto_layer_rf_info
        self.features = features
        in_ch = _first_add_on_channels(features)
        self.add_on_layers = _build_add_on(add_on_layers_type, in_ch, self.prototype_shape[1], bottleneck_stride)
        self._group_index_cache = None
        self._initialize_groups()
        if init_weights:
            self._initialize_weights()

    # ---- group bookkeeping ------------------------------------------------------------------------
    def _present_classes(self) -> List[int]:
        ident = self.prototype_class_identity
        return [k for k in range(self.num_classes) if int(ident[:, k].sum().item()) > 0]

    def _initialize_groups(self):
        """group_projection / group_class_identity / last_layer_group (model_multiscale_group.py:249-269)."""
        ident = self.prototype_class_identity
        present = self._present_classes()
        self.group_projection = nn.ModuleList(
            [nn.Linear(int(ident[:, k].sum().item()), self.num_groups, bias=False) for k in present]
        )
        n_groups = self.num_groups * len(present)
        self.group_class_identity = torch.zeros(n_groups, self.num_classes)
        for j, k in enumerate(present):
            self.group_class_identity[j * self.num_groups : (j + 1) * self.num_groups, k] = 1
        self.last_layer_group = nn.Linear(n_groups, self.num_classes, bias=False)
        dev = self.prototype_vectors.device          # re-initialisation after .cuda() (finetune_wandb_group.py:80, prune)
        self.group_projection.to(dev)
        self.last_layer_group.to(dev)
        self._group_index_cache = None

    def _group_index(self, device):
        """(rows, cols, number of units, GroupTables) of every group-projection weight inside the dense [NG, P] head matrix."""
        ident = self.prototype_class_identity
        # (the scale ranges: the ScaleMax spans hang on these tables, and ``scale_num_prototypes[s] = ...`` is an item edit of a
        # dict that passes no __setattr__)
        scales = tuple(tuple(int(v) for v in self.scale_num_prototypes[s]) for s in range(self.num_scales))
        extras = (self._tables_version, tuple(gp.weight.shape for gp in self.group_projection), scales, str(device))
        return cached(self, "_group_index_cache", (ident,), extras, lambda: self._group_index_build(ident, device))

    def _group_index_build(self, ident: torch.Tensor, device):
        P = self.num_prototypes
        rows, cols, r0 = [], [], 0
        col_block, col_local = torch.full((P,), -1, dtype=torch.int32), torch.zeros(P, dtype=torch.int32)
        row_block, row_local, block_cols = [], [], []
        for j, k in enumerate(self._present_classes()):
            idx = torch.nonzero(ident[:, k]).flatten()
            g = self.group_projection[j].weight.shape[0]
            rr = torch.arange(r0, r0 + g).repeat_interleave(idx.numel())
            cc = idx.repeat(g)
            rows.append(rr)
            cols.append(cc)
            col_block[idx] = j
            col_local[idx] = torch.arange(idx.numel(), dtype=torch.int32)
            row_block += [j] * g
            row_local += list(range(g))
            block_cols.append(int(idx.numel()))
            r0 += g
        rows_, cols_ = torch.cat(rows), torch.cat(cols)
        i32 = lambda t: torch.as_tensor(t, dtype=torch.int32).to(device).contiguous()
        tables = None
        if torch.device(device).type == "cuda" and len(block_cols) <= 192:
            tables = GroupTables(i32(row_block), i32(row_local), i32(col_block), i32(col_local), i32(rows_), i32(cols_),
                                 block_cols, r0, P)
            tables.reg = None
            gs = [int(gp.weight.shape[0]) for gp in self.group_projection]
            if gs and all(g == gs[0] for g in gs) and 1 <= gs[0] <= 16 and 1 <= self.num_scales <= 16:
                info, spans, nspans = group_scale_spans(ident, self.scale_num_prototypes, self.num_scales, gs[0])
                tables.reg = GroupRegTables(i32(info), i32(spans), nspans, gs[0], self.num_scales)
        return rows_.to(device), cols_.to(device), r0, tables

    def _dense_group_matrix(self) -> torch.Tensor:
        dev = self.prototype_vectors.device
        rows, cols, ng, tables = self._group_index(dev)
        if tables is not None:
            return group_dense(tables, [gp.weight for gp in self.group_projection])      # one launch (spx_group_dense)
        vals = torch.cat([gp.weight.reshape(-1) for gp in self.group_projection])
        return torch.zeros(ng, self.num_prototypes, device=dev, dtype=vals.dtype).index_put((rows, cols), vals)

    def _group_units(self, prototype_activations: torch.Tensor):
        """(units, g) behind ``prototype_activations``: what the forward that produced this very tensor left on it (the
        kernels' own unit product / group activations, still attached to the autograd graph), else the dense unit product
        act . Wd^T on the fp32 MFMA product kernels.  One of the two is None."""
        tag = getattr(prototype_activations, "spx_group", None)
        if tag is not None and tag[0] == prototype_activations._version:
            return tag[1], tag[2]
        if prototype_activations.dim() != 2 or prototype_activations.shape[1] != self.num_prototypes:
            raise SpxError(f"prototype activations must be [M, {self.num_prototypes}], got {tuple(prototype_activations.shape)}")
        return wide_linear(prototype_activations, self._dense_group_matrix()), None

    def compute_group(self, prototype_activations: torch.Tensor) -> List[torch.Tensor]:
        """List of per-class group activations exp(act[:, idx_k] @ W_k^T) (model_multiscale_group.py:283-303), as column
        blocks of the dense form exp(act . Wd^T): for the activations a forward of this module returned, views of the
        [M, U] tensor the fused kernel wrote (a gradient on them enters its backward as part of dUnits - the path
        KLDLossGroup takes, module_multiscale_group_train.py:242-262); for any other activations the same product on the
        fp32 MFMA kernels followed by the exp kernel.  No per-class gathers, no host syncs."""
        units, g = self._group_units(prototype_activations)
        if g is None:
            g = group_exp(units)
        return list(torch.split(g, [int(gp.weight.shape[0]) for gp in self.group_projection], dim=1))

    def run_last_layer(self, prototype_activations: torch.Tensor) -> torch.Tensor:
        """last_layer_group(cat(compute_group(act))) (model_multiscale_group.py:305-308): exp fused into the product kernel's
        operand staging."""
        units, g = self._group_units(prototype_activations)
        if units is None:
            return wide_linear(g, self.last_layer_group.weight)
        return wide_group_tail(units, self.last_layer_group.weight)

    # ---- forward ------------------------------------------------------------------------------------
    def forward_from_conv_features(
        self, conv_features, return_activations: bool = False, return_distances: bool = False, ce_target=None
    ) -> Any:
        """Same return-tuple rules as model_multiscale_group.py:404-452.  Extension: ``ce_target`` ([B, H, W] at the latent
        resolution, 0 = void, 1..K) computes the pixel-wise cross entropy in the kernel that produces the logits and hangs
        it on the returned logits (``logits.spx_ce``), exactly as the prototype-phase module does."""
        if isinstance(conv_features, PackedMaps):
            return self._forward_packed(conv_features, return_activations, return_distances, ce_target)
        if isinstance(conv_features, list):
            return [self.forward_from_conv_features(c) for c in conv_features]
        self._check_patch_classification()
        if self.scale_head is not None:
            if ce_target is not None:
                raise SpxError("ce_target lives in the fused distance kernel's epilogue, which does not carry a scale_head")
            return self._scale_head_forward(conv_features, return_activations, return_distances)
        self._check_1x1()                   # what _check_fusable asks beyond the scale_head that left above
        B, _, H, W = conv_features.shape
        if callable(self.prototype_activation_function):
            # model_multiscale_group.py:393-394: the user's function on the distance map as ordinary torch code; both head
            # products on the fp32 MFMA product kernels
            wd = self._dense_group_matrix()
            if ce_target is not None:
                raise SpxError("ce_target needs a built-in similarity ('log' or 'linear')")
            dist, act = self._callable_similarity(conv_features)
            units = wide_linear(act, wd)
            act.spx_group = (act._version, units, None)
            logits = wide_group_tail(units, self.last_layer_group.weight).reshape(B, H, W, -1)
            return self._result(logits, dist, act, return_activations, return_distances)
        r = self._head(conv_features, want_dist=self._wants_distances(return_activations, return_distances),
                       want_act=return_activations, ce_target=ce_target)
        if r.act is not None:
            r.act.spx_group = (r.act._version, r.units, r.g)
        logits = r.logits.reshape(B, H, W, -1)
        logits.spx_group_wd = self._group_wd_tag(r.wd)
        self._attach_ce(logits, r.ce, ce_target)
        return self._result(logits, r.dist, r.act, return_activations, return_distances)

    def _head(self, x: torch.Tensor, *, want_dist: bool, want_act: bool, ce_target=None) -> _HeadOut:
        """Distances, similarity and the grouping head over the pixels of ``x`` ([B, C, H, W] or a packed [1, C, 1, M]), on the
        one branch this bank takes.  The record holds the units or - where the kernel applied the exp itself - exp(units)."""
        wd, wg = self._dense_group_matrix(), self.last_layer_group.weight
        rows, k2 = int(wd.shape[0]), int(wg.shape[0])
        ce_labels = self._ce_labels(ce_target, x)
        kw = dict(want_distances=want_dist, epsilon=self.epsilon, activation=self.prototype_activation_function)
        units = g = ce = None
        units_in_kernel = rows <= MAX_FUSED_HEAD_ROWS
        if units_in_kernel and k2 <= MAX_FUSED_TAIL_CLASSES:
            # whole grouping head in the kernels: units = act . Wd^T, exp, last_layer_group (:303-308)
            out = proto_head_forward(x, self.prototype_vectors, wd, self._layout(rows), want_activations=want_act, group_tail=wg,
                                     ce_labels=ce_labels, **kw)
            logits, dist, act = out[:3]
            if ce_labels is not None:
                ce = out[3]
            g = out[-1]                                             # exp(units) [M, U], written by the kernel
        elif units_in_kernel:
            # up to 160 units but more than 32 classes: the unit product stays in the kernel, the tail is the fp32 MFMA product kernel (exp fused into its operand staging)
            units, dist, act = proto_head_forward(x, self.prototype_vectors, wd, self._layout(rows), want_activations=want_act, **kw)
            logits = wide_group_tail(units, wg)
        else:
            # group_scaleproto_ade.gin (150 classes x 3 groups = 450 units) / _coco.gin (546): the kernel hands out the
            # [pixel][P] activations once, both products are the fp32 MFMA product kernels (csrc/spx_gemm.hip) on them
            _, dist, act = proto_head_forward(x, self.prototype_vectors, None, self._layout(1), want_activations=True, **kw)
            units = wide_linear(act, wd)
            logits = wide_group_tail(units, wg)
        if ce_labels is not None and ce is None:
            ce = cross_entropy_from_logits(logits, ce_labels)       # heads the fused kernels do not carry
        return _HeadOut(logits, dist, act, ce, None, units, g, wd)

    def _group_wd_tag(self, wd: torch.Tensor):
        """``spx_group_wd``: the dense group matrix a forward multiplied with (GroupRegularizers(logits=...) differentiates
        through it, so the group weights receive one scatter for both gradients); the weights' versions void it after an
        optimiser step."""
        return wd, self, tuple(gp.weight._version for gp in self.group_projection)

    _packed_ce_hint = "(module_multiscale_group_train.py:232-310); call SegmentedCrossEntropy on the segments' logits"

    def _forward_packed(self, pk: PackedMaps, return_activations, return_distances, ce_target):
        """The four training maps on one pixel axis (``pk.features`` [1, C, 1, M]; module_multiscale_group_train.py:232,
        forward :396-402): ONE launch of the distance kernel for all segments, then the head branch this bank takes on a single
        map.  Units, group activations and logits are per-pixel quantities like the distances, so they split like them
        (``_split_packed``; units and group activations are row slices).  Every segment's activations carry ``spx_group`` with
        ITS rows of the one [M, U] tensor - ``compute_group`` returns views of it and a KLD gradient on them enters the one
        backward as part of dUnits - and every segment's logits carry ``spx_group_wd`` and ``spx_packed``
        (``SegmentedCrossEntropy`` then runs on the packed logits as they are)."""
        self._refuse_packed(ce_target)
        lay = pk.layout
        want_dist = self._wants_distances(return_activations, return_distances)
        r = self._head(pk.features, want_dist=want_dist, want_act=return_activations)
        logits_k, dists_k, acts_k = self._split_packed(lay, r, want_dist, return_activations)
        tag = self._group_wd_tag(r.wd)
        for l in logits_k:
            l.spx_group_wd = tag
        if return_activations:
            units_k = lay.split_rows(r.units) if r.units is not None else [None] * len(lay)
            g_k = lay.split_rows(r.g) if r.g is not None else [None] * len(lay)
            for a, u, gg in zip(acts_k, units_k, g_k):
                a.spx_group = (a._version, u, gg)
        return [self._result(l, d, a, return_activations, return_distances) for l, d, a in zip(logits_k, dists_k, acts_k)]

    def forward_packed(self, x, **kwargs):
        """``forward`` with MSC's training maps packed (after ``fuse_feature_epilogue(dtype)``): in training
        ``features.fused_packed(x, "sigmoid", dtype)`` - the four maps in one launch - and the packed forward above, one tuple
        per segment; in eval, or with ``scales = []``, exactly ``forward(x, **kwargs)``.  (``fuse_feature_epilogue(dtype,
        packed=True)`` stays refused for this class; this method is the opt-in.)"""
        if self._feature_epilogue is None:
            raise SpxError("forward_packed: call fuse_feature_epilogue(dtype) first (features must be scaleprotoseg_amd.MSC)")
        if not self.training or len(self.features.scales) == 0:
            return self.forward(x, **kwargs)
        return self.forward_from_conv_features(self.features.fused_packed(x, "sigmoid", self._feature_epilogue), **kwargs)

    def prune_prototypes(self, prototypes_to_prune: List[int]):
        """Not in the upstream group class (it receives an already pruned bank by attribute assignment,
        finetune_wandb_group.py:74-80); provided so a post-push prototype-phase checkpoint loads through
        ``checkpoint.load_reference_state_dict``: prunes the bank and the class / scale tables, then rebuilds
        ``group_projection`` / ``group_class_identity`` / ``last_layer_group`` for the new table (fresh default-initialised
        layers, as ``_initialize_groups`` upstream: call ``_initialize_weights`` or load a state_dict next)."""
        self._prune_bank(prototypes_to_prune)
        self._initialize_groups()

    # ---- init ---------------------------------------------------------------------------------------
    def set_last_layer_incorrect_connection(self):
        pos = torch.t(self.group_class_identity).to(self.last_layer_group.weight.device)  # :480-491
        self.last_layer_group.weight.data.copy_(1 * pos + self.incorrect_strength * (1 - pos))
        invalidate_pack_cache()

    def project_group_simplex_(self, z: float = 1.0):
        """Re-project every ``group_projection`` weight onto the simplex in place (the step after ``optimizer.step()`` in the
        group phase, module_multiscale_group_train.py:337-338): one launch, storages kept (``utils.projection_simplex_sort_``)."""
        projection_simplex_sort_([gp.weight for gp in self.group_projection], z)
        invalidate_pack_cache()

    def _initialize_weights(self, equiv_path=None, equiv_scale_weight: float = 0.25):
        self._initialize_add_on()  # :493-519
        if equiv_path is not None:
            raise SpxError("equiv_path initialisation is deprecated in the reference (NOT USED) and not built")
        for gp in self.group_projection:
            gp.weight.data = projection_simplex_sort(gp.weight.data)
        self.set_last_layer_incorrect_connection()


PPNetMultiScaleGroup = PPNetMultiScale


def construct_PPNet_Group(
    features: nn.Module,
    img_size: int = 224,
    prototype_shape: Tuple[int, int, int, int] = (2000, 512, 1, 1),
    num_classes: int = 200,
    prototype_activation_function: str = "log",
    add_on_layers_type: str = "bottleneck",
    scale_head_type: Optional[str] = None,
    **kwargs,
) -> PPNetMultiScale:
    """Factory with the reference's argument meaning (model_multiscale_group.py:589-624)."""
    return PPNetMultiScale(
        features=features, img_size=img_size, prototype_shape=prototype_shape, proto_layer_rf_info=[],
        num_classes=num_classes, init_weights=True, prototype_activation_function=prototype_activation_function,
        add_on_layers_type=add_on_layers_type, scale_head_type=scale_head_type, **kwargs,
    )
