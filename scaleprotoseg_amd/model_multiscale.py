"""Drop-in ``PPNetMultiScale`` (prototype phase) on the MI355X kernels.

Mirrors the public surface of the reference class
(segmentation/model/model_multiscale.py:71-477: constructor, properties,
``forward`` / ``forward_from_conv_features`` / ``push_forward`` / ``prune_prototypes``,
``state_dict`` keys ``prototype_vectors``, ``ones``, ``last_layer.weight``,
``features.*``) while the distance -> similarity -> head chain runs in one HIP
kernel (scaleprotoseg_amd.functional).  There is no CPU path: tensors must live
on an AMD GPU when the distance methods are called.
"""
from __future__ import annotations

from typing import Any, Dict, List, NamedTuple, Optional, Tuple, Union

import torch
import torch.nn as nn

from ._cache import cached
from .functional import (MAX_FUSED_HEAD_ROWS, BankLayout, ClassGather, FusedCrossEntropy, SpxError, class_gather_table,
                         cross_entropy_from_logits, identity_is_one_hot, invalidate_pack_cache, proto_head_forward,
                         push_min_from_features, shifted_labels_i32, wide_linear)
from .loss import ClassDistances
from .msc import MSC, PackedMaps
from .scale_head import WeightedAgg


def _first_add_on_channels(features: nn.Module) -> int:
    """Backbone output width, by the reference's name dispatch (model_multiscale.py:153-171)."""
    name = str(features).upper()
    convs = lambda m: [i for i in m.modules() if isinstance(i, nn.Conv2d)]
    if name.startswith("VGG") or name.startswith("RES"):
        return convs(features)[-1].out_channels
    if name.startswith("DENSE"):
        return [i for i in features.modules() if isinstance(i, nn.BatchNorm2d)][-1].num_features
    if name.startswith("DEEPLAB"):
        return convs(features)[-2].out_channels
    if name.startswith("MSC"):
        return convs(features.base)[-2].out_channels
    raise Exception(f"{name[:10]} base_architecture NOT implemented")


def _build_add_on(kind: str, in_ch: int, proto_ch: int, bottleneck_stride: Optional[int]) -> nn.Sequential:
    """Add-on stack between backbone and prototype layer (model_multiscale.py:173-218)."""
    if kind == "deeplab_simple":
        return nn.Sequential(nn.Sigmoid())
    layers: List[nn.Module] = []
    if kind == "bottleneck_pool":
        layers += [nn.Conv2d(in_ch, in_ch, kernel_size=3, padding=1, stride=bottleneck_stride), nn.ReLU()]
    if kind.startswith("bottleneck"):
        cur = in_ch
        while cur > proto_ch or len(layers) == 0:
            out = max(proto_ch, cur // 2)
            layers += [nn.Conv2d(cur, out, kernel_size=1), nn.ReLU(), nn.Conv2d(out, out, kernel_size=1)]
            if out > proto_ch:
                layers.append(nn.ReLU())
            else:
                assert out == proto_ch
                layers.append(nn.Sigmoid())
            cur = cur // 2
        return nn.Sequential(*layers)
    return nn.Sequential(
        nn.Conv2d(in_ch, proto_ch, kernel_size=1), nn.ReLU(), nn.Conv2d(proto_ch, proto_ch, kernel_size=1), nn.Sigmoid()
    )


class _HeadOut(NamedTuple):
    """What a class's ``_head`` computed, flat over the pixels of its input ([B, C, H, W] or a packed [1, C, 1, M]), whatever
    branch produced it."""

    logits: torch.Tensor                         # [M, K]
    dist: Optional[torch.Tensor]                 # [B, P, H, W], or [B, J, H*W] with ``gather``
    act: Optional[torch.Tensor]                  # [M, P]
    ce: Optional[FusedCrossEntropy] = None       # of ``ce_target``, from whichever kernel carried it
    gather: Optional[ClassGather] = None         # prototype phase: ``dist`` holds each pixel's own class alone
    units: Optional[torch.Tensor] = None         # group phase: act . wd^T [M, U] or ``g`` = exp(units), one of the two per branch
    g: Optional[torch.Tensor] = None
    wd: Optional[torch.Tensor] = None            # ... and the dense group matrix the forward multiplied with


class _PrototypeBankMixin:
    """State and helpers shared by the prototype-phase and group-phase modules."""

    _tables_version = 0

    def __setattr__(self, name, value):
        # prototype_class_identity / scale_num_prototypes are plain attributes that callers re-assign
        # (finetune_wandb_group.py:77-78, prune_prototypes): every derived cache is keyed on this counter
        if name in ("prototype_class_identity", "scale_num_prototypes"):
            object.__setattr__(self, "_tables_version", self._tables_version + 1)
        super().__setattr__(name, value)

    def _init_bank(self, prototype_shape, num_classes: int, num_scales: int):
        self.epsilon = 1e-4  # model_multiscale.py:106
        self.num_scales = num_scales
        self.prototype_vectors = nn.Parameter(torch.rand(prototype_shape), requires_grad=True)  # :111
        P = self.prototype_vectors.shape[0]
        # one-hot prototype -> class table, scale-major / class-minor blocks (:129-141)
        self.prototype_class_identity = torch.zeros(P, num_classes)
        per_scale = P // num_scales
        per_cs = P // num_classes // num_scales
        for s in range(num_scales):
            for k in range(num_classes):
                self.prototype_class_identity[s * per_scale + k * per_cs : s * per_scale + (k + 1) * per_cs, k] = 1
        self.scale_num_prototypes: Dict[int, Tuple[int, int]] = {
            s: (s * per_scale, (s + 1) * per_scale) for s in range(num_scales)
        }  # :146-149
        # kept for state_dict parity only: the kernels never read it (|x|^2 is computed from the staged tile)
        self.ones = nn.Parameter(torch.ones(prototype_shape), requires_grad=False)  # :222

    @property
    def prototype_shape(self):
        return self.prototype_vectors.shape

    @property
    def num_prototypes(self) -> int:
        return self.prototype_vectors.shape[0]

    @property
    def num_classes(self) -> int:
        return self.prototype_class_identity.shape[1]

    def _layout(self, head_rows: int) -> BankLayout:
        cs = int(self.prototype_vectors.shape[1]) * int(self.prototype_vectors.shape[2]) * int(self.prototype_vectors.shape[3])
        return BankLayout(
            num_prototypes=self.num_prototypes,
            num_classes=head_rows,
            num_scales=self.num_scales,
            channels_per_scale=cs,
            scale_ranges=tuple(tuple(int(v) for v in self.scale_num_prototypes[s]) for s in range(self.num_scales)),
        )

    def _class_gather(self, target_labels: torch.Tensor, layout: BankLayout, device) -> ClassGather:
        """Kernel-side description of 'only my class's prototypes' for labels in the reference's convention
        (0 = void, 1..K = class; module_multiscale.py:234-242, loss.py:73).  The (class, slot) table is cached
        until prototype_class_identity is re-assigned (prune_prototypes, attribute assignment), edited in place
        (tensor version counter) or the scale table changes."""
        ident = self.prototype_class_identity
        keys, width, table = cached(self, "_gather_cache", (ident,), (self._tables_version, layout.scale_ranges, str(device)),
                                    lambda: class_gather_table(layout, ident, device))
        B = target_labels.shape[0]
        labels0 = shifted_labels_i32(target_labels.reshape(B, -1), device)
        return ClassGather(labels=labels0, keys=keys, width=width, table=table)

    def _init_scale_head(self, scale_head_type: Optional[str], prototype_shape):
        """model_multiscale.py:113-117: the cross-scale aggregation layer, or None."""
        self.scale_head = None
        if scale_head_type is not None:
            self.scale_head = WeightedAgg(output_type=scale_head_type, channel_dim=prototype_shape[1])

    def _refuse_scale_head(self, what: str):
        """Paths that live inside the fused distance kernel see every scale's ORIGINAL features: under a scale_head the lower
        scales' distances are taken from aggregated features, so these paths refuse instead of answering for another model."""
        if getattr(self, "scale_head", None) is not None:
            raise SpxError(f"{what} runs inside the fused distance kernel, which does not carry a scale_head "
                           "(the written distance map of forward / push_forward does)")

    def _check_1x1(self):
        if self.prototype_vectors.shape[2] != 1 or self.prototype_vectors.shape[3] != 1:
            raise SpxError("only 1x1 prototypes are supported (all reference configs)")

    def _check_fusable(self):
        self._refuse_scale_head("this path")
        self._check_1x1()

    def _scale_head_chain(self, x: torch.Tensor) -> torch.Tensor:
        """``_scale_l2_convolution`` under a scale_head (model_multiscale.py:299-317): the scales run S-1 .. 0; every scale but
        the last first combines its channel slice with the activations of the scale above (csrc/spx_scale_agg.hip: the
        similarity on load, s = proto^T . a on the fp32 matrix pipe, the combine in the epilogue), then the distance kernel
        runs on that scale alone.  Autograd links the pieces: a scale's distance map receives the aggregation's gradient on
        top of whatever else reads it."""
        self._check_1x1()
        if x.dim() != 4 or x.shape[1] % self.num_scales:
            raise SpxError(f"features must be [B, {self.num_scales} x Cs, H, W], got shape {tuple(x.shape)}")
        Cs = int(x.shape[1]) // self.num_scales
        fn = self.prototype_activation_function
        ranges = [tuple(int(v) for v in self.scale_num_prototypes[s]) for s in range(self.num_scales)]
        outs: List[torch.Tensor] = []
        for i in range(self.num_scales - 1, -1, -1):
            lo, hi = ranges[i]
            if hi <= lo:
                raise SpxError(f"scale {i} has no prototypes: a scale_head cannot aggregate an empty scale")
            xs = x[:, i * Cs:(i + 1) * Cs]
            if i < self.num_scales - 1:
                above = self.prototype_vectors[ranges[i + 1][0]:ranges[i + 1][1]]
                if callable(fn):
                    xs = self.scale_head(xs, fn(outs[-1]), above)
                else:
                    xs = self.scale_head.from_distances(xs, outs[-1], above, fn, self.epsilon)
            layout = BankLayout(num_prototypes=hi - lo, num_classes=1, num_scales=1, channels_per_scale=Cs, scale_ranges=((0, hi - lo),))
            _, d, _ = proto_head_forward(xs, self.prototype_vectors[lo:hi], None, layout, want_distances=True,
                                         epsilon=self.epsilon, activation="linear")
            outs.append(d)
        return torch.cat(outs[::-1], dim=1)

    def _scale_head_forward(self, conv_features, return_activations: bool, return_distances: bool):
        """``forward_from_conv_features`` under a scale_head, in the reference's op order (model_multiscale.py:362-388): the
        chained distance map, the similarity on it as ordinary torch code, the head on the fp32 MFMA product kernels."""
        B, _, H, W = conv_features.shape
        dist = self._scale_head_chain(conv_features)
        act = self.distance_2_similarity(dist).permute(0, 2, 3, 1).reshape(B * H * W, -1)
        logits = self.run_last_layer(act).reshape(B, H, W, -1)
        return self._result(logits, dist, act, return_activations, return_distances)

    # -- the rules both classes' forward_from_conv_features follow, each stated here alone ---------
    def _check_patch_classification(self):
        if not getattr(self, "patch_classification", False):
            raise Exception("Original Prototype Network Implementation")

    @staticmethod
    def _wants_distances(return_activations: bool, return_distances: bool) -> bool:
        return return_distances or not return_activations

    @staticmethod
    def _result(logits, dist, act, return_activations: bool, return_distances: bool):
        """The reference's return tuple (model_multiscale.py:377-388)."""
        if return_activations and not return_distances:
            return logits, act
        if return_activations and return_distances:
            return logits, dist, act
        return logits, dist

    @staticmethod
    def _ce_labels(ce_target, x: torch.Tensor):
        """``ce_target`` ([B, H, W] on the grid of ``x``, 0 = void, 1..K) as the kernels' int32 [B, H*W] class index, or None."""
        if ce_target is None:
            return None
        B, _, H, W = x.shape
        if tuple(ce_target.shape) != (B, H, W):
            raise SpxError(f"ce_target must be [{B}, {H}, {W}] (latent grid), got {tuple(ce_target.shape)}")
        return shifted_labels_i32(ce_target.reshape(B, -1), x.device)

    @staticmethod
    def _attach_ce(logits: torch.Tensor, fused_ce, ce_target):
        if fused_ce is not None:
            fused_ce.target = ce_target
            fused_ce.target_version = ce_target._version      # an in-place edit of the labels afterwards voids the attachment
            logits.spx_ce = fused_ce

    def _refuse_packed(self, ce_target) -> str:
        """What a ``PackedMaps`` cannot carry, in the order the refusals fire; returns the name the messages go by."""
        who = "forward_from_conv_features(PackedMaps)"
        self._check_patch_classification()
        if ce_target is not None:
            raise SpxError(f"{who}: ce_target is refused - the fused cross entropy has one mean and one backward coefficient per "
                           f"launch, the objective one per segment {self._packed_ce_hint}")
        if self.scale_head is not None:
            raise SpxError(f"{who}: a scale_head chains launches per scale and has no packed form")
        if callable(self.prototype_activation_function):
            raise SpxError(f"{who}: a callable similarity has no packed form ('log' or 'linear')")
        self._check_1x1()                   # what _check_fusable asks beyond the scale_head refused above
        return who

    @staticmethod
    def _split_packed(lay, r: "_HeadOut", want_dist: bool, want_act: bool):
        """The flat results of ONE launch over ``lay``'s pixel axis -> per segment (logits [B, h_k, w_k, K], distances
        [B, P, h_k, w_k] or [B, J, h_k w_k], activations [B h_k w_k, P]); what is not wanted is None.  Logits and activations
        are row slices, distances strided views of the one map; ``torch.split_with_sizes`` gives each output one backward that
        assembles the packed gradient in a single pass."""
        none = [None] * len(lay)
        logits_k = [t.reshape(lay.B, h, w, -1) for t, (h, w) in zip(lay.split_rows(r.logits), lay.grids)]
        for k, l in enumerate(logits_k):            # segment k of ONE packed forward: SegmentedCrossEntropy runs on ``logits`` as it is
            l.spx_packed = (r.logits, lay, k, r.logits._version)
        acts_k = lay.split_rows(r.act) if want_act else none
        dists_k = list(lay.split_columns(r.dist)) if want_dist else none
        return logits_k, dists_k, acts_k

    def _callable_similarity(self, conv_features: torch.Tensor):
        """(distances [B, P, H, W], activations [B*H*W, P]) under a user-supplied ``prototype_activation_function``
        (model_multiscale.py:329-330: any callable on the distance map): the distance kernel writes the map, the user's function
        runs on it as ordinary torch code (autograd included); the heads on its NHWC view are the fp32 MFMA product kernels."""
        B, _, H, W = conv_features.shape
        _, dist, _ = proto_head_forward(conv_features, self.prototype_vectors, None, self._layout(1), want_distances=True,
                                        epsilon=self.epsilon, activation="log")
        return dist, self.prototype_activation_function(dist).permute(0, 2, 3, 1).reshape(B * H * W, -1)

    def _initialize_add_on(self):
        for m in self.add_on_layers.modules():  # model_multiscale.py:466-476
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def __repr__(self):
        return (
            "PPNet(\n\tfeatures: {},\n\timg_size: {},\n\tprototype_shape: {},\n\tproto_layer_rf_info: {},\n"
            "\tnum_classes: {},\n\tepsilon: {}\n)"
        ).format(self.features, self.img_size, self.prototype_shape, self.proto_layer_rf_info, self.num_classes, self.epsilon)

    def _prune_bank(self, prototypes_to_prune) -> List[int]:
        """The bank half of ``prune_prototypes`` (model_multiscale.py:400-423, :428-432): shrinks ``prototype_vectors``,
        ``ones`` and ``prototype_class_identity`` to the kept rows and re-packs ``scale_num_prototypes``.  Returns the
        kept indices (ascending).  The parameters are re-created, as upstream (optimizers holding the old ones go stale)."""
        drop = set(int(i) for i in prototypes_to_prune)
        keep = sorted(set(range(self.num_prototypes)) - drop)
        prev_hi = 0
        for s in range(self.num_scales):
            lo, hi = self.scale_num_prototypes[s]
            n = len(set(range(lo, hi)) - drop)
            self.scale_num_prototypes[s] = (prev_hi, prev_hi + n)
            prev_hi += n
        self.prototype_vectors = nn.Parameter(self.prototype_vectors.data[keep, ...], requires_grad=True)
        self.ones = nn.Parameter(self.ones.data[keep, ...], requires_grad=False)
        self.prototype_class_identity = self.prototype_class_identity[keep, :]      # bumps _tables_version
        return keep

    # -- reference methods on the distance path ---------------------------------------------------
    _feature_epilogue = None
    _feature_packed = False
    _supports_packed = False      # packed=True: PPNetMultiScale alone sets it

    def fuse_feature_epilogue(self, dtype: Optional[torch.dtype] = torch.bfloat16, packed: bool = False):
        """Opt in (``None``: undo): ``conv_features`` calls ``features.fused(x, "sigmoid", dtype)`` - the MSC maximum, the add-on
        sigmoid and the cast in one launch (csrc/spx_msc.hip) - instead of ``add_on_layers(features(x))``, so that everything
        downstream receives ``dtype`` features without an fp32 round trip.  Accepted only when ``features`` is a
        ``scaleprotoseg_amd.MSC`` and ``add_on_layers`` is exactly ``nn.Sequential(nn.Sigmoid())`` (deeplab_simple).

        ``packed=True`` (``PPNetMultiScale`` only): in training ``conv_features`` returns the four maps as ONE ``PackedMaps``
        (``features.fused_packed``: one launch instead of four), and ``forward`` / ``forward_from_conv_features`` run ONE distance
        launch over all of them and split its outputs into the reference's list.  In eval nothing changes."""
        if packed and dtype is not None and not self._supports_packed:
            raise SpxError(f"fuse_feature_epilogue: packed=True is for PPNetMultiScale, not {type(self).__name__} "
                           "(the group model's spx_group / spx_group_wd attachments are per tensor)")
        if dtype is not None:
            add_on = self.add_on_layers
            if not isinstance(self.features, MSC):
                raise SpxError(f"fuse_feature_epilogue: features is {type(self.features).__name__}, not scaleprotoseg_amd.MSC")
            if type(add_on) is not nn.Sequential or len(add_on) != 1 or type(add_on[0]) is not nn.Sigmoid:
                raise SpxError("fuse_feature_epilogue: add_on_layers must be exactly nn.Sequential(nn.Sigmoid()) (deeplab_simple)")
            if dtype not in (torch.bfloat16, torch.float32):
                raise SpxError(f"fuse_feature_epilogue: dtype {dtype}; bfloat16 or float32")
        object.__setattr__(self, "_feature_epilogue", dtype)
        object.__setattr__(self, "_feature_packed", bool(packed) and dtype is not None)

    def conv_features(self, x):
        """features -> add_on_layers, list-aware for MSC training inputs (model_multiscale.py:246-253)."""
        if self._feature_epilogue is not None:
            if self._feature_packed:
                return self.features.fused_packed(x, "sigmoid", self._feature_epilogue)
            return self.features.fused(x, "sigmoid", self._feature_epilogue)
        x = self.features(x)
        if isinstance(x, list):
            return [self.add_on_layers(xs) for xs in x]
        return self.add_on_layers(x)

    def _scale_l2_convolution(self, x: torch.Tensor) -> torch.Tensor:
        """[B,S*Cs,H,W] -> distances [B,P,H,W] (model_multiscale.py:283-317), one HIP launch (a chain of launches under a
        scale_head)."""
        if getattr(self, "scale_head", None) is not None:
            return self._scale_head_chain(x)
        self._check_fusable()
        _, d, _ = proto_head_forward(
            x, self.prototype_vectors, None, self._layout(1), want_distances=True, epsilon=self.epsilon,
            activation="linear",
        )
        return d

    def prototype_distances(self, x: torch.Tensor) -> torch.Tensor:
        return self._scale_l2_convolution(self.conv_features(x))  # :319-322

    def distance_2_similarity(self, distances: torch.Tensor) -> torch.Tensor:
        """Stand-alone similarity for callers outside the fused path (model_multiscale.py:324-330)."""
        if self.prototype_activation_function == "log":
            return torch.log((distances + 1) / (distances + self.epsilon))
        if self.prototype_activation_function == "linear":
            return -distances
        return self.prototype_activation_function(distances)

    def push_forward(self, x):
        """(conv_features, distances) for the push (model_multiscale.py:390-398)."""
        conv = self.conv_features(x)
        if isinstance(conv, PackedMaps):
            raise SpxError("push_forward: the push runs in eval mode; packed training maps have no push path")
        if isinstance(conv, list):
            return [(c, self._scale_l2_convolution(c)) for c in conv]
        return conv, self._scale_l2_convolution(conv)

    def push_min_distances(self, x, labels_for_grid, void_class=None, max_dist: float = 1e10):
        """Class-masked per-prototype minimum of the distance map of ``x`` over its latent grid, taken INSIDE the distance
        kernel (push_multiscale_optimization.py:68-91 without the [B, P, H, W] map): (indices int64 [B, P], values [B, P]).
        ``labels_for_grid((H, W))`` returns the label map [B, H, W] at the latent resolution (the grid is only known after
        the backbone has run).  Returns None when the fused kernel does not apply (MSC list input, a
        prototype_class_identity that is not one-hot, features off the GPU, a scale_head): the caller then reduces the written map."""
        return self.push_min_from_conv(self.conv_features(x), labels_for_grid, void_class=void_class, max_dist=max_dist)

    def push_min_from_conv(self, conv, labels_for_grid, void_class=None, max_dist: float = 1e10):
        """``push_min_distances`` on features that are already computed (the single-pass push encodes a run of images once and
        keeps the features for the gather)."""
        if isinstance(conv, PackedMaps):
            raise SpxError("push_min_from_conv: the push runs in eval mode; packed training maps have no push path")
        if isinstance(conv, list) or not conv.is_cuda or getattr(self, "scale_head", None) is not None:
            return None
        self._check_fusable()
        layout = self._layout(1)
        ident = self.prototype_class_identity
        keys = cached(self, "_push_key_cache", (ident,), (self._tables_version, layout.scale_ranges, str(conv.device)),
                      lambda: class_gather_table(layout, ident, conv.device)[0] if identity_is_one_hot(ident) else None)
        if keys is None:
            return None
        labels = labels_for_grid((conv.shape[2], conv.shape[3]))
        return push_min_from_features(conv, self.prototype_vectors, layout, labels, ident, void_class=void_class,
                                      max_dist=max_dist, keys=keys)

    def forward(self, x, **kwargs):
        conv = self.conv_features(x)
        if isinstance(conv, PackedMaps):  # MSC in training, one launch: the flags pass through, as upstream :336
            return self.forward_from_conv_features(conv, **kwargs)
        if isinstance(conv, list):  # MSC
            return [self.forward_from_conv_features(c, **kwargs) for c in conv]
        return self.forward_from_conv_features(conv, **kwargs)


class PPNetMultiScale(_PrototypeBankMixin, nn.Module):
    _supports_packed = True

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
    ):
        super().__init__()
        self.img_size = img_size
        self.bottleneck_stride = bottleneck_stride
        self.patch_classification = patch_classification
        self._init_scale_head(scale_head_type, prototype_shape)
        self.prototype_activation_function = prototype_activation_function
        self._init_bank(prototype_shape, num_classes, num_scales)
        self.proto_layer_rf_info = proto_layer_rf_info
        self.features = features
        in_ch = _first_add_on_channels(features)
        self.add_on_layers = _build_add_on(add_on_layers_type, in_ch, self.prototype_shape[1], bottleneck_stride)
        self.last_layer = nn.Linear(self.num_prototypes, self.num_classes, bias=False)  # :225
        if init_weights:
            self._initialize_weights()

    def run_last_layer(self, prototype_activations: torch.Tensor) -> torch.Tensor:
        """last_layer on given activations (model_multiscale.py:243-244; callers outside the fused path): the fp32 MFMA
        product kernel."""
        return wide_linear(prototype_activations, self.last_layer.weight)

    def forward_from_conv_features(
        self, conv_features, return_activations: bool = False, return_distances: bool = False, target_labels=None,
        ce_target=None,
    ) -> Any:
        """Same return-tuple rules as model_multiscale.py:340-388.

        Extension: with ``target_labels`` ([B, H, W] at the latent resolution, 0 = void, 1..K, i.e.
        the tensor the training step passes to the losses, module_multiscale.py:234-242) the distance entry of the
        tuple is a ``ClassDistances`` ([B, J, H*W]: per pixel only the distances to its own class's prototypes, the
        entries KLDLoss reads) and the P-wide fp32 map is never written; ``scaleprotoseg_amd.loss.KLDLoss`` takes it
        as is.  With ``ce_target`` (same convention and grid) the pixel-wise cross entropy of the logits is computed in the
        kernel's logits epilogue and travels on the returned logits as ``logits.spx_ce`` (loss, argmax prediction);
        ``scaleprotoseg_amd.loss.PixelWiseCrossEntropyLoss(ignore_index=-1)`` called with that ``logits`` and the same
        ``ce_target`` returns it instead of running a second pass (loss.py:9-48, caller module_multiscale.py:239).

        A ``PackedMaps`` (``msc_pack``; ``fuse_feature_epilogue(dtype, packed=True)`` in training) is taken as the list of its
        segments, computed by ONE launch: the result is a list with one tuple per segment, in the reference's order and tuple
        modes, and the flags apply to every segment.  ``target_labels`` is then a list of one [B, h_k, w_k] map per segment."""
        if isinstance(conv_features, PackedMaps):
            return self._forward_packed(conv_features, return_activations, return_distances, target_labels, ce_target)
        if isinstance(conv_features, list):
            return [self.forward_from_conv_features(c) for c in conv_features]  # flags dropped, as in :359
        self._check_patch_classification()
        if self.scale_head is not None:
            if target_labels is not None or ce_target is not None:
                raise SpxError("target_labels / ce_target live in the fused distance kernel's epilogues, which do not carry a scale_head")
            return self._scale_head_forward(conv_features, return_activations, return_distances)
        self._check_1x1()                   # what _check_fusable asks beyond the scale_head that left above
        B, _, H, W = conv_features.shape
        if callable(self.prototype_activation_function):
            return self._forward_callable_similarity(conv_features, return_activations, return_distances, target_labels, ce_target)
        want_dist = self._wants_distances(return_activations, return_distances)
        if target_labels is not None and want_dist and tuple(target_labels.shape) != (B, H, W):
            raise SpxError(f"target_labels must be [{B}, {H}, {W}] (latent grid), got {tuple(target_labels.shape)}")
        r = self._head(conv_features, want_dist=want_dist, want_act=return_activations, target_labels=target_labels,
                       ce_target=ce_target)
        dist = r.dist
        if r.gather is not None:
            dist = ClassDistances(values=dist, labels=r.gather.labels, table=r.gather.table, grid=(H, W), target=target_labels,
                                  target_version=target_labels._version)
        logits = r.logits.reshape(B, H, W, -1)
        self._attach_ce(logits, r.ce, ce_target)
        return self._result(logits, dist, r.act, return_activations, return_distances)

    def _head(self, x: torch.Tensor, *, want_dist: bool, want_act: bool, target_labels=None, ce_target=None) -> _HeadOut:
        """Distances, similarity and ``last_layer`` over the pixels of ``x`` ([B, C, H, W], or a packed [1, C, 1, M] with
        ``target_labels`` [1, M]), on the one branch this bank takes: the whole chain in the distance kernel, or - more classes
        than its head carries - the kernel hands out the activations once and the head is the fp32 MFMA product kernel
        (csrc/spx_gemm.hip) on them.  ``target_labels`` count only where distances are wanted (they replace the P-wide map)."""
        K = self.num_classes
        wide = K > MAX_FUSED_HEAD_ROWS          # e.g. scaleproto_coco.gin: 182 classes
        layout = self._layout(1 if wide else K)
        gather = self._class_gather(target_labels, layout, x.device) if target_labels is not None and want_dist else None
        ce_labels = self._ce_labels(ce_target, x)
        out = proto_head_forward(
            x, self.prototype_vectors, None if wide else self.last_layer.weight, layout,
            want_distances=want_dist and gather is None, want_activations=want_act or wide,
            epsilon=self.epsilon, activation=self.prototype_activation_function, class_gather=gather,
            ce_labels=None if wide else ce_labels,
        )
        logits, dist, act = out[:3]
        ce = None
        if wide:
            logits = wide_linear(act, self.last_layer.weight)
            if ce_labels is not None:
                ce = cross_entropy_from_logits(logits, ce_labels)
        elif ce_labels is not None:
            ce = out[3]
        return _HeadOut(logits, dist, act, ce, gather)

    _packed_ce_hint = "(module_multiscale.py:273); call PixelWiseCrossEntropyLoss on each segment's logits"

    def _forward_packed(self, pk: PackedMaps, return_activations, return_distances, target_labels, ce_target):
        """The four training maps on one pixel axis (``pk.features`` [1, C, 1, M]): one forward launch - and, through autograd,
        one pixel-side and one parameter-side backward launch - for all segments, on the head branch a single map takes.
        Distances, activations and logits are per-pixel quantities, so the outputs are split by columns / rows
        (``_split_packed``)."""
        who = self._refuse_packed(ce_target)
        lay = pk.layout
        want_dist = self._wants_distances(return_activations, return_distances)
        if target_labels is not None:
            lay.check_labels(target_labels, f"{who}: target_labels")                       # before any launch
        r = self._head(pk.features, want_dist=want_dist, want_act=return_activations,
                       target_labels=lay.pack_labels(target_labels) if target_labels is not None and want_dist else None)
        logits_k, dists_k, acts_k = self._split_packed(lay, r, want_dist, return_activations)
        if r.gather is not None:
            dists_k = [ClassDistances(values=v, labels=r.gather.labels[0, o:o + m].view(lay.B, -1), table=r.gather.table, grid=g,
                                      target=t, target_version=t._version)
                       for v, o, m, g, t in zip(dists_k, lay.offsets, lay.sizes, lay.grids, target_labels)]
        return [self._result(l, d, a, return_activations, return_distances) for l, d, a in zip(logits_k, dists_k, acts_k)]

    def _forward_callable_similarity(self, conv_features, return_activations, return_distances, target_labels, ce_target):
        """A user-supplied ``prototype_activation_function`` (``_callable_similarity``) and the head on the fp32 MFMA product
        kernel: the reference's op order with its two GEMM-shaped pieces on this package's kernels."""
        if target_labels is not None or ce_target is not None:
            raise SpxError("target_labels / ce_target need a built-in similarity ('log' or 'linear')")
        B, _, H, W = conv_features.shape
        dist, act = self._callable_similarity(conv_features)
        logits = wide_linear(act, self.last_layer.weight).reshape(B, H, W, -1)
        return self._result(logits, dist, act, return_activations, return_distances)

    def prune_prototypes(self, prototypes_to_prune: List[int]):
        """Drop prototype rows and re-pack the scale table (model_multiscale.py:400-432)."""
        keep = self._prune_bank(prototypes_to_prune)
        self.last_layer.in_features = self.num_prototypes
        self.last_layer.out_features = self.num_classes
        self.last_layer.weight.data = self.last_layer.weight.data[:, keep]

    def set_last_layer_incorrect_connection(self, incorrect_strength: float):
        """+1 own class / incorrect_strength elsewhere (model_multiscale.py:449-464)."""
        pos = torch.t(self.prototype_class_identity).to(self.last_layer.weight.device)
        self.last_layer.weight.data.copy_(1 * pos + incorrect_strength * (1 - pos))
        invalidate_pack_cache()

    def _initialize_weights(self):
        self._initialize_add_on()
        self.set_last_layer_incorrect_connection(incorrect_strength=-0.5)


def construct_PPNet(
    features: nn.Module,
    img_size: int = 224,
    prototype_shape: Tuple[int, int, int, int] = (2000, 512, 1, 1),
    num_classes: int = 200,
    prototype_activation_function: str = "log",
    add_on_layers_type: str = "bottleneck",
    scale_head_type: Optional[str] = None,
    **kwargs,
) -> PPNetMultiScale:
    """Factory with the reference's argument meaning (model_multiscale.py:480-515); the backbone is passed
    in as a module because the reference's backbone zoo (absent submodule, URL downloads) is out of scope."""
    return PPNetMultiScale(
        features=features, img_size=img_size, prototype_shape=prototype_shape, proto_layer_rf_info=[],
        num_classes=num_classes, init_weights=True, prototype_activation_function=prototype_activation_function,
        add_on_layers_type=add_on_layers_type, scale_head_type=scale_head_type, **kwargs,
    )
