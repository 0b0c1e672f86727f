"""Loss of the hot path's distance output: KLDLoss (segmentation/model/loss.py:51-146), vectorised, and its
class-gathered form.

The reference's KLDLoss reads, for a pixel of class c, only the distance columns of class c's prototypes
(loss.py:89-107).  ``ClassDistances`` carries exactly those entries ([B, J, H*W] slot planes, produced by the fused kernels
with ``forward_from_conv_features(..., target_labels=...)``), so the fp32 [B, P, H, W] map and its gradient never
cross HBM.  ``KLDLoss`` accepts either form and returns the same value; on fp32 GPU tensors the pixel loops run in the
HIP kernels of csrc/spx_kld.hip (differentiable through ``ClassDistances.values``).  There is no other backend: inputs the
kernels do not take (CPU tensors, fp64, more than 16 slots per class) raise ``SpxError``.  (The torch restatement of the same
algebra that the tests hold the kernels against is test infrastructure and lives outside the package.)
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple, Union

import torch
from torch import nn

from . import _gathered, _lib
from ._cache import cached
from ._gathered import ClassDistances, Gathered, class_slot_table, gather_class_distances, slot_scale_table  # noqa: F401
from ._lib import SpxError
from .functional import SegmentedCE, cross_entropy_from_logits, segmented_cross_entropy, shifted_labels_i32


class PixelWiseCrossEntropyLoss(nn.Module):
    """Drop-in for segmentation/model/loss.py:9-48: cross entropy over the [..., K] logits with labels shifted by one
    (1..K -> 0..K-1; the training modules pass ``ignore_index=-1`` so that void = 0 is skipped,
    module_multiscale.py:162-164), optionally with the per-pixel correctness of the non-ignored pixels.

    On GPU tensors the loss runs in HIP: if the logits come from ``forward_from_conv_features(..., ce_target=target)``
    the value was already computed in the logits epilogue (``logits.spx_ce``) and is returned as is;
    otherwise the stand-alone kernels of csrc/spx_ce.hip run.  Labels outside 0..K-1 other than ``ignore_index`` make
    torch raise; here they are ignored.  Logits that are not on the GPU raise ``SpxError``: there is no other backend."""

    def __init__(self, ignore_index: int = 255, return_correct: bool = False) -> None:
        super().__init__()
        self.return_correct = return_correct
        self.ignore_index = ignore_index

    def forward(self, predicted_logits: torch.Tensor, target_labels: torch.Tensor):
        _lib.require_gpu(predicted_logits, "cross entropy: logits")
        fused = getattr(predicted_logits, "spx_ce", None)
        K = predicted_logits.size(-1)
        ignores_a_class = self.ignore_index is not None and 0 <= self.ignore_index < K
        stale = fused is not None and (fused.target is not target_labels or fused.target_version != target_labels._version)
        if fused is not None and not stale and not ignores_a_class and not self.return_correct:
            return fused.loss                       # the epilogue's value: not one more launch here
        labels0 = target_labels.reshape(-1).to(predicted_logits.device) - 1                  # loss.py:32
        if fused is None or stale or ignores_a_class:
            lab = labels0 if not ignores_a_class else torch.where(labels0 == self.ignore_index, torch.full_like(labels0, -1), labels0)
            fused = cross_entropy_from_logits(predicted_logits, lab)
        if not self.return_correct:
            return fused.loss
        correct = fused.pred.reshape(-1).to(labels0.dtype) == labels0
        mask = (labels0 != self.ignore_index).nonzero().squeeze()                             # loss.py:43-46
        return fused.loss, correct[mask]


class SegmentedCrossEntropy(nn.Module):
    """The cross entropy of every segment of an MSC training step in three launches (module_multiscale.py:232-310 calls
    ``PixelWiseCrossEntropyLoss`` once per map: three launches, a division and - with ``return_correct`` - a ``nonzero()`` host
    sync each).  ``forward(logits, targets)`` takes the forward's per-segment logits ``[o[0] for o in outputs]`` ([..., K] each)
    and the list of their targets (0 = void, 1..K, ``ignore_index`` as in ``PixelWiseCrossEntropyLoss``) and returns a
    ``SegmentedCE``: ``losses`` [S] and ``mean`` [] (differentiable), ``valid`` / ``correct`` int32 [S] - the reference's
    ``correct.shape[0]`` and ``sum(correct)`` as device counters - ``pred`` and ``labels`` int32 [M].  Nothing reads the host, so
    the step stays capturable.

    Segments of ONE packed forward (``forward_from_conv_features(PackedMaps)``: every segment's logits carry ``spx_packed``)
    run on the packed [M, K] logits as they are and send their gradient straight to them; any other list is reshaped and
    concatenated once.  Up to 16 segments, none empty; GPU fp32 logits only - anything else raises ``SpxError``."""

    def __init__(self, ignore_index: int = 255) -> None:
        super().__init__()
        self.ignore_index = ignore_index

    @staticmethod
    def _packed_base(logits):
        """(packed logits [M, K], layout) when ``logits`` are the segments of one packed forward, in order and unedited."""
        tags = [getattr(l, "spx_packed", None) for l in logits]
        if any(t is None for t in tags):
            return None
        base, layout = tags[0][0], tags[0][1]
        if len(layout) != len(tags) or base.dim() != 2 or base.dtype != torch.float32 or not base.is_contiguous():
            return None
        for k, (t, l) in enumerate(zip(tags, logits)):
            if t[0] is not base or t[1] is not layout or t[2] != k or t[3] != base._version or l._version != t[3]:
                return None
        return base, layout

    def forward(self, logits, targets) -> SegmentedCE:
        who = "SegmentedCrossEntropy"
        if isinstance(logits, torch.Tensor) or isinstance(targets, torch.Tensor):
            raise SpxError(f"{who}: a list of per-segment logits and the list of their targets")
        logits, targets = list(logits), list(targets)
        S = len(logits)
        if not 1 <= S <= _lib.SPX_CE_MAX_SEGMENTS:
            raise SpxError(f"{who}: {S} segments (1 to {_lib.SPX_CE_MAX_SEGMENTS})")
        if len(targets) != S:
            raise SpxError(f"{who}: {len(targets)} target maps for {S} segments")
        K = int(logits[0].shape[-1]) if logits[0].dim() else 0
        for k, (l, t) in enumerate(zip(logits, targets)):
            _lib.require_gpu(l, f"{who}: logits[{k}]")
            if l.dtype != torch.float32:
                raise SpxError(f"{who}: logits[{k}] are {l.dtype}; the kernels take fp32")
            if l.dim() < 1 or int(l.shape[-1]) != K or K < 1:
                raise SpxError(f"{who}: logits[{k}] {tuple(l.shape)} do not end in the {K} classes of logits[0]")
            if l.numel() == 0:
                raise SpxError(f"{who}: segment {k} is empty")
            if tuple(t.shape) != tuple(l.shape[:-1]):
                raise SpxError(f"{who}: targets[{k}] must be {tuple(l.shape[:-1])} (the segment's pixels), got {tuple(t.shape)}")
        packed = self._packed_base(logits)
        if packed is not None:
            base, layout = packed
            offsets = tuple(layout.offsets) + (layout.M,)
            raw = layout.pack_labels(targets).reshape(-1)
        else:
            base = torch.cat([l.reshape(-1, K) for l in logits]) if S > 1 else logits[0].reshape(-1, K).contiguous()
            offsets = [0]
            for l in logits:
                offsets.append(offsets[-1] + l.numel() // K)
            raw = torch.cat([t.reshape(-1) for t in targets]) if S > 1 else targets[0].reshape(-1)
        labels0 = shifted_labels_i32(raw, base.device)                                        # loss.py:32, one launch
        if self.ignore_index is not None and 0 <= self.ignore_index < K:
            labels0 = torch.where(labels0 == self.ignore_index, torch.full_like(labels0, -1), labels0)
        return segmented_cross_entropy(base, labels0, offsets)


def _kld_segment_passes(lib, v, lab, K, Wk, s):
    """The three reduction passes over the gathered planes (csrc/spx_kld.hip): (a_fx int64 [B,K,J,J], counts [B,K], lse [B,K,J],
    scale double [1]).  One zero-filled workspace holds the integer tables: [a_fx | ssum_fx | scale | keys | counts | range keys];
    the fixed-point scale of the pair sums is derived on the device (segment-lse kernel) from the value range pass 0 collects:
    |p_j (l_k - l_j)| is bounded by twice the range, and HW terms must stay inside int64 - no host sync, no torch glue."""
    B, J, HW = v.shape
    dev = v.device
    n_a, n_s = B * K * J * J, B * K * J
    ws = torch.zeros(n_a + n_s + 1 + (n_s + B * K + 2 + 1) // 2, dtype=torch.int64, device=dev)
    a_fx, ssum_fx = ws[:n_a].view(B, K, J, J), ws[n_a:n_a + n_s]
    scale = ws[n_a + n_s:n_a + n_s + 1].view(torch.float64)
    tail32 = ws[n_a + n_s + 1:].view(torch.int32)
    keys, counts, rng = tail32[:n_s], tail32[n_s:n_s + B * K].view(B, K), tail32[n_s + B * K:n_s + B * K + 2]
    _lib.check(lib.spx_kld_segment_max(_lib.ptr(v), _lib.ptr(lab), B, J, HW, Wk, K, _lib.ptr(keys), _lib.ptr(counts), _lib.ptr(rng), s))
    _lib.check(lib.spx_kld_segment_sumexp(_lib.ptr(v), _lib.ptr(lab), B, J, HW, Wk, K, _lib.ptr(keys), _lib.ptr(ssum_fx), s))
    lse = torch.empty((B, K, J), dtype=torch.float32, device=dev)
    _lib.check(lib.spx_kld_segment_lse(_lib.ptr(keys), _lib.ptr(ssum_fx), n_s, _lib.ptr(lse), _lib.ptr(rng), HW, _lib.ptr(scale), s))
    _lib.check(lib.spx_kld_pair_sums(_lib.ptr(v), _lib.ptr(lab), B, J, HW, Wk, K, _lib.ptr(lse), _lib.ptr(scale), _lib.ptr(a_fx), s))
    return a_fx, counts, lse, scale


class _KLDFusedLoss(torch.autograd.Function):
    """The whole loss of class-gathered planes on the GPU in SIX launches (workspace fill, segment max + value range, segment
    sum-exp, lse + fixed-point scale, pair sums, and spx_kld_gram_loss: symmetric KL of the slot pairs, exp(-kld), mean and its
    gradient with respect to the pair sums, loss.py:113-142); backward: one scalar multiply + the per-pixel gradient pass."""

    @staticmethod
    def forward(ctx, planes, g, pair_ok):
        lib = _lib.load()
        v, lab = _gathered.launch_operands(g)                                   # g.planes is ``planes``
        B, J, HW = v.shape
        K = g.table.shape[0]
        s = _lib.stream_ptr()
        a_fx, counts, lse, scale = _kld_segment_passes(lib, v, lab, K, g.walk_w, s)
        n = B * K * J * J
        out = torch.empty((2 * n + 2,), dtype=torch.float32, device=v.device)
        A, cf, loss = out[:n], out[n:2 * n], out[2 * n:]                       # loss = (value, 1 / number of valid pairs)
        part = torch.empty((2 * B * K,), dtype=torch.float64, device=v.device)
        _lib.check(lib.spx_kld_gram_loss(_lib.ptr(a_fx), _lib.ptr(scale), _lib.ptr(counts), _lib.ptr(pair_ok), B * K, K, J,
                                         _lib.ptr(A), _lib.ptr(cf), _lib.ptr(part), _lib.ptr(loss), s))
        ctx.save_for_backward(v, lab, lse, A, cf, loss)
        ctx.K = K
        return loss[0].reshape(())

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        v, lab, lse, A, cf, loss = ctx.saved_tensors
        B, J, HW = v.shape
        grad = torch.empty_like(v)
        coef = (g.reshape(()).float() * loss[1]).reshape(1).contiguous()       # dLoss_total/dloss x 1/n, on the device
        _lib.check(lib.spx_kld_backward(_lib.ptr(v), _lib.ptr(lab), B, J, HW, ctx.K, _lib.ptr(lse), _lib.ptr(A), _lib.ptr(cf), _lib.ptr(coef),
                                        _lib.ptr(grad), _lib.stream_ptr()))
        return grad, None, None


def segment_pair_sums(planes: torch.Tensor, labels0: torch.Tensor, K: int, W: int = 0) -> torch.Tensor:
    """A [B, K, J, J] = sum over the segment's pixels of p_j (l_k - l_j) (= -KL(j || k); diagonal 0) of class-gathered planes
    [B, J, H*W] through the three reduction passes of csrc/spx_kld.hip - what ``KLDLoss`` builds its value from (no autograd;
    diagnostics and tests).  ``W``: row length of the pixel grid (0 = unknown: linear walk)."""
    lib = _lib.load()
    _gathered.check_domain(planes, K, "segment_pair_sums")
    v, lab = _gathered.launch_operands(Gathered(planes, labels0, None, 0))
    a_fx, _, _, scale = _kld_segment_passes(lib, v, lab, K, _gathered.walk_width(W, v.shape[2]), _lib.stream_ptr())
    return (a_fx.to(torch.float64) / scale).float()


class _SlotTable:
    def _slot_table(self) -> torch.Tensor:
        """class_slot_table of the loss's identity, built once per identity object and in-place version."""
        ident = self.prototype_class_identity
        return cached(self, "_slot_table_cache", (ident,), (), lambda: class_slot_table(ident))


class KLDLoss(_SlotTable, nn.Module):
    """Drop-in for segmentation/model/loss.py:51-146: same constructor, same ``forward(prototype_distances,
    target_labels)`` (labels 0 = void, 1..K = class); ``prototype_distances`` may be the [B, P, H, W] map or a
    ``ClassDistances``.  One pass of segment reductions instead of the reference's (image, class, scale, pair)
    Python loops with host syncs."""

    def __init__(self, prototype_class_identity: torch.Tensor, num_scales: int, scale_num_prototypes: Dict[int, Tuple[int, int]]) -> None:
        super().__init__()
        self.prototype_class_identity = prototype_class_identity
        self.num_scales = num_scales
        self.scale_num_prototypes = scale_num_prototypes

    def _pair_mask(self, table: torch.Tensor) -> torch.Tensor:
        """[K, J, J] bool: slots j < k of class c are prototypes of the same scale (loss.py:99-104, :118-121); host-side work
        with a device read-back, not something to redo per step."""
        scales = tuple(sorted((int(s), tuple(r)) for s, r in self.scale_num_prototypes.items()))
        return cached(self, "_pair_mask_cache", (table,), (scales,), lambda: self._pair_mask_build(table).to(table.device))

    def _table_on(self, table: torch.Tensor, dev) -> torch.Tensor:
        """``table`` on ``dev`` (the same object every step, so the pair-mask cache keyed on it holds)."""
        if table.device == dev:
            return table
        return cached(self, "_table_dev_cache", (table,), (str(dev),), lambda: table.to(dev))

    def _pair_mask_build(self, table: torch.Tensor) -> torch.Tensor:
        K, J = table.shape
        scale = torch.full((K, J), -1, dtype=torch.long)
        t = table.cpu()
        for s in range(self.num_scales):
            lo, hi = self.scale_num_prototypes[s]
            scale[(t >= lo) & (t < hi)] = s
        same = (scale.unsqueeze(2) == scale.unsqueeze(1)) & (scale.unsqueeze(2) >= 0)
        upper = torch.triu(torch.ones(J, J, dtype=torch.bool), diagonal=1)
        return same & upper

    def _gathered(self, prototype_distances, target_labels: torch.Tensor) -> Gathered:
        if isinstance(prototype_distances, ClassDistances):
            table = self._table_on(prototype_distances.table, prototype_distances.values.device)
            return _gathered.from_class_distances(prototype_distances, target_labels, table)
        return _gathered.from_distance_map(prototype_distances, target_labels, self._table_on(self._slot_table(), prototype_distances.device))

    def forward(self, prototype_distances: Union[torch.Tensor, ClassDistances], target_labels: torch.Tensor) -> torch.Tensor:
        # the gathered planes on the GPU: segment statistics and the gradient run in the HIP kernels; nothing on this path reads
        # a value back to the host (capturable in a HIP graph)
        g = self._gathered(prototype_distances, target_labels)
        _gathered.check_domain(g.planes, g.table.shape[0], "KLD loss")
        loss = _KLDFusedLoss.apply(g.planes, g, self._pair_mask_u8(g.table, g.planes.device))
        return loss if g.poison is None else loss * g.poison                   # NaN when the planes were gathered under other classes

    def _pair_mask_u8(self, table: torch.Tensor, dev) -> torch.Tensor:
        """The [K, J, J] pair mask as uint8 on ``dev`` (cached with the mask it is made from)."""
        m = self._pair_mask(table)
        return cached(self, "_pair_u8_cache", (m,), (torch.device(dev),), lambda: m.to(device=dev, dtype=torch.uint8).contiguous())


class KLDLossGroup(KLDLoss):
    """Drop-in for segmentation/model/loss.py:461-545: same constructor, same ``forward(list_group_activation,
    target_labels)``.  The groups of a pixel's class play the role KLDLoss gives the class's prototypes (every group
    pair of a class is compared, loss.py:527-536), so the segment kernels are shared; ``list_group_activation`` may
    also be the concatenated [M, n_projections * num_groups] tensor the grouping head produces."""

    scale_num_prototypes: Dict[int, Tuple[int, int]] = {}      # no scales here: every group pair of a class is compared

    def __init__(self, prototype_class_identity: torch.Tensor, group_class_identity: torch.Tensor, num_groups: int) -> None:
        nn.Module.__init__(self)
        self.prototype_class_identity = prototype_class_identity
        self.group_class_identity = group_class_identity
        self.num_groups = num_groups

    def _class_tables(self):
        """``_gathered.group_class_tables`` of the two identities, rebuilt when either is edited in place or re-assigned
        (finetune_wandb_group.py:77-78)."""
        ident, gci, G = self.prototype_class_identity, self.group_class_identity, self.num_groups
        return cached(self, "_class_tables_cache", (ident, gci), (G,), lambda: _gathered.group_class_tables(ident, gci, G))

    def _pair_mask_build(self, table: torch.Tensor) -> torch.Tensor:
        K, J = table.shape
        upper = torch.triu(torch.ones(J, J, dtype=torch.bool), diagonal=1)
        return upper.unsqueeze(0) & (table.cpu()[:, :1] >= 0).unsqueeze(2)

    def _gathered(self, list_group_activation, target_labels: torch.Tensor) -> Gathered:
        proj, table = self._class_tables()
        dev = (list_group_activation if isinstance(list_group_activation, torch.Tensor) else list_group_activation[0]).device
        # (the projection table on the device once, not a host copy per call: the loss stays legal inside a captured step)
        proj = cached(self, "_proj_dev_cache", (proj,), (str(dev),), lambda: proj.to(dev))
        return _gathered.from_groups(list_group_activation, target_labels, proj, self._table_on(table, dev))

    def forward(self, list_group_activation, target_labels: torch.Tensor) -> torch.Tensor:       # the reference's argument names
        return super().forward(list_group_activation, target_labels)


# ---- weight-side regularisers (segmentation/model/loss.py:351-464, module_multiscale*.py L1) ----------------------------
REG_ENT, REG_CEG, REG_SMAX, REG_L1 = 1, 2, 4, 8        # SPX_REG_* of include/spx_hip.h: term b <-> bit b
_GROUP_TERMS = REG_ENT | REG_CEG | REG_SMAX


class _RegSpec:
    """Everything the regulariser kernels read besides the two weight tensors: the module's GroupTables with their block /
    span tables, the fp32 device copy of the L1 head's class identity, the zero-filled workspace (whose ticket word the
    forward leaves zeroed) and the constant part of the spx_reg descriptor."""

    def __init__(self, tables, ident, terms: int, weights, epsilon: float, device):
        self.tables, self.ident, self.terms = tables, ident, int(terms)
        r = _lib.SpxReg()
        if terms & _GROUP_TERMS:
            reg = tables.reg
            r.U, r.P = tables.U, tables.P
            r.row_block, r.row_local = _lib.ptr(tables.row_block), _lib.ptr(tables.row_local)
            r.col_block, r.col_local = _lib.ptr(tables.col_block), _lib.ptr(tables.col_local)
            r.flat_col, r.block_info, r.spans = _lib.ptr(tables.flat_col), _lib.ptr(reg.block_info), _lib.ptr(reg.spans)
            r.nblocks, r.G, r.S, r.nspans = len(tables.block_cols), reg.G, reg.S, reg.nspans
        if terms & REG_L1:
            r.ident = _lib.ptr(ident)
            r.Uh, r.K = int(ident.shape[0]), int(ident.shape[1])
        r.epsilon = float(epsilon)
        r.weights = (C.c_float * 4)(*[float(w) for w in weights])
        r.terms = int(terms)
        self.desc = r
        nbytes = _lib.load().spx_reg_workspace_bytes(C.byref(r))
        if nbytes == 0:
            raise SpxError(_lib.load().spx_last_error().decode("utf-8", "replace"))
        self.workspace = torch.zeros(((nbytes + 7) // 8,), dtype=torch.float64, device=device)

    def bind(self, wd: Optional[torch.Tensor], head: Optional[torch.Tensor]):
        r = self.desc
        if self.terms & _GROUP_TERMS:
            if tuple(wd.shape) != (r.U, r.P):
                raise SpxError(f"regularisers: Wd {tuple(wd.shape)} does not match the group tables [{r.U}, {r.P}]")
            r.wd = _lib.ptr(wd)
        if self.terms & REG_L1:
            if tuple(head.shape) != (r.K, r.Uh):
                raise SpxError(f"regularisers: head {tuple(head.shape)} does not match the identity's [{r.K}, {r.Uh}]")
            r.head = _lib.ptr(head)
        return C.byref(r)


class _RegFn(torch.autograd.Function):
    """(total, terms[4]) of the enabled terms in ONE launch (spx_reg_fwd); backward ONE launch (spx_reg_bwd) writing d Wd
    (dense [U, P]) and d head, scaled by the upstream gradients read on the device - no host synchronisation either way."""

    @staticmethod
    def forward(ctx, wd, head, spec):
        lib = _lib.load()
        wd_c = wd.detach().contiguous() if wd is not None else None
        head_c = head.detach().contiguous() if head is not None else None
        dev = (wd_c if wd_c is not None else head_c).device
        total = torch.empty((), dtype=torch.float32, device=dev)
        terms = torch.empty((4,), dtype=torch.float32, device=dev)
        _lib.check(lib.spx_reg_fwd(spec.bind(wd_c, head_c), _lib.ptr(total), _lib.ptr(terms), _lib.ptr(spec.workspace),
                                   _lib.stream_ptr()))
        ctx.save_for_backward(wd_c, head_c)
        ctx.spec = spec
        ctx.set_materialize_grads(False)
        return total, terms

    @staticmethod
    def backward(ctx, g_total, g_terms):
        if g_total is None and g_terms is None:
            return None, None, None
        wd, head = ctx.saved_tensors
        gt = g_total.float().contiguous() if g_total is not None else None
        gs = g_terms.float().contiguous() if g_terms is not None else None
        d_wd = torch.empty_like(wd) if wd is not None else None
        d_head = torch.empty_like(head) if head is not None else None
        _lib.check(_lib.load().spx_reg_bwd(ctx.spec.bind(wd, head), _lib.ptr(gt), _lib.ptr(gs), _lib.ptr(d_wd), _lib.ptr(d_head),
                                           _lib.stream_ptr()))
        return d_wd, d_head, None


def _is_group_model(ppnet) -> bool:
    return hasattr(ppnet, "group_projection") and hasattr(ppnet, "last_layer_group")


def _check_weights(ws, what: str) -> None:
    for w in ws:
        _lib.require_gpu(w, f"{what}: a weight")
        if w.dtype != torch.float32:
            raise SpxError(f"{what}: weights are {w.dtype}; the kernels take fp32")


def _reg_spec(net, terms: int, weights, epsilon: float, device, holder) -> _RegSpec:
    """The kernel-side spec of ``net``, cached in ``holder._spx_reg_spec`` on the group tables' identity (rebuilt with every
    table version: a pruned bank or re-assigned identity gives new tables), the L1 identity tensor and its version."""
    tables = src = version = None
    if terms & _GROUP_TERMS:
        _, _, _, tables = net._group_index(device)
        if tables is None or getattr(tables, "reg", None) is None:
            raise SpxError("regularisers: the group tables are outside the kernels' domain (GPU, <= 192 classes with "
                           "prototypes, the same number of groups <= 16 for every class, <= 16 scales)")
    if terms & REG_L1:
        src = net.group_class_identity if _is_group_model(net) else net.prototype_class_identity
        version = getattr(net, "_tables_version", 0)

    def build():
        ident = src.detach().to(device=device, dtype=torch.float32).contiguous() if terms & REG_L1 else None
        return _RegSpec(tables, ident, terms, weights, epsilon, device)

    return cached(holder, "_spx_reg_spec", (tables, src), (str(device), version), build)


def _reg_apply(net, terms: int, weights, epsilon: float, holder, logits: Optional[torch.Tensor] = None):
    head = None
    if terms & REG_L1:
        head = net.last_layer_group.weight if _is_group_model(net) else net.last_layer.weight
        _check_weights([head], "regularisers")
        dev = head.device
    wd = None
    if terms & _GROUP_TERMS:
        ws = [gp.weight for gp in net.group_projection]
        _check_weights(ws, "regularisers")
        dev = ws[0].device
        tag = getattr(logits, "spx_group_wd", None) if logits is not None else None
        if tag is not None and tag[1] is net and tag[2] == tuple(w._version for w in ws):
            wd = tag[0]                              # the Wd this very forward multiplied with: one scatter for both gradients
        else:
            wd = net._dense_group_matrix()
    return _RegFn.apply(wd, head, _reg_spec(net, terms, weights, epsilon, dev, holder))


class _RegBase(nn.Module):
    def __init__(self, ppnet, terms: int, weights, epsilon: float) -> None:
        super().__init__()
        self.ppnet = ppnet
        self.epsilon = epsilon
        self._terms, self._weights = int(terms), tuple(float(w) for w in weights)

    def _run(self, logits: Optional[torch.Tensor] = None):
        return _reg_apply(self.ppnet, self._terms, self._weights, float(self.epsilon), self, logits)


class GroupRegularizers(_RegBase):
    """The weight-side terms of the group phase's objective in one forward launch and one backward launch
    (segmentation/model/module_multiscale_group_train.py:274-297): ``forward(logits=None)`` returns ``(total, terms)``
    with terms = [group entropy, group cross entropy, scale max, L1] (fp32 [4], for logging without a sync) and total =
    the weighted sum in the reference's order.  Every term is computed and differentiated whatever its weight, as in the
    reference (a weight of 0 times a non-finite term is NaN there too).  ``logits``: the output of this model's forward
    of the same step; the terms then differentiate through the dense group matrix that forward used, so the group
    weights still receive their gradient from one scatter.  On a prototype-phase model only the L1 of ``last_layer``
    exists (the group weights must be 0)."""

    def __init__(self, ppnet, group_ent: float = 0.0, crs_ent_group: float = 0.0, scale_max: float = 0.0, l1: float = 0.0,
                 epsilon: float = 1e-5) -> None:
        if _is_group_model(ppnet):
            terms = _GROUP_TERMS | REG_L1
        else:
            if group_ent or crs_ent_group or scale_max:
                raise SpxError("GroupRegularizers: a prototype-phase model has no group projections (group weights must be 0)")
            terms = REG_L1
        super().__init__(ppnet, terms, (group_ent, crs_ent_group, scale_max, l1), epsilon)

    def forward(self, logits: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        return self._run(logits)


class _OneTerm(_RegBase):
    BIT = 0

    def __init__(self, ppnet, epsilon: float = 1e-5) -> None:
        if not _is_group_model(ppnet):
            raise SpxError(f"{type(self).__name__} needs a group-phase model (group_projection, last_layer_group)")
        weights = [1.0 if (1 << b) == self.BIT else 0.0 for b in range(4)]
        super().__init__(ppnet, self.BIT, weights, epsilon)

    def forward(self) -> torch.Tensor:
        return self._run()[0]          # total = 1 * term: a 0-d output of the kernel itself, no view to differentiate


class EntropyGroup(_OneTerm):
    """Drop-in for segmentation/model/loss.py:398-426 (``EntropyGroup(ppnet, epsilon)``, ``forward()``) on the GPU kernels."""

    BIT = REG_ENT


class CrossEntropyGroup(_OneTerm):
    """Drop-in for segmentation/model/loss.py:429-464 on the GPU kernels."""

    BIT = REG_CEG


class ScaleMax(_OneTerm):
    """Drop-in for segmentation/model/loss.py:351-395 (``ScaleMax(ppnet)``) on the GPU kernels; the gradient goes to the first
    maximal column of every span, as torch's ``max(dim)``."""

    BIT = REG_SMAX

    def __init__(self, ppnet) -> None:
        super().__init__(ppnet, 1e-5)


def head_l1(ppnet) -> torch.Tensor:
    """``(W * (1 - identity^T)).norm(p=1)`` of ``last_layer`` (prototype phase, module_multiscale.py:260-261, module.py:218-220)
    or ``last_layer_group`` (group phase, module_multiscale_group_train.py:283-285) in one launch; differentiable to W."""
    return _reg_apply(ppnet, REG_L1, (0.0, 0.0, 0.0, 1.0), 1e-5, ppnet)[0]


# ---- activation losses of the labelled pixels (segmentation/model/loss.py:149-348) ---------------------------------------
ACT_SPAT, ACT_SAMPL, ACT_NORM = 1, 2, 4                # SPX_ACT_* of include/spx_hip.h: term b <-> bit b
_ACT_MODES = {"log": 1, "linear": 2}
_NORM_TYPES = {"l1": 0, "linf": 1}


def _act_desc(v, lab, sid, W, K, cfg):
    B, J, HW = v.shape
    d = _lib.SpxActLoss()
    d.vals, d.labels, d.slot_scale = _lib.ptr(v), _lib.ptr(lab), _lib.ptr(sid)
    d.B, d.J, d.HW, d.W, d.K = B, J, HW, W, K
    d.mode, d.terms, d.norm_type = cfg["mode"], cfg["terms"], cfg["norm_type"]
    d.epsilon = cfg["epsilon"]
    d.weights = (C.c_float * 3)(*cfg["weights"])
    return d


class _ActLossFn(torch.autograd.Function):
    """(total, terms[3]) of class-gathered planes in FOUR launches (workspace fill, segment maxima, segment sums, finish:
    csrc/spx_actloss.hip); backward ONE launch, scaled by the upstream gradients read on the device."""

    @staticmethod
    def forward(ctx, planes, g, sid, cfg):
        lib = _lib.load()
        v, lab = _gathered.launch_operands(g)                                   # g.planes is ``planes``
        B, J, HW = v.shape
        s = _lib.stream_ptr()
        ctx.WK = W, K = g.walk_w, g.table.shape[0]
        d = _act_desc(v, lab, sid, W, K, cfg)
        nbytes = lib.spx_actloss_workspace_bytes(C.byref(d))
        if nbytes == 0:
            raise SpxError(lib.spx_last_error().decode("utf-8", "replace"))
        ws = torch.zeros((nbytes // 8,), dtype=torch.int64, device=v.device)
        coef = torch.empty((B * K, 6, J), dtype=torch.float32, device=v.device)
        out = torch.empty((7,), dtype=torch.float32, device=v.device)
        _lib.check(lib.spx_actloss_segment_max(C.byref(d), _lib.ptr(ws), s))
        _lib.check(lib.spx_actloss_segment_sums(C.byref(d), _lib.ptr(ws), s))
        _lib.check(lib.spx_actloss_finish(C.byref(d), _lib.ptr(ws), _lib.ptr(coef), _lib.ptr(out), s))
        ctx.save_for_backward(v, lab, sid, coef)
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)
        return out[6].reshape(()), out[:3]

    @staticmethod
    def backward(ctx, g_total, g_terms):
        if g_total is None and g_terms is None:
            return None, None, None, None
        v, lab, sid, coef = ctx.saved_tensors
        gt = g_total.float().reshape(1).contiguous() if g_total is not None else None
        gs = g_terms.float().contiguous() if g_terms is not None else None
        grad = torch.empty_like(v)
        d = _act_desc(v, lab, sid, *ctx.WK, ctx.cfg)
        _lib.check(_lib.load().spx_actloss_backward(C.byref(d), _lib.ptr(coef), _lib.ptr(gt), _lib.ptr(gs), _lib.ptr(grad), _lib.stream_ptr()))
        return grad, None, None, None


class ActivationRegularizers(_SlotTable, nn.Module):
    """The activation-side terms of the training objective (segmentation/model/loss.py:149-348; module_multiscale.py:170-175,
    module_multiscale_group_train.py:189-190) in one pipeline: ``forward(prototype_activations, target_labels)`` returns
    ``(total, terms)`` with terms = [spatial entropy, sample entropy, norm] (fp32 [3], for logging without a sync) and total =
    ent_spat * terms[0] + ent_sampl * terms[1] + norm * terms[2].  The analogue of ``GroupRegularizers`` for the terms that read
    the prototype activations of the labelled pixels; ``EntropySpatLoss``, ``EntropySamplLoss`` and ``NormLoss`` are this class
    with one term.

    ``prototype_activations`` is the [M, P] / [B, H*W, P] activation tensor (its class-gathered entries are taken with torch), or
    the ``ClassDistances`` of ``forward_from_conv_features(..., target_labels=...)``: the activation (``activation`` = "log":
    log((d+1)/(d+epsilon)), or "linear": -d) is then applied inside the kernels and the gradient reaches the distances, so
    neither the P-wide map nor an activation plane crosses HBM.  Labels: 0 = void, 1..K = class, anything else no class.

    Divergence from the reference, sample entropy: a (class, scale) with fewer than two prototypes is skipped.  The reference
    divides by ln 1 = 0 there (NaN for one prototype) and raises from ``torch.stack([])`` for none.  A term without any segment
    is a device scalar 0 (the reference returns a CPU tensor).  GPU fp32 only, at most 16 prototypes per class: anything else
    raises ``SpxError``; there is no other backend."""

    def __init__(self, prototype_class_identity: torch.Tensor, num_scales: int, scale_num_prototypes: Dict[int, Tuple[int, int]],
                 ent_spat: float = 0.0, ent_sampl: float = 0.0, norm: float = 0.0, norm_type: str = "l1", epsilon: float = 1e-4,
                 activation: str = "log") -> None:
        super().__init__()
        self._setup(prototype_class_identity, num_scales, scale_num_prototypes, ACT_SPAT | ACT_SAMPL | ACT_NORM,
                    (ent_spat, ent_sampl, norm), norm_type, epsilon, activation)

    def _setup(self, ident, num_scales, scale_num_prototypes, terms, weights, norm_type, epsilon, activation) -> None:
        if norm_type not in _NORM_TYPES:
            raise ValueError(f"norm_type must be 'l1' or 'linf', got {norm_type!r}")
        if activation not in _ACT_MODES:
            raise ValueError(f"activation must be 'log' or 'linear', got {activation!r}")
        self.prototype_class_identity = ident
        self.num_scales = num_scales
        self.scale_num_prototypes = scale_num_prototypes
        self.norm_type = norm_type
        self.epsilon = epsilon
        self.activation = activation
        self._terms, self._weights = int(terms), tuple(float(w) for w in weights)

    def _tables_on(self, table: torch.Tensor, dev):
        """(table on ``dev``, its slot-scale table on ``dev``), cached per table, scale ranges and device: host work with a
        read-back, done once.  A few entries, so that one module can serve the model's table (a ``ClassDistances``) and its
        own (an activation tensor) in turn."""
        scales = tuple((int(s), tuple(int(x) for x in self.scale_num_prototypes[s])) for s in range(int(self.num_scales)))
        build = lambda: (table.to(dev), slot_scale_table(table, self.num_scales, self.scale_num_prototypes).to(dev))
        return cached(self, "_act_tables_cache", (table,), (scales, str(dev)), build, ways=4)

    def _run(self, prototype_activations, target_labels: torch.Tensor):
        if isinstance(prototype_activations, ClassDistances):                           # the activation is applied in the kernels
            table, sid = self._tables_on(prototype_activations.table, prototype_activations.values.device)
            g, mode = _gathered.from_class_distances(prototype_activations, target_labels, table), _ACT_MODES[self.activation]
        else:
            table, sid = self._tables_on(self._slot_table(), prototype_activations.device)
            g, mode = _gathered.from_activations(prototype_activations, target_labels, table), 0
        _gathered.check_domain(g.planes, table.shape[0], "activation losses")
        cfg = {"mode": mode, "terms": self._terms, "norm_type": _NORM_TYPES[self.norm_type], "epsilon": float(self.epsilon),
               "weights": self._weights}
        total, terms = _ActLossFn.apply(g.planes, g, sid, cfg)
        if g.poison is not None:                                                        # NaN when the planes were gathered under other classes
            total, terms = total * g.poison, terms * g.poison
        return total, terms

    def forward(self, prototype_activations: Union[torch.Tensor, ClassDistances], target_labels: torch.Tensor):
        return self._run(prototype_activations, target_labels)


class _OneActTerm(ActivationRegularizers):
    def forward(self, prototype_activations: Union[torch.Tensor, ClassDistances], target_labels: torch.Tensor) -> torch.Tensor:
        return self._run(prototype_activations, target_labels)[0]       # total = 1 * term


class EntropySpatLoss(_OneActTerm):
    """Drop-in for segmentation/model/loss.py:149-211 on the GPU kernels (see ``ActivationRegularizers``); ``epsilon`` and
    ``activation`` are used only when a ``ClassDistances`` is passed."""

    def __init__(self, prototype_class_identity: torch.Tensor, *, epsilon: float = 1e-4, activation: str = "log") -> None:
        nn.Module.__init__(self)
        self._setup(prototype_class_identity, 0, {}, ACT_SPAT, (1.0, 0.0, 0.0), "l1", epsilon, activation)


class EntropySamplLoss(_OneActTerm):
    """Drop-in for segmentation/model/loss.py:214-284 on the GPU kernels.  Divergence: a (class, scale) with fewer than two
    prototypes is skipped (the reference is NaN for one and raises for none); see ``ActivationRegularizers``."""

    def __init__(self, prototype_class_identity: torch.Tensor, num_scales: int, scale_num_prototypes: Dict[int, Tuple[int, int]], *,
                 epsilon: float = 1e-4, activation: str = "log") -> None:
        nn.Module.__init__(self)
        self._setup(prototype_class_identity, num_scales, scale_num_prototypes, ACT_SAMPL, (0.0, 1.0, 0.0), "l1", epsilon, activation)


class NormLoss(_OneActTerm):
    """Drop-in for segmentation/model/loss.py:287-348 on the GPU kernels: ``norm_type`` "l1" or "linf" (anything else raises
    ``ValueError`` here; the reference fails in forward); the linf gradient is shared evenly by the pixels at the maximum."""

    def __init__(self, prototype_class_identity: torch.Tensor, norm_type: str, *, epsilon: float = 1e-4, activation: str = "log") -> None:
        nn.Module.__init__(self)
        self._setup(prototype_class_identity, 0, {}, ACT_NORM, (0.0, 0.0, 1.0), norm_type, epsilon, activation)
