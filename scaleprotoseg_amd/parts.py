"""Part consistency and stability on the GPU (segmentation/analysis/metrics/consistency.py, stability.py; the paper's two
quantitative interpretability scores): which prototypes or groups of a class fire at the centroids of the annotated object parts.

Definition (the contract; tests/consistency_restatement.py restates it in NumPy).

Inputs.  Activation planes ``a[n, c, y, x]`` (fp32, latent grid ``h x w``; [N, C, h, w] with any strides, or pixel-major [M, C] with
``grid``), ``labels [N, H, W]`` (0 = void, k + 1 = class k, anything else no class; uint8 / int32 / int64), ``parts [N, H, W]`` of
the same integer types (``t`` in 1..M = part t, values <= 0 no part, values above ``M = max_parts`` no part either: the reference
raises ``IndexError`` there), a slot table ``[K, J]`` of the ``class_slot_table`` kind (-1 = no slot), optionally ``include`` (the
bank indices kept; ``non_zero_proto(group_net)`` reproduces the reference's ``proto_filter``) and ``skip_classes``.

Per image ``n`` and class ``k`` whose label occurs in ``labels[n]`` and which is not skipped:

1. ``B_t = (labels == k + 1) & (parts == t)`` for t in 1..M.  If every ``B_t`` is empty the pair (n, k) produces nothing
   (consistency.py:237-238): its row is not *valid*.
2. Centroids of part t: one per 8-connected component of ``B_t``, ``(sum X / count, sum Y / count)`` in float64 from integer sums,
   and one more for the complement of ``B_t`` within the image: ``cv2.connectedComponentsWithStats`` returns its label-0 row and
   consistency.py:264 walks all rows; that is reproduced, not "fixed".  Each coordinate is rounded half to even (``np.round``).  If
   ``B_t`` is the whole image the complement is empty and contributes no centroid (the reference has a NaN centroid there and is
   undefined).
3. For each slot j of the class with channel c, restricted to ``include``:
   ``u[Y, X] = a[n, c, sy(Y), sx(X)] * [labels[n, Y, X] == k + 1]`` with the source index OpenCV's ``INTER_NEAREST`` computes,
   ``sx(X) = min(floor(X * (1.0 / (W / w))), w - 1)`` in float64 with the operations in exactly that order, ``sy`` alike with
   ``H / h``.  ``cv2`` is not needed and was never run against this rule.
4. Threshold T.  The reference's ``quantile_map`` (``segmentation.analysis.equivariance``) is not part of the reference checkout, so
   the rule is a parameter and neither quantile reading is claimed to be upstream's:
   ``threshold="image"``: ``np.quantile`` (linear) of all ``H W`` values of u, the zeros outside the class included;
   ``threshold="nonzero"``: ``np.quantile`` of the non-zero values of u, ``+inf`` when there are none;
   ``thresholds=`` fp32 [C]: explicit per-channel values, the reference's own ``quantiles.json`` branch (consistency.py:258-259).
   Rank and interpolation are those of ``overlap._rank`` and numpy's fp32 ``_lerp``, as in ``high_activation_threshold``.
5. ``present[t] = 1`` if ``u[y, x] > T`` (strict) at any centroid of part t, else 0.  Parts with an empty ``B_t``, and column 0, are
   *absent*: NaN for consistency (consistency.py:242), 0 for stability (stability.py:242).

One batch gives a dense uint8 table ``[N, K, J, M + 1]`` with the values 0, 1 and 255 (absent; every entry of a row that is not
valid and of a slot that does not exist or is not included) and uint8 row-valid flags ``[N, K]``, both on the device, with no host
read.

Consistency (consistency.py:165-178, restated): per (class, slot) over the images whose row is valid, per part,
``mean = ones / times_present`` (NaN for a part that was always absent), ``flag = mean > consistency_threshold`` (NaN compares
false), ``is_consistent = max over the parts``, ``score`` = the mean of ``is_consistent`` over the (class, slot) pairs with at least
one valid row.  The running state is int64 counters; ``compute`` finalises in float64 on the host after one copy.

Stability (stability.py:169-175): two tables from the same labels and parts, clean and perturbed activations, absent = 0; a valid
row is stable when all ``M + 1`` entries agree; ``score = stable rows / valid rows``.  Producing the noisy activations
(``img + sigma * randn`` and a second forward) is the caller's ordinary torch code.  stability.py's own ``part_intersect`` cannot
run as written: its call sites pass ``proto_ids, std_dev`` into the parameters ``noise, filter_class_ids`` and its body names an
undefined ``filter_proto_ids``; it differs from consistency's function only in the initial list value (0 for NaN) and the noise.

Kernels (csrc/spx_parts.hip): ``spx_part_components`` labels all classes and parts of a batch in one union-find pass over the
joint key (class, part); ``spx_part_thresholds`` counts the class pixels per latent cell and selects over the ``h w`` cell values
with those multiplicities, so the ``[H, W]`` plane is never formed; ``spx_part_presence`` tests every slot at every centroid.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple, Union

import torch

from . import _lib, _maps
from ._lib import SpxError
from ._maps import LABEL_BYTES, strides
from .overlap import _rank

ABSENT = 255
MAX_PARTS = 254
_MODES = {"image": 0, "nonzero": 1}


def _check_parts(max_parts) -> int:
    M = int(max_parts)
    if not 1 <= M <= MAX_PARTS:
        raise SpxError(f"max_parts must be in 1..{MAX_PARTS} (got {max_parts})")
    return M


def _check_maps(labels, parts, N: Optional[int], what: str) -> Tuple[int, int]:
    H, W = _maps.label_map(labels, N, what)
    if not isinstance(parts, torch.Tensor) or parts.dtype not in LABEL_BYTES or tuple(parts.shape) != tuple(labels.shape):
        got = f"{parts.dtype} {tuple(parts.shape)}" if isinstance(parts, torch.Tensor) else type(parts).__name__
        raise SpxError(f"parts must be uint8, int32 or int64 {tuple(labels.shape)} like the labels (got {got})")
    return H, W


def _mode(threshold: str) -> int:
    if threshold not in _MODES:
        raise SpxError(f"threshold must be 'image' or 'nonzero' (got {threshold!r})")
    return _MODES[threshold]


def _effective_table(slot_table, include, skip_classes) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(host int32 [K, J] with the slots outside ``include`` struck out, host uint8 [K] skip mask or None)."""
    table = _maps.slot_table(slot_table).clone()
    if include is not None:
        keep = torch.as_tensor(include).detach().cpu().to(torch.int64).flatten()
        table[~torch.isin(table.to(torch.int64), keep)] = -1
    skip = None
    ks = [int(k) for k in skip_classes]
    if ks:
        if min(ks) < 0 or max(ks) >= table.shape[0]:
            raise SpxError(f"skip_classes {ks} outside 0..{table.shape[0] - 1}")
        skip = torch.zeros(table.shape[0], dtype=torch.uint8)
        skip[ks] = 1
    return table, skip


@dataclass
class PartComponents:
    """What ``spx_part_components`` leaves on the device."""

    parent: torch.Tensor            # int32 [N, H, W]: the smallest pixel index Y * W + X of the pixel's component, -1 = no part
    count: torch.Tensor             # int32 [N, H, W]: the component's pixels at its root, 0 elsewhere
    sum_x: torch.Tensor             # int64 [N, H, W]: at the root
    sum_y: torch.Tensor             # int64 [N, H, W]
    totals: torch.Tensor            # int64 [N, K, M, 3] = (count, sum X, sum Y) of every B_t
    workspace: torch.Tensor         # the buffer the four maps are views of

    def table(self, labels: torch.Tensor, parts: torch.Tensor) -> list:
        """Host list of (n, key, count, sum X, sum Y), sorted; key = k * M + t - 1.  Reads the device."""
        M = self.totals.shape[2]
        n, y, x = self.count.nonzero(as_tuple=True)
        key = (labels[n, y, x].to(torch.int64) - 1) * M + parts[n, y, x].to(torch.int64) - 1
        rows = torch.stack([n, key, self.count[n, y, x].to(torch.int64), self.sum_x[n, y, x], self.sum_y[n, y, x]], 1)
        return sorted(tuple(r) for r in rows.cpu().tolist())


def _components(lib, lab: torch.Tensor, par: torch.Tensor, K: int, M: int) -> PartComponents:
    N, H, W = (int(v) for v in lab.shape)
    nbytes = lib.spx_part_components_workspace_bytes(N, H, W)
    if nbytes == 0:
        raise SpxError(lib.spx_last_error().decode("utf-8", "replace"))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=lab.device)
    totals = torch.empty(N, K, M, 3, dtype=torch.int64, device=lab.device)
    _lib.check(lib.spx_part_components(lab.data_ptr(), LABEL_BYTES[lab.dtype], par.data_ptr(), LABEL_BYTES[par.dtype], N, K, M, H, W,
                                       _lib.ptr(ws), _lib.ptr(totals), _lib.stream_ptr()))
    px = N * H * W
    sums = ws[:16 * px].view(torch.int64)
    words = ws[16 * px:].view(torch.int32)
    return PartComponents(words[:px].view(N, H, W), words[px:].view(N, H, W), sums[:px].view(N, H, W), sums[px:].view(N, H, W),
                          totals, ws)


def part_components(labels: torch.Tensor, parts: torch.Tensor, max_parts: int, num_classes: Optional[int] = None) -> PartComponents:
    """The 8-connected components of every ``B_t`` of every image, labelled in one pass over the joint key (class, part), with
    their pixel counts and integer coordinate sums, and the totals of every ``B_t``.  ``num_classes``: K; None reads the largest
    label from the device."""
    M = _check_parts(max_parts)
    _check_maps(labels, parts, None, "")
    _maps.on_device(((labels, "labels"), (parts, "parts")), labels.device if labels.is_cuda else parts.device, "labels")
    lib = _lib.load()
    K = max(1, int(labels.max())) if num_classes is None else int(num_classes)
    if K < 1:
        raise SpxError(f"num_classes must be positive (got {K})")
    return _components(lib, labels.detach().contiguous(), parts.detach().contiguous(), K, M)


class _Inputs:
    """The checked inputs of one batch: shape and type checks first, then the device."""

    def __init__(self, planes: torch.Tensor, labels, parts, table_host: torch.Tensor, device: Optional[torch.device], owner: str):
        self.N, self.C, self.h, self.w = (int(v) for v in planes.shape)
        if parts is None:
            self.H, self.W = _maps.label_map(labels, self.N, "activations")
        else:
            self.H, self.W = _check_maps(labels, parts, self.N, "activations")
        self.K, self.J = (int(v) for v in table_host.shape)
        _lib.require_gpu(planes, "activations")
        dev = planes.device if device is None else device
        _maps.on_device(((planes, "activations"), (labels, "labels"), (parts, "parts")), dev, owner)
        self.planes, self.device = planes, dev
        self.labels = labels.detach().contiguous()
        self.parts = None if parts is None else parts.detach().contiguous()


def _thresholds(lib, x: _Inputs, table: torch.Tensor, skip: Optional[torch.Tensor], q: float, mode: int) -> torch.Tensor:
    nbytes = lib.spx_part_thresholds_workspace_bytes(x.N, x.K, x.h, x.w)
    if nbytes == 0:
        raise SpxError(lib.spx_last_error().decode("utf-8", "replace"))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    out = torch.empty(x.N, x.K, x.J, dtype=torch.float32, device=x.device)
    _lib.check(lib.spx_part_thresholds(x.planes.data_ptr(), strides(x.planes), x.labels.data_ptr(), LABEL_BYTES[x.labels.dtype],
                                       _lib.ptr(table), _lib.ptr(skip), x.N, x.C, x.K, x.J, x.h, x.w, x.H, x.W, float(q), mode,
                                       _lib.ptr(ws), _lib.ptr(out), _lib.stream_ptr()))
    return out


def _explicit(x: _Inputs, table: torch.Tensor, thresholds: torch.Tensor) -> torch.Tensor:
    """T[n, k, j] = thresholds[channel of (k, j)], NaN without a channel."""
    per = thresholds.to(x.device)[table.clamp(min=0).to(torch.int64)]
    per = torch.where(table >= 0, per, torch.full_like(per, float("nan")))
    return per.unsqueeze(0).expand(x.N, x.K, x.J).contiguous()


def _check_explicit(thresholds, C: int) -> Optional[torch.Tensor]:
    if thresholds is None:
        return None
    if not isinstance(thresholds, torch.Tensor) or thresholds.dtype != torch.float32 or tuple(thresholds.shape) != (C,):
        got = f"{thresholds.dtype} {tuple(thresholds.shape)}" if isinstance(thresholds, torch.Tensor) else type(thresholds).__name__
        raise SpxError(f"thresholds must be fp32 [{C}], one per channel of the activations (got {got})")
    return thresholds.detach()


def _presence(lib, x: _Inputs, table: torch.Tensor, skip: Optional[torch.Tensor], M: int, comp: PartComponents,
              thr: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    out = torch.empty(x.N, x.K, x.J, M + 1, dtype=torch.uint8, device=x.device)
    valid = torch.empty(x.N, x.K, dtype=torch.uint8, device=x.device)
    _lib.check(lib.spx_part_presence(x.planes.data_ptr(), strides(x.planes), x.labels.data_ptr(), LABEL_BYTES[x.labels.dtype],
                                     x.parts.data_ptr(), LABEL_BYTES[x.parts.dtype], _lib.ptr(table), _lib.ptr(skip), _lib.ptr(thr),
                                     _lib.ptr(comp.workspace), _lib.ptr(comp.totals), x.N, x.C, x.K, x.J, M, x.h, x.w, x.H, x.W,
                                     _lib.ptr(out), _lib.ptr(valid), _lib.stream_ptr()))
    return out, valid


def part_thresholds(act: torch.Tensor, labels: torch.Tensor, slot_table, q: float = 0.8, threshold: str = "nonzero",
                    grid: Optional[Tuple[int, int]] = None, include=None, skip_classes: Sequence[int] = ()) -> torch.Tensor:
    """fp32 [N, K, J]: the threshold T of step 4 for every (image, class, slot); NaN for a slot that does not exist or is not
    included and for a skipped class, ``+inf`` in ``"nonzero"`` mode when the masked plane has no non-zero value."""
    mode = _mode(threshold)
    _rank(q, 2)
    planes = _maps.planes(act, grid, "activations")
    table_host, skip_host = _effective_table(slot_table, include, skip_classes)
    x = _Inputs(planes, labels, None, table_host, None, "activations")
    lib = _lib.load()
    table = _maps.upload(table_host, x.device)
    skip = None if skip_host is None else _maps.upload(skip_host, x.device)
    return _thresholds(lib, x, table, skip, q, mode)


def part_presence(act: torch.Tensor, labels: torch.Tensor, parts: torch.Tensor, slot_table, max_parts: int, q: float = 0.8,
                  threshold: str = "nonzero", thresholds: Optional[torch.Tensor] = None, grid: Optional[Tuple[int, int]] = None,
                  include=None, skip_classes: Sequence[int] = ()) -> Tuple[torch.Tensor, torch.Tensor]:
    """(table uint8 [N, K, J, M + 1] with 0 / 1 / 255 = absent, valid uint8 [N, K]) of one batch, on the device."""
    M = _check_parts(max_parts)
    mode = _mode(threshold)
    _rank(q, 2)
    planes = _maps.planes(act, grid, "activations")
    explicit = _check_explicit(thresholds, int(planes.shape[1]))
    table_host, skip_host = _effective_table(slot_table, include, skip_classes)
    x = _Inputs(planes, labels, parts, table_host, None, "activations")
    lib = _lib.load()
    table = _maps.upload(table_host, x.device)
    skip = None if skip_host is None else _maps.upload(skip_host, x.device)
    comp = _components(lib, x.labels, x.parts, x.K, M)
    thr = _explicit(x, table, explicit) if explicit is not None else _thresholds(lib, x, table, skip, q, mode)
    return _presence(lib, x, table, skip, M, comp, thr)


@dataclass
class PartConsistencyResult:
    """What consistency.py:165-178 reports, from the exact integer counters."""

    mean: torch.Tensor              # float64 [K, J, M + 1]: ones / times present; NaN for a part that was always absent
    is_consistent: torch.Tensor     # int64 [K, J]: max over the parts of mean > consistency_threshold; -1 for a pair without a row
    score: float                    # mean of is_consistent over the pairs with at least one valid row (NaN without any)
    ones: torch.Tensor              # int64 [K, J, M + 1]
    times_present: torch.Tensor     # int64 [K, J, M + 1]
    rows: torch.Tensor              # int64 [K, J]: valid rows of the pair


@dataclass
class PartStabilityResult:
    score: float                    # stable rows / valid rows (NaN without a valid row)
    stable_rows: int
    valid_rows: int


class _PartMetric:
    """What the two running metrics share: the slot table with ``include`` applied, the threshold rule, and a batch's tables."""

    def __init__(self, num_classes: int, slot_table, max_parts: int, device, q: float = 0.8, threshold: str = "nonzero",
                 thresholds: Optional[torch.Tensor] = None, include=None, skip_classes: Sequence[int] = ()):
        self.max_parts = _check_parts(max_parts)
        self.mode = _mode(threshold)
        _rank(q, 2)
        self.quantile = float(q)
        self.num_classes = K = int(num_classes)
        self.slot_table_host, skip_host = _effective_table(slot_table, include, skip_classes)
        if K < 1 or self.slot_table_host.shape[0] != K:
            raise SpxError(f"slot_table must be [{K}, J] with J >= 1")
        self.num_slots = int(self.slot_table_host.shape[1])
        self.num_channels = int(_maps.slot_table(slot_table).max().item()) + 1
        self.device = torch.device(device)
        _lib.require_gpu(self.device, type(self).__name__)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._explicit = thresholds
        self.slot_table = self.slot_table_host.to(self.device)
        self._skip = None if skip_host is None else skip_host.to(self.device)
        self._similarity = None
        self._group_sizes = None

    @classmethod
    def for_prototypes(cls, ppnet, max_parts: int, device=None, **kw):
        """Slots = the prototypes of each class (``prototype_class_identity``); inputs may then be ``distances``, to which the
        model's ``distance_2_similarity`` is applied on the latent grid first (consistency.py:244)."""
        from .loss import class_slot_table

        if device is None:
            device = ppnet.prototype_vectors.device
        m = cls(ppnet.num_classes, class_slot_table(ppnet.prototype_class_identity), max_parts, device, **kw)
        m.num_channels = int(ppnet.prototype_class_identity.shape[0])
        m._similarity = ppnet.distance_2_similarity
        return m

    @classmethod
    def for_groups(cls, ppnet, max_parts: int, device=None, **kw):
        """Slots = the groups of each class: class k owns the channels of ``compute_group(...)[k]`` in the concatenation of that
        list.  Inputs are the list or its concatenation ([M, U] with ``grid``, or [N, U, h, w])."""
        if device is None:
            device = ppnet.prototype_vectors.device
        table, sizes = _maps.group_slot_table(ppnet)
        m = cls(ppnet.num_classes, table, max_parts, device, **kw)
        m.num_channels = sum(sizes)
        m._group_sizes = sizes
        return m

    def _inputs(self, activations, distances, labels, parts, grid) -> _Inputs:
        if labels is None or parts is None:
            raise SpxError("labels and parts are required")
        planes = _maps.input_planes(activations, distances, grid, self._similarity, self._group_sizes, type(self).__name__)
        if planes.shape[1] < self.num_channels:
            raise SpxError(f"activations have {planes.shape[1]} channels, the slot table names channel {self.num_channels - 1}")
        return _Inputs(planes, labels, parts, self.slot_table_host, self.device, "counters")

    def _table(self, lib, x: _Inputs, comp: PartComponents) -> Tuple[torch.Tensor, torch.Tensor]:
        explicit = _check_explicit(self._explicit, x.C)
        thr = (_explicit(x, self.slot_table, explicit) if explicit is not None
               else _thresholds(lib, x, self.slot_table, self._skip, self.quantile, self.mode))
        return _presence(lib, x, self.slot_table, self._skip, self.max_parts, comp, thr)

    def all_reduce(self, group=None) -> None:
        """Sum the counters of every rank (dp._all_reduce_sum)."""
        from .dp import _all_reduce_sum

        _all_reduce_sum(self._buf, group)

    def reset(self) -> None:
        self._buf.zero_()


class PartConsistency(_PartMetric):
    """Running part-consistency counters on one GPU.

        m = PartConsistency.for_prototypes(ppnet, max_parts=5)
        for img, ann, part_ann in loader:
            logits, distances = ppnet(img)                          # distances [N, P, h, w]
            m.update(labels=ann, parts=part_ann, distances=distances)
        res = m.compute()                                           # res.score, res.mean, res.is_consistent

    The counters live in one int64 device buffer [ones K*J*(M+1) | times present K*J*(M+1) | rows K*J]; ``update`` never waits for
    the device, ``compute`` is one copy and ``all_reduce`` one collective."""

    def __init__(self, num_classes: int, slot_table, max_parts: int, device, consistency_threshold: float = 0.8, **kw):
        super().__init__(num_classes, slot_table, max_parts, device, **kw)
        self.consistency_threshold = float(consistency_threshold)
        K, J, M1 = self.num_classes, self.num_slots, self.max_parts + 1
        self._buf = torch.zeros(2 * K * J * M1 + K * J, dtype=torch.int64, device=self.device)

    def update(self, activations: Union[torch.Tensor, Sequence[torch.Tensor], None] = None, labels: Optional[torch.Tensor] = None,
               parts: Optional[torch.Tensor] = None, *, distances: Optional[torch.Tensor] = None,
               grid: Optional[Tuple[int, int]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Count one batch and return its (table, valid).  Enqueues work on the current stream only; never synchronises."""
        x = self._inputs(activations, distances, labels, parts, grid)
        lib = _lib.load()
        table, valid = self._table(lib, x, _components(lib, x.labels, x.parts, x.K, self.max_parts))
        _lib.check(lib.spx_part_fold_consistency(_lib.ptr(table), _lib.ptr(valid), _lib.ptr(self.slot_table), x.N, x.C, x.K, x.J,
                                                 self.max_parts, _lib.ptr(self._buf), _lib.stream_ptr()))
        return table, valid

    def compute(self) -> PartConsistencyResult:
        host = self._buf.cpu()
        K, J, M1 = self.num_classes, self.num_slots, self.max_parts + 1
        per = K * J * M1
        return finalize_consistency(host[:per].view(K, J, M1), host[per:2 * per].view(K, J, M1), host[2 * per:].view(K, J),
                                    self.consistency_threshold)


def finalize_consistency(ones: torch.Tensor, times: torch.Tensor, rows: torch.Tensor, threshold: float = 0.8) -> PartConsistencyResult:
    """Host-side float64 finalisation of the int64 counters."""
    ones, times, rows = ones.to(torch.int64).cpu(), times.to(torch.int64).cpu(), rows.to(torch.int64).cpu()
    mean = ones.to(torch.float64) / times.to(torch.float64)
    mean[times == 0] = float("nan")
    cons = (mean > threshold).to(torch.int64).max(dim=-1).values
    cons[rows == 0] = -1
    have = rows > 0
    score = cons[have].to(torch.float64).mean().item() if bool(have.any()) else float("nan")
    return PartConsistencyResult(mean, cons, score, ones, times, rows)


class PartStability(_PartMetric):
    """Running part-stability counters on one GPU: [stable rows, valid rows] int64.

        m = PartStability.for_prototypes(ppnet, max_parts=5)
        for img, ann, part_ann in loader:
            _, clean = ppnet(img)
            _, noisy = ppnet(img + sigma * torch.randn_like(img))
            m.update(labels=ann, parts=part_ann, clean_distances=clean, noisy_distances=noisy)
        res = m.compute()                                           # res.score"""

    def __init__(self, num_classes: int, slot_table, max_parts: int, device, **kw):
        super().__init__(num_classes, slot_table, max_parts, device, **kw)
        self._buf = torch.zeros(2, dtype=torch.int64, device=self.device)

    def update(self, labels: Optional[torch.Tensor] = None, parts: Optional[torch.Tensor] = None, clean=None, noisy=None, *,
               clean_distances: Optional[torch.Tensor] = None, noisy_distances: Optional[torch.Tensor] = None,
               grid: Optional[Tuple[int, int]] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Count one batch and return (clean table, noisy table, valid); ``clean`` / ``noisy`` as ``PartConsistency.update`` takes
        activations.  The components are labelled once for both.  Never synchronises."""
        a = self._inputs(clean, clean_distances, labels, parts, grid)
        b = self._inputs(noisy, noisy_distances, labels, parts, grid)
        if (a.N, a.C, a.h, a.w) != (b.N, b.C, b.h, b.w):
            raise SpxError(f"clean activations {tuple(a.planes.shape)} and noisy activations {tuple(b.planes.shape)} differ in shape")
        lib = _lib.load()
        comp = _components(lib, a.labels, a.parts, a.K, self.max_parts)
        ta, valid = self._table(lib, a, comp)
        tb, _ = self._table(lib, b, comp)
        _lib.check(lib.spx_part_fold_stability(_lib.ptr(ta), _lib.ptr(tb), _lib.ptr(valid), _lib.ptr(self.slot_table), a.N, a.C, a.K,
                                               a.J, self.max_parts, _lib.ptr(self._buf), _lib.stream_ptr()))
        return ta, tb, valid

    def compute(self) -> PartStabilityResult:
        stable, rows = (int(v) for v in self._buf.cpu().tolist())
        return PartStabilityResult(stable / rows if rows else float("nan"), stable, rows)
