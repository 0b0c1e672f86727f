"""Failure cases on the GPU (segmentation/analysis/failure_cases.py) and the label maps a benchmark server takes
(segmentation/eval_test.py:99-111): which (image, class) pairs a model gets wrong, what it mistook them for, and the heat maps
that show why, as uint8 arrays.

Definitions.  ``logits`` fp32 ``[N, h, w, K]`` (any strides, ``1 <= K <= 256``), labels ``[N, H, W]`` (uint8, int32 or int64;
0 = void, k + 1 = class k).

* Label map.  ``k*`` is the first argmax over the classes of the bilinear (``align_corners=False``) upsample of the logits to
  ``H x W``, with the bits of ``upsample_argext(..., largest=True)``.  ``pred`` uint8 ``[N, H, W]`` holds ``id_map[k*]``, or
  ``k*`` without a map: one byte per pixel, every byte written exactly once, packed into dwords.
* Per-image confusion.  ``conf`` int64 ``[N, K+1, K]``: ``conf[n, r, k*] += 1`` per pixel with ``label != 0``, ``r = label - 1``
  for ``1 <= label <= K``, else ``K``: the rule of ``SegmentationMetrics``, per image.  It is added to, not overwritten.
* Failure table of image ``n`` and class ``k``: present when ``sum_j conf[n, k, j] > 0``; ``I = conf[n, k, k]``;
  ``U = sum_j conf[n, k, j] + sum_{r <= K} conf[n, r, k] - I`` (the reference's ``(pr | gt) & (ann != 0)``);
  ``iou = I / U`` in float64; ``fail = iou < threshold`` (strict); ``miss`` = the argmax over ``j != k`` of ``conf[n, k, j]``,
  the lowest ``j`` among equal counts, -1 when all are zero.  A class that is not present has ``iou = NaN``, ``miss = -1``,
  ``fail = 0``.  The reference leaves two things open: ``Counter.most_common`` breaks ties by first appearance in raster order
  (here: the lowest class), and a failing class without a misprediction raises ``IndexError`` (here: ``miss = -1`` and the case
  is reported without maps).
* Paired heat maps (failure_cases.py:188-420).  This is NOT the arithmetic of ``ExplanationMaps``: the slots of the failing class
  ``a`` and of the class ``miss`` are both drawn over the pixels of ``a``; the range is shared per group index between the two
  classes; and the divisor is the maximum, not the width of the range.  A row ``(n, c, a, q)`` is plane ``c`` of image ``n``
  masked with class ``a`` and normalised by range slot ``q``: ``m = [label == a + 1] ? u[n, c] : 0`` with ``u`` the cubic
  upsample every map pass shares; ``lo_q`` / ``hi_q`` the minimum / maximum of ``m`` over all pixels of all rows naming ``q``;
  ``x = (m - lo_q) / hi_q`` in fp32, each operation rounded on its own; ``heat = (uint8) trunc(255.0f * x)``.  Where the
  reference's ``np.uint8`` conversion is undefined: ``255 x >= 256`` (only when ``lo_q < 0``) gives 255, and a slot with
  ``hi_q <= 0`` gives all-zero rows.  Outputs ``heat`` uint8 ``[R, H, W]`` and ``ranges`` fp32 ``[Q, 2]``.

One launch (``spx_predict_accumulate``) interpolates, reduces, writes the bytes and counts; ``spx_failure_table`` is one small
launch over the counters; ``spx_paired_range`` / ``spx_paired_heat`` recompute the pixels and store packed bytes.  Nothing here
waits for the device except ``FailureCases.rows_for`` and ``FailureCases.compute``, which say so.

Not built: PNG files, colour maps and overlays; data-set id tables (``id_map`` is an argument); images of different sizes in one
batch; the tables under a sharded run.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import torch

from . import _lib, _maps
from ._lib import SpxError
from ._maps import LABEL_BYTES, MAX_MAP_ROWS as MAX_ROWS, bad_row, byte_output as _output, host_rows, strides, upload as _upload

MAX_CLASSES = 256                # a prediction is one byte


def predict_label_maps(logits: torch.Tensor, size: Optional[Tuple[int, int]] = None, *, labels: Optional[torch.Tensor] = None,
                       id_map: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                       conf: Optional[torch.Tensor] = None, want_pred: bool = True):
    """``pred`` uint8 [N, H, W] without ``labels``; ``(pred, conf)`` with them, ``conf`` int64 [N, K+1, K] (module header).

    ``logits``: fp32 [N, h, w, K], read through its strides.  ``size`` = (H, W); with ``labels`` [N, H, W] it may be left out
    (given, it must be the labels' size).  ``id_map``: uint8 [K] on the device.  ``out``: a contiguous uint8 [N, H, W] tensor of
    any alignment to write ``pred`` into.  ``conf``: an int64 [N, K+1, K] tensor to ADD to (default: fresh zeros).
    ``want_pred=False`` (with ``labels``) counts only and returns ``(None, conf)``.  Enqueues one launch on the current stream;
    never synchronises."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 4 or logits.dtype != torch.float32:
        raise SpxError("logits must be fp32 [N, h, w, K]")
    N, h, w, K = (int(v) for v in logits.shape)
    if K < 1 or K > MAX_CLASSES:
        raise SpxError(f"{K} classes: a predicted label is one byte (1 <= K <= {MAX_CLASSES})")
    if labels is not None:
        H, W = _maps.label_map(labels, N, "logits")
        if size is not None and (int(size[0]), int(size[1])) != (H, W):
            raise SpxError(f"size {tuple(size)} is not the labels' {(H, W)}")
    elif size is None:
        raise SpxError("pass size=(H, W) or labels")
    else:
        H, W = int(size[0]), int(size[1])
        if H < 1 or W < 1:
            raise SpxError(f"size must be positive (got {(H, W)})")
        if conf is not None or not want_pred:
            raise SpxError("the confusion counters need labels")
    if id_map is not None and (not isinstance(id_map, torch.Tensor) or id_map.dtype != torch.uint8 or tuple(id_map.shape) != (K,)):
        raise SpxError(f"id_map must be uint8 [{K}]")
    if conf is not None and (conf.dtype != torch.int64 or tuple(conf.shape) != (N, K + 1, K) or not conf.is_contiguous()):
        raise SpxError(f"conf must be a contiguous int64 [{N}, {K + 1}, {K}] tensor")
    lg = logits.detach()
    _maps.on_device(((lg, "logits"), (labels, "labels"), (id_map, "id_map"), (conf, "conf")), lg.device, "logits")
    lib = _lib.load()
    pred = _output(out, (N, H, W), lg.device) if want_pred else None
    lab = None
    if labels is not None:
        lab = labels.detach().contiguous()
        if conf is None:
            conf = torch.zeros(N, K + 1, K, dtype=torch.int64, device=lg.device)
    idm = None if id_map is None else id_map.detach().contiguous()
    _lib.check(lib.spx_predict_accumulate(lg.data_ptr(), strides(lg, (0, 3, 1, 2)), _lib.ptr(lab), LABEL_BYTES[lab.dtype] if lab is not None else 0,
                                          _lib.ptr(idm), N, K, h, w, H, W, None if pred is None else pred.data_ptr(), _lib.ptr(conf),
                                          _lib.stream_ptr()))
    return pred if labels is None else (pred, conf)


def failure_table(conf: torch.Tensor, threshold: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(``iou`` f64 [N, K], ``miss`` int32 [N, K], ``fail`` uint8 [N, K]) of the per-image confusion ``conf`` int64 [N, K+1, K]
    on the device, as the module's header defines them.  One small launch, no host read; never synchronises."""
    if not isinstance(conf, torch.Tensor) or conf.dtype != torch.int64 or conf.dim() != 3 or conf.shape[1] != conf.shape[2] + 1 \
            or conf.shape[0] < 1 or conf.shape[2] < 1:
        raise SpxError("conf must be int64 [N, K+1, K]")
    threshold = float(threshold)
    if threshold != threshold:
        raise SpxError("the threshold is NaN")
    _lib.require_gpu(conf, "conf")
    c = conf.detach().contiguous()
    N, K = int(c.shape[0]), int(c.shape[2])
    iou = torch.empty(N, K, dtype=torch.float64, device=c.device)
    miss = torch.empty(N, K, dtype=torch.int32, device=c.device)
    fail = torch.empty(N, K, dtype=torch.uint8, device=c.device)
    _lib.check(_lib.load().spx_failure_table(c.data_ptr(), N, K, threshold, iou.data_ptr(), miss.data_ptr(), fail.data_ptr(),
                                             _lib.stream_ptr()))
    return iou, miss, fail


def paired_heat_maps(activations: torch.Tensor, labels: torch.Tensor, rows, num_ranges: int, grid: Optional[Tuple[int, int]] = None,
                     *, out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(heat uint8 [R, H, W], ranges fp32 [Q, 2] = (lo, hi)) as the module's header defines them.

    ``activations``: fp32 [N, C, h, w] with any strides, or pixel-major [M, C] with ``grid`` = (h, w).  ``labels``: [N, H, W]
    uint8 / int32 / int64 on the device.  ``rows``: integer [R, 4] = (n, c, a, q) in host memory, ``Q = num_ranges``; before
    anything is launched every field is checked, every ``q`` in ``0 .. Q-1`` must be named, and rows sharing a ``q`` must share
    ``n`` and ``a``.  ``out``: a contiguous uint8 [R, H, W] tensor of any alignment.  Never synchronises."""
    planes = _maps.planes(activations, grid, "activations")
    N, C, h, w = (int(v) for v in planes.shape)
    H, W = _maps.label_map(labels, N, "activations")
    rows = host_rows(rows, 4, "(n, c, a, q)")
    R, Q = int(rows.shape[0]), int(num_ranges)
    if R > MAX_ROWS:
        raise SpxError(f"{R} rows (at most {MAX_ROWS} in one call: the rows of a range slot go through one launch)")
    n, c, a, q = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
    if Q < 1:
        raise SpxError(f"num_ranges must be >= 1 (got {Q})")
    bad_row(rows, (n < 0) | (n >= N) | (c < 0) | (c >= C) | (a < 0) | (a >= 2 ** 31 - 1) | (q < 0) | (q >= Q), f"outside N={N}, C={C}, Q={Q}")
    used = torch.zeros(Q, dtype=torch.bool).index_fill_(0, q, True)
    if not bool(used.all()):
        raise SpxError(f"no row names range slot {int((~used).nonzero()[0])} of {Q}")
    first = torch.full((Q,), R, dtype=torch.int64).scatter_reduce_(0, q, torch.arange(R), "amin")[q]
    bad_row(rows, (n != n[first]) | (a != a[first]), "shares its range slot with a row of another image or class")
    lab = _maps.device_labels(planes, labels)
    lib = _lib.load()
    heat = _output(out, (R, H, W), planes.device)
    ranges = torch.empty(Q, 2, dtype=torch.float32, device=planes.device)
    host = rows.to(torch.int32).contiguous()
    dev = _upload(host, planes.device)
    keys = torch.empty(2 * Q, dtype=torch.int32, device=planes.device)
    common = (planes.data_ptr(), strides(planes), lab.data_ptr(), LABEL_BYTES[lab.dtype], dev.data_ptr(), host.data_ptr(), R, Q, N, C, h, w,
              H, W, keys.data_ptr())
    stream = _lib.stream_ptr()
    _lib.check(lib.spx_paired_range(*common, stream))
    _lib.check(lib.spx_paired_heat(*common, heat.data_ptr(), ranges.data_ptr(), stream))
    return heat, ranges


class BatchFailures(NamedTuple):
    """What ``FailureCases.update`` returns, all on the device."""

    pred: torch.Tensor            # uint8 [N, H, W]
    conf: torch.Tensor            # int64 [N, K+1, K]
    iou: torch.Tensor             # float64 [N, K]
    miss: torch.Tensor            # int32 [N, K]
    fail: torch.Tensor            # uint8 [N, K]


@dataclass
class FailureReport:
    """What ``FailureCases.compute`` returns, on the host.  One row per failing (image, class) that the ``ignore_miss`` rule
    keeps, in ascending (image, class) order; ``miss`` is -1 for a failing class without a misprediction."""

    image: torch.Tensor           # int64 [F]: index among the images seen so far
    cls: torch.Tensor             # int64 [F]
    iou: torch.Tensor             # float64 [F]
    miss: torch.Tensor            # int64 [F]
    image_confusion: torch.Tensor  # int64 [N, K+1, K]
    confusion: torch.Tensor       # int64 [K+1, K]: the sum over the images, what SegmentationMetrics counts on the same batches


class FailureCases:
    """The failure cases of one model.

        fc = FailureCases.for_prototypes(ppnet, threshold=0.5)      # or .for_groups(ppnet)
        logits, distances = ppnet(img)
        b = fc.update(logits, ann)                                  # BatchFailures on the device; no synchronisation
        cases, rows = fc.rows_for(b)                                # the ONE host synchronisation
        heat, ranges = fc.heat_maps(rows, labels=ann, distances=distances)
        report = fc.compute()                                       # per image seen so far; one copy
    """

    def __init__(self, num_classes: int, slot_table, threshold: float, ignore_miss: Optional[int] = None, shared_ranges: bool = False):
        self.num_classes = K = int(num_classes)
        if K < 1 or K > MAX_CLASSES:
            raise SpxError(f"{K} classes: a predicted label is one byte (1 <= K <= {MAX_CLASSES})")
        self.slot_table = _maps.slot_table(slot_table)
        if self.slot_table.shape[0] != K:
            raise SpxError(f"slot_table must be [{K}, J] with J >= 1")
        self.threshold = float(threshold)
        if self.threshold != self.threshold:
            raise SpxError("the threshold is NaN")
        self.ignore_miss = None if ignore_miss is None else int(ignore_miss)
        self.shared_ranges = bool(shared_ranges)              # one range per (case, slot index), shared by the two classes
        self._similarity = None
        self._group_sizes = None
        self._conf: List[torch.Tensor] = []

    @classmethod
    def for_prototypes(cls, ppnet, threshold: float = 0.5, ignore_miss: Optional[int] = None) -> "FailureCases":
        """Slots = the prototypes of each class; one range per plane (``proto_max[p]``, failure_cases.py:338-360).  ``heat_maps``
        then also takes ``distances=`` and applies the model's ``distance_2_similarity`` on the latent grid first.
        ``ignore_miss``: the Pascal rule of failure_cases.py:155, a case whose ``miss`` equals it is dropped."""
        from .loss import class_slot_table

        fc = cls(ppnet.num_classes, class_slot_table(ppnet.prototype_class_identity), threshold, ignore_miss)
        fc._similarity = ppnet.distance_2_similarity
        return fc

    @classmethod
    def for_groups(cls, ppnet, threshold: float = 0.5, ignore_miss: Optional[int] = None) -> "FailureCases":
        """Slots = the groups of each class, as ``ExplanationMaps.for_groups`` numbers them; one range per (case, group index),
        shared by the two classes (``group_max[i]``, failure_cases.py:246-271)."""
        table, sizes = _maps.group_slot_table(ppnet)
        fc = cls(ppnet.num_classes, table, threshold, ignore_miss, shared_ranges=True)
        fc._group_sizes = sizes
        return fc

    def reset(self) -> None:
        self._conf = []

    def update(self, logits: torch.Tensor, labels: torch.Tensor, id_map: Optional[torch.Tensor] = None) -> BatchFailures:
        """Predict and count one batch (``logits`` [N, h, w, K], ``labels`` [N, H, W]) and keep a private copy of its per-image
        counters for ``compute``: (K+1) K int64 per image seen (180 KB at K = 150) stay on the device until ``reset``, so the
        memory grows with the validation set.  The returned tensors are the caller's to change.  Two launches and one small
        copy on the current stream; never synchronises."""
        if not isinstance(logits, torch.Tensor) or logits.dim() != 4 or logits.shape[3] != self.num_classes:
            raise SpxError(f"logits must be [N, h, w, {self.num_classes}]")
        pred, conf = predict_label_maps(logits, labels=labels, id_map=id_map)
        iou, miss, fail = failure_table(conf, self.threshold)
        self._conf.append(conf.clone())
        return BatchFailures(pred, conf, iou, miss, fail)

    def _kept(self, fail: torch.Tensor, miss: torch.Tensor) -> torch.Tensor:
        keep = fail.bool()
        if self.ignore_miss is not None:
            keep &= miss != self.ignore_miss
        return keep

    def rows_for(self, batch: BatchFailures) -> Tuple[torch.Tensor, torch.Tensor]:
        """(cases int64 [F, 3] = (n, a, miss), rows int64 [R, 4] = (n, c, a, q)), host tensors, ``n`` counted inside the batch.
        ``cases``: the failing (image, class) pairs with a misprediction that ``ignore_miss`` keeps, in ascending (n, a) order,
        the reference's order of visits.  ``rows``: per case the slots of ``a``, then the slots of ``miss``, what
        ``paired_heat_maps`` takes with ``num_ranges = rows[:, 3].max() + 1``.  ONE host synchronisation (one copy)."""
        both = torch.stack([batch.fail.to(torch.int32), batch.miss]).cpu()          # the synchronisation
        fail, miss = both[0], both[1].to(torch.int64)
        keep = self._kept(fail, miss) & (miss >= 0)
        where = keep.nonzero()
        cases = torch.cat([where, miss[keep][:, None]], dim=1)
        table = self.slot_table.tolist()
        rows, slots = [], {}
        for i, (n, a, m) in enumerate(cases.tolist()):
            for k in (a, m):
                for j, c in enumerate(table[k]):
                    if c >= 0:
                        q = slots.setdefault((i, j) if self.shared_ranges else (i, c), len(slots))
                        rows.append((n, c, a, q))
        return cases, torch.tensor(rows, dtype=torch.int64).reshape(-1, 4)

    def heat_maps(self, rows, activations: Union[torch.Tensor, Sequence[torch.Tensor], None] = None,
                  labels: Optional[torch.Tensor] = None, *, distances: Optional[torch.Tensor] = None,
                  grid: Optional[Tuple[int, int]] = None, out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``paired_heat_maps`` of the rows ``rows_for`` returned.  The inputs are those of ``ExplanationMaps.heat_maps``:
        activations ([N, C, h, w], pixel-major [M, C] with ``grid``, or - ``for_groups`` - the list ``compute_group`` returns) or
        ``distances=`` (``for_prototypes``).  Never synchronises."""
        if labels is None:
            raise SpxError("labels are required")
        rows = host_rows(rows, 4, "(n, c, a, q)")
        planes = _maps.input_planes(activations, distances, grid, self._similarity, self._group_sizes, "FailureCases")
        return paired_heat_maps(planes, labels, rows, int(rows[:, 3].max()) + 1, out=out)

    def compute(self) -> FailureReport:
        """The failing (image, class) pairs of every image seen so far, the per-image confusion and its sum.  One launch and
        one device-to-host copy."""
        if not self._conf:
            raise SpxError("no batch has been counted")
        conf = torch.cat(self._conf)
        iou, miss, fail = failure_table(conf, self.threshold)
        N, K = int(conf.shape[0]), self.num_classes
        host = torch.cat([conf.reshape(-1), iou.view(torch.int64).reshape(-1), miss.to(torch.int64).reshape(-1),
                          fail.to(torch.int64).reshape(-1)]).cpu()
        n0 = N * (K + 1) * K
        conf = host[:n0].view(N, K + 1, K)
        iou = host[n0:n0 + N * K].view(torch.float64).view(N, K)
        miss = host[n0 + N * K:n0 + 2 * N * K].view(N, K)
        keep = self._kept(host[n0 + 2 * N * K:].view(N, K), miss)
        where = keep.nonzero()
        return FailureReport(where[:, 0], where[:, 1], iou[keep], miss[keep], conf, conf.sum(0))
