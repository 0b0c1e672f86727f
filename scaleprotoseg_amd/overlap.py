"""Overlap of the high-activation regions of one class's prototypes or groups on the GPU
(segmentation/analysis/prototype_overlap.py:28-92, group_overlap.py:28-87; the paper's prototype / group mIoU).

Definition.  Activation planes ``a[n, c, y, x]`` (fp32, latent grid ``h x w``), labels ``[N, H, W]`` (0 = void, k + 1 =
class k, anything else belongs to no class), a slot table ``[K, J]`` (channel of (class, slot) or -1, the
``class_slot_table`` kind) and a quantile ``q``:

* ``u[n, c, Y, X]``: the plane upsampled to ``H x W`` as OpenCV ``INTER_CUBIC`` defines it, which is also
  ``F.interpolate(mode="bicubic", align_corners=False)``: source coordinate ``(X + 0.5) * w / W - 0.5``, four taps per axis
  with Keys' kernel at a = -0.75, tap indices clamped to the grid.  ``tests/overlap_restatement.py`` restates this rule in
  float64 and is the contract (``cv2`` itself was never run against it).
* ``T[n, c] = np.quantile(u[n, c].ravel(), q)``, the linear method: ``k = floor(q (HW - 1))`` and ``gamma`` = the fractional
  part, in float64 on the host; ``T`` = numpy's ``_lerp`` of the order statistics ``v[k]``, ``v[k + 1]`` in fp32.
* mask ``u > T`` (strict: a constant plane has an empty mask).
* For image ``n`` and each class ``k`` that occurs in ``labels[n]``: ``area[k, j] += |mask_j|``,
  ``inter[k, j, j'] += |mask_j & mask_j'|`` for every slot pair ``j < j'`` of the class, ``images[k] += 1``.
* ``class_iou[k] = sum inter / sum union`` over the class's pairs with ``union = area_j + area_j' - inter``, for the classes
  whose union is above 0; ``total`` the same over everything: the reference's ``final_mIoU`` entries, as fractions.

The reference resizes and sorts every map once per pair on the host.  Here ``spx_overlap_thresholds`` finds the exact
thresholds by a radix select that recomputes the upsampled values from the latent planes in every round, and
``spx_overlap_accumulate`` counts with ballots and integer atomics; the upsampled ``[C, H, W]`` tensor is never written.
``update`` never waits for the device; ``compute`` makes the one device-to-host copy and finalises in float64.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple, Union

import torch

from . import _lib, _maps
from ._lib import SpxError
from ._maps import LABEL_BYTES, dev_ptr, strides


def _rank(q: float, count: int) -> Tuple[int, float]:
    """(k, gamma) of numpy's linear quantile for ``count`` values: float64 on the host, gamma then rounded to fp32."""
    q = float(q)
    if not 0.0 < q < 1.0:
        raise SpxError(f"quantile must satisfy 0 < q < 1 (got {q})")
    virtual = q * (count - 1)
    k = int(math.floor(virtual))
    gamma = C.c_float(virtual - k).value
    if gamma >= 1.0:
        gamma = 1.0 - 2.0 ** -24
    return k, gamma


def _workspace(lib, N: int, Cn: int, K: int, device) -> torch.Tensor:
    nbytes = lib.spx_overlap_workspace_bytes(N, Cn, K)
    if nbytes == 0:
        raise SpxError(lib.spx_last_error().decode("utf-8", "replace"))
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _thresholds(lib, planes: torch.Tensor, size, q: float, workspace: torch.Tensor) -> torch.Tensor:
    N, Cn, h, w = planes.shape
    H, W = int(size[0]), int(size[1])
    if H < 1 or W < 1:
        raise SpxError(f"size must be positive (got {H} x {W})")
    k, gamma = _rank(q, H * W)
    out = torch.empty(N, Cn, dtype=torch.float32, device=planes.device)
    _lib.check(lib.spx_overlap_thresholds(dev_ptr(planes, "activations"), strides(planes), N, Cn, h, w, H, W, k, gamma,
                                          _lib.ptr(workspace), _lib.ptr(out), _lib.stream_ptr()))
    return out


def high_activation_threshold(activations: torch.Tensor, size, q: float = 0.95, grid: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """fp32 [N, C]: ``np.quantile`` at ``q`` of every plane of ``activations`` upsampled (cubic) to ``size`` = (H, W), the
    threshold of the reference's high-activation masks and push bounding boxes, without writing the upsampled planes.
    ``activations`` is [N, C, h, w] with any strides, or pixel-major [M, C] with ``grid`` = (h, w)."""
    lib = _lib.load()
    _rank(q, 2)
    planes = _maps.planes(activations, grid, "activations")
    dev_ptr(planes, "activations")
    N, Cn = int(planes.shape[0]), int(planes.shape[1])
    return _thresholds(lib, planes, size, q, _workspace(lib, N, Cn, 1, planes.device))


@dataclass
class OverlapResult:
    """What prototype_overlap.py:151-160 / group_overlap.py:149-158 report, from the exact integer counters."""

    class_iou: Dict[int, float]     # {k: sum inter / sum union over the class's slot pairs} for the classes with union > 0
    total: float                    # the same over every class (nan when no union is above 0)
    inter: torch.Tensor             # int64 [K, J, J], filled for j < j'
    area: torch.Tensor              # int64 [K, J]
    images: torch.Tensor            # int64 [K]: images in which the class occurred


def finalize(inter: torch.Tensor, area: torch.Tensor, images: torch.Tensor, slot_table: torch.Tensor) -> OverlapResult:
    """Host-side float64 finalisation of the int64 counters; ``slot_table`` [K, J] names the slots that exist (>= 0)."""
    inter, area, images = inter.to(torch.int64).cpu(), area.to(torch.int64).cpu(), images.to(torch.int64).cpu()
    K, J = area.shape
    valid = slot_table.cpu() >= 0
    pair = torch.triu(torch.ones(J, J, dtype=torch.bool), diagonal=1) & valid[:, :, None] & valid[:, None, :]
    union = (area[:, :, None] + area[:, None, :] - inter) * pair
    i_k = (inter * pair).sum((1, 2)).to(torch.float64)
    u_k = union.sum((1, 2)).to(torch.float64)
    class_iou = {k: i_k[k].item() / u_k[k].item() for k in range(K) if u_k[k].item() > 0}
    total = i_k.sum().item() / u_k.sum().item() if u_k.sum().item() > 0 else float("nan")
    return OverlapResult(class_iou, total, inter, area, images)


class ActivationOverlap:
    """Running overlap counters on one GPU.

        m = ActivationOverlap.for_prototypes(ppnet)
        for img, ann in loader:
            logits, distances = ppnet(img)                  # distances [N, P, h, w]
            m.update(labels=ann, distances=distances)       # ann [N, H, W]
        res = m.compute()                                   # res.class_iou, res.total

    All counters live in one int64 device buffer [inter K*J*J | area K*J | images K], so ``compute`` is one copy and
    ``all_reduce`` one collective."""

    def __init__(self, num_classes: int, slot_table: torch.Tensor, device, quantile: float = 0.95):
        self.device = torch.device(device)
        _lib.require_gpu(self.device, "ActivationOverlap")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.num_classes = K = int(num_classes)
        table = _maps.slot_table(slot_table)
        if K < 1 or table.shape[0] != K:
            raise SpxError(f"slot_table must be [{K}, J] with J >= 1")
        _rank(quantile, 2)
        self.quantile = float(quantile)
        self.slot_table_host = table
        self.num_slots = J = int(table.shape[1])
        self.num_channels = int(table.max().item()) + 1
        self.slot_table = self.slot_table_host.to(self.device)
        self._similarity = None
        self._group_sizes = None
        self._buf = torch.zeros(K * J * J + K * J + K, dtype=torch.int64, device=self.device)
        self.inter = self._buf[:K * J * J].view(K, J, J)
        self.area = self._buf[K * J * J:K * J * J + K * J].view(K, J)
        self.images = self._buf[K * J * J + K * J:]

    @classmethod
    def for_prototypes(cls, ppnet, device=None, quantile: float = 0.95) -> "ActivationOverlap":
        """Slots = the prototypes of each class (``prototype_class_identity``).  ``update`` then also takes ``distances=``
        and applies the model's ``distance_2_similarity`` on the latent grid first (prototype_overlap.py:60)."""
        from .loss import class_slot_table

        if device is None:
            device = ppnet.prototype_vectors.device
        m = cls(ppnet.num_classes, class_slot_table(ppnet.prototype_class_identity), device, quantile)
        m.num_channels = int(ppnet.prototype_class_identity.shape[0])
        m._similarity = ppnet.distance_2_similarity
        return m

    @classmethod
    def for_groups(cls, ppnet, device=None, quantile: float = 0.95) -> "ActivationOverlap":
        """Slots = the groups of each class: class k owns the channels of ``compute_group(...)[k]`` in the concatenation of
        that list.  ``update`` takes the list or its concatenation ([M, U] with ``grid``, or [N, U, h, w])."""
        if device is None:
            device = ppnet.prototype_vectors.device
        table, sizes = _maps.group_slot_table(ppnet)
        m = cls(ppnet.num_classes, table, device, quantile)
        m.num_channels = sum(sizes)
        m._group_sizes = sizes
        return m

    def reset(self) -> None:
        self._buf.zero_()

    def update(self, activations: Union[torch.Tensor, Sequence[torch.Tensor], None] = None, labels: Optional[torch.Tensor] = None,
               *, distances: Optional[torch.Tensor] = None, grid: Optional[Tuple[int, int]] = None) -> None:
        """Count one batch.  ``activations``: [N, C, h, w] (any strides), or pixel-major [M, C] with ``grid`` = (h, w), or
        (``for_groups``) the list ``compute_group`` returns; ``labels`` [N, H, W] uint8 / int32 / int64 set the output size.
        ``distances=`` [N, P, h, w] (``for_prototypes``) instead of activations.  Enqueues work on the current stream only;
        never synchronises."""
        lib = _lib.load()
        if labels is None:
            raise SpxError("labels are required")
        planes = _maps.input_planes(activations, distances, grid, self._similarity, self._group_sizes, "ActivationOverlap")
        N, Cn, h, w = (int(v) for v in planes.shape)
        H, W = _maps.label_map(labels, N, "activations")
        if Cn < self.num_channels:
            raise SpxError(f"activations have {Cn} channels, the slot table names channel {self.num_channels - 1}")
        lab = _maps.device_labels(planes, labels, "activations", self.device, "counters")
        ws = _workspace(lib, N, Cn, self.num_classes, self.device)
        thr = _thresholds(lib, planes, (H, W), self.quantile, ws)
        _lib.check(lib.spx_overlap_accumulate(planes.data_ptr(), strides(planes), _lib.ptr(thr), lab.data_ptr(),
                                              LABEL_BYTES[lab.dtype], _lib.ptr(self.slot_table), N, Cn, self.num_classes,
                                              self.num_slots, h, w, H, W, _lib.ptr(self.inter), _lib.ptr(self.area),
                                              _lib.ptr(self.images), _lib.ptr(ws), _lib.stream_ptr()))

    def all_reduce(self, group=None) -> None:
        """Sum the counters of every rank (dp._all_reduce_sum)."""
        from .dp import _all_reduce_sum

        _all_reduce_sum(self._buf, group)

    def compute(self) -> OverlapResult:
        host = self._buf.cpu()
        K, J = self.num_classes, self.num_slots
        a, b = K * J * J, K * J * J + K * J
        return finalize(host[:a].view(K, J, J), host[a:b].view(K, J), host[b:], self.slot_table_host)
