"""Explanation maps on the GPU (segmentation/analysis/sample_activations_prototype.py:71-133, sample_activations_group.py:72-131):
the two pictures a user looks at, as uint8 arrays.  (failure_cases.py:188-420 looks like the same code but is not: it masks two
classes' slots with one class, shares the range between them and divides by the maximum; that is ``failures.py``.)

Definition.  Activation planes ``a[n, c, y, x]`` (fp32, latent grid ``h x w``, any strides), labels ``[N, H, W]`` (uint8, int32
or int64; 0 = void, k + 1 = class k, anything else belongs to no class), a slot table ``[K, J]`` (channel of (class, slot) or
-1, ``J <= 32``).  ``u[n, c, Y, X]`` is the plane upsampled to ``H x W`` by the rule of ``overlap.py`` (OpenCV ``INTER_CUBIC``),
computed in fp32 by the one function every pass of the library shares, so every pass sees the same bits.

* Heat map of a row ``(n, k, j)`` with channel ``c = table[k, j] >= 0``: ``m = u * [label == k + 1]`` (0 outside the class),
  ``lo = min m`` and ``hi = max m`` over the whole image, ``d = hi - lo``, ``r = m - lo``, ``x = r / d``, all in fp32 with the
  division correctly rounded, and ``heat = (uint8) trunc(255.0f * x)``: the reference's
  ``np.uint8(255 * ((m - amin) / amax(m - amin)))`` in its own float32 arithmetic.  Where ``d == 0`` (a constant plane, a class
  absent from the image) the map is all zeros; the reference divides 0 by 0 there and the bytes it converts from NaN are
  undefined.  Outputs: ``heat`` uint8 ``[R, H, W]`` and ``ranges`` fp32 ``[R, 2] = (lo, hi)``.
* Dominant slot of a row ``(n, k)``: ``dom[Y, X] = argmax_j (wgt[k, j] * u_j)`` over the class's slots with a channel, the
  product in fp32, the first maximum on ties (``np.argmax``); ``wgt`` is 1 for prototypes and
  ``last_layer_group.weight[k, channel of (k, j)]`` for groups.  The value is the column ``j`` of the table.  Pixels with
  ``label != k + 1`` are 255 (the reference blanks them with ``y_mask`` after the argmax), and so is every pixel of a class
  without a slot.  Output: uint8 ``[R2, H, W]``.

The reference resizes every plane to the image on the host and walks NumPy arrays of 4 bytes per pixel.  Here
``spx_explain_range`` finds ``lo`` / ``hi`` (integer min / max atomics on the order-preserving key: run-to-run identical),
``spx_explain_heat`` and ``spx_explain_dominant`` recompute the pixels and store packed bytes; the fp32 map is never written.
Nothing here waits for the device except ``rows_for``, which says so.

Not built: colour maps, overlays and PNG files.  The arrays are what ``cv2.applyColorMap`` or a ``ListedColormap`` take.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple, Union

import torch

from . import _lib, _maps
from ._lib import SpxError
from ._maps import LABEL_BYTES, bad_row, byte_output as _output, host_rows, strides, upload as _upload

OFF_CLASS = 255                  # the dominant map outside the class
MAX_ROWS = _maps.MAX_MAP_ROWS    # rows of one launch; longer row tables are cut into launches


def _check_channels(table: torch.Tensor, C: int) -> None:
    if int(table.max()) >= C:
        raise SpxError(f"activations have {C} channels, the slot table names channel {int(table.max())}")


def _checked(activations, labels, grid):
    """(planes, N, C, h, w, H, W) of inputs whose shapes and types fit; nothing here needs the device."""
    planes = _maps.planes(activations, grid, "activations")
    N, C, h, w = (int(v) for v in planes.shape)
    return (planes, N, C, h, w, *_maps.label_map(labels, N, "activations"))


def activation_heat_maps(activations: torch.Tensor, labels: torch.Tensor, rows, slot_table, grid: Optional[Tuple[int, int]] = None,
                         *, out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(heat uint8 [R, H, W], ranges fp32 [R, 2] = (lo, hi)) as the module's header defines them.

    ``activations``: fp32 [N, C, h, w] with any strides, or pixel-major [M, C] with ``grid`` = (h, w).  ``labels``: [N, H, W]
    uint8 / int32 / int64 on the device; its shape is the image size.  ``rows``: integer [R, 3] = (n, k, j) in host memory; a
    row out of range, or one whose slot ``slot_table[k, j]`` is -1, raises before anything is launched.  ``out``: a contiguous
    uint8 [R, H, W] tensor to write into (any alignment; every byte is written exactly once).  Enqueues work on the current
    stream only; never synchronises."""
    planes, N, C, h, w, H, W = _checked(activations, labels, grid)
    table = _maps.slot_table(slot_table)
    _check_channels(table, C)
    K, J = (int(v) for v in table.shape)
    rows = host_rows(rows, 3, "(n, k, j)")
    n, k, j = rows[:, 0], rows[:, 1], rows[:, 2]
    bad_row(rows, (n < 0) | (n >= N) | (k < 0) | (k >= K) | (j < 0) | (j >= J), f"outside N={N}, K={K}, J={J}")
    c = table.to(torch.int64)[k, j]
    bad_row(rows, c < 0, "the class has no such slot")
    lab = _maps.device_labels(planes, labels)
    lib = _lib.load()
    R = int(rows.shape[0])
    heat = _output(out, (R, H, W), planes.device)
    ranges = torch.empty(R, 2, dtype=torch.float32, device=planes.device)
    host = torch.stack([n, c, k], dim=1).to(torch.int32).contiguous()
    dev = _upload(host, planes.device)
    keys = torch.empty(2 * min(R, MAX_ROWS), dtype=torch.int32, device=planes.device)
    st, stream = strides(planes), _lib.stream_ptr()
    for r0 in range(0, R, MAX_ROWS):
        r1 = min(R, r0 + MAX_ROWS)
        common = (planes.data_ptr(), st, lab.data_ptr(), LABEL_BYTES[lab.dtype], dev[r0:r1].data_ptr(), host[r0:r1].data_ptr(),
                  r1 - r0, N, C, h, w, H, W, keys.data_ptr())
        _lib.check(lib.spx_explain_range(*common, stream))
        _lib.check(lib.spx_explain_heat(*common, heat[r0:r1].data_ptr(), ranges[r0:r1].data_ptr(), stream))
    return heat, ranges


def dominant_slot_maps(activations: torch.Tensor, labels: torch.Tensor, rows, slot_table, weights: Optional[torch.Tensor] = None,
                       grid: Optional[Tuple[int, int]] = None, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [R, H, W]: per row (n, k) the slot that dominates each pixel of class k in image n, 255 elsewhere, as the module's
    header defines it.  ``rows``: integer [R, 2] = (n, k) in host memory, checked there.  ``slot_table``: integer [K, J], read
    on the host (pass a host tensor: a device tensor is copied back first).  ``weights``: fp32 [K, J] on the device (read
    there, never by the host), or None = 1.  The other arguments as ``activation_heat_maps`` takes them.  Enqueues work on the
    current stream only; never synchronises."""
    return _dominant(activations, labels, rows, _maps.slot_table(slot_table), None, weights, grid, out)


def _dominant(activations, labels, rows, table: torch.Tensor, dev_table: Optional[torch.Tensor], weights, grid, out) -> torch.Tensor:
    planes, N, C, h, w, H, W = _checked(activations, labels, grid)
    _check_channels(table, C)
    K, J = (int(v) for v in table.shape)
    rows = host_rows(rows, 2, "(n, k)")
    bad_row(rows, (rows[:, 0] < 0) | (rows[:, 0] >= N) | (rows[:, 1] < 0) | (rows[:, 1] >= K), f"outside N={N}, K={K}")
    if weights is not None and (not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32 or tuple(weights.shape) != (K, J)):
        raise SpxError(f"weights must be fp32 [{K}, {J}]")
    lab = _maps.device_labels(planes, labels)
    if weights is not None:
        _lib.require_gpu(weights, "weights")
        if weights.device != planes.device:
            raise SpxError(f"weights are on {weights.device}, activations on {planes.device}")
        weights = weights.detach().contiguous()
    lib = _lib.load()
    R = int(rows.shape[0])
    dom = _output(out, (R, H, W), planes.device)
    host = rows.to(torch.int32).contiguous()
    dev = _upload(host, planes.device)
    if dev_table is None:
        dev_table = _upload(table, planes.device)
    st, stream = strides(planes), _lib.stream_ptr()
    for r0 in range(0, R, MAX_ROWS):
        r1 = min(R, r0 + MAX_ROWS)
        _lib.check(lib.spx_explain_dominant(planes.data_ptr(), st, lab.data_ptr(), LABEL_BYTES[lab.dtype], dev[r0:r1].data_ptr(),
                                            host[r0:r1].data_ptr(), dev_table.data_ptr(), _lib.ptr(weights), r1 - r0, N, C, K, J, h, w,
                                            H, W, dom[r0:r1].data_ptr(), stream))
    return dom


class ExplanationMaps:
    """The explanation maps of one model.

        ex = ExplanationMaps.for_prototypes(ppnet)                  # or .for_groups(ppnet)
        logits, distances = ppnet(img)                              # distances [N, P, h, w]
        rows, rows2 = ex.rows_for(ann)                              # ann [N, H, W]; the ONE host synchronisation
        heat, ranges = ex.heat_maps(rows, labels=ann, distances=distances)
        dom = ex.dominant_slots(rows2, labels=ann, distances=distances)

    The slot table lives on the host (rows are checked against it there); its device copy is made once per device."""

    def __init__(self, num_classes: int, slot_table, weight_source=None):
        self.num_classes = K = int(num_classes)
        self.slot_table = _maps.slot_table(slot_table)
        if K < 1 or self.slot_table.shape[0] != K:
            raise SpxError(f"slot_table must be [{K}, J] with J >= 1")
        self.num_slots = int(self.slot_table.shape[1])
        self._similarity = None
        self._group_sizes = None
        self._weight_source = weight_source                   # None, or a callable returning fp32 [K, J] on the given device
        self._device_tables: Dict[torch.device, torch.Tensor] = {}

    @classmethod
    def for_prototypes(cls, ppnet) -> "ExplanationMaps":
        """Slots = the prototypes of each class (``prototype_class_identity``), weights 1.  The methods then also take
        ``distances=`` and apply the model's ``distance_2_similarity`` on the latent grid first
        (sample_activations_prototype.py:85)."""
        from .loss import class_slot_table

        ex = cls(ppnet.num_classes, class_slot_table(ppnet.prototype_class_identity))
        ex._similarity = ppnet.distance_2_similarity
        return ex

    @classmethod
    def for_groups(cls, ppnet) -> "ExplanationMaps":
        """Slots = the groups of each class, as ``ActivationOverlap.for_groups`` numbers them; the weight of (k, j) is
        ``last_layer_group.weight[k, channel of (k, j)]`` (sample_activations_group.py:92-95), gathered on the device at every
        call: an optimizer step or a loaded checkpoint is seen without any cache to invalidate."""
        table, sizes = _maps.group_slot_table(ppnet)
        index = (torch.arange(table.shape[0]).unsqueeze(1).expand_as(table).contiguous(), table.clamp_min(0), table >= 0)
        head = ppnet.last_layer_group
        on: Dict[torch.device, tuple] = {}

        def weights(device):
            wt = head.weight.detach()
            if wt.device != device:
                raise SpxError(f"last_layer_group is on {wt.device}, activations on {device}")
            if device not in on:
                on[device] = tuple(t.to(device) for t in index)
            k, c, valid = on[device]
            return (wt.to(torch.float32)[k, c] * valid).contiguous()

        ex = cls(ppnet.num_classes, table, weights)
        ex._group_sizes = sizes
        return ex

    def _inputs(self, activations, distances, grid):
        return _maps.input_planes(activations, distances, grid, self._similarity, self._group_sizes, "ExplanationMaps")

    def _table_on(self, device: torch.device) -> torch.Tensor:
        """The device copy of the slot table, made at the first call on ``device`` (a blocking copy, once)."""
        if device not in self._device_tables:
            self._device_tables[device] = self.slot_table.to(device)
        return self._device_tables[device]

    def rows_for(self, labels: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(rows int64 [R, 3] = (n, k, j), rows2 int64 [R2, 2] = (n, k)), host tensors: every slot, and every class with a
        slot, of the classes present in each image, in ascending (n, k, j) order: what the reference's loop over
        ``np.unique(gt_ann)`` plots.  Presence is counted where the labels live and copied once: ONE host synchronisation."""
        _maps.label_map(labels)
        N, K = int(labels.shape[0]), self.num_classes
        lab = labels.detach().reshape(N, -1).to(torch.int64)
        lab = torch.where((lab >= 1) & (lab <= K), lab, torch.zeros_like(lab))
        seen = torch.zeros(N, K + 1, dtype=torch.int32, device=labels.device).scatter_(1, lab, 1)
        present = seen[:, 1:].cpu().bool()                              # the synchronisation
        valid = self.slot_table >= 0
        rows = (present[:, :, None] & valid[None]).nonzero()
        rows2 = (present & valid.any(1)[None]).nonzero()
        return rows, rows2

    def heat_maps(self, rows, activations: Union[torch.Tensor, Sequence[torch.Tensor], None] = None,
                  labels: Optional[torch.Tensor] = None, *, distances: Optional[torch.Tensor] = None,
                  grid: Optional[Tuple[int, int]] = None, out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``activation_heat_maps`` for this model's slots.  The inputs are those of ``ActivationOverlap.update``: activations
        ([N, C, h, w], pixel-major [M, C] with ``grid``, or - ``for_groups`` - the list ``compute_group`` returns) or
        ``distances=`` (``for_prototypes``).  Never synchronises."""
        if labels is None:
            raise SpxError("labels are required")
        return activation_heat_maps(self._inputs(activations, distances, grid), labels, rows, self.slot_table, out=out)

    def dominant_slots(self, rows, activations: Union[torch.Tensor, Sequence[torch.Tensor], None] = None,
                       labels: Optional[torch.Tensor] = None, *, distances: Optional[torch.Tensor] = None,
                       grid: Optional[Tuple[int, int]] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``dominant_slot_maps`` for this model's slots and weights; inputs as ``heat_maps`` takes them.  Never synchronises."""
        if labels is None:
            raise SpxError("labels are required")
        planes = self._inputs(activations, distances, grid)
        _checked(planes, labels, None)
        _lib.require_gpu(planes, "activations")
        weights = None if self._weight_source is None else self._weight_source(planes.device)
        return _dominant(planes, labels, rows, self.slot_table, self._table_on(planes.device), weights, None, out)
