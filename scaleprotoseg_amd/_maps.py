"""The inputs of the full-resolution map operators (``metrics``, ``overlap``, ``pushbox``, ``explain``), stated once: fp32 planes
``[N, C, h, w]`` with any strides (or pixel-major ``[M, C]`` with ``grid``), a label map ``[N, H, W]`` of uint8 / int32 / int64
that sets the output size, a slot or row table, and everything on one device, which must be the current one.  Shape and type
checks need no device and come first; ``on_device`` / ``device_labels`` are the only steps that ask for the GPU.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import SpxError

LABEL_BYTES = {torch.uint8: 1, torch.int32: 4, torch.int64: 8}      # the label byte code of the C entry points
MAX_SLOTS = 32


def dev_ptr(t: torch.Tensor, name: str) -> int:
    _lib.require_gpu(t, name)
    return t.data_ptr()


def strides(t: torch.Tensor, order=(0, 1, 2, 3)) -> C.Array:
    st = t.stride()
    return (C.c_int64 * 4)(*[int(st[i]) for i in order])


def planes(t: torch.Tensor, grid: Optional[Tuple[int, int]], name: str) -> torch.Tensor:
    """[N, C, h, w] view (any strides) of ``t``: 4-D as it is, or the pixel-major [M, C] output of
    ``forward_from_conv_features(return_activations=True)`` with ``grid`` = (h, w)."""
    if t.dtype != torch.float32:
        raise SpxError(f"{name} must be fp32 (got {t.dtype})")
    if t.dim() == 4:
        return t.detach()
    if t.dim() == 2 and grid is not None:
        h, w = int(grid[0]), int(grid[1])
        if h < 1 or w < 1 or t.shape[0] % (h * w) != 0:
            raise SpxError(f"{name} has {t.shape[0]} rows, not a multiple of the grid {h} x {w}")
        return t.detach().view(t.shape[0] // (h * w), h, w, t.shape[1]).permute(0, 3, 1, 2)
    raise SpxError(f"{name} must be [N, C, h, w], or [M, C] with grid=(h, w)")


def input_planes(activations, distances, grid, similarity, group_sizes, owner: str) -> torch.Tensor:
    """The [N, C, h, w] planes of what ``update`` (and the explanation maps) accept: activations as ``planes`` takes them,
    ``distances=`` through the model's ``similarity`` (``for_prototypes``), or the list ``compute_group`` returns, concatenated
    (``for_groups``, ``group_sizes`` = its widths)."""
    if (activations is None) == (distances is None):
        raise SpxError("pass either activations or distances=")
    if distances is not None:
        if similarity is None:
            raise SpxError(f"distances= needs {owner}.for_prototypes(ppnet)")
        dev_ptr(distances, "distances")
        activations = similarity(planes(distances, grid, "distances"))
    elif isinstance(activations, (list, tuple)):
        if group_sizes is None or [int(t.shape[-1]) for t in activations] != group_sizes:
            raise SpxError(f"a list of activations must be what compute_group returns for {owner}.for_groups(ppnet)")
        for t in activations:
            dev_ptr(t, "activations")
        activations = torch.cat([t.detach() for t in activations], dim=1)
    return planes(activations, grid, "activations")


def group_slot_table(ppnet) -> Tuple[torch.Tensor, list]:
    """([K, J] channel of (class, group) in the concatenation of ``compute_group``'s list, -1 = no such group; its widths)."""
    sizes = [int(gp.weight.shape[0]) for gp in ppnet.group_projection]
    if len(sizes) != ppnet.num_classes:
        raise SpxError(f"{len(sizes)} group projections for {ppnet.num_classes} classes")
    table = torch.full((len(sizes), max(1, max(sizes))), -1, dtype=torch.long)
    c0 = 0
    for k, g in enumerate(sizes):
        table[k, :g] = torch.arange(c0, c0 + g)
        c0 += g
    return table, sizes


def label_map(labels, N: Optional[int] = None, what: str = "") -> Tuple[int, int]:
    """(H, W) of a label map, which holds as many images as the ``N`` of ``what`` (None: any number); nothing here needs the
    device."""
    if not isinstance(labels, torch.Tensor) or labels.dim() != 3 or labels.dtype not in LABEL_BYTES:
        got = f"{labels.dtype} {tuple(labels.shape)}" if isinstance(labels, torch.Tensor) else type(labels).__name__
        raise SpxError(f"labels must be uint8, int32 or int64 [N, H, W] (got {got})")
    if N is not None and labels.shape[0] != N:
        raise SpxError(f"labels hold {labels.shape[0]} images, {what} {N}")
    return int(labels.shape[1]), int(labels.shape[2])


def on_device(tensors, device: torch.device, owner: str) -> None:
    """Every (tensor, name) of ``tensors`` that is not None is on the GPU ``device``, where the ``owner`` lives, and ``device``
    is the current one."""
    for t, name in tensors:
        if t is not None:
            _lib.require_gpu(t, name)
            if t.device != device:
                raise SpxError(f"{name} on {t.device}, the {owner} on {device}")
    if torch.cuda.current_device() != device.index:
        raise SpxError(f"current device cuda:{torch.cuda.current_device()} is not the {owner}' {device}: the kernels run on the "
                       "current device's stream")


def device_labels(maps: torch.Tensor, labels: torch.Tensor, name: str = "activations", device: Optional[torch.device] = None,
                  owner: Optional[str] = None) -> torch.Tensor:
    """The device step of the label rule: ``on_device`` for the planes ``maps`` (called ``name``) and the labels, on the planes'
    device unless an ``owner``'s ``device`` is given; returns the labels detached and contiguous."""
    on_device(((maps, name), (labels, "labels")), maps.device if device is None else device, owner or name)
    return labels.detach().contiguous()


MAX_MAP_ROWS = 65535             # rows of one launch of a byte-map kernel (a grid dimension)


def upload(host: torch.Tensor, device) -> torch.Tensor:
    """Device copy of a small host table through pinned memory: an asynchronous copy that never waits for the device."""
    return host.pin_memory().to(device, non_blocking=True)


def byte_output(out: Optional[torch.Tensor], shape, device) -> torch.Tensor:
    """The uint8 output of a byte-map operator: ``out`` when it fits (contiguous, any alignment), else a fresh tensor."""
    if out is None:
        return torch.empty(shape, dtype=torch.uint8, device=device)
    if out.dtype != torch.uint8 or tuple(out.shape) != tuple(shape) or out.device != device or not out.is_contiguous():
        raise SpxError(f"out must be a contiguous uint8 {tuple(shape)} tensor on {device}")
    return out


def slot_table(table) -> torch.Tensor:
    """Host int32 [K, J] copy of a slot table (channel of (class, slot) or -1) with ``J <= MAX_SLOTS``."""
    table = torch.as_tensor(table).detach().cpu()
    if table.dim() != 2 or table.shape[0] < 1 or table.shape[1] < 1 or table.is_floating_point():
        raise SpxError(f"slot_table must be integer [K, J] with K, J >= 1 (got {table.dtype} {tuple(table.shape)})")
    if table.shape[1] > MAX_SLOTS:
        raise SpxError(f"{table.shape[1]} slots per class (at most {MAX_SLOTS})")
    return table.to(torch.int32).contiguous()


def host_rows(rows, width: int, what: str) -> torch.Tensor:
    """int64 copy of a host row table [R, ``width``] = ``what``, whose rows the caller then checks with ``bad_row``."""
    if not isinstance(rows, torch.Tensor):
        rows = torch.as_tensor(rows)
    if rows.is_cuda:
        raise SpxError("rows must be a host tensor: every row is checked on the host before any launch (rows_for returns such)")
    if rows.dim() != 2 or rows.shape[1] != width or rows.shape[0] < 1 or rows.is_floating_point():
        raise SpxError(f"rows must be integer [R, {width}] = {what} with R >= 1 (got {rows.dtype} {tuple(rows.shape)})")
    return rows.detach().to(torch.int64)


def bad_row(rows: torch.Tensor, bad: torch.Tensor, why: str) -> None:
    """Raise for the first row that ``bad`` marks."""
    if bool(bad.any()):
        r = int(bad.nonzero()[0])
        raise SpxError(f"row {r} = {tuple(rows[r].tolist())}: {why}")
