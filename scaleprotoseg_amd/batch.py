"""Training-batch preparation on the GPU (segmentation/data/dataset.py:143-186 and the per-step ``resize_label`` of
module_multiscale.py:234-236): raw ``uint8`` images and integer labels go up once, ONE launch (spx_batch_prepare) writes the
scaled, padded, cropped, flipped and normalised window batch, the window labels and the latent labels of every grid.

    p = draw_augmentation(rng, label.shape, window_size, scales)        # the reference's draws, in its order
    batch = prepare_batch(images, labels, params, window=(513, 513), mean=m, std=s, grids=[(65, 65)])
    lat = resize_labels(labels_dev, grids=[(65, 65), (33, 33)])         # the latent-label half alone

The labels follow PIL's NEAREST rule through the index tables of ``utils._pil_nearest_index`` (pinned to the reference); the image
follows the restated float rule of include/spx_hip.h - OpenCV's fixed-point INTER_LINEAR was never run against it.
``ColorJitter`` is left out: ``normalize=False`` or ``dtype=torch.uint8`` give the un-normalised window a caller's own jitter takes.

Everything is validated on the host before the library is touched.  The descriptors, the index tables and the id table (a host
table) travel in one pinned buffer with one non-blocking copy into a ``BatchTable``: a temporary one per call, or the caller's
(``table=``), which a captured step needs.

Capture (``graphs.capture_step``).  A captured launch reads the table's device buffer at every replay, and the kernel arguments
(outputs, window, grids, batch size) are frozen with it.  So: create ``tbl = BatchTable(device, batch, index_entries)`` outside
the step, pass ``table=tbl`` and keep ``tbl`` as long as the graph.  The warm-up uploads the table; the captured call finds the
same bytes there and records no copy (other bytes while capturing raise).  Replays therefore repeat ONE geometry - the same
sources, scaled sizes, origins and flips - until the caller refills the table between replays with
``fill_batch_table(tbl, images, labels, params, window=..., grids=..., id_map=...)`` on the stream that replays: new pointers,
sizes, origins and flips, the same batch size, window, grids and id table.  One table serves one stream at a time.
"""
from __future__ import annotations

import ctypes as C
from functools import lru_cache
from typing import List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._lib import SpxError
from .utils import _pil_nearest_index

MAX_GRIDS = _lib.SPX_BATCH_MAX_GRIDS
_LABEL_CODES = {torch.uint8: 1, torch.int16: 2, torch.int32: 4, torch.int64: 8}
_SAMPLE_DTYPE = np.dtype({
    "names": ["image", "label", "image_row_stride", "label_row_stride", "image_pixel_stride", "label_dtype", "h", "w", "hs", "ws",
              "y0", "x0", "flip", "row_tab", "col_tab", "reserved"],
    "formats": ["<u8", "<u8", "<i8", "<i8"] + ["<i4"] * 12,
})
assert _SAMPLE_DTYPE.itemsize == C.sizeof(_lib.SpxBatchSample) == 80
assert all(_SAMPLE_DTYPE.fields[n][1] == getattr(_lib.SpxBatchSample, n).offset for n in _SAMPLE_DTYPE.names)


class AugmentParams(NamedTuple):
    """What ``PatchClassificationDataset.__getitem__`` draws for one sample."""

    scaled: Tuple[int, int]     # (hs, ws) = (int(h * f), int(w * f))
    origin: Tuple[int, int]     # (y0, x0) of the crop in the scaled, padded image
    flip: bool


class PreparedBatch(NamedTuple):
    image: Optional[torch.Tensor]               # [B, 3, Hc, Wc] fp32 or uint8
    labels: Optional[torch.Tensor]              # [B, Hc, Wc] int64, the reference's convention (0 = void)
    latent: List[torch.Tensor]                  # per grid [B, h_g, w_g] int64
    latent0: Optional[List[torch.Tensor]]       # per grid int32, shifted_labels_i32 of the above
    table: Optional["BatchTable"] = None        # the table the launch read (the caller's own, or this call's temporary)


def draw_augmentation(rng, label_shape: Sequence[int], window_size: Optional[Sequence[int]] = None,
                      scales: Sequence[float] = (1.0,)) -> AugmentParams:
    """The reference's draws in the reference's order (dataset.py:145-184) from ``rng``, a ``random.Random`` or the ``random``
    module: the same seed yields the reference's parameters.  ``window_size=None`` is the label's own shape."""
    h, w = int(label_shape[0]), int(label_shape[1])
    Hc, Wc = (h, w) if window_size is None else (int(window_size[0]), int(window_size[1]))
    f = 1.0 if len(scales) < 2 else rng.uniform(scales[0], scales[1])
    hs, ws = int(h * f), int(w * f)
    y0 = rng.randint(0, max(hs, Hc) - Hc)
    x0 = rng.randint(0, max(ws, Wc) - Wc)
    flip = rng.random() < 0.5
    return AugmentParams((hs, ws), (y0, x0), bool(flip))


@lru_cache(maxsize=512)
def _table(n_in: int, n_out: int) -> np.ndarray:
    t = _pil_nearest_index(n_in, n_out).astype(np.int32)
    t.setflags(write=False)
    return t


class _Index:
    """The int32 index buffer of one call: every (n_in, n_out) table once."""

    def __init__(self) -> None:
        self.parts: List[np.ndarray] = []
        self.where = {}
        self.n = 0

    def add(self, arr: np.ndarray) -> int:
        at = self.n
        self.parts.append(arr)
        self.n += int(arr.size)
        return at

    def table(self, n_in: int, n_out: int) -> int:
        key = (n_in, n_out)
        if key not in self.where:
            self.where[key] = self.add(_table(n_in, n_out))
        return self.where[key]


class BatchTable:
    """Descriptors and index tables of a launch: a pinned host buffer and its device copy, ``batch`` descriptors of 80 bytes and
    ``index_entries`` int32 entries (the latent grids' tables first, then the id table, then the samples' tables, so that what a
    captured launch froze stays where it is when the samples change).  Owned by the caller; see the module docstring."""

    def __init__(self, device, batch: int = 8, index_entries: int = 1 << 16) -> None:
        self.device = torch.device(device)
        _lib.require_gpu(self.device, "BatchTable")
        self.batch, self.index_entries = int(batch), int(index_entries)
        if self.batch < 1 or self.index_entries < 1:
            raise SpxError(f"BatchTable: batch {batch}, index_entries {index_entries}")
        nbytes = self.batch * 80 + 4 * self.index_entries
        self.pinned = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)     # only what a packing wrote is ever read
        self.dev = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.layout = None          # (window, grids, id table) of the last packing: what a captured launch froze
        self._copied: Optional[torch.cuda.Event] = None

    def send(self, desc: np.ndarray, index: "_Index", layout) -> None:
        """Pack and upload on the current stream.  While the stream is capturing nothing is copied: the bytes must be there."""
        B = int(desc.shape[0])
        if B > self.batch or index.n > self.index_entries:
            raise SpxError(f"BatchTable: {B} samples and {index.n} index entries do not fit ({self.batch}, {self.index_entries})")
        head = desc.view(np.uint8)
        tail = np.concatenate(index.parts).view(np.uint8)
        at = self.batch * 80
        host = self.pinned.numpy()
        if torch.cuda.is_current_stream_capturing():
            same = self._copied is not None and np.array_equal(host[:head.size], head) and np.array_equal(host[at:at + tail.size], tail)
            if not same:
                raise SpxError("batch: the stream is capturing and the table does not hold this call's descriptors; run the same call "
                               "with the same table once before the capture (graphs.capture_step's warm-up does)")
            return
        if self._copied is not None:
            self._copied.synchronize()                      # the last copy out of the pinned buffer has to be over before it is rewritten
        host[:head.size] = head
        host[at:at + tail.size] = tail
        self.dev.copy_(self.pinned, non_blocking=True)
        self._copied = torch.cuda.Event()
        self._copied.record()
        self.layout = layout


def _grids(grids) -> List[Tuple[int, int]]:
    out = [(int(g[0]), int(g[1])) for g in (grids or ())]
    if len(out) > MAX_GRIDS:
        raise SpxError(f"batch: {len(out)} latent grids, at most {MAX_GRIDS} per launch")
    for g in out:
        if g[0] < 1 or g[1] < 1:
            raise SpxError(f"batch: latent grid {g} is empty")
    return out


def _id_map_host(id_map) -> Optional[np.ndarray]:
    if id_map is None:
        return None
    if isinstance(id_map, torch.Tensor) and id_map.is_cuda:
        raise SpxError("batch: id_map is a host table (it travels with the descriptors); a device tensor would be read back")
    arr = id_map.numpy() if isinstance(id_map, torch.Tensor) else np.asarray(id_map)
    if arr.ndim != 1 or arr.size < 1 or not np.issubdtype(arr.dtype, np.integer):
        raise SpxError("batch: id_map must be a non-empty 1-D integer table (raw value -> class id)")
    return np.ascontiguousarray(arr.astype(np.int32))


def _as_list(x, stacked_dim: int, what: str) -> List[torch.Tensor]:
    if isinstance(x, torch.Tensor):
        if x.dim() != stacked_dim:
            raise SpxError(f"batch: a stacked {what} tensor has {stacked_dim} dimensions, got {tuple(x.shape)}")
        return list(x.unbind(0))
    out = list(x)
    if not out or not all(isinstance(t, torch.Tensor) for t in out):
        raise SpxError(f"batch: {what} must be a tensor or a non-empty sequence of tensors")
    return out


def _latent_out(out_list, grids, B, dtype, device, what):
    if out_list is None:
        return [torch.empty((B, h, w), dtype=dtype, device=device) for h, w in grids]
    res = list(out_list)
    if len(res) != len(grids):
        raise SpxError(f"batch: out.{what} has {len(res)} tensors for {len(grids)} grids")
    for t, (h, w) in zip(res, grids):
        _check_out(t, (B, h, w), dtype, device, what)
    return res


def _check_out(t: torch.Tensor, shape, dtype, device, what: str) -> None:
    if tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != device or not t.is_contiguous():
        raise SpxError(f"batch: out.{what} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {device}, got "
                       f"{tuple(t.shape)} {t.dtype} on {t.device}")


def _fill_grids(args: _lib.SpxBatch, index: _Index, grids, Hc: int, Wc: int) -> None:
    args.G = len(grids)
    for g, (h, w) in enumerate(grids):
        args.grid_h[g], args.grid_w[g] = h, w
        args.grid_rt[g], args.grid_ct[g] = index.table(Hc, h), index.table(Wc, w)


class _Packed(NamedTuple):
    B: int
    device: torch.device
    grids: List[Tuple[int, int]]
    window: Tuple[int, int]
    args: "_lib.SpxBatch"
    desc: np.ndarray
    index: _Index
    id_at: int
    id_len: int
    layout: tuple


def _pack(images, labels, params, window, grids, id_map) -> _Packed:
    """Validate the samples and pack their descriptors and tables on the host (no library, no device work)."""
    grid_list = _grids(grids)
    Hc, Wc = int(window[0]), int(window[1])
    if Hc < 1 or Wc < 1 or Hc * Wc >= 2 ** 31 - 256:
        raise SpxError(f"batch: window {Hc} x {Wc}")
    ids = _id_map_host(id_map)
    imgs = _as_list(images, 4, "images")
    labs = _as_list(labels, 3, "labels")
    plist = [AugmentParams((int(p[0][0]), int(p[0][1])), (int(p[1][0]), int(p[1][1])), bool(p[2])) for p in params]
    B = len(imgs)
    if len(labs) != B or len(plist) != B:
        raise SpxError(f"batch: {B} images, {len(labs)} labels, {len(plist)} parameter sets")
    if B > 65535:
        raise SpxError(f"batch: {B} samples, at most 65535 per launch")
    for n, (im, lb, p) in enumerate(zip(imgs, labs, plist)):
        if im.dtype != torch.uint8:
            raise SpxError(f"batch: image {n} has dtype {im.dtype}; raw images are torch.uint8")
        if lb.dtype not in _LABEL_CODES:
            raise SpxError(f"batch: label {n} has dtype {lb.dtype}; uint8, int16, int32 or int64")
        if im.dim() != 3 or im.shape[2] != 3 or lb.dim() != 2 or tuple(im.shape[:2]) != tuple(lb.shape) or lb.numel() == 0:
            raise SpxError(f"batch: sample {n}: image {tuple(im.shape)} must be [h, w, 3] and its label {tuple(lb.shape)} [h, w]")
        if im.stride(2) != 1 or lb.stride(1) != 1 or min(im.stride()) < 0 or min(lb.stride()) < 0:
            raise SpxError(f"batch: sample {n}: the image's channel stride and the label's column stride must be 1")
        (hs, ws), (y0, x0), _ = p
        if hs < 1 or ws < 1:
            raise SpxError(f"batch: sample {n} has a scaled size of zero: {hs} x {ws}")
        if not (0 <= y0 <= max(hs, Hc) - Hc and 0 <= x0 <= max(ws, Wc) - Wc):
            raise SpxError(f"batch: sample {n}: origin ({y0}, {x0}) outside 0..{max(hs, Hc) - Hc} x 0..{max(ws, Wc) - Wc}")
    for t in imgs + labs:
        _lib.require_gpu(t, "batch: input")
    device = imgs[0].device
    if any(t.device != device for t in imgs + labs):
        raise SpxError("batch: the inputs are on different devices")

    index = _Index()
    args = _lib.SpxBatch()
    _fill_grids(args, index, grid_list, Hc, Wc)                     # the grids' tables and the id table first: fixed places
    id_at = index.add(ids) if ids is not None else -1
    desc = np.zeros(B, dtype=_SAMPLE_DTYPE)
    for n, (im, lb, p) in enumerate(zip(imgs, labs, plist)):
        h, w = int(lb.shape[0]), int(lb.shape[1])
        d = desc[n]
        d["image"], d["label"] = im.data_ptr(), lb.data_ptr()
        d["image_row_stride"], d["image_pixel_stride"] = im.stride(0), im.stride(1)
        d["label_row_stride"], d["label_dtype"] = lb.stride(0), _LABEL_CODES[lb.dtype]
        d["h"], d["w"], d["hs"], d["ws"] = h, w, p.scaled[0], p.scaled[1]
        d["y0"], d["x0"], d["flip"] = p.origin[0], p.origin[1], int(p.flip)
        d["row_tab"], d["col_tab"] = index.table(h, p.scaled[0]), index.table(w, p.scaled[1])
    layout = (B, (Hc, Wc), tuple(grid_list), None if ids is None else ids.tobytes())
    return _Packed(B, device, grid_list, (Hc, Wc), args, desc, index, id_at, 0 if ids is None else int(ids.size), layout)


@torch.no_grad()
def fill_batch_table(table: BatchTable, images, labels, params: Sequence[AugmentParams], window: Sequence[int],
                     grids: Sequence[Sequence[int]] = (), id_map=None) -> None:
    """Refill ``table`` for the next replay of a graph that captured ``prepare_batch(..., table=table)``: new sources, scaled sizes,
    origins and flips; the batch size, window, grids and id table of the captured call (``SpxError`` otherwise).  The copy goes to
    the current stream, so call it on the stream that replays."""
    pk = _pack(images, labels, params, window, grids, id_map)
    if table.layout is None or table.layout != pk.layout:
        raise SpxError("batch: fill_batch_table needs the batch size, window, grids and id table of the call that used this table")
    with torch.cuda.device(pk.device):
        table.send(pk.desc, pk.index, pk.layout)


@torch.no_grad()
def prepare_batch(images, labels, params: Sequence[AugmentParams], window: Sequence[int], mean: Sequence[float],
                  std: Sequence[float], grids: Sequence[Sequence[int]] = (), id_map=None, normalize: bool = True,
                  round_u8: bool = True, dtype: torch.dtype = torch.float32, shifted: bool = True, want_labels: bool = True,
                  out: Optional[PreparedBatch] = None, table: Optional[BatchTable] = None) -> PreparedBatch:
    """The window batch of ``images`` / ``labels`` under ``params`` in one launch on the current stream (module docstring).

    ``images``: device ``uint8`` tensors ``[h, w, 3]`` with channel stride 1 - a margin view ``img[m:-m, m:-m]`` is read in place - or
    one stacked ``[B, h, w, 3]`` tensor; ``labels``: device ``uint8`` / ``int16`` / ``int32`` / ``int64`` tensors ``[h, w]`` with unit
    column stride, or one stacked tensor.  The sizes may differ between samples.  ``grids``: up to four latent ``(h_g, w_g)``.
    ``id_map``: an integer table, raw value -> class id (``convert_targets``); a raw value outside it becomes 0.  ``out``: a
    ``PreparedBatch`` of preallocated contiguous tensors to write into.  ``table``: the caller's ``BatchTable``; a captured call needs
    one.  Raises ``SpxError`` for host inputs, a scaled size of zero, an origin outside ``0..max(hs, Hc) - Hc``, more than four
    grids, a zero in ``std`` and wrong dtypes - before any launch."""
    if dtype not in (torch.float32, torch.uint8):
        raise SpxError(f"batch: output dtype {dtype}; torch.float32 or torch.uint8")
    if dtype == torch.uint8 and not round_u8:
        raise SpxError("batch: uint8 output dtype needs round_u8")
    mean_f = [float(v) for v in mean]
    std_f = [float(v) for v in std]
    if len(mean_f) != 3 or len(std_f) != 3 or not all(np.isfinite(mean_f + std_f)):
        raise SpxError("batch: mean and std are three finite values each")
    if any(np.float32(v) == 0 for v in std_f):
        raise SpxError(f"batch: std {std_f} has a zero")
    pk = _pack(images, labels, params, window, grids, id_map)
    B, device, grid_list, (Hc, Wc), args = pk.B, pk.device, pk.grids, pk.window, pk.args
    if table is not None and table.device != device:
        raise SpxError(f"batch: the table is on {table.device}, the inputs on {device}")

    if out is None:
        image = torch.empty((B, 3, Hc, Wc), dtype=dtype, device=device)
        win = torch.empty((B, Hc, Wc), dtype=torch.int64, device=device) if want_labels else None
        lat, lat0 = None, None
    else:
        image, win, lat, lat0 = out.image, out.labels, out.latent, out.latent0
        if image is not None:
            _check_out(image, (B, 3, Hc, Wc), dtype, device, "image")
        if win is not None:
            _check_out(win, (B, Hc, Wc), torch.int64, device, "labels")
    lat = _latent_out(lat, grid_list, B, torch.int64, device, "latent")
    lat0 = _latent_out(lat0, grid_list, B, torch.int32, device, "latent0") if (shifted or lat0 is not None) else None
    if image is None and win is None and not grid_list:
        raise SpxError("batch: nothing to write")

    lib = _lib.load()
    with torch.cuda.device(device):
        if table is None:
            if torch.cuda.is_current_stream_capturing():
                raise SpxError("batch: a captured prepare_batch needs the caller's BatchTable (table=), kept as long as the graph")
            table = BatchTable(device, B, pk.index.n)
        table.send(pk.desc, pk.index, pk.layout)
        base = table.dev.data_ptr()
        args.samples, args.index = base, base + table.batch * 80
        args.n_index = table.index_entries
        if pk.id_at >= 0:
            args.id_map, args.L = args.index + 4 * pk.id_at, pk.id_len
        args.image_out = image.data_ptr() if image is not None else None
        args.window_labels = win.data_ptr() if win is not None else None
        for g in range(len(grid_list)):
            args.latent[g] = lat[g].data_ptr()
            args.latent0[g] = lat0[g].data_ptr() if lat0 is not None else None
        args.B, args.Hc, args.Wc = B, Hc, Wc
        args.normalize, args.round_u8, args.out_u8 = int(bool(normalize)), int(bool(round_u8)), int(dtype == torch.uint8)
        for c in range(3):
            args.mean[c], args.std[c] = mean_f[c], std_f[c]
        _lib.check(lib.spx_batch_prepare(C.byref(args), _lib.stream_ptr()))
    return PreparedBatch(image, win, lat, lat0, table)


@torch.no_grad()
def resize_labels(labels: Union[torch.Tensor, Sequence[torch.Tensor]], grids: Sequence[Sequence[int]], id_map=None,
                  shifted: bool = False, out: Optional[Sequence[torch.Tensor]] = None,
                  table: Optional[BatchTable] = None) -> List[torch.Tensor]:
    """``torch.stack([resize_label(l, (w_g, h_g)) for l in labels])`` per grid, for labels ``[B, H, W]`` already on the device
    (``uint8`` / ``int16`` / ``int32`` / ``int64``; a sequence of equal shapes is stacked), every grid in one launch
    (spx_resize_labels) on the current stream.  ``id_map`` as in ``prepare_batch``.  ``shifted=True`` returns the int32 form of
    ``shifted_labels_i32`` (void = -1) instead of the int64 one.  ``table``: the caller's ``BatchTable`` (``batch`` is not used), which
    a captured call needs and must keep as long as the graph.  Host labels raise ``SpxError``."""
    grid_list = _grids(grids)
    if not grid_list:
        raise SpxError("batch: resize_labels needs a grid")
    ids = _id_map_host(id_map)
    if not isinstance(labels, torch.Tensor):
        seq = _as_list(labels, 3, "labels")
        if len({tuple(t.shape) for t in seq}) != 1:
            raise SpxError("batch: resize_labels takes labels of one shape; prepare_batch takes mixed sizes")
        for t in seq:
            _lib.require_gpu(t, "batch: labels")
        labels = torch.stack(seq)
    if labels.dim() != 3 or labels.numel() == 0:
        raise SpxError(f"batch: labels must be a non-empty [B, H, W], got {tuple(labels.shape)}")
    if labels.dtype not in _LABEL_CODES:
        raise SpxError(f"batch: labels have dtype {labels.dtype}; uint8, int16, int32 or int64")
    B, H, W = (int(v) for v in labels.shape)
    if B > 65535 or H * W >= 2 ** 31 - 256:
        raise SpxError(f"batch: labels {tuple(labels.shape)} are beyond one launch")
    _lib.require_gpu(labels, "batch: labels")
    labels = labels.contiguous()
    device = labels.device

    index = _Index()
    args = _lib.SpxBatch()
    _fill_grids(args, index, grid_list, H, W)
    id_at = index.add(ids) if ids is not None else -1
    res = _latent_out(out, grid_list, B, torch.int32 if shifted else torch.int64, device, "latent")

    lib = _lib.load()
    with torch.cuda.device(device):
        if table is None:
            if torch.cuda.is_current_stream_capturing():
                raise SpxError("batch: a captured resize_labels needs the caller's BatchTable (table=), kept as long as the graph")
            table = BatchTable(device, 1, index.n)
        elif table.device != device:
            raise SpxError(f"batch: the table is on {table.device}, the labels on {device}")
        table.send(np.zeros(0, dtype=_SAMPLE_DTYPE), index, ("resize", (H, W), tuple(grid_list), None if ids is None else ids.tobytes()))
        args.index, args.n_index = table.dev.data_ptr() + table.batch * 80, table.index_entries
        if ids is not None:
            args.id_map, args.L = args.index + 4 * id_at, int(ids.size)
        args.labels_in, args.labels_dtype = labels.data_ptr(), _LABEL_CODES[labels.dtype]
        args.B, args.Hc, args.Wc = B, H, W
        for g in range(len(grid_list)):
            (args.latent0 if shifted else args.latent)[g] = res[g].data_ptr()
        _lib.check(lib.spx_resize_labels(C.byref(args), _lib.stream_ptr()))
    return res
