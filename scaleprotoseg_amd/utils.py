"""Small host-side helpers the hot path's callers need."""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import SpxError

SIMPLEX_MAX_BLOCKS = 192    # tensors per spx_simplex_project launch
SIMPLEX_MAX_COLS = 1024     # longest row the kernel takes


@torch.no_grad()
def projection_simplex_sort(v: torch.Tensor, z: float = 1.0) -> torch.Tensor:
    """Row-wise Euclidean projection onto the probability simplex (segmentation/utils.py:113-124).

    Init-time / once-per-optimizer-step work on [G, n_k] matrices; stays stock PyTorch on v's device."""
    n = v.size(1)
    u, _ = torch.sort(v, descending=True)
    css = torch.cumsum(u, 1) - z
    k = torch.arange(n, device=v.device).type_as(v) + 1
    cond = (u - css / k) > 0
    rho, rho_idx = (k * cond).max(1)
    theta = torch.gather(css, 1, rho_idx[:, None]) / rho[:, None]
    return torch.clamp(v - theta, min=0)


@torch.no_grad()
def projection_simplex_sort_(weights: Sequence[torch.Tensor], z: float = 1.0) -> None:
    """``projection_simplex_sort`` of every ``[G, n]`` tensor of ``weights``, IN PLACE: one launch per 192 tensors
    (spx_simplex_project) on the current stream, no host sync, capturable.  Every tensor keeps its storage; its version counter
    is bumped (``torch.autograd.graph.increment_version``), so the host-side caches keyed on the parameters and autograd's
    saved-tensor checks see the edit.  ``nn.Parameter``s are taken as their data; no autograd node is recorded.  The result
    equals the stock formula on a CPU copy of the input bit for bit (include/spx_hip.h).

    The tensors must be fp32, contiguous and on the GPU (``SpxError`` otherwise: an in-place edit of a silent copy would do
    nothing).  Rows longer than 1024 are beyond the kernel: if ANY tensor has ``n > 1024`` the whole call takes the stock
    formula on the device, copied back in place - same storage and version rules, many launches."""
    ws: List[torch.Tensor] = [w.detach() for w in weights]
    if not ws:
        return
    for w in ws:
        _lib.require_gpu(w, "projection_simplex_sort_: weight")
        if w.dim() != 2 or w.dtype != torch.float32 or not w.is_contiguous() or w.shape[0] < 1 or w.shape[1] < 1:
            raise SpxError(f"projection_simplex_sort_: weights must be non-empty contiguous fp32 [G, n] matrices, got "
                           f"{tuple(w.shape)} {w.dtype} (contiguous: {w.is_contiguous()})")
    if len({w.data_ptr() for w in ws}) != len(ws):
        raise SpxError("projection_simplex_sort_: the same storage is listed twice (its rows would be projected concurrently)")
    if any(w.shape[1] > SIMPLEX_MAX_COLS for w in ws):
        for w in ws:
            w.copy_(projection_simplex_sort(w, z))              # (copy_ bumps the version counter the detached view shares)
        return
    lib = _lib.load()
    stream = _lib.stream_ptr()
    for i in range(0, len(ws), SIMPLEX_MAX_BLOCKS):
        chunk = ws[i:i + SIMPLEX_MAX_BLOCKS]
        m = len(chunk)
        ptrs = (C.c_void_p * m)(*[w.data_ptr() for w in chunk])
        rows = (C.c_int32 * m)(*[w.shape[0] for w in chunk])
        cols = (C.c_int32 * m)(*[w.shape[1] for w in chunk])
        _lib.check(lib.spx_simplex_project(ptrs, rows, cols, m, float(z), stream))
    torch.autograd.graph.increment_version(ws)


@torch.no_grad()
def threshold_group_projections_(ppnet, threshold: float) -> None:
    """Zero, in place, every group-projection weight below ``threshold`` (segmentation/analysis/threshold_save.py:27-28; no
    renormalisation, as upstream).  Offline, once per model: stock torch on the weights' device.  Bumps the weights' version
    counters and drops the pack cache."""
    from .functional import invalidate_pack_cache

    for gp in ppnet.group_projection:
        w = gp.weight.detach()
        w[w < float(threshold)] = 0                             # (the detached view shares the parameter's version counter)
    invalidate_pack_cache()


@torch.no_grad()
def non_zero_proto(ppnet) -> List[int]:
    """Sorted, unique bank indices of the prototypes with a non-zero weight in any group (segmentation/utils.py:140-154)."""
    used: List[int] = []
    # upstream pairs projection j with class j ('approximation': every class present); the module keeps one projection per
    # class PRESENT in the bank, in class order, which is the same pairing there and the right one after pruning
    present = ppnet._present_classes() if hasattr(ppnet, "_present_classes") else range(len(ppnet.group_projection))
    for k, gp in zip(present, ppnet.group_projection):
        proto_idx = torch.nonzero(ppnet.prototype_class_identity[:, k]).flatten().tolist()
        cols = torch.nonzero((gp.weight.detach() != 0).any(dim=0)).flatten().tolist()
        used.extend(proto_idx[c] for c in cols)
    return np.unique(np.array(used, dtype=np.int64)).tolist()


def _pil_nearest_index(n_in: int, n_out: int) -> np.ndarray:
    """Source index per output index of PIL's NEAREST resize: position (i + 0.5) * n_in / n_out, produced by
    repeated double-precision addition of the step (the accumulation order decides ties), truncated."""
    step = float(n_in) / float(n_out)
    inc = np.full(n_out, step, dtype=np.float64)
    inc[0] = 0.0 + step * 0.5
    pos = np.add.accumulate(inc)  # sequential, like the C loop
    return np.minimum(pos.astype(np.int64), n_in - 1)


def resize_label(label: np.ndarray, size) -> torch.Tensor:
    """Nearest-neighbour label resize with PIL's sampling rule (segmentation/data/dataset.py:22-30).

    size is (W, H).  The reference resizes through ``PIL.Image.resize(..., NEAREST)`` and warns that other
    nearest rules misalign labels; the rule is restated here (checked against PIL on 3000 random sizes and
    against the reference's own resize_label in tests/golden/push_argmin.npz) so the push path needs no PIL."""
    label = np.asarray(label)
    h_in, w_in = label.shape
    w_out, h_out = int(size[0]), int(size[1])
    rows = _pil_nearest_index(h_in, h_out)
    cols = _pil_nearest_index(w_in, w_out)
    return torch.from_numpy(np.ascontiguousarray(label[np.ix_(rows, cols)]).astype(np.int64))
