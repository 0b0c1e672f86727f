"""Bounding boxes of pushed prototypes on the GPU (segmentation/push_multiscale_optimization.py:416-497, the greedy crop
helpers.py:53-87): the ``proto_rf_boxes`` / ``proto_bound_boxes`` tables every "what does this prototype look like" step reads.

Definition, per row ``(n, c, k, f)`` = activation plane ``a[n, c]`` (fp32, latent grid ``h x w``), the prototype's class ``k``, the
flat latent index ``f`` of the pushed patch; labels ``y[n]`` of size ``H x W`` (0 = void, ``k + 1`` = class ``k``):

* patch box, in Python's float64: ``ph = H / h``, ``pw = W / w``, ``i = f // w``, ``j = f % w``,
  ``rf = [int(i*ph), int(i*ph + ph) + 1, int(j*pw), int(j*pw + pw) + 1]``; the ends may exceed ``H`` or ``W`` (the reference's
  behaviour) and are stored as they are.
* ``u`` = the plane upsampled to ``H x W`` by the rule of ``overlap.py``; ``T = np.percentile(u, 95)`` over the whole image
  = ``high_activation_threshold(q=0.95)``.
* ``hit = v >= T`` with ``v = u`` where ``y == k + 1`` and 0 elsewhere (non-strict, unlike the overlap masks; with ``T <= 0``
  every pixel outside the class is a hit).
* greedy crop from ``(sh, eh, sw, ew) = rf`` with four sticky ``stopped`` flags, until all four are set; a pass does, in this
  order and each step on the box as the step before left it:
  0. not stopped[0], ``sh > 0`` and a hit in row ``sh - 1``, columns ``sw..ew`` (inclusive, clipped to the image): ``sh -= 1``,
     else stopped[0];  1. the same below: ``eh < H - 1``, row ``eh + 1``: ``eh += 1``, else stopped[1];
  2. ``sw > 0`` and a hit in column ``sw - 1``, rows ``sh..eh``: ``sw -= 1``, else stopped[2];  3. ``ew < W - 1``, column
  ``ew + 1``: ``ew += 1``, else stopped[3].  Then ``box = (max(sh - m, 0), min(eh + m, H - 1) + 1, max(sw - m, 0),
  min(ew + m, W - 1) + 1)`` with ``m = add_margin``.

The reference resizes, sorts and walks NumPy rows on the host once per prototype.  Here ``spx_push_boxes`` walks the same
steps with one workgroup per row on values recomputed from the latent plane (the function the threshold select uses, so the
two agree on every pixel); the ``[H, W]`` map is never written.

The class-restricted crop (the reference's ``threshold_gt`` / ``_gt`` crop, :476-484) is the same walk from a threshold of the
row's own: ``row_thresholds=`` (``spx_push_boxes_rows``), selected by ``nearest.high_activation_threshold_masked``.

Not built: every image and plot dump, and boxes under a sharded (``torch.distributed``) push.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib, _maps
from ._lib import SpxError
from ._maps import LABEL_BYTES, strides
from .overlap import _rank, _thresholds, _workspace

_MAX_SELECT_PLANES = 4096       # channels of one spx_overlap_thresholds call


def _select_for(lib, planes: torch.Tensor, pairs: torch.Tensor, size, q: float) -> torch.Tensor:
    """fp32 [N, C] thresholds, selected for the planes ``pairs`` ([U, 2] device int64 = (n, c)) names and NaN elsewhere."""
    N, Cn = int(planes.shape[0]), int(planes.shape[1])
    out = torch.full((N, Cn), float("nan"), dtype=torch.float32, device=planes.device)
    for lo in range(0, int(pairs.shape[0]), _MAX_SELECT_PLANES):
        part = pairs[lo:lo + _MAX_SELECT_PLANES]
        named = planes[part[:, 0], part[:, 1]].unsqueeze(0)                      # [1, U', h, w], a copy of the named planes
        thr = _thresholds(lib, named, size, q, _workspace(lib, 1, int(named.shape[1]), 1, planes.device))
        out.index_put_((part[:, 0], part[:, 1]), thr[0])
    return out


def push_bounding_boxes(activations: torch.Tensor, labels: torch.Tensor, rows: torch.Tensor, *, thresholds: Optional[torch.Tensor] = None,
                        q: float = 0.95, add_margin: int = 5, grid: Optional[Tuple[int, int]] = None,
                        row_thresholds: Optional[torch.Tensor] = None):
    """(rf_boxes, bound_boxes), int64 [R, 4] device tensors ``(h0, h1, w0, w1)`` with exclusive ends, as the module's header
    defines them.

    ``activations``: fp32 [N, C, h, w] with any strides, or pixel-major [M, C] with ``grid`` = (h, w).  ``labels``: [N, H, W]
    uint8 / int32 / int64 on the device; its shape is the image size.  ``rows``: integer [R, 4] = (n, c, class, flat latent
    index).  A host tensor is checked on the host (a row out of range raises) and uploaded; a device tensor is never read by
    the host, and a row out of range comes back as -1.  ``thresholds``: fp32 [N, C] as ``high_activation_threshold`` returns
    them; None selects them at ``q`` for exactly the planes the rows name.  ``row_thresholds``: fp32 [R], one threshold per row
    instead (``thresholds`` must then be None); only with it may a row name class -1, which masks on label 0 as the reference
    does for a patch whose majority label is void, and a ``+inf`` entry leaves the crop at the patch box plus the margin.
    Enqueues work on the current stream only; never synchronises."""
    lib = _lib.load()
    _rank(q, 2)
    if thresholds is not None and row_thresholds is not None:
        raise SpxError("pass thresholds= ([N, C]) or row_thresholds= ([R]), not both")
    planes = _maps.planes(activations, grid, "activations")
    N, Cn, h, w = (int(v) for v in planes.shape)
    H, W = _maps.label_map(labels, N, "activations")
    host_rows = None
    if isinstance(rows, torch.Tensor) and rows.is_cuda:
        if rows.dim() != 2 or rows.shape[1] != 4 or rows.shape[0] < 1 or rows.is_floating_point():
            raise SpxError(f"rows must be integer [R, 4] with R >= 1 (got {rows.dtype} {tuple(rows.shape)})")
    else:
        rows = _maps.host_rows(rows, 4, "(n, c, class, flat latent index)")
        host_rows = rows.to(torch.int32).contiguous()
        if not torch.equal(host_rows.to(torch.int64), rows):
            raise SpxError("rows do not fit int32")
        if row_thresholds is None:
            _maps.bad_row(rows, rows[:, 2] < 0, "class -1 (a void patch) needs row_thresholds=")
        if thresholds is None and row_thresholds is None:      # the select below reads the planes the rows name
            n, c = rows[:, 0], rows[:, 1]
            _maps.bad_row(rows, (n < 0) | (n >= N) | (c < 0) | (c >= Cn), f"no plane of N={N}, C={Cn}")
    R = int(rows.shape[0])
    lab = _maps.device_labels(planes, labels)
    if host_rows is not None:
        dev_rows = host_rows.to(planes.device)
    else:
        if rows.device != planes.device:
            raise SpxError(f"rows are on {rows.device}, activations on {planes.device}")
        dev_rows = rows.detach().to(torch.int32).contiguous()
    if row_thresholds is not None:
        _lib.require_gpu(row_thresholds, "row_thresholds")
        if row_thresholds.dtype != torch.float32 or tuple(row_thresholds.shape) != (R,) or row_thresholds.device != planes.device:
            raise SpxError(f"row_thresholds must be fp32 [{R}] on {planes.device}")
        thresholds = row_thresholds.detach().contiguous()
    elif thresholds is None:
        if host_rows is not None:
            pairs = torch.unique(rows[:, :2], dim=0).to(planes.device)
        else:                                      # no host read: one select per row, rows out of range fold onto plane (0, 0)
            pairs = dev_rows[:, :2].to(torch.int64)
            ok = (pairs[:, 0] >= 0) & (pairs[:, 0] < N) & (pairs[:, 1] >= 0) & (pairs[:, 1] < Cn)
            pairs = pairs * ok.unsqueeze(1)
        thresholds = _select_for(lib, planes, pairs, (H, W), q)
    else:
        _lib.require_gpu(thresholds, "thresholds")
        if thresholds.dtype != torch.float32 or tuple(thresholds.shape) != (N, Cn) or thresholds.device != planes.device:
            raise SpxError(f"thresholds must be fp32 [{N}, {Cn}] on {planes.device}")
        thresholds = thresholds.detach().contiguous()
    rf = torch.empty(R, 4, dtype=torch.int32, device=planes.device)
    box = torch.empty(R, 4, dtype=torch.int32, device=planes.device)
    entry = lib.spx_push_boxes if row_thresholds is None else lib.spx_push_boxes_rows
    _lib.check(entry(planes.data_ptr(), strides(planes), lab.data_ptr(), LABEL_BYTES[lab.dtype],
                     _lib.ptr(dev_rows), None if host_rows is None else host_rows.data_ptr(), _lib.ptr(thresholds), R, N,
                     Cn, h, w, H, W, int(add_margin), _lib.ptr(rf), _lib.ptr(box), _lib.stream_ptr()))
    return rf.to(torch.int64), box.to(torch.int64)
