"""Nearest-image tables and class-restricted activation crops on the GPU (segmentation/analysis/nearest_img.py: for every
prototype the ``n`` training images whose nearest patch is closest to it, with the crops the script cuts out of them;
segmentation/analysis/nearest_proto.py:54-66: for chosen pixels the ``n`` nearest prototypes a grouping still uses).

Definitions (``u`` = an activation plane upsampled to the label size ``H x W`` by the rule of ``overlap.py``; labels 0 = void,
``k + 1`` = class ``k``; ``rf`` = the float64 patch box of ``pushbox.py``):

* masked threshold of a row ``(n, c, L)``: ``np.percentile(u[n, c][labels[n] == L], 100 q)``, numpy's linear method on the
  fp32 values: ``count`` = the number of such pixels, ``virtual = q (count - 1)``, ``k = floor(virtual)``, ``gamma`` = the
  fractional part (float64, rounded to fp32), ``T = _lerp(v[k], v[min(k + 1, count - 1)], gamma)`` in fp32; ``+inf`` when no
  pixel holds ``L`` (the reference's ``np.inf``, nearest_img.py:293-296).  ``spx_masked_thresholds`` is the exact radix select
  of the unmasked threshold restricted to the class, with the rank formed on the device: no host read.
* majority label of a patch: ``np.bincount(labels[n][rf[0]:rf[1], rf[2]:rf[3]].ravel()).argmax()`` (the slice clips the box
  to the image; the smallest label on a tie); ``patch_class = majority - 1``, so a void patch has class -1 (nearest_img.py:260-264).
* the ``_gt`` crop: the greedy crop of ``pushbox.py`` on ``u`` masked to the class, from the masked threshold of that class
  (nearest_img.py:292-300; the push uses the prototype's own class, push_multiscale_optimization.py:476-484).  With ``T = +inf``
  nothing hits and the crop is the patch box plus the margin.
* nearest images: per image the UNMASKED minimum of every prototype's distance over the latent grid (nearest_img.py:53-57), then
  per prototype the ``n`` images of smallest minimum, ascending by (distance, image index).  The reference's ``topk`` leaves
  the order among equal distances unspecified; here the earlier image comes first.
* nearest prototypes of a pixel ``(n, y, x)``: the ``n`` smallest ``distances[n, :, y, x]``, ascending by (distance, prototype);
  with ``window`` the reference's rule: the ``window = n + 10`` nearest overall, of which the included ones are kept, ``n`` at
  the most (nearest_proto.py:61-63).

The reference resizes every plane with ``cv2``, sorts a boolean-indexed copy and walks NumPy rows on the host, once per
(prototype, image), and encodes ``n * P`` images.  Here every distinct winning image is encoded once and the select and the
walk recompute a pixel from the latent plane with one function, so they see the same bits.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib, _maps
from ._lib import SpxError
from ._maps import LABEL_BYTES, strides
from .overlap import _rank, high_activation_threshold
from .pushbox import push_bounding_boxes

MAX_ROWS = 4096                # rows of one spx_masked_thresholds call
MAX_NEAREST = 64               # entries per query / per prototype
MAX_LABELS = 1024              # label values 0..K of spx_patch_majority (an LDS histogram)


def _host_table(rows, width: int, what: str) -> Optional[torch.Tensor]:
    """The int64 host copy of a row table [R, ``width``] for the caller to check, or None for a device table, which the host
    never reads."""
    if isinstance(rows, torch.Tensor) and rows.is_cuda:
        if rows.dim() != 2 or rows.shape[1] != width or rows.shape[0] < 1 or rows.is_floating_point():
            raise SpxError(f"rows must be integer [R, {width}] = {what} with R >= 1 (got {rows.dtype} {tuple(rows.shape)})")
        return None
    checked = _maps.host_rows(rows, width, what)
    if int(checked.abs().max()) >= 2 ** 31:
        raise SpxError("rows do not fit int32")
    return checked


def _upload(rows, checked: Optional[torch.Tensor], device) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(int32 rows on ``device``, their int32 host copy or None) after ``_host_table``."""
    if checked is None:
        if rows.device != device:
            raise SpxError(f"rows are on {rows.device}, the maps on {device}")
        return rows.detach().to(torch.int32).contiguous(), None
    host = checked.to(torch.int32).contiguous()
    return host.to(device), host


def high_activation_threshold_masked(activations: torch.Tensor, labels: torch.Tensor, rows, q: float = 0.95,
                                     grid: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """fp32 [R]: the class-restricted threshold of every row ``(n, c, L)`` of ``rows`` (integer [R, 3]), as the module's header
    defines it; ``+inf`` where ``labels[n]`` holds no ``L``.  ``activations`` and ``labels`` as ``push_bounding_boxes`` takes
    them.  A host table is checked before any launch (``n``, ``c`` in range, ``L >= 0``); a device table is never read by the
    host and a row out of range yields NaN.  Enqueues work on the current stream only; never synchronises."""
    lib = _lib.load()
    _rank(q, 2)
    planes = _maps.planes(activations, grid, "activations")
    N, Cn, h, w = (int(v) for v in planes.shape)
    H, W = _maps.label_map(labels, N, "activations")
    checked = _host_table(rows, 3, "(n, c, label value)")
    if checked is not None:
        n, c = checked[:, 0], checked[:, 1]
        _maps.bad_row(checked, (n < 0) | (n >= N) | (c < 0) | (c >= Cn), f"no plane of N={N}, C={Cn}")
        _maps.bad_row(checked, checked[:, 2] < 0, "a label value is not negative")
    lab = _maps.device_labels(planes, labels)
    dev_rows, host = _upload(rows, checked, planes.device)
    R = int(dev_rows.shape[0])
    out = torch.empty(R, dtype=torch.float32, device=planes.device)
    for lo in range(0, R, MAX_ROWS):
        part = min(MAX_ROWS, R - lo)
        nbytes = lib.spx_masked_workspace_bytes(part)
        if nbytes == 0:
            raise SpxError(lib.spx_last_error().decode("utf-8", "replace"))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=planes.device)
        _lib.check(lib.spx_masked_thresholds(planes.data_ptr(), strides(planes), lab.data_ptr(), LABEL_BYTES[lab.dtype],
                                             dev_rows[lo:].data_ptr(), None if host is None else host[lo:].data_ptr(), part, N, Cn, h, w,
                                             H, W, float(q), _lib.ptr(ws), out[lo:].data_ptr(), _lib.stream_ptr()))
    return out


def patch_majority(labels: torch.Tensor, rows, grid: Tuple[int, int], num_classes: int) -> torch.Tensor:
    """int32 [R] on the device: the majority label of the patch box of every row ``(n, flat latent index)`` of a latent grid
    ``grid`` = (h, w) in ``labels`` [N, H, W] (values 0..``num_classes``, at most 1024 of them).  ``patch_class`` is this
    minus one.  Rows as ``high_activation_threshold_masked`` takes them; a device row out of range yields -1."""
    lib = _lib.load()
    H, W = _maps.label_map(labels)
    N = int(labels.shape[0])
    h, w = int(grid[0]), int(grid[1])
    K = int(num_classes)
    if K < 0 or K + 1 > MAX_LABELS:
        raise SpxError(f"labels 0..{K}: at most {MAX_LABELS} label values (the histogram lives in LDS)")
    if h < 1 or w < 1:
        raise SpxError(f"grid must be positive (got {h} x {w})")
    checked = _host_table(rows, 2, "(n, flat latent index)")
    if checked is not None:
        n, f = checked[:, 0], checked[:, 1]
        _maps.bad_row(checked, (n < 0) | (n >= N) | (f < 0) | (f >= h * w), f"no patch of N={N}, grid {h} x {w}")
    _lib.require_gpu(labels, "labels")
    lab = labels.detach().contiguous()
    dev_rows, host = _upload(rows, checked, lab.device)
    R = int(dev_rows.shape[0])
    out = torch.empty(R, dtype=torch.int32, device=lab.device)
    _lib.check(lib.spx_patch_majority(lab.data_ptr(), LABEL_BYTES[lab.dtype], _lib.ptr(dev_rows), None if host is None else host.data_ptr(),
                                      R, N, h, w, H, W, K + 1, _lib.ptr(out), _lib.stream_ptr()))
    return out


def nearest_prototypes(distances: torch.Tensor, pixels, n: int = 3, include=None, window: Optional[int] = None,
                       ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(prototypes int64 [Q, n], distances fp32 [Q, n]) on the device: the ``n`` <= 64 nearest prototypes of every pixel
    ``(image, y, x)`` of ``pixels`` (integer [Q, 3]) in ``distances`` fp32 [B, P, h, w], ascending by (distance, prototype);
    missing entries are -1 / +inf.  ``include``: a bool / uint8 mask [P] or a list of prototypes (``non_zero_proto``'s); the others
    are no candidates.  ``window``: the reference's rule instead - the ``window`` nearest of all prototypes (``n + 10`` there),
    of which the included ones are kept.  Never synchronises."""
    lib = _lib.load()
    n = int(n)
    if not 1 <= n <= MAX_NEAREST:
        raise SpxError(f"n = {n} outside 1..{MAX_NEAREST}")
    if window is not None and int(window) < 1:
        raise SpxError(f"window = {window} must be positive")
    if not isinstance(distances, torch.Tensor) or distances.dim() != 4 or distances.dtype != torch.float32:
        raise SpxError("distances must be fp32 [B, P, h, w]")
    B, P, h, w = (int(v) for v in distances.shape)
    mask = None
    if include is not None:
        if isinstance(include, torch.Tensor) and include.dtype in (torch.bool, torch.uint8):
            if tuple(include.shape) != (P,):
                raise SpxError(f"an include mask must be [{P}] (got {tuple(include.shape)})")
            mask = include.to(torch.uint8)
        else:
            idx = torch.as_tensor(include, dtype=torch.int64).reshape(-1).cpu()
            if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= P):
                raise SpxError(f"include names a prototype outside 0..{P - 1}")
            mask = torch.zeros(P, dtype=torch.uint8)
            mask[idx] = 1
    checked = _host_table(pixels, 3, "(image, y, x)")
    if checked is not None:
        _maps.bad_row(checked, (checked[:, 0] < 0) | (checked[:, 0] >= B) | (checked[:, 1] < 0) | (checked[:, 1] >= h)
                      | (checked[:, 2] < 0) | (checked[:, 2] >= w), f"no pixel of B={B}, grid {h} x {w}")
    _lib.require_gpu(distances, "distances")
    d = distances.detach().contiguous()
    dev_rows, host = _upload(pixels, checked, d.device)
    if mask is not None:
        mask = mask.to(d.device).contiguous()
    Q = int(dev_rows.shape[0])
    index = torch.empty(Q, n, dtype=torch.int64, device=d.device)
    value = torch.empty(Q, n, dtype=torch.float32, device=d.device)
    _lib.check(lib.spx_nearest_protos(_lib.ptr(d), _lib.ptr(dev_rows), None if host is None else host.data_ptr(), _lib.ptr(mask), Q, B,
                                      P, h, w, n, 0 if window is None else int(window), _lib.ptr(index), _lib.ptr(value),
                                      _lib.stream_ptr()))
    return index, value


def gt_crops(act: torch.Tensor, labels: torch.Tensor, chan: torch.Tensor, flat: torch.Tensor, num_classes: int, q: float = 0.95,
             add_margin: int = 5):
    """The crop chain of one image on the device, for rows ``r`` = (channel ``chan[r]`` of ``act`` [1, U, h, w], flat latent
    index ``flat[r]``), both int32 device vectors [R]; ``labels`` [1, H, W] on the device.  Returns device tensors
    (rf int64 [R, 4], patch_class int32 [R], threshold fp32 [R], threshold_gt fp32 [R], box int64 [R, 4], box_gt int64 [R, 4]):
    the patch's majority class, the all-pixel and the class-restricted threshold and the crop grown from each on the plane
    masked to that class.  No host read."""
    R = int(chan.shape[0])
    zero = torch.zeros_like(chan)
    major = patch_majority(labels, torch.stack([zero, flat], dim=1), tuple(act.shape[2:]), num_classes)
    thr = high_activation_threshold(act, tuple(labels.shape[1:]), q)[0][chan.to(torch.int64)]
    thr_gt = high_activation_threshold_masked(act, labels, torch.stack([zero, chan, major], dim=1), q)
    rows = torch.stack([zero, chan, major - 1, flat], dim=1)
    rf, box = push_bounding_boxes(act, labels, torch.cat([rows, rows]), row_thresholds=torch.cat([thr, thr_gt]), add_margin=add_margin)
    return rf[:R], major - 1, thr, thr_gt, box[:R], box[R:]


@dataclass
class NearestImages:
    """Host tensors, rows [P, n] ascending by (distance, image); every entry of a prototype that met fewer than ``n`` images is -1.

    image         int64  dataset index
    flat          int64  flat latent index of the image's nearest patch
    distance      fp32   its distance
    rf_box        int64  [P, n, 4] patch box (h0, h1, w0, w1) in image pixels
    patch_class   int64  majority label of the patch box minus one (-1 = a void patch)
    threshold, threshold_gt   fp32   np.percentile(u, 100 q) over the image / over the patch class's pixels (+inf: no such pixel)
    bound_box, bound_box_gt   int64  [P, n, 4] the crop grown from each on the plane masked to the patch class"""

    image: torch.Tensor
    flat: torch.Tensor
    distance: torch.Tensor
    rf_box: Optional[torch.Tensor] = None
    patch_class: Optional[torch.Tensor] = None
    threshold: Optional[torch.Tensor] = None
    threshold_gt: Optional[torch.Tensor] = None
    bound_box: Optional[torch.Tensor] = None
    bound_box_gt: Optional[torch.Tensor] = None


def nearest_run_minima(net, conv: torch.Tensor) -> torch.Tensor:
    """Device step 1 of pass 1: keys int64 [B, P] (fp32 bits of the distance above, flat latent index below) of every
    prototype's unmasked minimum over each image's latent grid, taken inside the distance kernel
    (``prune_nearest_from_features`` with no void label)."""
    from .functional import prune_nearest_from_features
    from .prune import _NO_VOID

    net._check_fusable()
    B, _, H, W = conv.shape
    none = torch.zeros(B, H, W, dtype=torch.int32, device=conv.device)
    return prune_nearest_from_features(conv, net.prototype_vectors, net._layout(1), none, void_label=_NO_VOID)


def nearest_run_merge(table, keys: torch.Tensor, W: int, image0: int) -> None:
    """Device step 2 of pass 1: the keys of images image0 .. image0 + B - 1 into the running [P, n] table (spx_prune_merge).  Of
    the pruning search's footprint fields only the box matters here: the merge skips a candidate whose box is empty, so every
    candidate gets the one-pixel box (0, 1, 0, 1)."""
    B, P = keys.shape
    box = torch.tensor([0, 1, 0, 1], dtype=torch.int32, device=keys.device).expand(B, P, 4)
    table.merge(keys, torch.zeros(B, P, dtype=torch.int32, device=keys.device), box, W, image0)


def winning_image_planes(net, img: torch.Tensor, protos, device) -> torch.Tensor:
    """Device step 1 of pass 2: fp32 [1, len(protos), h, w], the activation planes of the prototypes ``protos`` on one image."""
    conv, dist = net.push_forward(img.unsqueeze(0).to(device) if img.dim() == 3 else img.to(device))
    if isinstance(conv, list):
        raise SpxError("nearest images need one feature map per image (MSC list input is not supported)")
    return net.distance_2_similarity(dist[:, torch.tensor(protos, dtype=torch.int64, device=dist.device)]).float()


def image_labels(dataset, target) -> torch.Tensor:
    """The converted target of an image as a host label map [H, W] of a dtype the kernels read."""
    from .scan import converted

    labels = torch.as_tensor(np.ascontiguousarray(converted(dataset, target)))
    if labels.dim() != 2:
        raise SpxError(f"a target must be [H, W] (got {tuple(labels.shape)})")
    if labels.dtype not in LABEL_BYTES:
        labels = labels.to(torch.int64)
    return labels


@torch.no_grad()
def nearest_images_to_prototypes(dataset, ppnet, n: int = 3, *, batch_size: int = 8, crops: bool = True, q: float = 0.95,
                                 add_margin: int = 5, image_range: Optional[range] = None) -> NearestImages:
    """For every prototype the ``n`` images whose nearest patch is closest to it and, with ``crops``, what nearest_img.py cuts
    out of each: the patch box, the patch's majority class, both thresholds and both crops (``NearestImages``; the module's
    header has the definitions).  Among equal distances the earlier image comes first (the reference's ``topk`` leaves that
    order unspecified).

    Pass 1 encodes runs of equally sized images ``batch_size`` at a time, takes every prototype's unmasked minimum inside the
    distance kernel and keeps the running [P, n] table on the device (``prune.NearestTable``); one device-to-host copy brings
    it.  Pass 2 encodes every distinct winning image once, applies ``distance_2_similarity`` on the channels its rows name,
    uploads its labels once and runs the crop chain (``gt_crops``) without a host read; one more copy brings the results.
    Dataset protocol as ``push_prototypes_multiscale``."""
    from .prune import NearestTable, _unpack
    from .push import _by_winning_image
    from .scan import batches, encode_run, scan_range, unwrap

    net = unwrap(ppnet)
    n = int(n)
    if not 1 <= n <= MAX_NEAREST:
        raise SpxError(f"n = {n} outside 1..{MAX_NEAREST}")
    if int(batch_size) < 1:
        raise SpxError(f"batch_size = {batch_size} must be positive")
    _rank(q, 2)
    if getattr(net, "scale_head", None) is not None:
        net._refuse_scale_head("nearest_images_to_prototypes")
    net.eval()
    dev = torch.device(str(net.prototype_vectors.device))
    P = net.num_prototypes
    table = NearestTable(P, n, dev)
    width = {}
    for run in batches(dataset, scan_range(dataset, image_range=image_range), int(batch_size)):
        conv, _ = encode_run(net, dataset, run, dev, "nearest images need one feature map per image (MSC list input is not supported)")
        conv = conv.detach().contiguous()
        nearest_run_merge(table, nearest_run_minima(net, conv), int(conv.shape[3]), run[0][0])
        width.update({i: int(conv.shape[3]) for i, _, _ in run})             # latent row length of every image, for `flat`
    found = _unpack(table.packed().cpu())                                    # pass 1's one device-to-host copy
    image = found.image
    out = NearestImages(image=image, flat=torch.full((P, n), -1, dtype=torch.int64),
                        distance=torch.where(image >= 0, found.distance, torch.full_like(found.distance, -1.0)))
    slots = [(p, j) for p in range(P) for j in range(n) if int(image[p, j]) >= 0]
    by_image = _by_winning_image([int(image[p, j]) for p, j in slots])       # image -> positions in `slots`
    if crops:
        out.rf_box = torch.full((P, n, 4), -1, dtype=torch.int64)
        out.bound_box = torch.full((P, n, 4), -1, dtype=torch.int64)
        out.bound_box_gt = torch.full((P, n, 4), -1, dtype=torch.int64)
        out.patch_class = torch.full((P, n), -1, dtype=torch.int64)
        out.threshold = torch.full((P, n), -1.0, dtype=torch.float32)
        out.threshold_gt = torch.full((P, n), -1.0, dtype=torch.float32)
    order, parts = [], []
    for i, members in sorted(by_image.items()):
        rows = [slots[m] for m in members]
        flat = [int(found.latent[p, j, 0]) * width[i] + int(found.latent[p, j, 1]) for p, j in rows]
        for (p, j), f in zip(rows, flat):
            out.flat[p, j] = f
        if not crops:
            continue
        img, target = dataset[i]
        protos = sorted({p for p, _ in rows})
        col = {p: c for c, p in enumerate(protos)}
        act = winning_image_planes(net, img, protos, dev)
        labels = image_labels(dataset, target).unsqueeze(0).to(dev)           # the image's one label upload
        table_rows = torch.tensor([[col[p], f] for (p, _), f in zip(rows, flat)], dtype=torch.int32).to(dev)
        rf, cls, thr, thr_gt, box, box_gt = gt_crops(act, labels, table_rows[:, 0].contiguous(), table_rows[:, 1].contiguous(),
                                                     net.num_classes, q, add_margin)
        order += rows
        parts.append(torch.cat([rf, box, box_gt, cls.to(torch.int64)[:, None], thr.view(torch.int32).to(torch.int64)[:, None],
                                thr_gt.view(torch.int32).to(torch.int64)[:, None]], dim=1))
    if crops and parts:
        got = torch.cat(parts, dim=0).cpu()                                  # pass 2's one device-to-host copy, [rows, 15]
        for r, (p, j) in enumerate(order):
            out.rf_box[p, j], out.bound_box[p, j], out.bound_box_gt[p, j] = got[r, 0:4], got[r, 4:8], got[r, 8:12]
            out.patch_class[p, j] = got[r, 12]
        pj = torch.tensor(order, dtype=torch.int64)
        out.threshold[pj[:, 0], pj[:, 1]] = got[:, 13].to(torch.int32).view(torch.float32)
        out.threshold_gt[pj[:, 0], pj[:, 1]] = got[:, 14].to(torch.int32).view(torch.float32)
    return out
