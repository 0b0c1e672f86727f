"""Prototype push on the MI355X kernels.

Mirrors the numerical part of segmentation/push_multiscale_optimization.py (lines 34-190 and 323-335):
``compute_distances`` -> ``min_across_dataset`` -> ``global_min`` -> commit + de-dup.  Of the plotting half
(``update_prototypes_on_image``, :341-685) the two integer tables ``proto_rf_boxes`` / ``proto_bound_boxes`` are computed
(``push_box_tables``, the kernel behind ``pushbox.push_bounding_boxes``), and on request the crop from the class-restricted
threshold ``threshold_gt`` (:476-484, which the reference cuts a PNG from and never stores); every image and plot dump is
visualisation and is not part of this package.

``push_prototypes_multiscale(batch_size=...)`` runs the same push in ONE pass over the data set (``push_single_pass``): images
are encoded in batches and a ``PushTable`` on the device keeps every prototype's running winner and its feature vector
(spx_push_merge), so no image is encoded twice and the loop never synchronises.

Dataset protocol (image decoding / normalisation is the data layer, out of scope): ``len(dataset)`` and
``dataset[i] -> (image, target)`` with ``image`` a normalised float tensor [3, h, w] and ``target`` an
integer label map [h, w] (0 = void, 1..K), optionally ``dataset.convert_targets``.  For the box tables the target's own
shape is the image size ``(H, W)`` the boxes are expressed in (the reference reads it from the annotation file, :385-404).
"""
from __future__ import annotations

import json
import os
import time
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import SpxError
from .functional import argmin_over_images, push_masked_argmin, push_merge
from .scan import batches, converted, dp_world as _dp_world, encode_run, image_batch, scan_range, unwrap
from .utils import resize_label


@torch.no_grad()
def compute_distances(
    ppnet,
    dataset,
    img: torch.Tensor,
    target: np.ndarray,
    num_classes: int,
    max_dist: float = 1e10,
    device: Optional[str] = None,
    void_class: Optional[int] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-prototype class-masked minimum over one image -> (indices int64 [1,P], values f32 [1,P]).

    Same contract as push_multiscale_optimization.py:34-91; the one_hot / matmul / masked add / two min()
    passes are one HIP reduction (spx_push_argmin)."""
    device = device or str(ppnet.prototype_vectors.device)
    ppnet.eval()
    x = image_batch(img, device)
    target = converted(dataset, target)
    fused = getattr(ppnet, "push_min_distances", None)
    if fused is not None:
        # the minimum is taken inside the distance kernel: the [1, P, H, W] map is never written (spx_dist_push_min)
        out = fused(x, lambda hw: resize_label(np.asarray(target), (hw[1], hw[0])).unsqueeze(0), void_class=void_class,
                    max_dist=max_dist)
        if out is not None:
            return out
    _, distances = ppnet(x, return_activations=False)
    lab = resize_label(np.asarray(target), (distances.shape[3], distances.shape[2])).unsqueeze(0)
    return push_masked_argmin(
        distances, lab, ppnet.prototype_class_identity, void_class=void_class, max_dist=max_dist
    )


def min_across_dataset(
    dataset,
    ppnet,
    num_classes: int,
    void_class: Optional[int] = None,
    device: Optional[str] = None,
    image_range: Optional[range] = None,
    return_values: bool = False,
):
    """(best image per prototype int64 [P], per-image flat indices) — push_multiscale_optimization.py:94-137.

    ``image_range`` restricts the scan to a shard of the image list (data-parallel push, see dp.py); the
    returned image ids are then positions inside the shard.  ``return_values=True`` appends the per-image minima
    ([n_images, P] fp32) the sharded reduction needs."""
    list_idx, list_val = [], []
    for i in scan_range(dataset, image_range=image_range):
        img, target = dataset[i]
        idx, val = compute_distances(ppnet, dataset, img, target, num_classes, void_class=void_class, device=device)
        list_idx.append(idx)
        list_val.append(val)
    tot = torch.cat(list_val, dim=0)
    best = argmin_over_images(tot)
    return (best, list_idx, tot) if return_values else (best, list_idx)


def _winners(best, list_min_patch: Optional[Sequence[torch.Tensor]], flat=None) -> torch.Tensor:
    """int64 [2, P]: the winners' images and flat latent indices; the latter as given, else ``list_min_patch[best[p]][0, p]``."""
    if flat is None:
        tot = torch.cat(list(list_min_patch), dim=0)
        best = torch.as_tensor(best).to(tot.device)
        flat = tot[best, torch.arange(tot.shape[1], device=tot.device)]
    flat = torch.as_tensor(flat).to(torch.int64)
    return torch.stack([torch.as_tensor(best).to(device=flat.device, dtype=torch.int64), flat])


def _by_winning_image(best: Sequence[int], only: Optional[Sequence[bool]] = None) -> Dict[int, List[int]]:
    """Winning image -> its prototypes in increasing order (those outside ``only`` left out), images as first met."""
    by_image: Dict[int, List[int]] = {}
    for p, i in enumerate(best):
        if only is None or only[p]:
            by_image.setdefault(int(i), []).append(p)
    return by_image


@torch.no_grad()
def _winning_patches(best: Sequence[int], flat: Sequence[int], dataset, ppnet, device, image_offset: int = 0,
                     only: Optional[Sequence[bool]] = None) -> torch.Tensor:
    """[P, Cs] feature vectors of the winning latent pixels (rows outside ``only`` stay zero); ``best`` / ``flat`` are the
    winners' images and flat indices as host integers.  Each winning image is encoded once, the reference
    re-runs the backbone once per prototype."""
    P, S = ppnet.num_prototypes, ppnet.num_scales
    out = torch.zeros((P, int(ppnet.prototype_shape[1])), dtype=torch.float32, device=device)
    for i, protos in _by_winning_image(best, only).items():
        conv = ppnet.conv_features(image_batch(dataset[image_offset + i][0], device))
        _, C, H, W = conv.shape
        cv = conv.view(S, C // S, H, W)
        for p in protos:
            out[p] = cv[p // (P // S), :, flat[p] // W, flat[p] % W].detach().float()
    return out


@torch.no_grad()
def global_min(
    proto_min_dist: torch.Tensor,
    list_min_patch: Sequence[torch.Tensor],
    dataset,
    ppnet,
    device: Optional[str] = None,
    image_offset: int = 0,
) -> List[np.ndarray]:
    """Feature vector [Cs,1,1] of every prototype's winning latent pixel (push_multiscale_optimization.py:140-190)."""
    device = device or str(ppnet.prototype_vectors.device)
    best, flat = _winners(proto_min_dist, list_min_patch).tolist()       # the one device-to-host copy of the winners
    rows = _winning_patches(best, flat, dataset, ppnet, device, image_offset).cpu().numpy()
    return [rows[p].reshape(-1, 1, 1) for p in range(rows.shape[0])]


def commit_push(ppnet, patches: Sequence[np.ndarray], root_dir: Optional[os.PathLike] = None, log: Callable = print):
    """Overwrite the bank with the pushed patches and drop exact duplicates
    (push_multiscale_optimization.py:323-335; prune semantics model_multiscale.py:400-432)."""
    shape = tuple(ppnet.prototype_shape)
    update = np.reshape(patches, shape)
    ppnet.prototype_vectors.data.copy_(torch.tensor(update, dtype=torch.float32).to(ppnet.prototype_vectors.device))
    from .functional import invalidate_pack_cache

    invalidate_pack_cache()                  # (an in-place write through .data is invisible to the parameter's version counter)
    _, unique_index = np.unique(update, axis=0, return_index=True)
    keep = set(int(i) for i in unique_index)
    dup = [i for i in range(ppnet.num_prototypes) if i not in keep]
    log(f"Removing {len(dup)} duplicate prototypes.")
    ppnet.prune_prototypes(dup)
    if root_dir is not None:
        os.makedirs(root_dir, exist_ok=True)
        with open(os.path.join(root_dir, "unique_prototypes.json"), "w") as fp:
            json.dump([int(i) for i in sorted(unique_index)], fp)
    return dup


def _winners_to_host(image: torch.Tensor, flat: torch.Tensor, patch: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(image int64 [P], flat int64 [P], patch fp32 [P, Cs]) on the host, in ONE device-to-host copy."""
    P = image.shape[0]
    words = torch.cat([image.view(torch.int32), flat.view(torch.int32), patch.view(torch.int32).reshape(-1)]).cpu()
    return words[: 2 * P].view(torch.int64), words[2 * P : 4 * P].view(torch.int64), words[4 * P :].view(torch.float32).reshape(patch.shape)


class PushTable:
    """The running winner of every prototype on the device (spx_push_merge), the push's counterpart of ``prune.NearestTable``:
    ``best_value`` fp32 [P] (+inf = nothing merged), ``best_image`` int64 [P] (global image index, -1), ``best_flat`` int64 [P]
    (flat latent index) and ``best_patch`` fp32 [P, Cs] (the winner's feature vector, gathered while its image's features were
    on the device).  Batches are merged in increasing image order; a later image replaces the winner only with a strictly
    smaller value, so the final state is ``argmin(dim=0)`` over all images with the lowest image on ties."""

    def __init__(self, P: int, Cs: int, device):
        if int(P) < 1 or int(Cs) < 1:
            raise SpxError(f"a push table needs P >= 1 and Cs >= 1 (got P={P}, Cs={Cs})")
        self.P, self.Cs = int(P), int(Cs)
        self.best_value = torch.full((self.P,), float("inf"), dtype=torch.float32, device=device)
        self.best_image = torch.full((self.P,), -1, dtype=torch.int64, device=device)
        self.best_flat = torch.zeros((self.P,), dtype=torch.int64, device=device)
        self.best_patch = torch.zeros((self.P, self.Cs), dtype=torch.float32, device=device)
        self.next_image = 0                                   # host side: the first image index a later batch may start at

    def check(self, idx: torch.Tensor, val: torch.Tensor, conv: torch.Tensor, proto_scale: torch.Tensor, image0: int) -> int:
        """Shapes, dtypes, contiguity and image order of one batch (host integers only, no sync).  Returns B."""
        if val.dim() != 2 or val.shape[1] != self.P:
            raise SpxError(f"candidates for {tuple(val.shape)[-1] if val.dim() else 0} prototypes, table holds {self.P}")
        B = int(val.shape[0])
        if B < 1 or tuple(idx.shape) != (B, self.P):
            raise SpxError(f"indices {tuple(idx.shape)} / values {tuple(val.shape)} must both be [B >= 1, {self.P}]")
        if idx.dtype != torch.int64 or val.dtype != torch.float32:
            raise SpxError(f"indices must be int64 and values float32 (got {idx.dtype}, {val.dtype})")
        if conv.dim() != 4 or conv.shape[0] != B or conv.dtype not in (torch.bfloat16, torch.float32):
            raise SpxError(f"features must be bfloat16 or float32 [{B}, C, H, W], got {conv.dtype} {tuple(conv.shape)}")
        if conv.shape[1] < self.Cs or conv.shape[2] * conv.shape[3] < 1:
            raise SpxError(f"features {tuple(conv.shape)} hold no block of {self.Cs} channels / no pixel")
        if tuple(proto_scale.shape) != (self.P,) or proto_scale.dtype != torch.int32:
            raise SpxError(f"proto_scale must be int32 [{self.P}], got {proto_scale.dtype} {tuple(proto_scale.shape)}")
        for name, t in (("indices", idx), ("values", val), ("features", conv), ("proto_scale", proto_scale)):
            if not t.is_contiguous():
                raise SpxError(f"{name} must be contiguous")
        if int(image0) < self.next_image:
            raise SpxError(f"batches must arrive in increasing image order: image0 = {int(image0)} after image {self.next_image - 1}")
        return B

    def merge(self, idx: torch.Tensor, val: torch.Tensor, conv: torch.Tensor, proto_scale: torch.Tensor, image0: int) -> None:
        """Merge the minima ``idx`` / ``val`` [B, P] of images image0 .. image0 + B - 1 and gather the new winners' feature
        vectors from ``conv`` [B, C, H, W]; ``proto_scale`` int32 [P] = the channel block of every prototype."""
        B = self.check(idx, val, conv, proto_scale, image0)
        for name, t in (("indices", idx), ("values", val), ("features", conv), ("proto_scale", proto_scale),
                        ("the push table", self.best_value)):
            _lib.require_gpu(t, name)
        push_merge(idx, val, conv, proto_scale, int(image0), self.best_value, self.best_image, self.best_flat, self.best_patch)
        self.next_image = int(image0) + B

    def to_host(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(best_image int64 [P], best_flat int64 [P], best_patch fp32 [P, Cs]) on the host, in ONE device-to-host copy."""
        return _winners_to_host(self.best_image, self.best_flat, self.best_patch)


def proto_scale_table(P: int, S: int) -> List[int]:
    """Channel block of every prototype by the reference's rule ``p // (P // S)`` (push_multiscale_optimization.py:166).  When S
    does not divide P the rule names blocks that do not exist: refused here, before any image is encoded."""
    if S < 1 or P < S:
        raise SpxError(f"{P} prototypes cannot be spread over {S} scales")
    table = [p // (P // S) for p in range(P)]
    if table[-1] >= S:
        raise SpxError(f"the push's rule p // (P // S) puts prototype {P - 1} in channel block {table[-1]} of {S}: "
                       f"{P} prototypes are not a multiple of {S} scales")
    return table


def push_run_minima(net, conv: torch.Tensor, labels: torch.Tensor, void_class: Optional[int], max_dist: float = 1e10):
    """Device step 1 of the single-pass push: (indices int64 [B, P], values fp32 [B, P]) of a run's class-masked minima, taken
    inside the distance kernel (the cached keys of ``push_min_distances``); a class identity that is not one-hot takes the
    written map and ``push_masked_argmin``, as ``compute_distances`` does."""
    out = net.push_min_from_conv(conv, lambda hw: labels, void_class=void_class, max_dist=max_dist)
    if out is not None:
        return out
    _, distances = net.forward_from_conv_features(conv, return_activations=False)
    return push_masked_argmin(distances, labels, net.prototype_class_identity, void_class=void_class, max_dist=max_dist)


def push_run_merge(table: PushTable, idx: torch.Tensor, val: torch.Tensor, conv: torch.Tensor, proto_scale: torch.Tensor,
                   image0: int) -> None:
    """Device step 2 of the single-pass push: one ``PushTable.merge``."""
    table.merge(idx, val, conv, proto_scale, image0)


@torch.no_grad()
def push_single_pass(dataset, ppnet, batch_size: int = 8, void_class: Optional[int] = 0, image_range: Optional[range] = None,
                     device: Optional[str] = None) -> PushTable:
    """The push's scan in one pass over ``image_range`` (default: the whole data set): runs of consecutive, equally sized
    images (``scan.batches``) are encoded ``batch_size`` at a time, their minima are taken inside the distance kernel and
    merged into a ``PushTable`` together with the winners' feature vectors - no [N, P] value table, no per-image index list,
    no second encoding of the winning images, no host sync inside the loop.  Image indices in the table are GLOBAL dataset
    indices."""
    net = unwrap(ppnet)
    if int(batch_size) < 1:
        raise SpxError(f"batch_size = {batch_size} must be positive")
    if getattr(net, "scale_head", None) is not None:
        net._refuse_scale_head("the single-pass push (batch_size=)")
    net.eval()
    dev = torch.device(device or str(net.prototype_vectors.device))
    P, S, Cs = net.num_prototypes, net.num_scales, int(net.prototype_shape[1])
    proto_scale = torch.tensor(proto_scale_table(P, S), dtype=torch.int32).to(dev)
    table = PushTable(P, Cs, dev)
    for run in batches(dataset, scan_range(dataset, image_range=image_range), int(batch_size)):
        conv, targets = encode_run(net, dataset, run, dev,
                                   "the single-pass push needs one feature map per image (MSC list input is not supported)")
        if conv.dim() != 4 or conv.shape[1] != S * Cs:
            raise SpxError(f"features {tuple(conv.shape)} are not [B, {S} x {Cs}, H, W]")
        conv = conv.detach().contiguous()
        labels = torch.stack([resize_label(t, (conv.shape[3], conv.shape[2])) for t in targets])
        idx, val = push_run_minima(net, conv, labels, void_class)
        push_run_merge(table, idx, val, conv, proto_scale, run[0][0])
    return table


@torch.no_grad()
def push_box_tables(best: torch.Tensor, list_min_patch: Optional[Sequence[torch.Tensor]], dataset, ppnet,
                    device: Optional[str] = None, q: float = 0.95, add_margin: int = 5,
                    flat: Optional[torch.Tensor] = None, gt_boxes: bool = False) -> Tuple[np.ndarray, ...]:
    """(proto_rf_boxes, proto_bound_boxes), int64 [P, 6] = [image index, h0, h1, w0, w1, class] of every prototype's winning
    patch (push_multiscale_optimization.py:254-321, 416-497), on the model as it is BEFORE the bank is overwritten.

    The winners' images and flat indices come to the host in one copy; each winning image is encoded once and its labels are
    uploaded once (the reference re-runs the backbone once per prototype); ``distance_2_similarity`` runs on the channels of
    that image's winners only; the thresholds and the crops are ``pushbox.push_bounding_boxes``.

    ``flat`` (int64 [P], the winners' flat latent indices, as the single-pass push keeps them) replaces the per-image index
    list ``list_min_patch``, which may then be None.

    ``gt_boxes=True`` appends ``proto_bound_boxes_gt``, the same table with every crop grown from the threshold over the pixels
    of the prototype's own class only (:476-484; ``nearest.high_activation_threshold_masked`` with ``L = class + 1``), from the
    activations already at hand."""
    from .metrics import prototype_classes
    from .nearest import high_activation_threshold_masked
    from .pushbox import push_bounding_boxes

    device = device or str(ppnet.prototype_vectors.device)
    P = ppnet.num_prototypes
    img_of, flat_of = _winners(best, list_min_patch, flat).tolist()      # the one device-to-host copy of the winners
    cls_of = prototype_classes(ppnet.prototype_class_identity).tolist()
    order, parts = [], []
    for i, protos in sorted(_by_winning_image(img_of).items()):
        img, target = dataset[i]
        conv, dist = ppnet.push_forward(image_batch(img, device))
        if isinstance(conv, list):
            raise SpxError("push boxes need one feature map per image (MSC list input is not supported)")
        chans = torch.tensor(protos, dtype=torch.int64, device=dist.device)
        act = ppnet.distance_2_similarity(dist[:, chans]).float()            # [1, winners of this image, h, w]
        labels = torch.as_tensor(np.ascontiguousarray(converted(dataset, target)))
        if labels.dim() != 2:
            raise SpxError(f"target of image {i} must be [H, W] (got {tuple(labels.shape)})")
        if labels.dtype not in (torch.uint8, torch.int32, torch.int64):
            labels = labels.to(torch.int64)
        rows = torch.tensor([[0, j, cls_of[p], int(flat_of[p])] for j, p in enumerate(protos)], dtype=torch.int32)
        labels = labels.unsqueeze(0).to(device)
        rf, box = push_bounding_boxes(act, labels, rows, q=q, add_margin=add_margin)
        order += protos
        if gt_boxes:
            masked = rows[:, :3].clone()
            masked[:, 2] += 1
            thr_gt = high_activation_threshold_masked(act, labels, masked, q)
            parts.append(torch.cat([rf, box, push_bounding_boxes(act, labels, rows, row_thresholds=thr_gt, add_margin=add_margin)[1]], dim=1))
        else:
            parts.append(torch.cat([rf, box], dim=1))
    got = torch.cat(parts, dim=0).cpu().numpy()                              # [P, 8 or 12] in `order`
    proto_rf_boxes = np.full((P, 6), -1, dtype=np.int64)
    proto_bound_boxes = np.full((P, 6), -1, dtype=np.int64)
    for r, p in enumerate(order):
        proto_rf_boxes[p] = [img_of[p], *got[r, :4], cls_of[p]]
        proto_bound_boxes[p] = [img_of[p], *got[r, 4:8], cls_of[p]]
    if gt_boxes:
        proto_bound_boxes_gt = np.full((P, 6), -1, dtype=np.int64)
        for r, p in enumerate(order):
            proto_bound_boxes_gt[p] = [img_of[p], *got[r, 8:12], cls_of[p]]
        return proto_rf_boxes, proto_bound_boxes, proto_bound_boxes_gt
    return proto_rf_boxes, proto_bound_boxes


def save_box_tables(proto_rf_boxes: np.ndarray, proto_bound_boxes: np.ndarray, root_dir: os.PathLike, prefix: str,
                    epoch_number: int) -> Tuple[str, str]:
    """The reference's two files (push_multiscale_optimization.py:275-279, 311-321): ``<root>/epoch-<n>/<prefix>-receptive_field<n>.npy``
    and ``<root>/epoch-<n>/<prefix><n>.npy``."""
    epoch_dir = os.path.join(root_dir, "epoch-" + str(epoch_number))
    os.makedirs(epoch_dir, exist_ok=True)
    rf_path = os.path.join(epoch_dir, prefix + "-receptive_field" + str(epoch_number) + ".npy")
    box_path = os.path.join(epoch_dir, prefix + str(epoch_number) + ".npy")
    np.save(rf_path, proto_rf_boxes)
    np.save(box_path, proto_bound_boxes)
    return rf_path, box_path


def _two_pass_candidates(dataset, net, rng: range, device, world: int):
    """The two-pass scan of ``rng``: ((best image as a GLOBAL index, its value, its flat index), each [P], and the per-image
    index list)."""
    if len(rng) == 0 and world > 1:                                    # more ranks than images: this rank never wins
        zero = torch.zeros(net.num_prototypes, dtype=torch.int64, device=device)
        return (zero, torch.full_like(zero, float("inf"), dtype=torch.float32), zero), []
    # (an empty data set at one rank fails in min_across_dataset, as it always has)
    best, tot_idx, tot_val = min_across_dataset(dataset, net, net.num_classes, void_class=0, device=device, image_range=rng,
                                                return_values=True)     # tot_val: [n_local, P]
    return (best + rng.start, tot_val[best, torch.arange(tot_val.shape[1], device=tot_val.device)], _winners(best, tot_idx)[1]), tot_idx


def push_prototypes_multiscale(
    dataset,
    prototype_network_parallel,
    root_dir_for_saving_prototypes: Optional[os.PathLike] = None,
    log: Callable = print,
    device: Optional[str] = None,
    group=None,
    boxes: bool = False,
    epoch_number: Optional[int] = None,
    proto_bound_boxes_filename_prefix: Optional[str] = None,
    batch_size: Optional[int] = None,
    gt_boxes: bool = False,
    **_ignored,
):
    """Numerical part of push_multiscale_optimization.py:193-338 (the image / plot dump arguments are accepted and ignored).
    Returns (best image per prototype [P] as GLOBAL image indices, this rank's per-image flat indices, dropped duplicates).

    One flow for every form: this rank's shard of the image list (``dp.shard_range``; all of it at one rank, the reference's
    case) is scanned into one candidate per prototype, the candidates are combined with one all-gather and a lexicographic
    minimum on (value, global image index) - the reference's lowest-image tie-break (:137) - the winning feature vectors are
    assembled with one sum all-reduce (each row has exactly one contributor; both collectives hand back their input at one
    rank), and EVERY rank commits the same bank, de-dup and pruning; rank 0 alone writes ``unique_prototypes.json``.  The
    data-parallel form is new capability (SURVEY.md 8e "Push").

    ``batch_size=None`` scans in the reference's two passes (``min_across_dataset``, then the winning images once more).  An
    integer runs the single-pass scan (``push_single_pass``): runs of equally sized images are encoded ``batch_size`` at a time,
    every image exactly once, the winners and their feature vectors are kept in a ``PushTable`` on the device, and one
    device-to-host copy brings them for the commit.  The second entry of the result is then the winners' flat latent indices,
    int64 [P], instead of the per-image index list.

    With ``boxes=True``, or when ``proto_bound_boxes_filename_prefix`` is given, the reference's ``proto_rf_boxes`` and
    ``proto_bound_boxes`` tables (int64 [P, 6], ``push_box_tables``) are computed before the bank is overwritten and appended
    to the result.  With ``root_dir_for_saving_prototypes``, the prefix and ``epoch_number`` all set they are also saved under
    the reference's names (``save_box_tables``).  Not under a sharded push: with more than one rank this raises ``SpxError``.
    ``gt_boxes=True`` (with the boxes) appends a sixth result, ``proto_bound_boxes_gt``: the crops from the threshold over the
    prototype's own class (``push_box_tables``); nothing is saved for it, the reference stores none."""
    from . import dp

    net = unwrap(prototype_network_parallel)
    net.eval()
    log("\tpush")
    start = time.time()
    device = device or str(net.prototype_vectors.device)
    rank, world = _dp_world(group)
    want_boxes = bool(boxes) or proto_bound_boxes_filename_prefix is not None
    if want_boxes and world > 1:
        raise SpxError(f"push bounding boxes are not available under a sharded push ({world} ranks): run the push with boxes in "
                       "one process, or drop boxes=True / proto_bound_boxes_filename_prefix")
    rng = scan_range(dataset, rank, world)
    # this rank's candidates (best image as a GLOBAL index, value, flat index), each [P]; an empty shard never wins
    if batch_size is not None:
        if world == 1 and len(rng) == 0:
            raise SpxError("the push needs at least one image")
        table = push_single_pass(dataset, net, batch_size=batch_size, void_class=0, image_range=rng, device=device)
        local = (table.best_image, table.best_value, table.best_flat)
    else:
        local, tot_idx = _two_pass_candidates(dataset, net, rng, device, world)
    best, _, flat = dp.reduce_push_candidates(*local, 0, group=group)                 # global, identical on every rank
    owner = (best >= rng.start) & (best < rng.stop)
    if batch_size is not None:
        patch = table.best_patch
    else:
        winners = torch.stack([best - rng.start, flat, owner.to(torch.int64)]).tolist()    # one copy for the second pass
        patch = _winning_patches(winners[0], winners[1], dataset, net, device, image_offset=rng.start, only=winners[2])
    full = dp.gather_push_patches(patch, owner, group=group)                                # [P, Cs], identical on every rank
    best_host, flat_host, patch_host = _winners_to_host(best, flat, full)                  # the single pass's one device-to-host copy
    tables = push_box_tables(best_host, None, dataset, net, device=device, flat=flat_host,
                             gt_boxes=bool(gt_boxes)) if want_boxes else None
    dup = commit_push(net, patch_host.numpy().reshape(tuple(net.prototype_shape)), root_dir_for_saving_prototypes if rank == 0 else None,
                      log=log)
    if tables is not None and None not in (root_dir_for_saving_prototypes, proto_bound_boxes_filename_prefix, epoch_number):
        save_box_tables(tables[0], tables[1], root_dir_for_saving_prototypes, proto_bound_boxes_filename_prefix, epoch_number)
    log("\tpush time: \t{0}".format(time.time() - start))
    return (best, flat if batch_size is not None else tot_idx, dup) + (tuple(tables) if tables is not None else ())
