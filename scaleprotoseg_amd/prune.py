"""Prototype pruning on the MI355X kernels.

Mirrors the numerical part of find_nearest.py (``find_k_nearest_patches_to_prototypes`` with ``full_save=True``, as
prune.py:22-30 calls it) and prune.py:11-74: every prototype's k nearest training patches, then the prototypes whose k
patches hold fewer than ``prune_threshold`` patches of their own class are dropped.  The plotting half (patch PNGs,
heatmaps, ``find_high_activation_crop``) is visualisation and is not part of this package; the result carries what it
needs (image, latent cell, footprint box, distance).

Per batch of equal-size images the GPU finds each prototype's nearest latent pixel (void-masked, not class-masked; fused
into the distance kernel or on a written map), the label of its footprint in the full-resolution label, and merges the
candidates into a running [P, k] table.  The whole search makes one device-to-host copy, at the end.

Tie rule: a row holds the k smallest candidates by (all-void flag, distance, image index) - the order of the reference's
float64 distance ``d + 1e7 * void`` for distances below 1e7, earlier images first on an equal distance (a new candidate
replaces the current worst only if strictly nearer, as ``heapq.heappushpop`` does).  One divergence: when several kept
candidates tie at the k-th distance and a strictly nearer one arrives, ``heapq`` evicts whichever tied entry sits at its
heap's root, which depends on the heap's layout; here the latest image of the tied ones leaves.

Dataset protocol as ``push_prototypes_multiscale``: ``len(dataset)``, ``dataset[i] -> (image [3, h, w], target [h, w])``
with 0 = void, optionally ``dataset.convert_targets``.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._lib import SpxError
from .functional import prune_footprint, prune_nearest_from_features, prune_nearest_from_map
from .scan import batches, dp_world, encode_run, scan_range, unwrap
from .utils import resize_label

MAX_K = 64
_NO_VOID = -(2 ** 31)          # a label value no converted target holds: no pixel is void
_FIELDS = 9                    # packed table row: key, image, label, box (4), latent cell (2)


@dataclass
class NearestPatches:
    """The k nearest training patches of every prototype, ascending (rows [P, k]; image -1 where fewer than k exist).

    distance   fp32   the latent distance d (without the reference's 1e7 void offset)
    all_void   bool   the candidate came from an image without a non-void latent pixel (ranked after all others)
    image      int64  dataset index
    latent     int64  [P, k, 2] latent cell (row, col)
    box        int64  [P, k, 4] footprint (h0, h1, w0, w1) in the full-resolution label / image
    label      int64  the footprint's label (find_nearest.py:206-213; -1 = void)"""

    distance: torch.Tensor
    all_void: torch.Tensor
    image: torch.Tensor
    latent: torch.Tensor
    box: torch.Tensor
    label: torch.Tensor

    def class_ids(self) -> Union[np.ndarray, List[np.ndarray]]:
        """The reference's ``labels_all_prototype``: int64 [P, k], or one array per prototype when some prototype found
        fewer than k patches (the reference's rows are then ragged too)."""
        rows = [self.label[j][self.image[j] >= 0].numpy() for j in range(self.label.shape[0])]
        if all(len(r) == self.label.shape[1] for r in rows):
            return self.label.numpy().copy()
        return rows


def _sort_keys(packed: torch.Tensor) -> torch.Tensor:
    """One int64 per packed entry that orders as (key bits 63..32, image); empty slots last."""
    hi = (packed[..., 0] >> 32) & 0xFFFFFFFF
    img = packed[..., 1]
    return torch.where(img >= 0, (hi << 31) | img, torch.full_like(img, torch.iinfo(torch.int64).max))


def merge_nearest_tables(tables: Sequence[torch.Tensor], k: int) -> torch.Tensor:
    """Merge packed tables [P, k_i, 9] (key, image, label, box, cell) into the k smallest entries per prototype under the
    table's rule: ordered by (distance key, image), empty slots (image -1) last.  Exact whenever image indices differ
    between the tables, as they do for the contiguous shards of a data-parallel search."""
    cat = torch.cat(list(tables), dim=1)
    order = torch.sort(_sort_keys(cat), dim=1, stable=True).indices
    if order.shape[1] < k:
        pad = torch.zeros((cat.shape[0], k - order.shape[1], _FIELDS), dtype=torch.int64, device=cat.device)
        pad[..., 0] = -1
        pad[..., 1] = -1
        cat = torch.cat([cat, pad], dim=1)
        order = torch.cat([order, torch.arange(order.shape[1], k, device=cat.device).expand(cat.shape[0], -1)], dim=1)
    sel = order[:, :k]
    return torch.gather(cat, 1, sel[..., None].expand(-1, -1, _FIELDS))


def prune_decision(result: NearestPatches, prototype_classes: torch.Tensor, prune_threshold: int) -> List[int]:
    """prune.py:36-42: prototype j goes when fewer than ``prune_threshold`` of its nearest patches carry its class."""
    cls = prototype_classes.to(torch.int64).cpu()
    hits = ((result.label == cls[:, None]) & (result.image >= 0)).sum(dim=1)
    return [int(j) for j in torch.nonzero(hits < int(prune_threshold)).flatten()]


def _unpack(packed: torch.Tensor) -> NearestPatches:
    key = packed[..., 0]
    hi = (key >> 32) & 0xFFFFFFFF
    dist = (hi & 0x7FFFFFFF).to(torch.int32).view(torch.float32)
    empty = packed[..., 1] < 0
    return NearestPatches(
        distance=torch.where(empty, torch.full_like(dist, float("inf")), dist),
        all_void=((hi >> 31) == 1) & ~empty,
        image=packed[..., 1].clone(),
        latent=packed[..., 7:9].clone(),
        box=packed[..., 3:7].clone(),
        label=packed[..., 2].clone(),
    )


class NearestTable:
    """The running [P, k] table on the device (spx_prune_merge)."""

    def __init__(self, P: int, k: int, device):
        if not 1 <= int(k) <= MAX_K:
            raise SpxError(f"k = {k} outside 1..{MAX_K}")
        self.P, self.k = int(P), int(k)
        self.key = torch.full((P, k), -1, dtype=torch.int64, device=device)
        self.image = torch.full((P, k), -1, dtype=torch.int64, device=device)
        self.label = torch.zeros((P, k), dtype=torch.int32, device=device)
        self.box = torch.zeros((P, k, 4), dtype=torch.int32, device=device)
        self.cell = torch.zeros((P, k, 2), dtype=torch.int32, device=device)

    def merge(self, keys: torch.Tensor, label: torch.Tensor, box: torch.Tensor, W: int, image0: int) -> None:
        """Insert the candidates of images image0 .. image0 + B - 1 (keys / label [B, P], box [B, P, 4])."""
        lib = _lib.load()
        B, P = keys.shape
        if P != self.P:
            raise SpxError(f"candidates for {P} prototypes, table holds {self.P}")
        keys, label, box = keys.contiguous(), label.to(torch.int32).contiguous(), box.to(torch.int32).contiguous()
        _lib.check(lib.spx_prune_merge(_lib.ptr(keys), _lib.ptr(label), _lib.ptr(box), B, P, int(W), int(image0), self.k,
                                       _lib.ptr(self.key), _lib.ptr(self.image), _lib.ptr(self.label), _lib.ptr(self.box),
                                       _lib.ptr(self.cell), _lib.stream_ptr()))

    def packed(self) -> torch.Tensor:
        """[P, k, 9] int64: key, image, label, box (4), latent cell (2)."""
        return torch.cat([self.key[..., None], self.image[..., None], self.label[..., None].long(), self.box.long(),
                          self.cell.long()], dim=2)


@torch.no_grad()
def find_k_nearest_patches_to_prototypes(
    dataset,
    ppnet,
    k: int = 5,
    *,
    batch_size: int = 8,
    void_class: Optional[int] = 0,
    image_range: Optional[range] = None,
    group=None,
    fused: bool = True,
    device: Optional[str] = None,
    log: Callable = print,
) -> NearestPatches:
    """The k nearest training patches of every prototype (find_nearest.py:70-225, ``full_save=True``), see the module
    docstring for the rule.  ``ppnet``: PPNetMultiScale, PPNet (S = 1) or the group class (or a wrapper with
    ``.module``).  Consecutive images of equal size go through the network ``batch_size`` at a time.  ``void_class``: the
    converted target value of void pixels (the reference's 0; None = no void pixels).  ``fused=False`` writes the
    distance map and reduces it (spx_prune_argmin) instead of reducing inside the distance kernel; the results are
    identical.  ``image_range`` restricts the search to those dataset indices.  With ``torch.distributed`` initialised
    and more than one rank (and no ``image_range``), every rank searches a contiguous shard and the ranks' tables are
    merged with one all-gather: every rank returns the single-process result."""
    from . import dp

    net = unwrap(ppnet)
    if not 1 <= int(k) <= MAX_K:
        raise SpxError(f"k = {k} outside 1..{MAX_K}")
    if batch_size < 1:
        raise SpxError(f"batch_size = {batch_size} must be positive")
    if getattr(net, "scale_head", None) is not None:
        net._refuse_scale_head("the pruning search")
    net.eval()
    dev = torch.device(device or str(net.prototype_vectors.device))
    _lib.require_gpu(dev, "the model")
    rank, world = dp_world(group) if image_range is None else (0, 1)
    P = net.num_prototypes
    target_class = net.prototype_class_identity.detach().cpu().argmax(dim=1).to(torch.int32).to(dev)
    void_label = _NO_VOID if void_class is None else int(void_class)
    table = NearestTable(P, k, dev)
    for run in batches(dataset, scan_range(dataset, rank, world, image_range), batch_size):
        conv, targets = encode_run(net, dataset, run, dev,
                                   "multi-scale (MSC) list features: the nearest patch of a prototype is ambiguous across the inputs")
        net._check_fusable()
        H, W = int(conv.shape[2]), int(conv.shape[3])
        latent = torch.stack([resize_label(t, (W, H)) for t in targets])
        if fused:
            keys = prune_nearest_from_features(conv, net.prototype_vectors, net._layout(1), latent, void_label=void_label)
        else:
            dist_map = net._scale_l2_convolution(conv)
            keys = prune_nearest_from_map(dist_map, latent, void_label=void_label)
        full = torch.from_numpy(np.stack(targets).astype(np.int64) - 1).to(device=dev, dtype=torch.int32)
        label, box = prune_footprint(full, keys, (H, W), target_class)
        table.merge(keys, label, box, W, run[0][0])
    packed = table.packed()
    if world > 1:
        packed = dp.reduce_prune_tables(packed, k, group=group)
    return _unpack(packed.cpu())                                      # the search's one device-to-host copy


def prune_prototypes(
    dataset,
    ppnet,
    k: int = 6,
    prune_threshold: int = 3,
    *,
    root_dir: Optional[os.PathLike] = None,
    batch_size: int = 8,
    void_class: Optional[int] = 0,
    group=None,
    fused: bool = True,
    log: Callable = print,
) -> Tuple[np.ndarray, List[int]]:
    """prune.py:11-74: find the k nearest patches, drop every prototype j whose patches hold fewer than
    ``prune_threshold`` of class_j = argmax(prototype_class_identity[j]), prune the model in place
    (``ppnet.prune_prototypes``).  Returns (prune_info int64 [n, 2] of (prototype, class), prototypes_to_keep).  With
    ``root_dir`` (rank 0 only under data parallelism) writes ``prune_info.npy`` and ``prototypes_to_keep.json`` there; the
    list loads through ``checkpoint.load_reference_state_dict(..., unique_prototypes=path)``."""
    net = unwrap(ppnet)
    result = find_k_nearest_patches_to_prototypes(dataset, net, k, batch_size=batch_size, void_class=void_class, group=group,
                                                  fused=fused, log=log)
    P0 = net.num_prototypes
    classes = net.prototype_class_identity.detach().cpu().argmax(dim=1)
    pruned = prune_decision(result, classes, prune_threshold)
    log(f"k = {k}, prune_threshold = {prune_threshold}")
    log(f"{len(pruned)} prototypes will be pruned")
    prune_info = np.stack([np.asarray(pruned, dtype=np.int64), classes[pruned].numpy().astype(np.int64)], axis=1) \
        if pruned else np.zeros((0, 2), dtype=np.int64)
    net.prune_prototypes(pruned)
    keep = sorted(set(range(P0)) - set(pruned))
    if root_dir is not None and dp_world(group)[0] == 0:
        os.makedirs(root_dir, exist_ok=True)
        np.save(os.path.join(root_dir, "prune_info.npy"), prune_info)
        with open(os.path.join(root_dir, "prototypes_to_keep.json"), "w") as fp:
            json.dump(keep, fp)
    return prune_info, keep
