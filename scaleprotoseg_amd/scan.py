"""The walk over a data set that the push (push.py) and the pruning search (prune.py) share: host code only, no kernels.

Dataset protocol: ``len(dataset)`` and ``dataset[i] -> (image, target)`` with ``image`` a normalised float tensor [3, h, w]
(or [1, 3, h, w]) and ``target`` an integer label map [h, w], optionally ``dataset.convert_targets``.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np
import torch

from ._lib import SpxError


def unwrap(ppnet):
    """The model itself, out of a wrapper with ``.module``."""
    return ppnet.module if hasattr(ppnet, "module") else ppnet


def dp_world(group) -> Tuple[int, int]:
    """(rank, world size) of a process group; (0, 1) without ``torch.distributed``."""
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(group), dist.get_world_size(group)
    return 0, 1


def scan_range(dataset, rank: int = 0, world: int = 1, image_range: Optional[range] = None) -> range:
    """The images of one scan: ``image_range`` where given, else this rank's contiguous shard (``dp.shard_range``; the whole
    data set at one rank)."""
    from .dp import shard_range

    return image_range if image_range is not None else shard_range(len(dataset), rank, world)


def image_batch(img: torch.Tensor, device) -> torch.Tensor:
    """One image as a [1, 3, h, w] batch on ``device``."""
    return img.unsqueeze(0).to(device) if img.dim() == 3 else img.to(device)


def converted(dataset, target):
    """``target`` through ``dataset.convert_targets`` where the data set has one."""
    convert = getattr(dataset, "convert_targets", None)
    return target if convert is None else convert(target)


def batches(dataset, rng: range, batch_size: int):
    """Runs of consecutive images of equal image and label size, at most ``batch_size`` long (image order kept)."""
    run, shape = [], None
    for i in rng:
        img, target = dataset[i]
        t = np.asarray(target)
        s = (tuple(img.shape), t.shape)
        if run and (s != shape or len(run) == batch_size):
            yield run
            run = []
        run.append((i, img, t))
        shape = s
    if run:
        yield run


def encode_run(net, dataset, run, device, msc_message: str) -> Tuple[torch.Tensor, List[np.ndarray]]:
    """Features [B, C, H, W] of one run of ``batches`` and its converted targets; an MSC list of feature maps is refused with
    ``msc_message``."""
    # image by image, stacked on the device: one pageable copy of a host-stacked run measured 5 GB/s against 23 .. 55 GB/s for its
    # images one by one, and the host-side stack cost as much again (profiles/push_single_pass_summary.md)
    x = torch.stack([image_batch(img, device)[0] for _, img, _ in run])
    conv = net.conv_features(x)
    if isinstance(conv, list):
        raise SpxError(msc_message)
    return conv, [np.asarray(converted(dataset, t)) for _, _, t in run]
