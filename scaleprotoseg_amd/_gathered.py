"""The inputs of the class-gathered losses (``KLDLoss``, ``KLDLossGroup``, ``ActivationRegularizers``, ``segment_pair_sums``),
stated once.  The kernels take ``Gathered``: fp32 slot planes [B, J, H*W] (entry (j, px) = the value of slot j of the pixel's
class), the label map shifted to classes (``labels0 = target - 1``: 0..K-1 a class, anything else no class), a slot table [K, J]
(>= 0: the slot exists) and a walk hint (the row length W of the pixel grid if it divides H*W, else 0 = linear walk).  Four
constructors lead there; they check shapes first, run on any device and dtype (the tests use them on the CPU, in fp64) and take
their tables from the caller, who caches them on the planes' device.  ``check_domain`` is the only step that asks for the GPU.

Slot rule: slot = rank among the class's prototypes, ascending index.  ``class_slot_table`` reads the identity [P, K] column-wise:
the prototypes of class c are the non-zero entries of column c.  ``row_class_slots`` (``functional.class_gather_table``) reads it
row-wise: the class of prototype p is the argmax of row p, none when the row's sum is not positive.  On identities whose rows
are one-hot or all zero the two give the same table, exactly.  Otherwise they differ: a row with several ones is a prototype of
each of those classes column-wise (a slot in every one, which can raise J) and of the first alone row-wise; a row whose entries
cancel (sum <= 0) still counts column-wise and has no class row-wise.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import NamedTuple, Optional, Tuple

import torch

from ._lib import SpxError


def class_slot_table(prototype_class_identity: torch.Tensor) -> torch.Tensor:
    """[K, J] prototype index of (class, slot) or -1, column-wise."""
    member = prototype_class_identity.detach().cpu() != 0
    p, c = member.nonzero(as_tuple=True)
    table = torch.full((member.shape[1], max(1, int(member.sum(dim=0).max()))), -1, dtype=torch.long)
    table[c, (member.cumsum(dim=0) - 1)[p, c]] = p
    return table


def row_class_slots(prototype_class_identity: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(class of prototype p or -1, slot of p; 0 without a class), int64 [P] on the host, row-wise."""
    ident = prototype_class_identity.detach().cpu()
    P, K = ident.shape
    cls = torch.where(ident.sum(dim=1) > 0, ident.argmax(dim=1), torch.full((P,), -1, dtype=torch.long))
    member = cls.unsqueeze(1) == torch.arange(K).unsqueeze(0)
    return cls, ((member.cumsum(dim=0) - 1) * member).sum(dim=1)


def slot_scale_table(table: torch.Tensor, num_scales: int, scale_num_prototypes) -> torch.Tensor:
    """[K, J] int32 scale id of (class, slot) for a ``class_slot_table``: -1 = the class has no such slot, -2 = a prototype
    that lies in no scale's range (it counts for the spatial entropy and the norm, not for the sample entropy)."""
    t = table.detach().cpu().long()
    sid = torch.where(t >= 0, torch.full_like(t, -2), torch.full_like(t, -1))
    for s in range(int(num_scales)):
        lo, hi = scale_num_prototypes[s]
        sid[(t >= int(lo)) & (t < int(hi))] = s
    return sid.to(torch.int32).contiguous()


def group_class_tables(ident: torch.Tensor, gci: torch.Tensor, G: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Host tables of the group form: (projection of class c or -1 [K], stand-in slot table [K, G]: the slot ids where the class
    has prototypes, else -1)."""
    K = ident.shape[1]
    has = ident.sum(dim=0) > 0                                              # loss.py:504
    proj = torch.where(has, gci.argmax(dim=0) // G, torch.full((K,), -1, dtype=torch.long)).cpu()   # :507
    table = torch.where(has.cpu().unsqueeze(1), torch.arange(G).unsqueeze(0).expand(K, G), torch.full((K, G), -1, dtype=torch.long))
    return proj, table.contiguous()


@dataclass
class ClassDistances:
    """values [B, J, H*W] (slot planes: entry (j, px) = distance to prototype j of the pixel's class), labels [B, H*W] int
    (class 0..K-1, anything else = no class), table [K, J] prototype index of (class, slot) or -1.

    The planes belong to the labels they were gathered under.  ``KLDLoss`` and ``ActivationRegularizers`` take the label
    map they are called with: handed ``target`` itself, unedited, they use ``labels`` as they are (no further launch); handed any
    other tensor (or ``target`` after an in-place edit) they shift that map and compare it with ``labels`` on the device.  Equal
    classes at every pixel (a clone, a reloaded batch) give the same value.  If a single pixel has another class the planes
    hold the wrong prototypes' distances for it and cannot be gathered again from here, so the loss - and with it every
    gradient - is NaN instead of a finite number that belongs to neither label map (no host synchronisation: the NaN is
    made on the device).  Run the forward again with the new labels."""

    values: torch.Tensor
    labels: torch.Tensor
    table: torch.Tensor
    grid: Tuple[int, int]
    target: Optional[torch.Tensor] = None      # the map ``labels`` was derived from (labels = target - 1) ...
    target_version: int = -1                   # ... and its version counter then


class Gathered(NamedTuple):
    planes: torch.Tensor
    labels0: torch.Tensor
    table: Optional[torch.Tensor]
    walk_w: int
    poison: Optional[torch.Tensor] = None      # device scalar the loss is multiplied with: 1, or NaN (see ``ClassDistances``)


def walk_width(W, HW: int) -> int:
    W = int(W)
    return W if W and HW % W == 0 else 0


def _labels0(target_labels: torch.Tensor, B: int, HW: int, what: str) -> torch.Tensor:
    labels0 = target_labels.reshape(target_labels.shape[0], -1).long() - 1          # loss.py:73, :167, :493
    if tuple(labels0.shape) != (B, HW):
        raise SpxError(f"labels {tuple(target_labels.shape)} do not match the {what}' {(B, HW)} pixels")
    return labels0


def _hint(target_labels: torch.Tensor, HW: int) -> int:
    return walk_width(target_labels.shape[-1], HW) if target_labels.dim() >= 3 else 0


def gather_class_distances(prototype_distances: torch.Tensor, labels0: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """torch gather of the P-wide map [B, P, H, W] into the class-gathered values [B, H*W, J]; entries without a class or a
    slot are zero."""
    B, P = prototype_distances.shape[:2]
    K, J = table.shape
    d = prototype_distances.reshape(B, P, -1).permute(0, 2, 1)
    lab = labels0.reshape(B, -1).long()
    ok = (lab >= 0) & (lab < K)
    idx = table.to(d.device)[lab.clamp(0, K - 1)]
    valid = ok.unsqueeze(-1) & (idx >= 0)
    out = torch.gather(d, 2, idx.clamp(min=0))
    return torch.where(valid, out, torch.zeros_like(out))


def from_class_distances(cd: ClassDistances, target_labels: torch.Tensor, table: Optional[torch.Tensor] = None) -> Gathered:
    """``cd.labels`` as they are when the map is the very tensor the planes were gathered under; else the shifted map and the
    poison: 1 where it names the same class at every pixel (out-of-range values are all "no class"), NaN otherwise."""
    planes, table = cd.values, cd.table if table is None else table
    if planes.dim() != 3 or table.shape[1] != planes.shape[1]:
        raise SpxError(f"ClassDistances: values {tuple(planes.shape)} are not [B, J, H*W] planes of the table's {table.shape[1]} slots")
    W = walk_width(cd.grid[-1], planes.shape[2])
    if cd.target is target_labels and cd.target_version == target_labels._version:
        return Gathered(planes, cd.labels, table, W)                              # already target - 1 (int32)
    labels0 = _labels0(target_labels, planes.shape[0], planes.shape[2], "ClassDistances")
    K = table.shape[0]
    cls = lambda t: torch.where((t >= 0) & (t < K), t, torch.full_like(t, -1))
    mine = cd.labels.reshape(labels0.shape).long()
    differ = (cls(labels0.to(mine.device)) != cls(mine)).any()
    return Gathered(planes, labels0, table, W, torch.where(differ, float("nan"), 1.0).to(planes.device))


def from_distance_map(prototype_distances: torch.Tensor, target_labels: torch.Tensor, table: torch.Tensor) -> Gathered:
    """The P-wide distance map [B, P, H, W] under a ``class_slot_table``."""
    B, HW = prototype_distances.shape[0], math.prod(prototype_distances.shape[2:])
    labels0 = _labels0(target_labels, B, HW, "distance map")
    planes = gather_class_distances(prototype_distances, labels0, table).permute(0, 2, 1).contiguous()
    return Gathered(planes, labels0, table, walk_width(prototype_distances.shape[-1], HW))


def from_activations(prototype_activations: torch.Tensor, target_labels: torch.Tensor, table: torch.Tensor) -> Gathered:
    """The P-wide activation tensor [M, P] / [B, H*W, P] under a ``class_slot_table``.  Entries without a class or a slot hold
    some prototype's activation (the clamped index): the kernels mask them."""
    B, P = target_labels.shape[0], prototype_activations.shape[-1]
    HW = prototype_activations.numel() // (B * P)
    labels0 = _labels0(target_labels, B, HW, "activations").to(prototype_activations.device)
    idx = table[labels0.clamp(0, table.shape[0] - 1)].clamp(min=0)                 # [B, HW, J]
    planes = torch.gather(prototype_activations.reshape(B, HW, P), 2, idx).permute(0, 2, 1).contiguous()
    return Gathered(planes, labels0, table, _hint(target_labels, HW))


def from_groups(group_activations, target_labels: torch.Tensor, proj: torch.Tensor, table: torch.Tensor) -> Gathered:
    """The group activations - the list of [M, G] per projection, or their concatenation [M, n_projections * G] - under the
    ``group_class_tables``: a pixel takes the projection of its class, whose groups are its slots."""
    K, G = table.shape
    first = group_activations if isinstance(group_activations, torch.Tensor) else group_activations[0]
    B, HW = target_labels.shape[0], first.numel() // (target_labels.shape[0] * first.shape[-1])
    labels0 = _labels0(target_labels, B, HW, "group activations").to(first.device)
    if first is group_activations:
        ga = first.reshape(B, HW, -1, G)
    else:
        ga = torch.stack([a.reshape(B, HW, G) for a in group_activations], dim=2)
    pix_proj = proj.to(ga.device)[labels0.clamp(0, K - 1)].clamp_min(0)             # [B, HW]; unused where no class
    vals = torch.gather(ga, 2, pix_proj.view(B, HW, 1, 1).expand(B, HW, 1, G)).squeeze(2)
    return Gathered(vals.permute(0, 2, 1).contiguous(), labels0, table, _hint(target_labels, HW))


def check_domain(planes: torch.Tensor, K: int, op: str) -> None:
    """fp32 planes on the GPU, at most 16 slots per class; the [K, J] segment tables of the reduction passes must fit the LDS
    (K*J*12 + K*4 + 8 bytes <= 60 KiB: 150 x 12 and 182 x 12 of the reference's ADE / COCO configs take 22 / 27 KiB); the
    [K, J, J] tables of the pair and gradient passes are tiled over class blocks and set no limit."""
    J = planes.shape[1]
    if not (planes.is_cuda and planes.dtype == torch.float32 and J <= 16 and K * J * 12 + K * 4 + 8 <= 60 * 1024):
        raise SpxError(f"{op}: planes {tuple(planes.shape)} {planes.dtype} on {planes.device} (K={K}, J={J}) are outside the HIP "
                       "kernels' domain (fp32 on the GPU, J <= 16, K*J*12 + K*4 + 8 <= 60 KiB); there is no other backend")


def launch_operands(g: Gathered) -> Tuple[torch.Tensor, torch.Tensor]:
    """(planes detached and contiguous, labels int32 contiguous on the planes' device): what the entry points are handed."""
    v = g.planes.detach().contiguous()
    return v, g.labels0.to(device=v.device, dtype=torch.int32).contiguous()
