"""Shared data of the packed-training-maps tests (tests/test_msc_pack_cpu.py, tests/test_gpu_msc_pack.py): the layouts of the
recorded MSC cases (tests/msc_cases.py), the float64 restatement of ``msc_pack`` - the per-segment results of
tests/msc_restatement.py laid out by ``PackedLayout`` -, its gradient with a per-element bound, and the recorded training forward
of the reference (tests/golden/msc_packed_forward.npz, tools/gen_msc_packed_golden.py).  Nothing here touches a device on import
and nothing is modified by a test.

The gradient bound (u = 2^-24).  Map k's gradient is ``own + gather``: ``own = g y (1 - y)`` at the map's own segment (``g``
without the sigmoid), ``gather`` the gradient of ``msc_max`` from the maximum's segment (tests/msc_restatement.py, bound
``gather_bound``).  The kernel starts its fp32 running sum at ``own`` and adds the gather's terms to it in order, so

    bound = gather_bound + 3 u |own| [sigmoid: the roundings of 1 - y, y (1 - y), g .] + (n + 1) u |own|

where n is the number of destination pixels that may contribute to the element (the restatement's widened footprint; 1 for map
0): each of the n additions rounds a partial sum that now holds ``own`` as well, which adds u |own| per addition to the
restatement's (9 + n) u |terms|; the + 1 is slack for the second order.  Without a maximum's segment the bound is the own term's
alone.  This is ``test_gpu_msc.py::test_backward``'s measure with the own term's roundings added."""
import functools

import numpy as np

import msc_cases as MC
import msc_restatement as MR
from support import load_cases

from scaleprotoseg_amd.msc import PackedLayout

U = MR.U
CASES = MC.SHAPE_SETS + MC.SPECIAL


def layout(name, with_max=True, K=None):
    maps = MC.case(name)["maps"][:K]
    return PackedLayout.of_maps(maps[0].shape[0], [m.shape[2:] for m in maps], with_max)


def pack(lay, segments):
    """One [B, C, h_k, w_k] array per segment -> [C, M] by the layout's column rule, element by element."""
    C = segments[0].shape[1]
    out = np.zeros((C, lay.M), dtype=segments[0].dtype)
    for k, (s, (h, w)) in enumerate(zip(segments, lay.grids)):
        assert s.shape == (lay.B, C, h, w), (k, s.shape)
        for b in range(lay.B):
            c0 = lay.column(k, b, 0)
            out[:, c0:c0 + h * w] = s[b].reshape(C, h * w)
    return out


def unpack(lay, packed, k):
    """Segment k of a [C, M] array as [B, C, h, w] (a copy)."""
    h, w = lay.grids[k]
    C = packed.shape[0]
    return np.stack([packed[:, lay.column(k, b, 0):lay.column(k, b, 0) + h * w].reshape(C, h, w) for b in range(lay.B)])


@functools.lru_cache(maxsize=None)
def restated(name, with_max=True):
    """(z [C, M] float64 before the activation, bound [C, M], index [B, C, H, W] or None): the maps themselves (bound 0) and
    ``MR.forward`` for the maximum's segment."""
    maps = [np.asarray(m, dtype=np.float64) for m in MC.case(name)["maps"]]
    lay = layout(name, with_max)
    segs, bounds, index = list(maps), [np.zeros_like(m) for m in maps], None
    if with_max:
        z, index, zb = MC.restated(name)[:3]
        segs.append(z)
        bounds.append(zb)
    return pack(lay, segs), pack(lay, bounds), index


def gradients(shapes, B, index, g, y=None, with_max=True):
    """Float64 gradients of ``msc_pack`` for a GIVEN index.  ``shapes``: the (h_k, w_k); ``g`` [C, M] the upstream gradient;
    ``y`` [C, M] the saved output under the sigmoid, else None.  -> (list of [B, C, h_k, w_k], list of bounds)."""
    lay = PackedLayout.of_maps(B, shapes, with_max)
    g = np.asarray(g, dtype=np.float64)
    gp = g * np.asarray(y, dtype=np.float64) * (1.0 - np.asarray(y, dtype=np.float64)) if y is not None else g
    K = len(shapes)
    own = [unpack(lay, gp, k) for k in range(K)]
    own_bound = [((3 * U) if y is not None else 0.0) * np.abs(o) for o in own]
    if not with_max:
        return own, own_bound
    gmax = unpack(lay, gp, K)
    gather, gb = MR.gradients(shapes, index, gmax, derivative=y is not None)
    H, W = shapes[0]
    grads, bounds = [], []
    for k, (h, w) in enumerate(shapes):
        m = (np.asarray(index) == k).astype(np.float64)
        if k == 0:
            n = m
        else:
            n = np.einsum("Yi,bcYX,Xj->bcij", MR._widen(MR.weights(h, H)), m, MR._widen(MR.weights(w, W)))
        grads.append(own[k] + gather[k])
        bounds.append(gb[k] + own_bound[k] + (n + 1) * U * np.abs(own[k]))
    return grads, bounds


# ---- the reference's training forward on four maps (tools/gen_msc_packed_golden.py) ---------------------------------------------
@functools.lru_cache(maxsize=None)
def recorded():
    c = dict(load_cases("msc_packed_forward")["train"])
    n = len(c["grids"])
    c["conv"] = [c[f"conv{k}"] for k in range(n)]
    for what in ("logits", "distances", "activations"):
        c[what] = [c[f"{what}{k}"] for k in range(n)]
    c["ranges"] = {s: (int(lo), int(hi)) for s, (lo, hi) in enumerate(c["scale_ranges"])}
    return c


# the distance path's second case: the Pascal grids at B = 2 (M = 9 528: 75 tiles of 128 pixels, the last one ragged, every
# segment and image boundary inside a tile)
PASCAL = dict(B=2, S=2, Cs=16, P=24, K=4, grids=((41, 41), (21, 21), (31, 31)))
SEGMENT_WEIGHTS = (1.0, 0.5, 2.0, 0.25)           # the loss weights of the four segments in the gradient checks
