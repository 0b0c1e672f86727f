"""NumPy restatement of the explanation maps (scaleprotoseg_amd/explain.py).

    u        overlap_restatement.upsample (float64) rounded to float32: what the fixture tool hands the reference in place of
             ``cv2.resize`` (tools/gen_explain_golden.py).
    heat     m = u * [label == k + 1]; lo = min m, hi = max m; np.uint8(255 * ((m - lo) / (hi - lo))) in float32, the
             reference's own arithmetic; all zeros where hi == lo (the reference's bytes are undefined there).
    dom      np.argmax over the class's slots of wgt * u in float32 (the first maximum), 255 where label != k + 1 and where the
             class has no slot.
tests/test_explain_cpu.py pins this to the fixture recorded from the reference's own functions.

Ambiguity (a condition on the inputs, not a tolerance of the kernel).  The kernel's fp32 sample lies within
m0 = 64 * 2^-23 * max|a| of the float64 value (overlap_restatement.MARGIN).  lo, hi and m each move by at most m0, so
x = (m - lo) / d moves by at most about 3 m0 / d: a heat pixel is ambiguous when the float64 value 255 x lies within
255 * 3 * m0 / d of an integer.  One kind of pixel is taken out of that set because nothing about it is rounded: outside the
class m is 0 exactly, and when lo (or hi) is that 0 and every sample of the class is above m0 (below -m0), the kernel's lo (hi)
is the same exact 0, so r = 0 and the byte is 0 (x = d / d = 1 and the byte is 255) in any arithmetic.  Without this every
pixel outside the class of a positive plane would count as ambiguous, 255 x being the integer 0.  A dominant pixel is
ambiguous when its two largest float64 products differ by at most 2 * m0 * max|wgt|."""
import numpy as np

import overlap_restatement as OR

OFF = 255


def upsample32(plane, size):
    return OR.upsample(plane, size).astype(np.float32)


def heat_map(plane, labels, k, size=None):
    """(heat uint8 [H, W], lo float32, hi float32) of one latent plane over class k of one image's labels."""
    size = labels.shape if size is None else size
    m = upsample32(plane, size) * (labels == k + 1)                       # float32 * bool -> float32, as the reference
    lo, hi = np.amin(m), np.amax(m)
    if hi == lo:
        return np.zeros(m.shape, np.uint8), lo, hi
    r = m - lo
    x = r / np.amax(r)
    return np.uint8(255 * x), lo, hi


def heat_ambiguous(plane, labels, k):
    """bool [H, W]: pixels whose byte may differ by one under an error of m0 per sample."""
    on = labels == k + 1
    m = OR.upsample(plane, labels.shape) * on
    lo, hi = m.min(), m.max()
    d = hi - lo
    if not d > 0:
        return np.zeros(m.shape, bool)
    m0 = OR.margin(plane)
    v = 255.0 * ((m - lo) / d)
    amb = np.abs(v - np.round(v)) <= 255.0 * 3.0 * m0 / d
    if on.any() and ((lo == 0 and m[on].min() > m0) or (hi == 0 and m[on].max() < -m0)):
        amb &= on
    return amb


def dominant(planes, weights, labels, k):
    """uint8 [H, W] from the latent planes of the class's slots (in slot order; None = no such slot) and their weights."""
    on = labels == k + 1
    slots = [j for j, p in enumerate(planes) if p is not None]
    if not slots:
        return np.full(labels.shape, OFF, np.uint8)
    stack = np.stack([upsample32(planes[j], labels.shape) * np.float32(weights[j]) for j in slots], axis=-1)
    arg = np.asarray(slots)[np.argmax(stack, axis=-1)]
    return np.where(on, arg, OFF).astype(np.uint8)


def dominant_top2(planes, weights, labels, k):
    """(ambiguous bool [H, W], first int [H, W], second int [H, W]): the two slots with the largest float64 products (second
    = first where the class has one slot) and whether they are within 2 m0 max|wgt| of each other.  Only pixels of the class
    can be ambiguous."""
    on = labels == k + 1
    slots = [j for j, p in enumerate(planes) if p is not None]
    if not slots:
        z = np.full(labels.shape, OFF, np.int64)
        return np.zeros(labels.shape, bool), z, z
    prod = np.stack([OR.upsample(planes[j], labels.shape) * float(weights[j]) for j in slots], axis=-1)
    order = np.argsort(-prod, axis=-1, kind="stable")
    first = order[..., 0]
    second = order[..., 1] if len(slots) > 1 else first
    m0 = max(OR.margin(planes[j]) for j in slots)
    wmax = max(abs(float(weights[j])) for j in slots)
    gap = np.take_along_axis(prod, first[..., None], -1)[..., 0] - np.take_along_axis(prod, second[..., None], -1)[..., 0]
    amb = on & (gap <= 2.0 * m0 * wmax) & (len(slots) > 1)
    s = np.asarray(slots)
    return amb, s[first], s[second]
