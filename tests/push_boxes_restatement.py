"""NumPy restatement of the push bounding boxes (scaleprotoseg_amd/pushbox.py; the reference's
push_multiscale_optimization.py:416-497 and helpers.find_continuous_high_activation_crop), with the float64 upsample of
tests/overlap_restatement.py, and a per-row robustness flag.

Definition (``boxes``):
    rf    ph = H / h, pw = W / w, i = f // w, j = f % w in Python floats:
          [int(i*ph), int(i*ph + ph) + 1, int(j*pw), int(j*pw + pw) + 1]
    u     float32(upsample(plane, (H, W)));  T = np.percentile(u, 100 q) over the whole image
    hit   v >= T with v = u where labels == k + 1 and 0 elsewhere
    walk  from rf, four sticky flags, the steps up / down / left / right in that order until all four flags are set, each a
          query "any hit in the segment next to the box"; then the margin and the clip (``walk``)

Robustness.  The kernel evaluates a sample in fp32 (within m = overlap_restatement.margin(plane) of the float64 value) and
selects its own threshold (within m of numpy's: tests/test_gpu_overlap.py).  So a pixel inside the class is AMBIGUOUS when
|u64 - T| <= 2 m, a pixel outside the class (value 0) only when |T| <= 2 m.  A query is robust when its segment holds a
non-ambiguous hit (the answer is "yes" whatever the ambiguous pixels do) or no ambiguous pixel at all; a row is robust when every
query of its walk is.  With identity resampling (H == h, W == w) the cubic weights are exactly 0 and 1 and the select is exact:
nothing is ambiguous."""
import numpy as np

import overlap_restatement as R


def rf_box(f, h, w, H, W):
    ph, pw = H / h, W / w
    i, j = f // w, f % w
    return [int(i * ph), int(i * ph + ph) + 1, int(j * pw), int(j * pw + pw) + 1]


def walk(hit, rf, add_margin=5, ambiguous=None):
    """The greedy enlargement on a boolean hit map [H, W] -> ((h0, h1, w0, w1), robust).  Segments are clipped as a NumPy
    slice clips them."""
    H, W = hit.shape
    sh, eh, sw, ew = rf
    stopped = [False] * 4
    robust = True

    def query(ys, xs):
        nonlocal robust
        seg = hit[ys, xs]
        if ambiguous is not None:
            amb = ambiguous[ys, xs]
            if not ((seg & ~amb).any() or not amb.any()):
                robust = False
        return bool(seg.any())

    while not all(stopped):
        if not stopped[0] and sh > 0 and query(sh - 1, slice(sw, ew + 1)):
            sh -= 1
        else:
            stopped[0] = True
        if not stopped[1] and eh < H - 1 and query(eh + 1, slice(sw, ew + 1)):
            eh += 1
        else:
            stopped[1] = True
        if not stopped[2] and sw > 0 and query(slice(sh, eh + 1), sw - 1):
            sw -= 1
        else:
            stopped[2] = True
        if not stopped[3] and ew < W - 1 and query(slice(sh, eh + 1), ew + 1):
            ew += 1
        else:
            stopped[3] = True
    sh, sw = max(sh - add_margin, 0), max(sw - add_margin, 0)
    eh, ew = min(eh + add_margin, H - 1), min(ew + add_margin, W - 1)
    return (sh, eh + 1, sw, ew + 1), robust


def boxes(plane, labels, k, f, q=0.95, add_margin=5, threshold=None, u32=None):
    """One row: dict(rf, box, threshold, robust).  ``u32``: the float32 map, when the caller already holds it (it must be
    float32(upsample(plane))); ``threshold``: T, when not numpy's percentile of that map."""
    plane = np.asarray(plane)
    labels = np.asarray(labels)
    h, w = plane.shape
    H, W = labels.shape
    rf = rf_box(int(f), h, w, H, W)
    u64 = R.upsample(plane, (H, W))
    if u32 is None:
        u32 = u64.astype(np.float32)
    T = np.float32(np.percentile(u32, 100.0 * q) if threshold is None else threshold)
    inside = labels == k + 1
    hit = np.where(inside, u32, np.float32(0.0)) >= T
    if (H, W) == (h, w):
        amb = np.zeros((H, W), bool)
    else:
        m2 = 2.0 * R.margin(plane)
        amb = np.where(inside, np.abs(u64 - np.float64(T)) <= m2, abs(float(T)) <= m2)
    box, robust = walk(hit, rf, add_margin, amb)
    return dict(rf=rf, box=list(box), threshold=T, robust=robust)
