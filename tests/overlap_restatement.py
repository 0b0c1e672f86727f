"""Float64 restatement of the activation-overlap definition (scaleprotoseg_amd/overlap.py), NumPy only.

    u[Y, X]  cubic upsample of a latent plane: source coordinate (X + 0.5) * w / W - 0.5, taps floor - 1 .. floor + 2 clamped
             to the grid, Keys' kernel with a = -0.75 (OpenCV INTER_CUBIC, torch's bicubic with align_corners = False),
             summed in float64.  ``cv2`` itself was never run against this.
    T        numpy's linear quantile of the float32 values: k = floor(q (HW - 1)), gamma = the fractional part (float64),
             T = numpy's _lerp of the order statistics v[k], v[k + 1] in float32.
    mask     u > T.
tests/test_overlap_cpu.py pins this to the fixture recorded from the reference's own functions
(tools/gen_overlap_golden.py uses ``upsample`` rounded to float32 in place of ``cv2.resize``); the GPU tests use it for
shapes the fixture does not hold."""
import numpy as np

A = -0.75
MARGIN = 64.0 * 2.0 ** -23       # x max|a|: rounding bound of the 16 fp32 products and sums (sum |w| <= 1.375^2), ~3x slack


def _cc1(x):
    return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0


def _cc2(x):
    return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A


def taps(n_in, n_out):
    """(indices int64 [n_out, 4], weights float64 [n_out, 4]) of one axis."""
    s = (np.arange(n_out, dtype=np.float64) + 0.5) * n_in / n_out - 0.5
    i = np.floor(s)
    t = s - i
    idx = np.clip(i[:, None].astype(np.int64) + np.arange(-1, 3), 0, n_in - 1)
    wgt = np.stack([_cc2(t + 1.0), _cc1(t), _cc1(1.0 - t), _cc2(2.0 - t)], axis=1)
    return idx, wgt


def upsample(plane, size):
    """float64 [H, W] from a latent plane [h, w]."""
    a = np.asarray(plane, dtype=np.float64)
    H, W = int(size[0]), int(size[1])
    iy, wy = taps(a.shape[0], H)
    ix, wx = taps(a.shape[1], W)
    rows = (a[:, ix] * wx[None]).sum(-1)                    # [h, W]
    return (rows[iy] * wy[:, :, None]).sum(1)               # [H, W]


def rank(q, count):
    v = float(q) * (count - 1)
    k = int(np.floor(v))
    return k, np.float32(v - k)


def threshold(u32, q):
    """numpy's linear quantile of a float32 array with k, gamma from float64 (the definition's form)."""
    v = np.sort(np.asarray(u32, dtype=np.float32).ravel())
    k, g = rank(q, v.size)
    lo, hi = v[k], v[min(k + 1, v.size - 1)]
    d = np.float32(hi - lo)
    if g >= 0.5:
        return np.float32(hi - np.float32(d * np.float32(np.float32(1.0) - g)))
    return np.float32(lo + np.float32(d * g))


def margin(plane):
    return MARGIN * float(np.abs(np.asarray(plane, dtype=np.float64)).max())


def overlap_counts(planes, labels, table, q, size=None):
    """The definition on planes [N, C, h, w], labels [N, H, W], slot table [K, J] (-1 = no slot).
    Returns dict: thresholds float32 [N, C] (nan where no present class uses the plane), ambiguous int64 [N, C] (pixels within
    the margin of the threshold), area int64 [K, J], inter int64 [K, J, J] (j < j'), images int64 [K]."""
    planes = np.asarray(planes)
    labels = np.asarray(labels)
    table = np.asarray(table)
    N, C = planes.shape[:2]
    K, J = table.shape
    H, W = labels.shape[1:] if size is None else size
    thr = np.full((N, C), np.nan, np.float32)
    amb = np.zeros((N, C), np.int64)
    area = np.zeros((K, J), np.int64)
    inter = np.zeros((K, J, J), np.int64)
    images = np.zeros(K, np.int64)
    for n in range(N):
        masks = {}
        for k in range(K):
            if not (labels[n] == k + 1).any():
                continue
            images[k] += 1
            slots = [(j, int(table[k, j])) for j in range(J) if table[k, j] >= 0]
            for j, c in slots:
                if c not in masks:
                    u = upsample(planes[n, c], (H, W))
                    thr[n, c] = threshold(u.astype(np.float32), q)
                    masks[c] = u.astype(np.float32) > thr[n, c]
                    amb[n, c] = int((np.abs(u - np.float64(thr[n, c])) <= margin(planes[n, c])).sum())
                area[k, j] += int(masks[c].sum())
            for a, (j, c) in enumerate(slots):
                for j2, c2 in slots[a + 1:]:
                    inter[k, j, j2] += int((masks[c] & masks[c2]).sum())
    return dict(thresholds=thr, ambiguous=amb, area=area, inter=inter, images=images)


def finalize(inter, area, table):
    """(class_iou dict, total) in float64 from the counters."""
    K, J = area.shape
    ci, tot_i, tot_u = {}, 0, 0
    for k in range(K):
        i_k = u_k = 0
        for j in range(J):
            for j2 in range(j + 1, J):
                if table[k, j] >= 0 and table[k, j2] >= 0:
                    i_k += int(inter[k, j, j2])
                    u_k += int(area[k, j] + area[k, j2] - inter[k, j, j2])
        if u_k > 0:
            ci[k] = i_k / u_k
        tot_i += i_k
        tot_u += u_k
    return ci, (tot_i / tot_u if tot_u > 0 else float("nan"))
