"""NumPy restatement of the part consistency / stability definition (scaleprotoseg_amd/parts.py), written from the contract and
from what segmentation/analysis/metrics/consistency.py:186-270, :165-178 and stability.py:169-175 compute, with its own
flood-fill labelling.  No SciPy, pandas or device.

The table has one byte per (image, class, slot, part column): 0, 1 or 255 = absent (the reference's NaN for consistency, its 0
for stability)."""
import math

import numpy as np

ABSENT = 255


# ---- components -------------------------------------------------------------------------------------------------------------
def components(mask):
    """[(count, sum X, sum Y)] of the 8-connected components of a boolean mask, in raster order of their first pixel."""
    mask = np.asarray(mask, dtype=bool)
    H, W = mask.shape
    seen = np.zeros((H, W), bool)
    out = []
    for y0 in range(H):
        for x0 in np.flatnonzero(mask[y0] & ~seen[y0]):
            if seen[y0, x0]:
                continue
            seen[y0, x0] = True
            stack = [(y0, int(x0))]
            cnt = sx = sy = 0
            while stack:
                y, x = stack.pop()
                cnt += 1
                sx += x
                sy += y
                for yy in range(max(0, y - 1), min(H, y + 2)):
                    for xx in range(max(0, x - 1), min(W, x + 2)):
                        if mask[yy, xx] and not seen[yy, xx]:
                            seen[yy, xx] = True
                            stack.append((yy, xx))
            out.append((cnt, sx, sy))
    return out


def part_masks(lab, par, K, M):
    """{(k, t): B_t} of one image for the pairs whose mask is not empty."""
    out = {}
    for k in range(K):
        cls = lab == k + 1
        if not cls.any():
            continue
        for t in range(1, M + 1):
            b = cls & (par == t)
            if b.any():
                out[(k, t)] = b
    return out


def component_table(labels, parts, K, M):
    """Sorted [(n, key, count, sum X, sum Y)] over every component of every B_t; key = k * M + t - 1."""
    rows = []
    for n in range(labels.shape[0]):
        for (k, t), b in part_masks(labels[n], parts[n], K, M).items():
            rows += [(n, k * M + t - 1, c, sx, sy) for c, sx, sy in components(b)]
    return sorted(rows)


def _round(sum_, count):
    return int(np.round(np.float64(sum_) / np.float64(count)))      # half to even


def centroids(b):
    """Rounded (x, y) of every component of B_t and of its complement within the image (none when B_t is the whole image)."""
    H, W = b.shape
    comps = components(b)
    pts = [(_round(sx, c), _round(sy, c)) for c, sx, sy in comps]
    cnt = sum(c for c, _, _ in comps)
    if cnt < H * W:
        allx, ally = H * (W * (W - 1) // 2), W * (H * (H - 1) // 2)
        rest = H * W - cnt
        pts.append((_round(allx - sum(s for _, s, _ in comps), rest), _round(ally - sum(s for _, _, s in comps), rest)))
    return pts


# ---- the masked, nearest-upsampled plane and its threshold -------------------------------------------------------------------
def source_index(out, inn):
    """OpenCV INTER_NEAREST: min(floor(d * (1.0 / (out / inn))), inn - 1) in float64, in that order."""
    inv = 1.0 / (np.float64(out) / np.float64(inn))
    return np.minimum(np.floor(np.arange(out, dtype=np.float64) * inv).astype(np.int64), inn - 1)


def masked_plane(plane, cls):
    H, W = cls.shape
    h, w = plane.shape
    up = np.asarray(plane, np.float32)[source_index(H, h)][:, source_index(W, w)]
    return np.where(cls, up, np.float32(0.0)).astype(np.float32)


def rank(q, count):
    virtual = float(q) * (count - 1)
    k = int(math.floor(virtual))
    g = np.float32(virtual - k)
    if g >= 1.0:
        g = np.float32(1.0 - 2.0 ** -24)
    return k, g


def quantile(values, q):
    """np.quantile (linear) of float32 values with the rank from float64 and numpy's _lerp in float32."""
    v = np.sort(np.asarray(values, np.float32).ravel())
    k, g = rank(q, v.size)
    lo, hi = v[k], v[min(k + 1, v.size - 1)]
    d = np.float32(hi - lo)
    if g >= 0.5:
        return np.float32(hi - np.float32(d * np.float32(np.float32(1.0) - g)))
    return np.float32(lo + np.float32(d * g))


def threshold(u, q, mode):
    if mode == "image":
        return quantile(u, q)
    assert mode == "nonzero"
    nz = u[u != 0]
    return quantile(nz, q) if nz.size else np.float32(np.inf)


def slots_of(table, k, C, include):
    return [(j, int(c)) for j, c in enumerate(table[k]) if 0 <= c < C and (include is None or int(c) in include)]


def thresholds(act, labels, table, q, mode, include=None, skip_classes=()):
    """float32 [N, K, J]: NaN for a slot that does not exist or is not included and for a skipped class."""
    act, labels, table = np.asarray(act, np.float32), np.asarray(labels), np.asarray(table)
    N, C = act.shape[:2]
    K, J = table.shape
    include = None if include is None else {int(i) for i in include}
    out = np.full((N, K, J), np.nan, np.float32)
    for n in range(N):
        for k in range(K):
            if k in skip_classes:
                continue
            for j, c in slots_of(table, k, C, include):
                out[n, k, j] = threshold(masked_plane(act[n, c], labels[n] == k + 1), q, mode)
    return out


# ---- presence ----------------------------------------------------------------------------------------------------------------
def presence(act, labels, parts, table, M, q=0.8, mode="nonzero", explicit=None, include=None, skip_classes=()):
    """(table uint8 [N, K, J, M + 1], valid uint8 [N, K]).  ``explicit``: float32 [C] thresholds per channel instead of a mode."""
    act, labels, parts, table = np.asarray(act, np.float32), np.asarray(labels), np.asarray(parts), np.asarray(table)
    N, C = act.shape[:2]
    K, J = table.shape
    include = None if include is None else {int(i) for i in include}
    tab = np.full((N, K, J, M + 1), ABSENT, np.uint8)
    valid = np.zeros((N, K), np.uint8)
    for n in range(N):
        masks = part_masks(labels[n], parts[n], K, M)
        for k in range(K):
            mine = {t: b for (kk, t), b in masks.items() if kk == k}
            if k in skip_classes or not mine:
                continue
            valid[n, k] = 1
            cls = labels[n] == k + 1
            pts = {t: centroids(b) for t, b in mine.items()}
            for j, c in slots_of(table, k, C, include):
                u = masked_plane(act[n, c], cls)
                T = np.float32(explicit[c]) if explicit is not None else threshold(u, q, mode)
                for t, ps in pts.items():
                    tab[n, k, j, t] = 1 if any(u[y, x] > T for x, y in ps) else 0
    return tab, valid


def existing(table, C, include=None):
    table = np.asarray(table)
    ok = (table >= 0) & (table < C)
    if include is not None:
        ok &= np.isin(table, np.asarray(sorted(int(i) for i in include), dtype=np.int64))
    return ok


def consistency(tables, valids, slot_ok, threshold=0.8):
    """The aggregate of consistency.py:165-178 over a list of batches: dict of ones / times int64 [K, J, M + 1], rows int64 [K, J],
    mean float64 [K, J, M + 1], is_consistent int64 [K, J] (-1: the pair has no row), score."""
    K, J, M1 = tables[0].shape[1:]
    ones = np.zeros((K, J, M1), np.int64)
    times = np.zeros((K, J, M1), np.int64)
    rows = np.zeros((K, J), np.int64)
    for tab, valid in zip(tables, valids):
        use = (valid.astype(bool)[:, :, None] & slot_ok[None])[..., None]
        ones += ((tab == 1) & use).sum(0)
        times += ((tab != ABSENT) & use).sum(0)
        rows += use[..., 0].sum(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = ones / times.astype(np.float64)
    mean[times == 0] = np.nan
    with np.errstate(invalid="ignore"):
        flag = (mean > threshold).astype(np.int64)
    cons = flag.max(-1)
    cons[rows == 0] = -1
    have = rows > 0
    score = float(cons[have].mean()) if have.any() else float("nan")
    return {"ones": ones, "times": times, "rows": rows, "mean": mean, "is_consistent": cons, "score": score}


def stability(clean, noisy, valid, slot_ok):
    """(stable rows, valid rows) of one batch: all M + 1 entries agree with absent read as 0."""
    use = valid.astype(bool)[:, :, None] & slot_ok[None]
    same = ((clean == 1) == (noisy == 1)).all(-1)
    return int((same & use).sum()), int(use.sum())


def rows_to_table(rows, table, N, M):
    """Dense (table, valid) of recorded rows float64 [R, M + 4] = (the M + 1 entries with NaN, channel, class, image)."""
    table = np.asarray(table)
    K, J = table.shape
    tab = np.full((N, K, J, M + 1), ABSENT, np.uint8)
    valid = np.zeros((N, K), np.uint8)
    for r in np.asarray(rows):
        c, k, n = (int(v) for v in r[M + 1:])
        j = list(table[k]).index(c)
        tab[n, k, j] = np.where(np.isnan(r[:M + 1]), ABSENT, r[:M + 1]).astype(np.uint8)
        valid[n, k] = 1
    return tab, valid
