"""A second statement of ``msc_max`` (scaleprotoseg_amd/msc.py) in NumPy float64, with error bounds for an fp32 implementation.

It is not a copy of the kernel's fp32 steps: the source position is taken EXACTLY from the rational ``h_k / H`` in integer
arithmetic (``s = max(0, h (2 Y + 1) - H) / (2 H)``), the blend is float64, and the gradient is a pair of dense weight matrices.

Bounds (u = 2^-24, the unit roundoff of fp32):

* forward, candidate k >= 1:  ``3 u (h_k + w_k) (max tap - min tap) + 6 u max|tap|``.  The first term is the fp32 error of ``s``
  - of the order of ulp(h_k), as ``r (Y + 0.5) - 0.5`` is formed at the magnitude of the source index - turned into a weight
  error and multiplied by the range of the four taps (a weight error moves the blend inside that range only; the same holds when
  the rounding moves ``floor(s)`` across an integer, as the blend is continuous there).  The second is the six roundings of the
  blend.  Candidate 0 is the input itself: bound zero.
* the maximum: every candidate that can reach the largest lower end ``max_j (u_j - bound_j)`` may be the fp32 winner, so the
  bound of ``z`` is the largest bound among those contenders.
* gradient of map k >= 1, per source element: per contributing destination pixel the weight error ``3 u (h_k + w_k) |g'|`` over
  the footprint widened by one source index on each side (where fp32 may place a weight the exact rule does not), and one
  rounding per operation of a term (the two ``1 - l``, the two weight sums, the two products, the derivative's three) plus one per
  addition of the running sum: ``(9 + N) u |term|`` with N the pixels that may contribute.  Map 0 receives ``g'`` itself:
  ``3 u |g'|`` when a derivative was multiplied in, else zero.
"""
import numpy as np

U = 2.0 ** -24


def axis(n, D):
    """(i0, i1, lam) of the D destination indices on an axis of n source elements; lam exact up to one float64 rounding."""
    Y = np.arange(D, dtype=np.int64)
    num = np.maximum(0, n * (2 * Y + 1) - D)            # s = num / (2 D)
    i0 = np.minimum(num // (2 * D), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    lam = (num - i0 * 2 * D) / (2.0 * D)
    return i0, i1, lam


def weights(n, D):
    """Dense [D, n]: row Y holds (1 - lam) at i0 and lam at i1 (both on one column where they coincide)."""
    i0, i1, lam = axis(n, D)
    Wm = np.zeros((D, n))
    np.add.at(Wm, (np.arange(D), i0), 1.0 - lam)
    np.add.at(Wm, (np.arange(D), i1), lam)
    return Wm


def candidates(maps):
    """maps: list of [B, C, h_k, w_k] arrays -> (u [K, B, C, H, W] float64, bound [K, B, C, H, W])."""
    maps = [np.asarray(m, dtype=np.float64) for m in maps]
    H, W = maps[0].shape[2:]
    us, bs = [maps[0]], [np.zeros_like(maps[0])]
    for m in maps[1:]:
        h, w = m.shape[2:]
        i0, i1, ly = axis(h, H)
        j0, j1, lx = axis(w, W)
        ly, lx = ly[:, None], lx[None, :]
        v00, v01 = m[:, :, i0][:, :, :, j0], m[:, :, i0][:, :, :, j1]
        v10, v11 = m[:, :, i1][:, :, :, j0], m[:, :, i1][:, :, :, j1]
        u = (1 - ly) * ((1 - lx) * v00 + lx * v01) + ly * ((1 - lx) * v10 + lx * v11)
        taps = np.stack([v00, v01, v10, v11])
        with np.errstate(invalid="ignore"):
            rng = taps.max(0) - taps.min(0)
            big = np.abs(taps).max(0)
        us.append(u)
        bs.append(3 * U * (h + w) * rng + 6 * U * big)
    return np.stack(us), np.stack(bs)


def argmax_first(u):
    """torch.max(dim=0): the lowest k among equal values; a NaN wins and the first NaN stays."""
    best, idx = u[0].copy(), np.zeros(u[0].shape, dtype=np.uint8)
    for k in range(1, u.shape[0]):
        with np.errstate(invalid="ignore"):
            take = (u[k] > best) | (np.isnan(u[k]) & ~np.isnan(best))
        best = np.where(take, u[k], best)
        idx = np.where(take, np.uint8(k), idx)
    return best, idx


def forward(maps):
    """-> (z float64, index uint8, bound of z, u, bound of every candidate)."""
    u, b = candidates(maps)
    z, idx = argmax_first(u)
    with np.errstate(invalid="ignore"):
        floor_ = np.max(u - b, axis=0)
        contender = (u + b) >= floor_[None]
    zb = np.max(np.where(contender, b, 0.0), axis=0)
    return z, idx, zb, u, b


def decided(u, b):
    """Where the float64 argmax is safe from fp32 rounding: the gap between the best and the second candidate exceeds the sum of
    their bounds (always true with one candidate; false where a NaN is involved)."""
    if u.shape[0] == 1:
        return np.ones(u.shape[1:], dtype=bool)
    order = np.argsort(-u, axis=0, kind="stable")
    first, second = order[0][None], order[1][None]
    gap = np.take_along_axis(u, first, 0)[0] - np.take_along_axis(u, second, 0)[0]
    room = np.take_along_axis(b, first, 0)[0] + np.take_along_axis(b, second, 0)[0]
    with np.errstate(invalid="ignore"):
        return gap > room


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-np.asarray(z, dtype=np.float64)))


def _widen(Wm):
    """The footprint of a weight matrix widened by one source index on each side."""
    F = Wm > 0
    out = F.copy()
    out[:, 1:] |= F[:, :-1]
    out[:, :-1] |= F[:, 1:]
    return out.astype(np.float64)


def gradients(shapes, index, gprime, derivative=False):
    """Float64 gradients of every map for a GIVEN index map.  ``shapes``: the (h_k, w_k) of the maps; ``gprime``: the upstream
    gradient with the activation's derivative already multiplied in ([B, C, H, W]).  -> (list of grads, list of bounds)."""
    gprime = np.asarray(gprime, dtype=np.float64)
    H, W = shapes[0]
    grads, bounds = [], []
    for k, (h, w) in enumerate(shapes):
        m = (np.asarray(index) == k).astype(np.float64)
        gm = gprime * m
        if k == 0:
            grads.append(gm)
            bounds.append((3 * U if derivative else 0.0) * np.abs(gm))
            continue
        Wy, Wx = weights(h, H), weights(w, W)
        Fy, Fx = _widen(Wy), _widen(Wx)
        fold = lambda A, t, B_: np.einsum("Yi,bcYX,Xj->bcij", A, t, B_)
        grads.append(fold(Wy, gm, Wx))
        n = fold(Fy, m, Fx)
        bounds.append(U * (3 * (h + w) * fold(Fy, np.abs(gm), Fx) + (9 + n) * fold(Wy, np.abs(gm), Wx)))
    return grads, bounds
