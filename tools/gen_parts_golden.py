"""Write tests/golden/part_consistency.npz by driving the reference's own ``consistency.part_intersect``
(segmentation/analysis/metrics/consistency.py:186-270) whole, on the CPU.

    SPX_REFERENCE=/path/to/ScaleProtoSeg python tools/gen_parts_golden.py [output.npz]

The function is loaded from the reference checkout with the stand-ins of tools/reference_stubs.py around it and these of its own:

* ``cv2.connectedComponentsWithStats``: ``scipy.ndimage.label`` with a 3 x 3 structure plus the per-label coordinate means, the
  background row first (``cv2`` is not needed and was never run against this);
* ``cv2.resize(INTER_NEAREST)``: the source-index rule of tests/consistency_restatement.py;
* ``segmentation.analysis.equivariance.quantile_map``, which the reference checkout does not contain: one stand-in per threshold
  rule, ``"image"``, ``"nonzero"`` and explicit per-prototype values (the reference's own ``quantiles.json`` branch is dead code
  behind ``quantiles = None``, so the explicit values enter here too; the prototype is read off the reference's own indexing of
  the distance array);
* a fake ``ppnet`` that returns prepared distances.

SciPy and pandas are used by this tool only.  Data only is recorded: the inputs (distances, the activations ``log((d + 1) / (d +
eps))`` in NumPy float32 as the reference forms them, labels, parts, the class identity), per case the rows the reference returned
(``rows__<case>`` float64 [R, M + 4] = the M + 1 presence entries with NaN, prototype, class, image) and the aggregate computed with
real pandas on those rows (``mean__<case>`` [G, M + 3] = class, prototype, the M + 1 nan-means; ``cons__<case>`` [G]; ``score__<case>``).

The tool asserts per case that the reference ran without raising (no ``B_t`` covers a whole image, no part id exceeds M), that the
restatement reproduces every row and the aggregate, that ``"nonzero"`` gives mixed 0 / 1 rows and that ``"image"`` has a 0 (it needs
a class that covers more than ``q`` of an image)."""
from __future__ import annotations

import numpy as np
import pandas as pd
import torch
from scipy import ndimage

import reference_stubs as S
import consistency_restatement as CR

K, P, M = 3, 6, 4
h, w, H, W = 5, 7, 37, 53
Q = 0.8
EPS = 1e-4
SKIP = (2,)                     # the filtered case: class 2 skipped, prototypes 1 and 4 dropped
INCLUDE = (0, 2, 3, 5)


# ---- stand-ins ---------------------------------------------------------------------------------------------------------------
def _components_with_stats(mask, connectivity, ltype):
    assert connectivity == 8 and ltype == "CV_32S" and mask.dtype == np.uint8
    lab, n = ndimage.label(mask, structure=np.ones((3, 3), int))
    assert (lab == 0).any(), "a part covers the whole image: the reference's background centroid is NaN"
    cents = []
    for i in range(n + 1):
        ys, xs = np.nonzero(lab == i)
        cents.append((xs.mean(), ys.mean()))
    return n + 1, lab, None, np.array(cents, np.float64)


def _resize_nearest(src, dsize, interpolation):
    assert interpolation == "INTER_NEAREST" and src.dtype == np.float32
    if src.ndim == 3 and src.shape[2] == 1:                   # a one-channel image comes back 2-D from cv2.resize
        src = src[:, :, 0]
    return src[CR.source_index(dsize[1], src.shape[0])][:, CR.source_index(dsize[0], src.shape[1])]


class _Recording(np.ndarray):
    """The distance array the reference indexes with ``[:, :, p]``: remembers p for the explicit-threshold stand-in."""

    last = None

    def __getitem__(self, key):
        if isinstance(key, tuple) and len(key) == 3:
            _Recording.last = int(np.asarray(key[2]).reshape(-1)[0])
        return np.asarray(self).__getitem__(key)


class _Dist:
    """What ``distances[0]`` is to the reference: everything up to ``.numpy()``."""

    def __init__(self, d):
        self.d = d

    def __getitem__(self, i):
        assert i == 0
        return _Dist(self.d[0])

    def permute(self, *order):
        return _Dist(self.d.permute(*order))

    def detach(self):
        return self

    cpu = detach

    def numpy(self):
        return self.d.numpy().view(_Recording)


class _Net:
    epsilon = EPS

    def __init__(self, distances, identity):
        self.distances, self.prototype_class_identity = distances, identity

    def conv_features(self, img):
        return img

    def forward_from_conv_features(self, img):
        return None, _Dist(self.distances[img.n:img.n + 1])


RULE = {"mode": None, "explicit": None}


def _quantile_map(u, q):
    u = u.numpy()[0]
    if RULE["explicit"] is not None:
        T = np.float32(RULE["explicit"][_Recording.last])
    elif RULE["mode"] == "image":
        T = np.quantile(u, q)
    else:
        nz = u[u != 0]
        T = np.quantile(nz, q) if nz.size else np.inf
    return torch.from_numpy((u > T)[:, :, None])


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def _blocky(g, values, rows, cols):
    by, bx = max(1, H // rows), max(1, W // cols)
    grid = np.asarray(values)[torch.randint(0, len(values), (H // by + 1, W // bx + 1), generator=g).numpy()]
    return np.kron(grid, np.ones((by, bx), np.int64))[:H, :W]


def _inputs():
    g = torch.Generator().manual_seed(20250907)
    N = 4
    lab = np.zeros((N, H, W), np.uint8)
    par = np.zeros((N, H, W), np.int16)
    lab[0] = _blocky(g, [0, 1, 2, 3], 4, 5)
    lab[1] = 2                                                 # class 1 covers more than q of the image
    lab[1, :6, :9] = 0
    lab[1, 30:, 40:] = 1
    lab[2] = _blocky(g, [0, 1, 3], 3, 3)                       # class 1 absent
    lab[3] = _blocky(g, [1, 2, 3], 5, 6)
    lab[0, H - 1, W - 1] = K + 2                               # no class: void for the reference
    for n in range(N):
        par[n] = _blocky(g, [-1, 0, 1, 2, 3, 4], 6, 8)
    par[3][lab[3] == 3] = 0                                    # a class that occurs without any part: its row is not valid
    par[0, 5, 5:9] = 2                                         # thin pieces and single pixels
    par[2, 20, 20] = 4
    d = (4.0 * torch.rand(N, P, h, w, generator=g)).to(torch.float32)
    d[:, :, 0, 0] = 0.0
    identity = torch.zeros(P, K)
    identity[torch.arange(P), torch.arange(P) % K] = 1         # class k owns prototypes k, k + 3
    return lab, par, d.contiguous(), identity


def _aggregate(rows, threshold=0.8):
    """The aggregate with real pandas: nan-mean per (class, prototype), flag above the threshold, maximum over the parts."""
    cols = [f"part_{i}" for i in range(M + 1)]
    df = pd.DataFrame(rows, columns=cols + ["proto_id", "class", "img_id"])
    means = df.groupby(["class", "proto_id"])[cols].mean().reset_index()          # pandas' mean skips NaN
    cons = (means[cols] > threshold).astype(int).max(axis=1)
    table = means[["class", "proto_id"] + cols].to_numpy(np.float64)
    return table, cons.to_numpy(np.int64), float(cons.mean())


def main():
    S.stub_modules()
    S.mod("cv2", resize=_resize_nearest, INTER_NEAREST="INTER_NEAREST", CV_32S="CV_32S", connectedComponentsWithStats=_components_with_stats)
    names = ("CITYSCAPES_19_EVAL_CATEGORIES", "CITYSCAPES_CATEGORIES", "PASCAL_CATEGORIES", "PASCAL_ID_MAPPING")
    S.mod("segmentation.constants", MAX_PARTS_CITY=M, MAX_PARTS_PASCAL=M, PASCAL_FILTER_CLASS=[], **{n: {} for n in names})
    S.mod("segmentation.analysis").__path__ = []
    S.mod("segmentation.analysis.equivariance", quantile_map=_quantile_map)
    CONS = S.load("segmentation/analysis/metrics/consistency.py")
    CONS.MAX_PARTS = M

    lab, par, d, identity = _inputs()
    N = lab.shape[0]
    assert par.max() <= M
    act = np.log((d.numpy() + 1) / (d.numpy() + EPS)).astype(np.float32)
    assert act.dtype == np.float32
    table = np.full((K, P // K), -1, np.int64)
    for k in range(K):
        table[k] = np.flatnonzero(identity[:, k].numpy())
    explicit = np.quantile(act.transpose(1, 0, 2, 3).reshape(P, -1), 0.6, axis=1).astype(np.float32)
    ref_lab = S.for_reference(lab, K)
    net = _Net(d, identity)
    cases = {"nonzero": ("nonzero", None, None, ()), "image": ("image", None, None, ()), "explicit": (None, explicit, None, ()),
             "filtered": ("nonzero", None, INCLUDE, SKIP)}
    out = {"distances": d.numpy(), "activations": act, "labels": lab, "parts": par, "identity": identity.numpy().astype(np.uint8),
           "slot_table": table, "explicit": explicit, "include": np.array(INCLUDE), "skip": np.array(SKIP),
           "q": np.float64(Q), "max_parts": np.int64(M), "epsilon": np.float64(EPS)}
    for name, (mode, thr, include, skip) in cases.items():
        RULE["mode"], RULE["explicit"] = mode, thr
        rows = []
        for n in range(N):
            _, got = CONS.part_intersect(S.Sized(H, W, n), ref_lab[n].astype(np.int64), par[n].astype(np.int64), net,
                                         {k: k for k in range(K)}, n, Q, None if include is None else list(include),
                                         [k + 1 for k in skip], None)
            rows += got
        rows = np.array(rows, np.float64)
        tab, valid = CR.presence(act, lab, par, table, M, Q, mode or "nonzero", thr, include, skip)
        want = rows_of(tab, valid, table)
        assert want.shape == rows.shape and np.array_equal(want, rows, equal_nan=True), f"{name}: the restatement != the reference"
        mean, cons, score = _aggregate(rows)
        agg = CR.consistency([tab], [valid], CR.existing(table, P, include))
        for r, (k, p) in enumerate(mean[:, :2].astype(int)):
            j = list(table[k]).index(p)
            assert np.array_equal(agg["mean"][k, j], mean[r, 2:], equal_nan=True) and agg["is_consistent"][k, j] == cons[r]
        assert (agg["rows"] > 0).sum() == len(cons) and agg["score"] == score, f"{name}: aggregate"
        body = rows[:, :M + 1]
        if name == "nonzero":
            assert (body == 0).any() and (body == 1).any() and np.isnan(body).any()
        if name == "image":
            assert (body == 0).any(), "image mode is all ones: no class covers more than q of an image"
        out[f"rows__{name}"], out[f"mean__{name}"], out[f"cons__{name}"], out[f"score__{name}"] = rows, mean, cons, np.float64(score)
        print(name, rows.shape, "zeros", int((body == 0).sum()), "ones", int((body == 1).sum()), "score", score)
    path = S.out_path("part_consistency.npz")
    np.savez_compressed(path, **out)
    print("wrote", path)


def rows_of(tab, valid, table):
    """The reference's row order from a dense table: images, classes ascending, the class's prototypes ascending."""
    rows = []
    for n in range(tab.shape[0]):
        for k in range(tab.shape[1]):
            if not valid[n, k]:
                continue
            for j, p in enumerate(table[k]):
                if p < 0 or (tab[n, k, j] == CR.ABSENT).all():
                    continue
                body = np.where(tab[n, k, j] == CR.ABSENT, np.nan, tab[n, k, j].astype(np.float64))
                rows.append(list(body) + [p, k, n])
    return np.array(rows, np.float64)


if __name__ == "__main__":
    main()
