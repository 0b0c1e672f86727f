"""Write tests/golden/push_boxes.npz by driving the reference's own ``update_prototypes_on_image``
(segmentation/push_multiscale_optimization.py:341-497) and ``helpers.find_continuous_high_activation_crop`` (CPU only).

    SPX_REFERENCE=/path/to/ScaleProtoSeg python tools/gen_push_boxes_golden.py [output.npz]

The two functions are loaded from the reference checkout and called with stand-ins for everything around them (those of
tools/reference_stubs.py, and):

* a fake ``ppnet`` that returns prepared distances (``conv_features``, ``forward_from_conv_features``,
  ``prototype_class_identity``, ``prototype_shape``, ``num_scales``, ``epsilon``, ``prototype_activation_function``) and a fake
  dataset (``img_ids``, ``get_img_path``, ``annotations_dir``, ``image_margin_size = 0``, ``convert_targets = None``);
* PIL, ``to_normalized_tensor``, ``transforms.ToTensor`` and matplotlib stand-ins that only carry the image size (the "image
  file" of an id is a text file with its size and index); ``dir_for_saving_prototypes=None``, so nothing is plotted;
* the labels as ``.npy`` files in a temporary directory, as the reference loads them.

Data only is recorded, keys ``<case>__<field>``: the latent distances (bf16-representable; ``"log"`` cases, and the identity
case with the ``"linear"`` similarity ``max_dist - d``) or activations (the case with negative planes, recorded through the
helper directly with numpy's percentile as its threshold), labels, identity, per prototype the winning image and flat index,
the reference's two tables, numpy's thresholds and the robustness flag of tests/push_boxes_restatement.py.

Planes are a few smooth bumps plus small noise, so that crops really grow (on noise planes every crop stays at patch +- 5).
The tool asserts what the cases must contain between them (a crop at each image border, a patch in the last latent row and
column, a crop that does not grow, an absent class, T <= 0, ties under >= in the identity case), that the restated walk equals
the reference in every row, and per case that at most 1 row in 8 is non-robust (none in the identity case): the seeds below
satisfy it."""
from __future__ import annotations

import os
import tempfile

import numpy as np
import torch

import reference_stubs as S
import overlap_restatement as R
import push_boxes_restatement as PB

EPS = 1e-4
K = 4                                       # class 3 owns a prototype and occurs in no image


class _Net:
    num_scales = 2
    epsilon = EPS

    def __init__(self, ident, distances, activation, grid):
        self.prototype_class_identity = ident
        self.distances = distances
        self.prototype_activation_function = activation
        self.num_prototypes = ident.shape[0]
        self.prototype_shape = (ident.shape[0], 4, 1, 1)             # max_dist = 4 for the "linear" similarity
        self.grid = grid

    def to(self, _):
        return self

    def conv_features(self, x):
        self.current = x.n
        return torch.empty(1, 1, *self.grid)

    def forward_from_conv_features(self, conv):
        return torch.zeros(1, *self.grid, 2), self.distances[self.current:self.current + 1]


class _Data:
    image_margin_size = 0
    convert_targets = None

    def __init__(self, root, labels):
        self.annotations_dir = root
        self.img_ids = [f"img{n}" for n in range(labels.shape[0])]
        for n, i in enumerate(self.img_ids):
            np.save(os.path.join(root, i + ".npy"), labels[n].astype(np.int64))
            with open(self.get_img_path(i), "w") as fp:
                fp.write(f"{labels.shape[1]} {labels.shape[2]} {n}")

    def get_img_path(self, i):
        return os.path.join(self.annotations_dir, i + ".img")


def _labels(H, W):
    """Two images of large class regions (label k + 1 = class k) with void pieces; class 3 occurs nowhere."""
    lab = np.zeros((2, H, W), np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    lab[0] = np.where(x < 0.6 * W, 1, 2)
    lab[0][(x >= 0.6 * W) & (y >= 0.45 * H) & (y < 0.5 * H)] = 0
    lab[1] = np.where(y < 0.35 * H, 1, np.where(x < 0.45 * W, 3, 2))
    lab[1][(y >= 0.55 * H) & (y < 0.6 * H) & (x >= 0.1 * W) & (x < 0.2 * W)] = 0
    return lab


# (winning image, class, bumps [(cy, cx, sigma, height) in fractions of the latent grid], where the pushed patch lies)
SPECS = (
    (0, 0, [(0.0, 0.0, 0.22, 1.0)], "first"),                          # reaches the top and the left border
    (1, 1, [(1.0, 1.0, 0.22, 1.0)], "last"),                           # last latent row and column; bottom and right border
    (0, 0, [(0.5, 0.25, 0.12, 1.0), (0.2, 0.45, 0.08, 0.6)], "peak"),
    (1, 1, [(0.75, 0.78, 0.10, 1.0)], (0.42, 0.52)),                   # a patch far from the bump: the crop does not grow
    (0, 3, [(0.5, 0.5, 0.15, 1.0)], "peak"),                           # a class that occurs nowhere
    (1, 2, [(0.65, 0.2, 0.10, 1.0), (0.82, 0.34, 0.09, 0.9)], "peak"),
    (0, 1, [(0.3, 0.62, 0.12, 1.0)], "peak"),                          # a bump across the boundary of its class
    (1, 0, [(0.15, 0.5, 0.25, 1.0)], "peak"),                          # a broad bump
)


def _bumps(g, h, w):
    """[P, h, w] in about [0, 1]: the bumps of SPECS plus small noise, and the flat index of every pushed patch."""
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    planes, flat = [], []
    for _, _, bumps, where in SPECS:
        b = torch.zeros(h, w)
        for cy, cx, s, a in bumps:
            r2 = ((yy - cy * (h - 1)) / (s * h)) ** 2 + ((xx - cx * (w - 1)) / (s * w)) ** 2
            b = b + a * torch.exp(-0.5 * r2)
        b = b + 0.02 * torch.rand(h, w, generator=g)
        planes.append(b)
        if where == "first":
            flat.append(0)
        elif where == "last":
            flat.append(h * w - 1)
        elif where == "peak":
            flat.append(int(torch.argmax(b)))
        else:
            flat.append(int(round(where[0] * (h - 1))) * w + int(round(where[1] * (w - 1))))
    return torch.stack(planes), flat


def _place(planes, img):
    """[2, P, h, w]: every image holds a plane of every prototype; the winning image gets the prepared one, the other a
    mirrored decoy."""
    out = torch.stack([planes.flip(1), planes.flip(1)])
    for p, n in enumerate(img):
        out[n, p] = planes[p]
    return out


def _numpy_side(planes, labels, img, cls, flat, identity=False):
    """numpy's thresholds and the restatement's tables and robustness flags, per prototype."""
    P = len(img)
    thr = np.zeros(P, np.float32)
    robust = np.zeros(P, bool)
    rf = np.zeros((P, 6), np.int64)
    box = np.zeros((P, 6), np.int64)
    for p in range(P):
        got = PB.boxes(planes[img[p], p], labels[img[p]], cls[p], flat[p])
        thr[p], robust[p] = got["threshold"], got["robust"]
        rf[p] = [img[p], *got["rf"], cls[p]]
        box[p] = [img[p], *got["box"], cls[p]]
    bad = int((~robust).sum())
    assert bad <= (0 if identity else P // 8), (bad, P)
    return thr, robust, rf, box


def _features(ref_rf, ref_box, H, W):
    """What a case shows: the borders its crops reach, a patch box past the image, a crop that did not grow."""
    out = set()
    for r, b in zip(ref_rf, ref_box):
        out |= {n for n, hit in (("top", b[1] == 0), ("bottom", b[2] == H), ("left", b[3] == 0), ("right", b[4] == W)) if hit}
        if r[2] > H and r[4] > W:
            out.add("rf_past_image")
        still = [max(r[1] - 5, 0), min(r[2] + 5, H - 1) + 1, max(r[3] - 5, 0), min(r[4] + 5, W - 1) + 1]
        if list(b[1:5]) == still:
            out.add("no_growth")
        else:
            out.add("growth")
    return out


def _reference_case(name, PUSH, seed, h, w, H, W, identity=False):
    g = torch.Generator().manual_seed(seed)
    P = len(SPECS)
    img = [s[0] for s in SPECS]
    cls = [s[1] for s in SPECS]
    ident = torch.zeros(P, K)
    ident[torch.arange(P), torch.tensor(cls)] = 1
    b, flat = _bumps(g, h, w)
    if identity:
        d = torch.round((3.5 * (1.0 - b.clamp(0, 1)) + 0.25) * 4.0) / 4.0          # multiples of 0.25 in [0.25, 3.75]
    else:
        d = 1.5 * (1.0 - b).clamp_min(0) + 0.05
    d = S.bf16(_place(d, img))
    labels = _labels(H, W)
    net = _Net(ident, d, "linear" if identity else "log", (h, w))
    ref_rf = np.full((P, 6), -1)
    ref_box = np.full((P, 6), -1)
    with tempfile.TemporaryDirectory() as root:
        data = _Data(root, labels)
        patches = [torch.tensor([flat]) for _ in range(labels.shape[0])]
        PUSH.update_prototypes_on_image(data, net, img, patches, ref_rf, ref_box, cls2name={}, dir_for_saving_prototypes=None)
    dn = d.numpy()
    planes = (np.float32(4.0) - dn) if identity else np.log((dn + 1) / (dn + EPS))   # as the reference computes them, float32
    assert planes.dtype == np.float32
    thr, robust, rf, box = _numpy_side(planes, labels, img, cls, flat, identity)
    assert np.array_equal(rf, ref_rf) and np.array_equal(box, ref_box), name       # the restated walk = the reference's
    feats = _features(ref_rf, ref_box, H, W)
    out = dict(kind=np.array("linear" if identity else "log"), distances=dn, ident=ident.numpy(), labels=labels,
               img=np.array(img, np.int64), flat=np.array(flat, np.int64), ref_rf=ref_rf.astype(np.int64),
               ref_box=ref_box.astype(np.int64), thresholds=thr, robust=robust)
    if identity:
        ties = sum(int((planes[img[p], p] == thr[p]).sum()) for p in range(P))
        assert ties > 0, "the identity case must hold values equal to their threshold"
    print(name, "non-robust", int((~robust).sum()), sorted(feats), "growth h/w",
          [(int(b_[2] - b_[1] - (r_[2] - r_[1])), int(b_[4] - b_[3] - (r_[4] - r_[3]))) for r_, b_ in zip(ref_rf, ref_box)])
    return {f"{name}__{k}": v for k, v in out.items()}, feats


def _negative_case(name, HELP, seed, h, w, H, W):
    """Negative activations, T <= 0: every pixel outside the class is a hit.  Recorded through the helper directly."""
    g = torch.Generator().manual_seed(seed)
    P = len(SPECS)
    img = [s[0] for s in SPECS]
    cls = [s[1] for s in SPECS]
    ident = torch.zeros(P, K)
    ident[torch.arange(P), torch.tensor(cls)] = 1
    b, flat = _bumps(g, h, w)
    a = S.bf16(_place(b - 2.0, img)).numpy()
    labels = _labels(H, W)
    ref_rf = np.full((P, 6), -1, np.int64)
    ref_box = np.full((P, 6), -1, np.int64)
    for p in range(P):
        u32 = R.upsample(a[img[p], p], (H, W)).astype(np.float32)
        T = np.percentile(u32, 95)
        assert T <= 0
        rf = PB.rf_box(flat[p], h, w, H, W)
        masked = u32 * (labels[img[p]] == cls[p] + 1)
        ref_rf[p] = [img[p], *rf, cls[p]]
        ref_box[p] = [img[p], *HELP.find_continuous_high_activation_crop(masked, rf, threshold=T), cls[p]]
    thr, robust, rf, box = _numpy_side(a, labels, img, cls, flat)
    assert np.array_equal(rf, ref_rf) and np.array_equal(box, ref_box), name
    print(name, "non-robust", int((~robust).sum()), "thresholds", thr.min(), thr.max())
    out = dict(kind=np.array("act"), activations=a, ident=ident.numpy(), labels=labels, img=np.array(img, np.int64),
               flat=np.array(flat, np.int64), ref_rf=ref_rf, ref_box=ref_box, thresholds=thr, robust=robust)
    return {f"{name}__{k}": v for k, v in out.items()}


def main():
    S.stub_modules()
    HELP = S.load("helpers.py", "helpers")
    PUSH = S.load(os.path.join("segmentation", "push_multiscale_optimization.py"), "ref_push_multiscale_optimization")
    cases, feats = {}, set()
    shapes = (("s5x7", 5, 7, 33, 50), ("s9x11", 9, 11, 70, 85), ("s17x17", 17, 17, 129, 129), ("s33x65", 33, 65, 257, 513))
    seed = 20241018
    for tag, h, w, H, W in shapes:
        seed += 1
        c, f = _reference_case(f"log_{tag}", PUSH, seed, h, w, H, W)
        cases.update(c)
        feats |= f
    c, f = _reference_case("exact_70x85", PUSH, seed + 1, 70, 85, 70, 85, identity=True)
    cases.update(c)
    cases.update(_negative_case("negative_9x11", HELP, seed + 2, 9, 11, 70, 85))
    want = {"top", "bottom", "left", "right", "rf_past_image", "no_growth", "growth"}
    assert want <= feats, want - feats
    out = S.out_path("push_boxes.npz")
    np.savez_compressed(out, **cases)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
