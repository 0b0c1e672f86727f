"""Write tests/golden/batch_prepare.npz by driving the reference's own ``PatchClassificationDataset.__getitem__``
(segmentation/data/dataset.py:116-198) and ``resize_label`` (dataset.py:22-30) under ``random.seed(s)`` on a temporary folder of
small ``.npy`` samples, on the CPU.

    SPX_REFERENCE=/path/to/ScaleProtoSeg python tools/gen_batch_golden.py [output.npz]

The file is loaded from the reference checkout (``reference_stubs.load``) with these stand-ins around it; PIL is the real one:

* ``gin``: ``configurable`` hands the class back, ``REQUIRED`` is a marker;
* ``torchvision``: ``VisionDataset`` keeps ``root`` / ``transform``, ``Compose`` and ``Normalize`` do in the tensor's own float64
  what torchvision's do (``(t - mean) / std`` per channel), ``ColorJitter`` raises (no case uses it);
* ``settings``: ``data_path`` points at the temporary folder, ``log`` is silent;
* ``segmentation.constants``: two small id tables of this tool's own (the raw values its samples hold);
* ``cv2``: OpenCV is not needed and was never run: ``resize`` ASSERTS that the target is the source's own size (scale 1.0, where
  ``INTER_LINEAR`` is the identity) and otherwise returns a marker image, after which the case's image is NOT recorded;
  ``copyMakeBorder`` is ``np.pad`` with the constant the reference passes;
* the module's ``random`` is wrapped so that the values it draws are recorded next to the outputs.

Data only is recorded, per case ``<k>``: ``image__<k>`` uint8 (margin included), ``label__<k>`` raw, ``meta__<k>`` int64 [margin,
Hc, Wc, hs, ws, y0, x0, flip, has_image, has_id_map], ``id_map__<k>``, ``mean_std__<k>`` float64 [2, 3], ``grids__<k>`` int64 [G, 2],
``seed__<k>`` int64 [1], ``scales__<k>`` float64 [1 or 2] and ``window_is_label__<k>`` int64 [1] (what the case's data set was
built with), ``out_label__<k>`` int64 [Hc, Wc], ``out_image__<k>`` float64 [3, Hc, Wc] (scale 1.0 only), ``latent<g>__<k>`` int64.  The tool
asserts that tests/batch_restatement.py reproduces every recorded label bit for bit and every recorded image within its bound."""
from __future__ import annotations

import json
import os
import random
import tempfile

import numpy as np
import torch

import reference_stubs as S
import batch_restatement as BR

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
ID_TABLE = {i: (i * 7 + 3) % 6 for i in range(12)}           # raw 0..11 -> class id 0..5
# name, (h, w), margin, window (None: the label's shape), scales, seed, data type, latent grids
CASES = [
    ("identity", (37, 53), 0, (33, 41), (1.0,), 9, "ade", [(5, 6), (9, 11), (33, 41)]),
    ("identity_pad", (23, 31), 2, (33, 41), (1.0,), 5, "ade", [(5, 6), (9, 11)]),
    ("identity_full", (19, 27), 0, None, (1.0,), 7, "pascal", [(3, 4)]),
    ("scaled_small", (23, 31), 0, (33, 41), (0.5, 0.7), 11, "ade", [(5, 6), (33, 41)]),
    ("scaled_large", (40, 40), 3, (33, 41), (1.3, 1.5), 12, "cityscapes", [(9, 11)]),
    ("scaled_mixed", (37, 53), 0, (33, 41), (0.5, 1.5), 17, "ade", [(5, 6)]),
    ("scaled_flip", (37, 53), 1, (17, 65), (0.5, 1.5), 23, "pascal", [(3, 9), (17, 65)]),
    ("scaled_mixed2", (45, 29), 0, (33, 41), (0.5, 1.5), 31, "ade", [(5, 6)]),
]
MARKER = 77


class _Random:
    """The module ``random`` with a log of what was drawn."""

    def __init__(self):
        self.log = []

    def _wrap(name):
        def f(self, *a):
            v = getattr(random, name)(*a)
            self.log.append((name, v))
            return v
        return f

    uniform, randint, random = _wrap("uniform"), _wrap("randint"), _wrap("random")


class _Normalize:
    def __init__(self, mean, std):
        self.mean, self.std = mean, std

    def __call__(self, t):
        m = torch.as_tensor(self.mean, dtype=t.dtype)[:, None, None]
        s = torch.as_tensor(self.std, dtype=t.dtype)[:, None, None]
        return (t - m) / s


class _Compose:
    def __init__(self, ts):
        self.ts = ts

    def __call__(self, t):
        for f in self.ts:
            t = f(t)
        return t


class _VisionDataset:
    def __init__(self, root=None, transform=None, target_transform=None):
        self.root, self.transform, self.target_transform = root, transform, target_transform


def _no_jitter(*a, **kw):
    raise AssertionError("ColorJitter is out of scope")


STATE = {"resized": False}


def _resize(image, dsize, interpolation):
    assert interpolation == "INTER_LINEAR" and image.dtype == np.uint8
    if (dsize[1], dsize[0]) == image.shape[:2]:
        return image.copy()                                  # scale 1.0: the identity
    STATE["resized"] = True
    return np.full((dsize[1], dsize[0], image.shape[2]), MARKER, np.uint8)


def _make_border(src, top, bottom, left, right, borderType, value):
    assert borderType == "BORDER_CONSTANT" and top == 0 and left == 0
    if src.ndim == 2:
        return np.pad(src, ((0, bottom), (0, right)), constant_values=value)
    out = np.empty((src.shape[0] + bottom, src.shape[1] + right, src.shape[2]), src.dtype)
    out[:] = np.asarray(value, dtype=src.dtype)
    out[:src.shape[0], :src.shape[1]] = src
    return out


def main():
    tmp = tempfile.mkdtemp()
    S.mod("gin", configurable=lambda **kw: (lambda cls: cls), REQUIRED=object())
    S.mod("cv2", resize=_resize, copyMakeBorder=_make_border, INTER_LINEAR="INTER_LINEAR", BORDER_CONSTANT="BORDER_CONSTANT")
    S.mod("torchvision", transforms=S.mod("torchvision.transforms", Compose=_Compose, Normalize=_Normalize, ColorJitter=_no_jitter),
          datasets=S.mod("torchvision.datasets", VisionDataset=_VisionDataset))
    S.mod("settings", data_path={k: os.path.join(tmp, k) for k in ("ade", "pascal", "cityscapes")}, log=lambda *a: None)
    S.mod("segmentation").__path__ = []
    S.mod("segmentation.constants", CITYSCAPES_19_EVAL_CATEGORIES=ID_TABLE, PASCAL_ID_MAPPING=ID_TABLE)
    D = S.load("segmentation/data/dataset.py")
    rec = _Random()
    D.random = rec

    out = {"cases": np.array([c[0] for c in CASES])}
    g = np.random.default_rng(20240229)
    n_images, image_flips = 0, set()
    for name, (h, w), m, window, scales, seed, dtype_, grids in CASES:
        root = os.path.join(tmp, dtype_)
        img_dir = os.path.join(root, f"img_with_margin_{m}", "train")
        ann_dir = os.path.join(root, "annotations", "train")
        os.makedirs(img_dir, exist_ok=True)
        os.makedirs(ann_dir, exist_ok=True)
        image = g.integers(0, 256, (h + 2 * m, w + 2 * m, 3)).astype(np.uint8)
        blocks = g.integers(0, 12 if dtype_ != "ade" else 7, (h // 5 + 1, w // 7 + 1))
        label = np.kron(blocks, np.ones((5, 7), np.int64))[:h, :w].astype(np.uint8 if dtype_ == "ade" else np.int64)
        np.save(os.path.join(img_dir, name + ".npy"), image)
        np.save(os.path.join(ann_dir, name + ".npy"), label)
        with open(os.path.join(root, "all_images.json"), "w") as fp:
            json.dump({"train": [name]}, fp)
        ds = D.PatchClassificationDataset("train", False, data_type=dtype_, mean=MEAN, std=STD, image_margin_size=m,
                                          window_size=window, scales=scales)
        rec.log.clear()
        STATE["resized"] = False
        random.seed(seed)
        ref_image, ref_label = ds[0]
        drawn = list(rec.log)
        f = 1.0
        if len(scales) >= 2:
            assert drawn[0][0] == "uniform"
            f = drawn.pop(0)[1]
        assert [d[0] for d in drawn] == ["randint", "randint", "random"]
        hs, ws = int(h * f), int(w * f)
        y0, x0, flip = drawn[0][1], drawn[1][1], drawn[2][1] < 0.5
        Hc, Wc = window if window is not None else (h, w)
        has_image = not STATE["resized"]
        assert has_image == (len(scales) < 2)
        id_map = None if dtype_ == "ade" else np.array([ID_TABLE[i] for i in range(12)], np.int64)
        ref_label = ref_label.numpy()
        assert ref_label.shape == (Hc, Wc) and ref_label.dtype == np.int64
        latents = [D.resize_label(ref_label, (wg, hg)).numpy() for hg, wg in grids]

        # the restatement reproduces what the reference returned
        inner = image[m:image.shape[0] - m, m:image.shape[1] - m] if m else image
        mine = BR.window_label(label, id_map, (hs, ws), (y0, x0), flip, (Hc, Wc))
        assert np.array_equal(mine, ref_label), name
        for got, want in zip(BR.latent_labels(mine, grids), latents):
            assert np.array_equal(got, want), name
        out[f"image__{name}"], out[f"label__{name}"] = image, label
        out[f"meta__{name}"] = np.array([m, Hc, Wc, hs, ws, y0, x0, int(flip), int(has_image), int(id_map is not None)], np.int64)
        out[f"seed__{name}"] = np.array([seed], np.int64)
        out[f"scales__{name}"] = np.array(scales, np.float64)
        out[f"window_is_label__{name}"] = np.array([int(window is None)], np.int64)
        out[f"id_map__{name}"] = id_map if id_map is not None else np.zeros(0, np.int64)
        out[f"mean_std__{name}"] = np.array([MEAN, STD], np.float64)
        out[f"grids__{name}"] = np.array(grids, np.int64)
        out[f"out_label__{name}"] = ref_label
        for k, lat in enumerate(latents):
            out[f"latent{k}__{name}"] = lat
        if has_image:
            ref64 = ref_image.numpy()
            assert ref64.dtype == np.float64 and ref64.shape == (3, Hc, Wc)
            got = BR.window_image_f32(inner, (hs, ws), (y0, x0), flip, (Hc, Wc), MEAN, STD)
            assert (np.abs(got.astype(np.float64) - ref64) <= BR.image_bound(ref64, MEAN, STD)).all(), name
            out[f"out_image__{name}"] = ref64
            n_images += 1
            image_flips.add(bool(flip))
        print(f"{name}: scaled {hs} x {ws}, origin ({y0}, {x0}), flip {flip}, image {'recorded' if has_image else 'not recorded'}")
    assert n_images >= 3 and image_flips == {False, True}
    path = S.out_path("batch_prepare.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
