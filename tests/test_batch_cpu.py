"""CPU checks of the training-batch preparation's definition: tests/batch_restatement.py against PIL and against what
tools/gen_batch_golden.py recorded from the reference's own ``PatchClassificationDataset.__getitem__`` (tests/golden/
batch_prepare.npz), ``draw_augmentation`` against a restatement of the reference's draws and against the draws its own run recorded, and the argument errors of
scaleprotoseg_amd.batch, which need neither a GPU nor the library."""
import os
import random
import sys

import numpy as np
import pytest
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import batch_restatement as BR  # noqa: E402

import scaleprotoseg_amd as spx  # noqa: E402
from scaleprotoseg_amd import batch as B_  # noqa: E402
from scaleprotoseg_amd.utils import _pil_nearest_index  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(HERE, "golden", "batch_prepare.npz")))


def random_cases(n, seed=7):
    """(source size, scale in [0.5, 1.5], window, origin, flip, latent grid) tuples."""
    g = random.Random(seed)
    for _ in range(n):
        h, w = g.randint(8, 70), g.randint(8, 70)
        f = g.uniform(0.5, 1.5)
        hs, ws = int(h * f), int(w * f)
        Hc, Wc = g.randint(5, 60), g.randint(5, 60)
        y0, x0 = g.randint(0, max(hs, Hc) - Hc), g.randint(0, max(ws, Wc) - Wc)
        yield (h, w), (hs, ws), (Hc, Wc), (y0, x0), g.random() < 0.5, (g.randint(1, Hc + 3), g.randint(1, Wc + 3))


def table_window_label(label, scaled, window, origin, flip):
    """What the kernel computes: src[rowtab[sy]][coltab[sx]] inside the scaled image, 0 in the pad."""
    h, w = label.shape
    (hs, ws), (Hc, Wc) = scaled, window
    rt, ct = _pil_nearest_index(h, hs), _pil_nearest_index(w, ws)
    x = np.arange(Wc)
    sx = origin[1] + (Wc - 1 - x if flip else x)
    sy = origin[0] + np.arange(Hc)
    inside = (sy < hs)[:, None] & (sx < ws)[None, :]
    val = label[rt[np.minimum(sy, hs - 1)]][:, ct[np.minimum(sx, ws - 1)]]
    return np.where(inside, val, 0).astype(np.int64)


def test_label_path_equals_pil_on_200_random_cases():
    g = np.random.default_rng(3)
    for (h, w), scaled, window, origin, flip, grid in random_cases(200):
        label = g.integers(0, 200, (h, w)).astype(np.int32)
        want = BR.window_label(label, None, scaled, origin, flip, window)         # through PIL itself
        got = table_window_label(label, scaled, window, origin, flip)
        assert np.array_equal(got, want), ((h, w), scaled, window, origin, flip)
        # the latent grid: the composed tables equal PIL on the window
        rt, ct = _pil_nearest_index(window[0], grid[0]), _pil_nearest_index(window[1], grid[1])
        assert np.array_equal(got[rt][:, ct], BR.latent_labels(want, [grid])[0])


def test_composed_tables_equal_resampling_twice():
    g = np.random.default_rng(4)
    for (h, w), (hs, ws), (Hc, Wc), _, _, (hg, wg) in random_cases(60, seed=11):
        label = g.integers(0, 1000, (h, w)).astype(np.int32)
        once = np.asarray(Image.fromarray(label).resize((ws, hs), resample=Image.NEAREST))
        twice = np.asarray(Image.fromarray(once).resize((wg, hg), resample=Image.NEAREST))
        rows = _pil_nearest_index(h, hs)[_pil_nearest_index(hs, hg)]
        cols = _pil_nearest_index(w, ws)[_pil_nearest_index(ws, wg)]
        assert np.array_equal(label[rows][:, cols], twice)


def reference_draws(shape, window, scales):
    """What segmentation/data/dataset.py:145-184 takes from the module ``random``, restated: a scale (only with two bounds), the two
    crop origins over the scaled image grown to the window, then the flip."""
    window = tuple(shape) if window is None else tuple(window)
    factor = random.uniform(*scales[:2]) if len(scales) >= 2 else 1.0
    scaled = tuple(int(n * factor) for n in shape)
    room = [max(n, c) - c for n, c in zip(scaled, window)]
    origin = tuple(random.randint(0, r) for r in room)
    return scaled, origin, random.random() < 0.5


@pytest.mark.parametrize("scales", [(1.0,), (0.5, 1.5)])
@pytest.mark.parametrize("window", [(20, 30), (60, 80), None])            # smaller and larger than the scaled 37 x 53 image
def test_draw_augmentation_makes_the_references_draws(scales, window):
    for seed in range(50):
        random.seed(seed)
        want = reference_draws((37, 53), window, scales)
        after = random.random()
        rng = random.Random(seed)
        got = spx.draw_augmentation(rng, (37, 53), window, scales)
        assert (got.scaled, got.origin, got.flip) == want and rng.random() == after
        random.seed(seed)
        assert spx.draw_augmentation(random, (37, 53), window, scales) == got       # the module itself is taken too


def case_of(fx, name):
    m, Hc, Wc, hs, ws, y0, x0, flip, has_image, has_ids = (int(v) for v in fx[f"meta__{name}"])
    image = fx[f"image__{name}"]
    inner = image[m:image.shape[0] - m, m:image.shape[1] - m] if m else image
    return dict(image=image, inner=inner, margin=m, label=fx[f"label__{name}"], window=(Hc, Wc), scaled=(hs, ws), origin=(y0, x0),
                flip=bool(flip), has_image=bool(has_image), id_map=fx[f"id_map__{name}"] if has_ids else None,
                mean=fx[f"mean_std__{name}"][0], std=fx[f"mean_std__{name}"][1], grids=[tuple(g) for g in fx[f"grids__{name}"].tolist()])


def test_restatement_reproduces_the_fixture(fx):
    names = [str(n) for n in fx["cases"]]
    assert len(names) >= 6 and sum(case_of(fx, n)["has_image"] for n in names) >= 3
    for name in names:
        c = case_of(fx, name)
        lab = BR.window_label(c["label"], c["id_map"], c["scaled"], c["origin"], c["flip"], c["window"])
        assert lab.dtype == np.int64 and np.array_equal(lab, fx[f"out_label__{name}"]), name
        for k, got in enumerate(BR.latent_labels(lab, c["grids"])):
            assert np.array_equal(got, fx[f"latent{k}__{name}"]), (name, k)
        # the drawn parameters are what draw_augmentation validates as legal
        assert 0 <= c["origin"][0] <= max(c["scaled"][0], c["window"][0]) - c["window"][0]
        if c["has_image"]:
            assert c["scaled"] == c["label"].shape[:2]
            ref64 = fx[f"out_image__{name}"]
            got = BR.window_image_f32(c["inner"], c["scaled"], c["origin"], c["flip"], c["window"], c["mean"], c["std"])
            err = np.abs(got.astype(np.float64) - ref64)
            assert (err <= BR.image_bound(ref64, c["mean"], c["std"])).all(), (name, err.max())
            mine64 = BR.window_image_f64(c["inner"], c["scaled"], c["origin"], c["flip"], c["window"], c["mean"], c["std"])
            assert np.abs(mine64 - ref64).max() <= 1e-15 * (1 + np.abs(ref64).max()), name


def test_draw_augmentation_equals_the_references_own_draws(fx):
    """``draw_augmentation`` under a case's seed gives, bit for bit, what the reference's own ``__getitem__`` drew under it."""
    names = [str(n) for n in fx["cases"]]
    seen = set()
    for name in names:
        c = case_of(fx, name)
        seed, scales = int(fx[f"seed__{name}"][0]), tuple(fx[f"scales__{name}"].tolist())
        window = None if int(fx[f"window_is_label__{name}"][0]) else c["window"]
        got = spx.draw_augmentation(random.Random(seed), c["label"].shape, window, scales)
        assert got == spx.AugmentParams(c["scaled"], c["origin"], c["flip"]), name
        random.seed(seed)
        assert reference_draws(c["label"].shape[:2], window, scales) == (c["scaled"], c["origin"], c["flip"]), name
        seen.add((len(scales) >= 2, window is None, c["flip"]))
    assert {s[0] for s in seen} == {False, True} and {s[1] for s in seen} == {False, True} and {s[2] for s in seen} == {False, True}


# ---- argument errors: raised on the host, before the library is loaded ------------------------------------------------------
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def good(**over):
    kw = dict(images=[torch.zeros(10, 12, 3, dtype=torch.uint8)], labels=[torch.zeros(10, 12, dtype=torch.int64)],
              params=[spx.AugmentParams((10, 12), (0, 0), False)], window=(8, 8), mean=MEAN, std=STD, grids=[(2, 2)])
    kw.update(over)
    return kw


@pytest.fixture()
def no_library(monkeypatch):
    from scaleprotoseg_amd import _lib

    def refuse():
        raise AssertionError("the library was loaded before the arguments were validated")

    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(B_, "BatchTable", lambda *a, **kw: refuse())


@pytest.mark.parametrize("over,match", [
    (dict(params=[spx.AugmentParams((0, 12), (0, 0), False)]), "scaled size of zero"),
    (dict(params=[spx.AugmentParams((10, 0), (0, 0), False)]), "scaled size of zero"),
    (dict(params=[spx.AugmentParams((10, 12), (3, 0), False)]), "origin"),
    (dict(params=[spx.AugmentParams((10, 12), (0, 5), False)]), "origin"),
    (dict(params=[spx.AugmentParams((10, 12), (-1, 0), False)]), "origin"),
    (dict(params=[spx.AugmentParams((4, 4), (1, 0), False)]), "origin"),           # padded to the window: only origin 0 is legal
    (dict(grids=[(2, 2)] * 5), "at most 4"),
    (dict(std=[0.229, 0.0, 0.225]), "zero"),
    (dict(dtype=torch.float16), "dtype"),
    (dict(dtype=torch.bfloat16), "dtype"),
    (dict(images=[torch.zeros(10, 12, 3, dtype=torch.float32)]), "dtype"),
    (dict(labels=[torch.zeros(10, 12, dtype=torch.float32)]), "dtype"),
    (dict(labels=[torch.zeros(10, 12, dtype=torch.bool)]), "dtype"),
    (dict(), "no CPU fallback"),                                                     # host inputs: there is no other backend
])
def test_prepare_batch_errors_before_the_library(no_library, over, match):
    with pytest.raises(spx.SpxError, match=match):
        spx.prepare_batch(**good(**over))


def test_resize_labels_errors_before_the_library(no_library):
    lab = torch.zeros(2, 10, 12, dtype=torch.int64)
    with pytest.raises(spx.SpxError, match="at most 4"):
        spx.resize_labels(lab, grids=[(2, 2)] * 5)
    with pytest.raises(spx.SpxError, match="dtype"):
        spx.resize_labels(lab.float(), grids=[(2, 2)])
    with pytest.raises(spx.SpxError, match="no CPU fallback"):
        spx.resize_labels(lab, grids=[(2, 2)])
    with pytest.raises(spx.SpxError, match="no CPU fallback"):
        spx.resize_labels([lab[0], lab[1]], grids=[(2, 2)])


def test_entry_points_are_declared_bound_and_exported():
    from scaleprotoseg_amd import _lib

    header = open(os.path.join(HERE, "..", "include", "spx_hip.h")).read()
    lib = _lib.load()
    for name in ("spx_batch_prepare", "spx_resize_labels"):
        assert "int %s(const spx_batch* args, void* stream);" % name in header and name in _lib.SIGNATURES and hasattr(lib, name)
    # the C side validates too: a NULL block, no outputs, too many grids
    assert lib.spx_batch_prepare(None, None) != 0 and b"NULL" in lib.spx_last_error()
    a = _lib.SpxBatch()
    a.index, a.n_index, a.B, a.Hc, a.Wc, a.G = 16, 4, 1, 4, 4, 5
    assert lib.spx_batch_prepare(a, None) != 0 and b"latent grids" in lib.spx_last_error()
    a.G = 0
    a.samples = 16
    assert lib.spx_batch_prepare(a, None) != 0 and b"no output" in lib.spx_last_error()
    assert lib.spx_resize_labels(a, None) != 0
