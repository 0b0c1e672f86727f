"""Record the reference's ``MSC.forward`` (segmentation/utils.py:71-111) on the CPU, in eval and in training mode:

    SPX_REFERENCE=<reference checkout> python tools/gen_msc_golden.py

loads the reference's REAL class (tools/reference_stubs.py, plus ``pytorch_lightning.LightningModule = object``) around a small
stand-in base that hands out prepared maps by the size of its input and records what it returned, and writes data only:
tests/golden/msc_features.npz and msc_features_pascal65.npz (two files, so that each stays below 1 MiB) with "case__field" keys
(tests/support.py::load_cases), per case

    map0, map1, ...     what the base returned at full scale and at each entry of ``scales`` (float32 [B, C, h_k, w_k])
    x_shape, scales     the input's shape (the input itself is never read by the stand-in) and the scale list
    logits_max          the eval-mode output
    train_shapes        the shapes of the training-mode list ([full] + pyramid + [max]; its last element equals logits_max and
                        the others are the maps: asserted here)
    index               torch.max's index over the stack the reference forms (uint8)
    g, d0, d1, ...      an upstream gradient on logits_max and the gradients the reference's autograd gives each map

Cases: five shape sets with B = 2, C = 5 and ``randn`` maps, one with an exact tie (map 1 is a constant that equals map 0 on a
few pixels: the bilinear blend of a constant is that constant) and one with NaNs.  The tool asserts that the restatement
(tests/msc_restatement.py) holds its own fixture within its bounds."""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import reference_stubs as RS  # noqa: E402
import msc_restatement as MR  # noqa: E402  (tests/ is on the path once reference_stubs is imported)

B, C = 2, 5
# name: (H, W), [(h_k, w_k) of the scaled outputs]; the input is (8 H, 8 W) and the scale of entry k is h_k / H
SHAPES = {
    "odd": ((7, 9), [(4, 5), (6, 7)]),
    "one_up": ((7, 9), [(1, 1), (9, 11)]),
    "pascal41": ((41, 41), [(21, 21), (31, 31)]),
    "pascal65": ((65, 65), [(33, 33), (49, 49)]),
    "wide": ((33, 65), [(17, 33), (25, 49)]),
}


class Base(nn.Module):
    """Hands out the prepared map whose key is the input's spatial size; keeps what it returned, in call order."""

    def __init__(self, table):
        super().__init__()
        self.table = table
        self.returned = []

    def forward(self, x):
        out = self.table[tuple(x.shape[2:])]
        self.returned.append(out)
        return out


def input_sizes(full, scaled):
    """An input size and scale factors for which F.interpolate(scale_factor=p) yields one distinct input size per map."""
    H, W = full
    x_hw = (8 * H, 8 * W)
    scales, sizes = [], []
    for h, w in scaled:
        p = h / H
        size = (int(np.floor(x_hw[0] * p)), int(np.floor(x_hw[1] * p)))
        scales.append(p)
        sizes.append(size)
    assert len(set(sizes + [x_hw])) == len(sizes) + 1
    return x_hw, scales, sizes


def same(a, b):
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(0.0), b.nan_to_num(0.0))


def record(MSC, name, full, scaled, maps):
    x_hw, scales, sizes = input_sizes(full, scaled)
    x = torch.zeros(B, 3, *x_hw)
    leaves = [m.clone().requires_grad_(True) for m in maps]
    base = Base(dict(zip([x_hw] + sizes, leaves)))
    msc = MSC(base=base, scales=scales)
    msc.eval()
    logits_max = msc(x)
    assert [t is l for t, l in zip(base.returned, leaves)] == [True] * len(leaves)
    msc.train()
    train = msc(x)
    assert len(train) == len(maps) + 1 and same(train[-1], logits_max)
    assert all(t is l for t, l in zip(train[:-1], leaves))
    H, W = full
    up = [leaves[0]] + [torch.nn.functional.interpolate(l, size=(H, W), mode="bilinear", align_corners=False) for l in leaves[1:]]
    val, index = torch.max(torch.stack(up), dim=0)
    assert same(val, logits_max)
    g = torch.round(torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(len(name))) * 2.0 ** 10) / 2.0 ** 10
    grads = torch.autograd.grad(logits_max, leaves, g)
    out = {f"{name}__map{k}": m.detach().numpy() for k, m in enumerate(maps)}
    out[f"{name}__x_shape"] = np.array(x.shape, dtype=np.int64)
    out[f"{name}__scales"] = np.array(scales, dtype=np.float64)
    out[f"{name}__logits_max"] = logits_max.detach().numpy()
    out[f"{name}__train_shapes"] = np.array([t.shape for t in train], dtype=np.int64)
    out[f"{name}__index"] = index.numpy().astype(np.uint8)
    out[f"{name}__g"] = g.numpy()
    for k, d in enumerate(grads):
        out[f"{name}__d{k}"] = d.numpy()
    check(name, out, len(maps))
    return out


def check(name, out, K):
    """The restatement holds this case within its own bounds."""
    maps = [out[f"{name}__map{k}"] for k in range(K)]
    z, idx, zb, u, b = MR.forward(maps)
    ref = out[f"{name}__logits_max"].astype(np.float64)
    nan = np.isnan(ref)
    assert np.array_equal(nan, np.isnan(z)), name
    err = np.abs(z - ref)[~nan]
    assert (err <= zb[~nan]).all(), (name, (err / np.maximum(zb[~nan], 1e-300)).max())
    sure = MR.decided(u, b) & ~nan
    assert np.array_equal(idx[sure], out[f"{name}__index"][sure]), name
    if not nan.any():
        grads, bounds = MR.gradients([m.shape[2:] for m in maps], out[f"{name}__index"], out[f"{name}__g"])
        for k in range(K):
            assert (np.abs(grads[k] - out[f"{name}__d{k}"]) <= bounds[k]).all(), (name, k)
    ratio = (err / np.maximum(zb[~nan], 1e-300))[zb[~nan] > 0]
    print(f"{name}: forward error / bound at most {ratio.max() if ratio.size else 0.0:.3f}; undecided argmax "
          f"{100.0 * (1 - sure.mean()):.4f} %")


def main():
    RS.stub_modules()
    RS.mod("pytorch_lightning", LightningModule=object)
    MSC = RS.load("segmentation/utils.py").MSC
    torch.set_num_threads(1)
    blob = {}
    for n, (name, (full, scaled)) in enumerate(SHAPES.items()):
        gen = torch.Generator().manual_seed(20261021 + n)
        maps = [torch.randn(B, C, h, w, generator=gen) for h, w in [full] + scaled]
        blob.update(record(MSC, name, full, scaled, maps))
    # an exact tie: map 1 is the constant 0.5 (its bilinear blend is exactly 0.5) and map 0 equals 0.5 on every third pixel;
    # map 2 is lower everywhere
    full, scaled = SHAPES["odd"]
    gen = torch.Generator().manual_seed(7)
    m0 = torch.randn(B, C, *full, generator=gen)
    m0.view(-1)[::3] = 0.5
    maps = [m0, torch.full((B, C, *scaled[0]), 0.5), torch.full((B, C, *scaled[1]), -9.0)]
    blob.update(record(MSC, "tie", full, scaled, maps))
    # NaNs: one in map 0, one in map 1 (it spreads over the pixels whose footprint holds it), and a pixel where both are NaN
    maps = [torch.randn(B, C, h, w, generator=gen) for h, w in [full] + scaled]
    maps[0][0, 1, 2, 3] = float("nan")
    maps[0][1, 0, 0, 0] = float("nan")
    maps[1][1, 0, 0, 0] = float("nan")
    maps[1][0, 3, 2, 2] = float("nan")
    blob.update(record(MSC, "nan", full, scaled, maps))
    # two files, so that each stays below 1 MiB (float32 noise does not compress)
    big = {k: v for k, v in blob.items() if k.startswith("pascal65__")}
    small = {k: v for k, v in blob.items() if k not in big}
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "..", "tests", "golden")
    for fname, part in (("msc_features.npz", small), ("msc_features_pascal65.npz", big)):
        path = os.path.join(out_dir, fname)
        np.savez_compressed(path, **part)
        print(path, os.path.getsize(path))
        assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
