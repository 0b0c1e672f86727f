"""bench.py --dump-outputs on CPU tensors: float32 .npy files, per-pixel arrays cut to one fixed pixel sample (pixel-major),
parameter gradients whole, the same files from call to call, and within the 64 MB budget at the largest workload."""
import os

import numpy as np
import torch

import bench


def _arrays(M, C=256, P=190, K=19, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {
        "logits": torch.randn(M, K, generator=g),
        "distances": torch.rand(1, P, M, generator=g),
        "dX": torch.randn(1, C, M, generator=g).to(torch.bfloat16),
        "dPrototypes": torch.randn(P, C, 1, 1, generator=g),
        "dLastLayer": torch.randn(K, P, generator=g),
        "dTail": None,
    }


def test_dump_samples_pixels_and_is_repeatable(tmp_path):
    M = 4 * bench.DUMP_PIXELS
    arrays = _arrays(M)
    bench.dump_outputs(str(tmp_path / "a"), M, arrays)
    bench.dump_outputs(str(tmp_path / "b"), M, arrays)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["dLastLayer.npy", "dPrototypes.npy", "dX.npy", "distances.npy", "logits.npy"]
    got = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    for n in names:
        assert np.array_equal(got[n[:-4]], np.load(tmp_path / "b" / n))
        assert got[n[:-4]].dtype == np.float32
    idx = torch.randperm(M, generator=torch.Generator().manual_seed(20220227))[: bench.DUMP_PIXELS].sort().values
    assert np.array_equal(got["logits"], arrays["logits"][idx].numpy())
    assert np.array_equal(got["distances"], arrays["distances"][0][:, idx].t().numpy())
    assert np.array_equal(got["dX"], arrays["dX"][0].float()[:, idx].t().numpy())
    assert np.array_equal(got["dPrototypes"], arrays["dPrototypes"].numpy())
    assert np.array_equal(got["dLastLayer"], arrays["dLastLayer"].numpy())


def test_dump_keeps_every_pixel_of_a_small_grid(tmp_path):
    M = 650
    arrays = _arrays(M)
    bench.dump_outputs(str(tmp_path), M, arrays)
    assert np.array_equal(np.load(tmp_path / "distances.npy"), arrays["distances"][0].t().numpy())


def test_dump_budget_at_the_widest_workload():
    # per sampled pixel: logits (K) + distances (P) + dX (C) in float32; parameter gradients whole
    worst = 0
    for C, P, S, K, H, W in bench.WORKLOADS.values():
        U = 3 * K                                          # --group-tail widens the head to 3K units
        per_px = 4 * (K + P + C)
        params = 4 * (P * (C // S) + U * P + K * U)
        worst = max(worst, min(H * W, bench.DUMP_PIXELS) * per_px + params)
    assert worst <= 64 * 2**20, worst
