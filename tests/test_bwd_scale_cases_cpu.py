"""Pins tests/bwd_scale_cases.py (references only, no GPU) and keeps tests/test_gpu_bwd_tile_scales.py from being vacuous:
every case walks several chunks per K2 workgroup by the library's own count, its tile pattern shows every kind of exponent
transition inside a walk, every checked row has a reference of its own magnitude, the float64 restatement of the crossing
meets a quarter of the bound the kernels are held to, and nothing leaves the normal fp32 range."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import bwd_scale_cases as S  # noqa: E402

NAMES = sorted(S.CASES)
FLT_MIN, FLT_MAX = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_cases():
    yield
    for f in (_refs, S.build, S.build_uneven_activations):
        f.cache_clear()


@functools.lru_cache(maxsize=None)
def _refs(name):
    pb = S.build(name)
    ref = S.reference(pb, pb.grads["tiles"])
    return pb, ref, S.restated(pb, pb.grads["tiles"], ref)


@pytest.mark.parametrize("name", NAMES)
def test_every_workgroup_walks_three_chunks_and_a_walk_crosses_an_image_end(name):
    sh = S.shape_of(name)
    n = S.nslabs(name)
    assert n == S.nslabs(name, B=-(-sh.B // 3)), "the slab count is not capped at a third of the chunks"
    per_img = sh.tiles * (S.TILE_PX // sh.cpx)
    assert per_img % n != 0, "chunks per image is a multiple of the slab count: no walk crosses an image end unevenly"
    walks = S.walks(name)
    assert len(walks) == n and min(len(w) for w in walks) >= 3
    assert any(len({b for b, _ in w}) > 1 for w in walks)
    assert sum(len(w) for w in walks) == sh.B * per_img


@pytest.mark.parametrize("name", NAMES)
def test_pattern_has_every_transition_inside_a_walk(name):
    sh = S.shape_of(name)
    cls = S.tile_classes(name)
    per_walk = S.transitions_per_walk(name)
    seen = set().union(*per_walk)
    assert seen == set(S.TRANSITIONS), f"missing {set(S.TRANSITIONS) - seen}"
    assert set(cls.ravel().tolist()) == set(range(7)), "a tile class no tile carries"
    assert sh.HW % S.TILE_PX != 0 or name == "dma"
    for b in range(sh.B):
        assert cls[b, -1] != S.ZERO and S.LEVELS[cls[b, -1]] != 0, "an image's last tile has a trivial scale"
    print(f"{name}: {len(per_walk)} walks, {sum(len(t) >= 3 for t in per_walk)} with three or more kinds of transition")


@pytest.mark.parametrize("name", NAMES)
def test_values_stay_in_the_normal_fp32_range(name):
    pb, ref, _ = _refs(name)
    gr = pb.grads["tiles"]
    cls = S.pixel_classes(name)
    for what, t in (("g_logits", gr.g_logits), ("g_dist", gr.g_dist), ("g_act", gr.g_act), ("G", ref.G),
                    ("dX", ref.dx), ("dPrototypes", ref.dp), ("dLastLayer", ref.dw)):
        a = t.double().abs()
        nz = a[a > 0]
        print(f"{name} {what}: |v| in [2^{np.log2(nz.min().item()):.1f}, 2^{np.log2(nz.max().item()):.1f}]")
        # (the smallest non-zero G or result is a cancellation; even that stays normal)
        assert nz.max().item() < 2.0 ** 24 < FLT_MAX and nz.min().item() > 2.0 ** -100 > FLT_MIN
        if what.startswith("g_"):
            assert nz.min().item() > 2.0 ** -80 > FLT_MIN
    # per tile the largest |G| - what sets the tile's exponent - sits where its class says
    e = S.tile_exponents(pb, ref.G)
    assert e.min().item() >= 15 - 14 and e.max().item() <= 15 + 50, (e.min().item(), e.max().item())
    zero_px = (cls == S.ZERO)
    assert (ref.G.permute(0, 2, 1)[zero_px] == 0).all() and (ref.dx.reshape(pb.sh.B, -1, pb.sh.HW).permute(0, 2, 1)[zero_px] == 0).all()
    # the span inside one launch stays far inside the 2^80 of K2's skip rule (a zero tile carries e_t = 15)
    assert e.max().item() - e.min().item() <= 60


@pytest.mark.parametrize("name", NAMES)
def test_every_checked_row_has_a_reference_of_one_magnitude(name):
    pb, ref, _ = _refs(name)
    sh = pb.sh
    assert (ref.dp.abs().amax(dim=(1, 2, 3)) > 0).all() and (ref.dw.abs().amax(dim=1) > 0).all()
    # row p of dPrototypes and row k of dLastLayer carry the magnitude of tile class p % 6 / k % 6: against the same gradients
    # without the scales, the row is the unscaled row times 2^k exactly (float64, powers of two)
    base = S.reference(pb, pb.grads["masked"])
    # (the unscaled run fills zero tiles with class 0's pattern, so class 0's rows differ; the others must agree)
    for rows, got, want in ((torch.arange(sh.P) % 6, ref.dp, base.dp), (torch.arange(sh.K) % 6, ref.dw, base.dw)):
        for c in range(1, 6):
            sel = rows == c
            assert torch.equal(got[sel], want[sel] * 2.0 ** S.LEVELS[c]), f"rows of class {c} mix magnitudes"


@pytest.mark.parametrize("name", NAMES)
def test_restatement_meets_a_quarter_of_the_bound(name):
    pb, ref, (dp, dw) = _refs(name)
    r_dp, z_dp = S.row_ratios(dp, ref.dp, 0)
    r_dw, z_dw = S.row_ratios(dw, ref.dw, 0)
    print(f"{name}: restatement against float64, worst row: dPrototypes {r_dp.max().item():.3e} (bound / 4 = {S.TOL_DP_ROW / 4:.1e}), "
          f"dLastLayer {r_dw.max().item():.3e} (bound / 4 = {S.tol_dw_row(name) / 4:.1e})")
    assert z_dp == 0 and z_dw == 0
    assert r_dp.max().item() <= S.TOL_DP_ROW / 4 and r_dw.max().item() <= S.tol_dw_row(name) / 4
    assert r_dp.max().item() > 0 and r_dw.max().item() > 0           # the restatement does round


def test_headless_restatement_meets_a_quarter_of_the_bound():
    pb = S.build("ksplit")
    ref = S.reference(pb, pb.grads["tiles"], head=False)
    dp, _ = S.restated(pb, pb.grads["tiles"], ref, head=False)
    r, z = S.row_ratios(dp, ref.dp, 0)
    print(f"ksplit without a head: restatement worst dPrototypes row {r.max().item():.3e}")
    assert z == 0 and 0 < r.max().item() <= S.TOL_DP_ROW / 4


def test_uneven_activations_differ_in_block_exponent_and_meet_a_quarter_of_the_bound():
    pb = S.build_uneven_activations()
    sh = pb.sh
    gr = pb.grads["plain"]
    ref = S.reference(pb, gr)
    a = ref.act.view(sh.B, sh.HW, sh.P)
    assert (a[pb.on_proto][:, 32:40].amax(dim=1) > 9.2).all()             # d = 0 on one prototype of block 1
    # block exponents of scale 0's two 32-prototype blocks (prototypes 0..31 and 32..56), per pixel
    a0 = a[:, :, :sh.per].reshape(-1, sh.per)
    ex = torch.stack([torch.frexp(a0[:, :32].amax(dim=1))[1], torch.frexp(a0[:, 32:].amax(dim=1))[1]], dim=1)
    print(f"uneven activations: block exponents from {ex.min().item()} to {ex.max().item()}, "
          f"{(ex[:, 0] != ex[:, 1]).sum().item()} pixels whose two blocks differ")
    assert ex.min().item() <= -6 and ex.max().item() == 4 and (ex[:, 0] != ex[:, 1]).any()
    _, dw = S.restated(pb, gr, ref)
    r, z = S.row_ratios(dw, ref.dw, 1)
    print(f"uneven activations: restatement worst dLastLayer column {r.max().item():.3e} (bound / 4 = {S.TOL_DW_COL / 4:.1e})")
    assert z == 0 and 0 < r.max().item() <= S.TOL_DW_COL / 4


@pytest.mark.parametrize("name", S.STAIR_CASES)
def test_staircase_descends_in_every_walk_and_its_restatement_meets_a_quarter_of_the_bound(name):
    pb = S.build(name)
    lv = S.stair_tile_levels(name)
    for w in S.walks(name):
        assert [lv[c] for c in w] == list(range(len(w))) and len(w) >= 3
    assert any(len(w) == len(S.STAIR_LEVELS) for w in S.walks(name))
    gr, _ = S.build_staircase(name)
    for t in (gr.g_logits, gr.g_dist, gr.g_act):
        a = t.abs()
        assert a.max().item() < 2.0 ** 36 and a[a > 0].min().item() > 2.0 ** -125 > FLT_MIN
    ref = S.reference(pb, gr)
    e = S.tile_exponents(pb, ref.G)
    assert e.max().item() - e.min().item() > 100 and e.max().item() < 115           # beyond the skip rule, inside the clamp of e_t
    dp, dw = S.restated(pb, gr, ref)
    r_dp, z_dp = S.row_ratios(dp, ref.dp, 0)
    r_dw, z_dw = S.row_ratios(dw, ref.dw, 0)
    print(f"{name} staircase: restatement worst row: dPrototypes {r_dp.max().item():.3e}, dLastLayer {r_dw.max().item():.3e}")
    assert z_dp == int((pb.pm >= len(S.STAIR_LEVELS)).sum()) and z_dw == int((pb.km >= len(S.STAIR_LEVELS)).sum())
    assert r_dp.max().item() <= S.TOL_DP_ROW / 4 and r_dw.max().item() <= S.tol_dw_row(name) / 4


def test_descending_staircase_overflows_a_last_chunk_rule_but_not_a_clamped_one():
    """chunk_scale in float32 (spx_bank.hip): the accumulators live in the units of the chunk added last, and the skip test
    compares with THAT chunk's exponent.  Tiles that each lie 2^-35 below the one before are never skipped (35 <= 80), so the
    first tile's sum - up to 2^15 per pixel and channel, 2^22 after 128 pixels of one sign - is multiplied by 2^35 per step:
    2^127 after three steps, infinity after four.  Compared with the smallest exponent seen (the largest tile), the fourth
    step is skipped and the sum stays finite; what it drops is below 2^-80 of it."""
    first = np.float32(2.0 ** 22)

    def walk(clamped):
        acc, e_acc, e_min = first, 0, 0
        for e_c in (35, 70, 105, 140):
            if (e_c - e_min if clamped else e_c - e_acc) > 80:
                continue
            with np.errstate(over="ignore"):
                acc = np.float32(acc * np.float32(2.0) ** np.float32(e_c - e_acc))
            e_acc = e_c
            acc = np.float32(acc + np.float32(2.0 ** 22))
        return acc, e_acc

    acc, _ = walk(clamped=False)
    assert np.isinf(acc)
    acc, e_acc = walk(clamped=True)
    assert np.isfinite(acc) and e_acc == 70 and float(acc) * 2.0 ** -e_acc == pytest.approx(2.0 ** 22, rel=1e-6)
