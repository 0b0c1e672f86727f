"""Are the inputs of tests/test_gpu_kld_float64.py value-bearing, and are its bounds something plain fp32 reaches?  On the CPU,
for every case of tests/kld_cases.py: oracle.loss_oracle.kld_loss in float64, and the same oracle on fp32 planes.

  - the float64 loss lies in [0.05, 0.95]: the value assertion relative to max(1, |loss|) cannot be met by a kernel that returns 0;
  - at least 90 % of the compared (segment, pair) entries have exp(-kld) >= 1e-3, a case's stated degenerate pairs aside: the
    assertions see all segments and pairs, not the one or two with the smallest KL;
  - the fp32 oracle stays within ONE QUARTER of each bound the GPU file sets (loss, gradient globally and per segment, pair
    sums, lse): the bounds leave fp32 arithmetic a margin and are not fitted to the kernels."""
import pytest
import torch

import kld_cases as KC


@pytest.fixture(scope="module", params=KC.CASE_NAMES)
def both(request):
    c = KC.case(request.param)
    return c, KC.reference(c, torch.float64), KC.reference(c, torch.float32)


def test_inputs_bear_on_the_value(both):
    c, r64, _ = both
    if c.zero:
        assert r64["loss"] == 0.0 and not r64["valid"].any() and not r64["grad"].any()
        return
    print(f"{c.name}: float64 loss {r64['loss']:.6f}")
    assert KC.MIN_LOSS <= r64["loss"] <= KC.MAX_LOSS
    valid = r64["valid"]
    # the restated exp(-kld) reproduces the oracle's value: the share below is about the terms the loss is made of
    assert abs(r64["e"][valid].mean().item() - r64["loss"]) <= 1e-12
    counted = valid if c.stated is None else valid & ~c.stated
    live = (r64["e"][counted] >= KC.LIVE_TERM).double().mean().item()
    print(f"{c.name}: {int(counted.sum())} compared entries, {live:.3f} with exp(-kld) >= {KC.LIVE_TERM}")
    assert live >= KC.LIVE_SHARE
    if c.stated is not None:                                           # the stated pairs are degenerate indeed, and are compared
        assert (valid & c.stated).any() and (r64["e"][valid & c.stated] < KC.LIVE_TERM).all()
    # the floor of the per-segment gradient bound loosens no segment that carries a gradient: every contributing segment's own
    # maximum is ten floors or more of the global one, a case's stated zero-gradient segments aside
    gmax = r64["grad"].abs().max().item()
    segmax = KC.segment_gradient_maxima(c, r64["grad"])
    carries = r64["counts"] >= 2
    for b, k in c.flat:
        assert carries[b, k] and segmax[b, k] <= 1e-12 * gmax
        carries[b, k] = False
    print(f"{c.name}: smallest contributing segment's max|g64| / global: {(segmax[carries].min().item() / gmax):.3g}")
    assert gmax > 0 and segmax[carries].min().item() >= 10 * KC.SEG_FLOOR * gmax


def test_fp32_oracle_keeps_a_quarter_of_each_bound(both):
    c, r64, r32 = both
    if c.zero:
        assert r32["loss"] == 0.0 and not r32["grad"].any()
        return
    g_all, g_seg, void = KC.gradient_ratios(c, r32["grad"], r64["grad"])
    ratios = {"loss": KC.loss_ratio(r32["loss"], r64), "grad": g_all, "grad/segment": g_seg, "A": KC.pair_ratio(c, r32["A"], r64),
              "lse": KC.lse_ratio(r32["lse"], r64)}
    print(f"{c.name}: fp32 oracle, error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert void == 0.0
    assert torch.equal(r32["counts"], r64["counts"])
    for k, v in ratios.items():
        assert v <= 0.25, (k, v)


def test_degenerate_segments_are_what_they_say():
    c = KC.case("degenerate")
    r = KC.reference(c, torch.float64)
    seg, ok = KC.segment_ids(c)
    cnt = r["counts"]
    assert cnt[0, 2] == 1 and cnt[0, 3] == 2 and (cnt[2] == 0).all() and cnt[1, 6] == 0 and cnt[0, 7] == 0 and cnt[1, 7] > 0
    assert not r["valid"][0, 2].any() and r["valid"][0, 3].any()
    g = r["grad"]
    lab = c.labels.reshape(3, -1)
    assert not g[0][:, lab[0] == 2].any()                              # a single pixel: no contribution, gradient exactly 0
    assert g[0][:, lab[0] == 3].abs().max() > 0
    # identical slots: kld = 0, every pair contributes exactly 1, the gradient vanishes (to float64 rounding)
    assert torch.equal(r["e"][0, 1][r["valid"][0, 1]], torch.ones(21, dtype=torch.float64))
    assert g[0][:, lab[0] == 1].abs().max().item() <= 1e-12 * g.abs().max().item()


@pytest.mark.parametrize("name,rows", [("tall_32rows", 32), ("tall_64rows", 64)])
def test_tall_maps_get_the_taller_tiles(name, rows):
    c = KC.case(name)
    B, H, W = c.shape
    assert KC.segment_tile_rows(B, H, W) == rows == c.tile_rows
    assert B * ((W + 63) // 64) * ((H + rows - 1) // rows) >= 512
    assert KC.segment_tile_rows(1, 512, 1024) == 16                    # the largest map of the older KLD tests
