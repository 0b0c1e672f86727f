"""Are the reference, the inputs and the bounds of tests/test_gpu_ce_float64.py sound?  On the CPU, for every case of
tests/ce_cases.py:

  - the float64 reference equals torch.nn.functional.cross_entropy(ignore_index=-1) in float64 and autograd, to 1e-12, and
    reproduces the ce_* arrays of tests/golden/kld_loss.npz;
  - every case with a loss has a float64 loss of at least 0.05;
  - the kernels' formula restated in NumPy fp32 stays within ONE QUARTER of every bound (lse, loss, d_logits per element, the
    grouping tail's d W_g), with pred and the count exact: the bounds leave v_exp_f32 / v_log_f32 and the fp32 order of the partial
    sums a factor of four and are not fitted to the kernels;
  - six wrong kernels, restated, each exceed a bound on at least one case (the cases are listed at WRONG)."""
import math

import numpy as np
import pytest
import torch

import ce_cases as CC


@pytest.fixture(scope="module", params=CC.CASE_NAMES)
def both(request):
    c = CC.case(request.param)
    return c, CC.reference(c.logits, c.labels), CC.restatement(c.logits, c.labels)


def _torch_labels(c):
    lab = c.labels.long()
    return torch.where((lab >= 0) & (lab < c.K), lab, torch.full_like(lab, -1))


def test_reference_is_torch_cross_entropy_and_autograd(both):
    c, ref, _ = both
    l = c.logits.double().clone().requires_grad_(True)
    lab = _torch_labels(c)
    loss = torch.nn.functional.cross_entropy(l, lab, ignore_index=-1)
    assert torch.equal(ref["valid"], lab >= 0) and ref["count"] == int((lab >= 0).sum())
    assert torch.equal(ref["pred"], c.logits.argmax(dim=1))          # torch.argmax: the first of equal maxima
    assert (ref["lse"] - torch.logsumexp(c.logits.double(), dim=1)).abs().max().item() <= 1e-12 * max(1.0, ref["lse"].abs().max().item())
    if c.no_loss == "nan":
        assert math.isnan(ref["loss"]) and math.isnan(loss.item()) and ref["count"] == 0 and not ref["d"].any()
        return
    loss.backward()
    print(f"{c.name}: float64 loss {ref['loss']:.9g}, count {ref['count']}")
    assert abs(ref["loss"] - loss.item()) <= 1e-12 * max(1.0, abs(loss.item()))
    assert (ref["d"] - l.grad).abs().max().item() <= 1e-12
    assert not ref["d"][~ref["valid"]].any()
    if c.no_loss == "zero":
        assert ref["loss"] == 0.0 and not ref["d"].any()
    else:
        assert ref["loss"] >= CC.MIN_LOSS


def test_reference_reproduces_the_golden(golden):
    g = golden("kld_loss")
    K = g["ce_logits"].shape[-1]
    logits = torch.from_numpy(g["ce_logits"]).reshape(-1, K)
    lab = torch.from_numpy(g["ce_target"]).reshape(-1) - 1            # 0 = void (loss.py:32)
    ref = CC.reference(logits, lab)
    assert abs(ref["loss"] - float(g["ce_loss"])) <= 2 * CC.EPS32 * abs(float(g["ce_loss"]))      # the golden is fp32
    scale = np.abs(g["ce_grad"]).max()
    assert np.abs(ref["d"].numpy() - g["ce_grad"].reshape(-1, K)).max() <= 2 * CC.EPS32 * scale
    correct = (ref["pred"] == lab)[ref["valid"]]
    np.testing.assert_array_equal(correct.numpy().astype(np.int64), g["ce_correct"])


def _ratios(c, ref, r32):
    """error / bound of a restatement's results; the reference's d is re-made with the coef the restatement used."""
    rc = CC.reference(c.logits, c.labels, coef=r32["coef"])
    d, ignored = CC.dlogits_ratio(r32["d"], rc)
    out = {"lse": CC.lse_ratio(r32["lse"], ref), "d_logits": d}
    if c.no_loss is None:
        out["loss"] = CC.loss_ratio(r32["loss"], ref)
    return out, ignored


def test_fp32_restatement_keeps_a_quarter_of_each_bound(both):
    c, ref, r32 = both
    ratios, ignored = _ratios(c, ref, r32)
    print(f"{c.name}: fp32 restatement, error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert CC.pred_mismatches(r32["pred"], ref) == 0 and r32["count"] == ref["count"] and ignored == 0.0
    if c.no_loss == "nan":
        assert math.isnan(r32["loss"]) and not r32["d"].any()
    elif c.no_loss == "zero":
        assert r32["loss"] == 0.0
    for k, v in ratios.items():
        assert v <= CC.QUARTER, (k, v)


def test_flushed_exponentials_stay_under_the_floor_term(both):
    """v_exp_f32 returns 0 below 2^-126 where NumPy returns a denormal: with that restated, d_logits is off by less than
    |coef| 2^-126 more - up to the whole floor term of the bound (0.998 of the bound on m300_k171_scale30, on the CPU as on the
    GPU), never past it; everything else is unchanged."""
    c, ref, r32 = both
    f32 = CC.restatement(c.logits, c.labels, flush=True)
    rc = CC.reference(c.logits, c.labels, coef=f32["coef"])
    flushed, ignored = CC.dlogits_ratio(f32["d"], rc)
    err = (f32["d"].double() - rc["d"]).abs() - abs(rc["coef"]) * CC.DL_FLOOR       # without the flush's share ...
    rel = float((err / (CC.dlogits_bound(rc) - abs(rc["coef"]) * CC.DL_FLOOR))[rc["valid"]].max()) if rc["count"] else 0.0
    print(f"{c.name}: d_logits error / bound with flushed exponentials {flushed:.3f}; net of the floor term {rel:.3f}")
    assert torch.equal(f32["lse"], r32["lse"]) and f32["loss"] == r32["loss"] or c.no_loss == "nan"
    assert flushed <= 1.0 and ignored == 0.0 and rel <= CC.QUARTER               # ... the rest keeps its quarter


def test_cases_hold_what_they_say():
    for name in CC.CASE_NAMES:
        c = CC.case(name)
        lab = c.labels.long()
        if c.no_loss is None and name not in ("last_pixel_only",):
            for v in (-1, -2, c.K, c.K + 7, CC.INT32_MIN, CC.INT32_MAX):
                assert bool((lab == v).any()), (name, v)
            if c.M >= 256:                                             # two whole waves without a valid pixel
                assert not ((lab[64:192] >= 0) & (lab[64:192] < c.K)).any()
    assert {(CC.case(n).M, CC.case(n).K) for n in CC.CASE_NAMES} >= set(CC.STANDALONE_SHAPES)
    big = CC.case("m33027_k19")
    assert (big.M + 63) // 64 > 2 * 256 and 4 * ((big.M + 255) // 256) == 520       # the finish kernel's strided loop runs
    t = CC.case("ties")
    top = t.logits == t.logits.max(dim=1, keepdim=True).values
    assert bool((top.sum(1) == t.K).any()) and bool((top.sum(1) == 2).any()) and bool((top.sum(1) == 1).any())
    two = top.sum(1) == 2
    hi = torch.where(top, torch.arange(t.K), torch.zeros((), dtype=torch.long)).max(dim=1).values
    assert bool((hi[two] >= 8).any()) and bool((hi[two] < 8).any())
    last = CC.case("last_pixel_only")
    v = (last.labels >= 0) & (last.labels < last.K)
    assert int(v.sum()) == 1 and bool(v[-1])
    assert CC.case("offset_plus200").logits.min().item() > 150 and CC.case("span_3e4").logits.abs().max().item() > 5e4


# the wrong kernels, and the cases on which each must break a bound (a subset of what it breaks: asserted, not fitted)
WRONG = {
    "no_max": ("m300_k171_scale30", "offset_plus200", "span_3e4"),                      # exp overflows: lse is inf
    "drop_block": ("m300_k33_scale4", "m300_k150_scale1", "m300_k171_scale30"),         # classes 32 - 63 exist
    "drop_half": ("m37_k5_scale1", "m833_k19_scale4", "m33027_k19", "ties"),
    "mean_all": ("m37_k5_scale1", "m833_k19_scale4", "m33027_k19", "last_pixel_only"),
    "tie_high": ("ties",),
    "onehot_plus1": ("m37_k5_scale1", "m833_k19_scale4", "last_pixel_only"),
}


@pytest.mark.parametrize("variant", CC.VARIANTS)
def test_the_bounds_tell_wrong_kernels_apart(variant):
    caught = []
    for name in CC.CASE_NAMES:
        c = CC.case(name)
        ref = CC.reference(c.logits, c.labels)
        r32 = CC.restatement(c.logits, c.labels, variant)
        ratios, ignored = _ratios(c, ref, r32)
        worst = max(ratios.values())
        wrong_pred = CC.pred_mismatches(r32["pred"], ref)
        if worst > 1.0 or wrong_pred or ignored:
            caught.append(name)
        print(f"{variant} on {name}: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()) + f", pred off on {wrong_pred}")
    print(f"{variant}: caught on {caught}")
    assert set(WRONG[variant]) <= set(caught), (variant, caught)


# ---- the grouping tail's d W_g = d_logits^T . gact
TAIL_SHAPES = ((15, 5, 256), (57, 19, 65), (63, 21, 63), (160, 32, 191))      # (U, K2, M) of tests/test_gpu_ce_float64.py


@pytest.mark.parametrize("U,K2,M", TAIL_SHAPES)
def test_fp32_restatement_of_the_tail_weight_gradient(U, K2, M):
    gen = torch.Generator().manual_seed(U * 1000 + M)
    gact = torch.exp(torch.randn(M, U, generator=gen) * 0.5).float()
    wg = torch.randn(K2, U, generator=gen) * 0.1
    logits = (gact @ wg.t()).float()
    lab = CC.mixed_labels(M, K2, gen)
    r32 = CC.restatement(logits, lab)
    ref = CC.reference(logits, lab, coef=r32["coef"])
    dw = (r32["d"].numpy().astype(np.float32)[:, :, None] * gact.numpy()[:, None, :]).astype(np.float32).astype(np.float64).sum(0)
    r = CC.dw_ratio(torch.from_numpy(dw), ref["d"], gact)
    print(f"d W_g U={U} K2={K2} M={M}: fp32 restatement, error / bound {r:.3f}")
    assert r <= CC.QUARTER


def test_crafted_inputs_of_the_finish_and_label_kernels():
    for n in CC.FINISH_SIZES:
        pairs, count, total = CC.finish_pairs(n)
        assert pairs.shape == (n, 2) and count > 0 and count < 2 ** 24 and total / count >= CC.MIN_LOSS
        assert float(pairs[:, 1].sum()) == count and bool((pairs[:, 1] == pairs[:, 1].round()).all())
        if n > 1:
            assert bool((pairs[1:, 1] != pairs[:-1, 1]).all())           # a pair taken twice for its neighbour changes the count
        s32, c32, l32 = CC.finish_restatement(pairs)                    # the kernel's order in fp32: a quarter of the loss bound
        r_sum = abs(s32 - total) / (CC.LOSS_TOL * max(1.0, abs(total)))
        r_loss = abs(l32 - total / count) / (CC.LOSS_TOL * max(1.0, abs(total / count)))
        print(f"finish n={n}: fp32 restatement, error / bound: sum {r_sum:.3f}, loss {r_loss:.3f}")
        assert c32 == count and r_sum <= CC.QUARTER and r_loss <= CC.QUARTER
    K = 19
    for dtype in (torch.int64, torch.int32):
        v = CC.shift_values(1000, K, dtype)
        exact, w = CC.shift_expected(v)
        assert bool(exact.any()) and (dtype == torch.int32 or bool((~exact).any()))
        if dtype == torch.int64:                                        # low words that alias to a valid class
            for big in (2 ** 32 + 3, 2 ** 40 + 3):
                assert bool((v == big).any()) and 0 <= ((big & 0xFFFFFFFF) - 1) < K
        # shifted_labels_i32 off the device (no kernel): the same rule as spx_shift_labels, not a 32-bit wrap
        from scaleprotoseg_amd.functional import shifted_labels_i32

        got = shifted_labels_i32(v, "cpu")
        assert got.dtype == torch.int32 and torch.equal(got.long()[exact], w[exact]) and bool((got[~exact] == -1).all())
    assert torch.equal(shifted_labels_i32(torch.tensor([0, 1, 255], dtype=torch.uint8), "cpu"), torch.tensor([-1, 0, 254], dtype=torch.int32))
