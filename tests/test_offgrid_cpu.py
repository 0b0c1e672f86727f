"""Pins tests/offgrid_restatement.py (reference only, no GPU) and keeps tests/test_gpu_offgrid.py from being vacuous: the
references it distinguishes - the oracle at (x, p) against the oracle at (x~, p~), straight-through gradients against the
per-site restatement, round-to-nearest against truncation - must lie further apart than the tolerance the kernels are held to,
at every case the GPU tests run."""
import functools
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import offgrid_restatement as R  # noqa: E402
from oracle import ppnet_oracle as O  # noqa: E402

FP32 = [(c, torch.float32) for c in R.FP32_CASES]
BF16 = [(c, torch.bfloat16) for c in R.BF16_CASES]


def _id(v):
    return v if isinstance(v, str) else str(v).replace("torch.", "")


@functools.lru_cache(maxsize=None)
def _refs(case, x_dtype):
    pb = R.build(case, x_dtype)
    return pb, R.straight_through(pb), R.restated_gradients(pb)


def test_bf16_rne_is_the_torch_cast_and_the_planted_values_round_as_stated():
    g = torch.Generator().manual_seed(1)
    t = torch.cat([torch.randn(4096, generator=g) * 3, torch.rand(4096, generator=g), torch.tensor([0.0, -0.0, 1.0, -1.0, 65504.0])])
    assert torch.equal(R.bf16_rne(t), O.bf16_representable(t))
    assert torch.equal(R.bf16_rne(-t), -R.bf16_rne(t))
    vals = torch.tensor([v for v, _ in R.PLANTED], dtype=torch.float64)
    want = torch.tensor([w for _, w in R.PLANTED], dtype=torch.float32)
    assert torch.equal(vals.float().double(), vals)                       # representable in fp32: ties stay ties
    assert torch.equal(R.bf16_rne(vals.float()), want)                    # ties to even, carry into the next binade
    assert torch.equal(O.bf16_representable(vals.float()), want)
    assert torch.equal(R.bf16_rne(-vals.float()), -want)
    tr = R.bf16_trunc(vals.float())
    assert (tr <= vals.float()).all() and (tr != want).sum().item() >= 4  # truncation is told apart by the planted values alone
    assert torch.equal(R.bf16_trunc(t).abs() <= t.abs(), torch.ones_like(t, dtype=torch.bool))


@pytest.mark.parametrize("case", R.FP32_CASES)
def test_the_builder_plants_the_values_and_leaves_the_rest_off_the_grid(case):
    pb, _, _ = _refs(case, torch.float32)
    for t, index in ((pb.conv, pb.planted.x_index), (pb.bank, pb.planted.p_index)):
        assert len(set(index)) == len(index) == 2 * len(R.PLANTED)
        assert torch.equal(t.reshape(-1)[index], pb.planted.values)
        assert torch.equal(R.bf16_rne(t).reshape(-1)[index], pb.planted.rounded)
        assert (R.bf16_rne(t) != t).float().mean().item() > 0.98


def test_fp16_rtz():
    g = torch.Generator().manual_seed(2)
    t = torch.cat([torch.randn(4096, generator=g) * 10, torch.rand(4096, generator=g) * 1e-3])
    h = R.fp16_rtz(t)
    assert torch.equal(h.half().float(), h)                               # fp16 values ...
    assert (h.abs() <= t.abs()).all()                                     # ... never above |t| ...
    up = torch.nextafter(h.half(), (torch.sign(t) * 65504).half()).float()
    assert ((up.abs() > t.abs()) | (h == t)).all()                        # ... and the next code is
    assert (h != t.half().float()).any()                                  # not the nearest-even cast
    assert torch.equal(R.fp16_rtz(torch.tensor([1e6, -1e6, 65504.0, 65519.9, 65520.0])),
                       torch.tensor([65504.0, -65504.0, 65504.0, 65504.0, 65504.0]))
    x = R.bf16_rne(torch.sigmoid(torch.randn(4096, generator=g)))
    assert torch.equal(R.fp16_rtz(x), x) and torch.equal(R.fp16_rtz(-2 * x), -2 * x)     # bf16 values in the normal range: exact


@pytest.mark.parametrize("case,x_dtype", FP32 + BF16, ids=_id)
def test_on_the_grid_the_restatement_is_autograd(case, x_dtype):
    pb = R.on_grid(R.build(case, x_dtype))
    op = R.site_operands(pb.conv, pb.bank)
    assert all(torch.equal(op[k], pb.conv) for k in "ac") and all(torch.equal(op[k], pb.bank) for k in "bd")
    dX, dP, dW = R.restated_gradients(pb)                                 # (asserts the 1e-12 agreement itself)
    ax, ap, aw, _ = R.autograd_f64(pb, pb.conv, pb.bank)
    for got, ref in ((dX, ax), (dP, ap), (dW, aw)):
        assert R.max_normalised(got, ref) <= 1e-12


def test_a_drifted_site_operand_is_refused():
    pb = R.build("F3")
    op = R.site_operands(pb.conv, pb.bank)
    op["d"] = op["d"] * (1 + 2.0 ** -7)
    with pytest.raises(AssertionError, match="site d"):
        R.restated_gradients(pb, sites=op)


@pytest.mark.parametrize("case,x_dtype", FP32 + BF16, ids=_id)
def test_the_grid_moves_the_distances_by_ten_tolerances(case, x_dtype):
    pb, _, _ = _refs(case, x_dtype)
    d_raw = O.scale_l2_convolution(pb.conv, pb.bank, pb.ranges, pb.shape[1])
    d_rne = R.forward_reference(pb)[1]
    d_trunc = R.forward_reference(pb, R.bf16_trunc)[1]
    assert R.distance_ratio(d_raw, d_rne) >= 10.0                         # a kernel that skipped a rounding ...
    assert R.distance_ratio(d_trunc, d_rne) >= 10.0                       # ... or truncated would be seen


@pytest.mark.parametrize("case,x_dtype", FP32 + BF16, ids=_id)
def test_straight_through_is_not_the_restatement(case, x_dtype):
    """fp32 features: dX (site a) and dP (site d) both lie 2 GRAD_TOL or more from straight-through.  bf16 features: x = x~,
    every X site coincides and dX has no gap by construction; the bank's site d still moves dP."""
    pb, (sx, sp, sw, _), (rx, rp, rw) = _refs(case, x_dtype)
    assert R.max_normalised(sp, rp) >= 2 * R.GRAD_TOL
    if x_dtype == torch.float32:
        assert R.max_normalised(sx, rx) >= 2 * R.GRAD_TOL
    else:
        assert R.max_normalised(sx, rx) <= 1e-12
    assert R.max_normalised(sw, rw) <= 1e-12                              # the head does not meet these sites


@pytest.mark.parametrize("case", R.FP32_CASES)
def test_a_swapped_site_or_rounding_moves_the_reference_past_the_tolerance(case):
    """What a reviewer would do by hand: site a <- x~, site d <- p~, site c <- fp16_rtz(x) (no bf16 rounding first): each moves
    the gradient reference by more than GRAD_TOL.  Truncation for round-to-nearest moves the forward reference by more than ten
    distance tolerances (test_the_grid_moves_the_distances_by_ten_tolerances); in the gradients it only perturbs G."""
    pb, _, (rx, rp, _) = _refs(case, torch.float32)
    for site, value, which in (("a", R.bf16_rne(pb.conv), 0), ("d", R.bf16_rne(pb.bank), 1), ("c", R.fp16_rtz(pb.conv), 1)):
        op = R.site_operands(pb.conv, pb.bank)
        op[site] = value
        moved = R.restated_gradients(pb, sites=op)[which]
        assert R.max_normalised(moved, (rx, rp)[which]) > R.GRAD_TOL, site
