"""The pixel-side backward kernel's dispatch, one smallest shape per instance family (spx_bwd_impl.h: launch_bwd_gd).

The launcher reads the plan: when no two panels share a scale it takes the single-panel-per-scale instances, which neither
load nor add a previous partial dX; a scale that spans panels keeps the accumulating code (in dX itself for fp32 features, in
the fp32 scratch for bf16 ones).  Which instance ran cannot be seen from outside, but a wrong choice can: the single-panel
code on a two-panel scale returns the last panel's share of dX alone, far outside the oracle's bound.

Every case
  * holds dX, dPrototypes and dLastLayer to oracle.ppnet_oracle.fwd_bwd_reference at the suite's gradient bounds
    (tests/test_gpu_parity.py: 1e-3 of the largest reference element; 4e-3 for dX returned in bf16),
  * runs the whole forward + backward twice and requires bit-identical gradients,
  * has the backward's dX buffer filled with NaN before the kernel sees it (the buffer is allocated inside the autograd
    function with torch.empty_like; the test wraps that call) and requires every element finite afterwards: dX has exactly the
    image's pixels, so a finite tensor means no pixel inside the image was left unwritten.
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ppnet_oracle as O
from support import BF16_DX_TOL, gpu_device, GRAD_TOL


K = 19
# name: (S, Cs, per-scale prototype counts, H, W)
CASES = {
    "a_six_blocks_partial_last": (1, 64, (190,), 16, 16),        # 6 blocks, 30 of 32 rows in the last; two full tiles
    "b_ragged_tile_odd_grid": (1, 64, (190,), 17, 19),           # 323 px: ragged last tile, H*W % 8 != 0
    "c_two_blocks": (1, 64, (64,), 16, 16),
    "d_one_scale_two_panels": (1, 64, (230,), 17, 19),           # 2 panels of 115: must accumulate
    "e_four_single_panel_scales": (4, 64, (57, 57, 57, 57), 9, 15),
    "f_single_beside_two_panel_scale": (2, 32, (40, 210), 16, 16),
}


# (local: a cached case with its oracle gradients; parity_cases.problem only draws inputs)
@functools.lru_cache(maxsize=None)
def _problem(name):
    """Inputs, upstream gradients and the oracle's results of one case; computed once, shared by the tests, never modified."""
    S, Cs, per_scale, H, W = CASES[name]
    P = sum(per_scale)
    ranges, lo = {}, 0
    for s, n in enumerate(per_scale):
        ranges[s] = (lo, lo + n)
        lo += n
    g = torch.Generator().manual_seed(4100 + sorted(CASES).index(name))
    conv = O.bf16_representable(torch.sigmoid(torch.randn(1, S * Cs, H, W, generator=g)))
    bank = O.bf16_representable(torch.rand(P, Cs, 1, 1, generator=g))
    Wl = torch.randn(K, P, generator=g) * 0.3
    g_logits = torch.randn(1, H, W, K, generator=g) * 1e-3
    g_dist = torch.randn(1, P, H, W, generator=g) * 1e-3
    refs = {"both": O.fwd_bwd_reference(conv, bank, ranges, S, Wl, g_logits, g_dist)[3:]}
    if name.startswith("a_"):
        refs["no_ddist"] = O.fwd_bwd_reference(conv, bank, ranges, S, Wl, g_logits, torch.zeros_like(g_dist))[3:]
        refs["no_dlogits"] = O.fwd_bwd_reference(conv, bank, ranges, S, Wl, torch.zeros_like(g_logits), g_dist)[3:]
    return dict(S=S, Cs=Cs, P=P, H=H, W=W, ranges=ranges, conv=conv, bank=bank, Wl=Wl, g_logits=g_logits, g_dist=g_dist, refs=refs)


def _layout(pr, K_):
    from scaleprotoseg_amd.functional import BankLayout

    return BankLayout(pr["P"], K_, pr["S"], pr["Cs"], tuple(pr["ranges"][s] for s in range(pr["S"])))


def _close(got, ref, what, tol):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    scale = ref.abs().max().item() + 1e-30
    err = (got - ref).abs().max().item()
    print(f"{what}: err {err:.3e} of scale {scale:.3e} = {err / scale:.3e} (bound {tol:.1e})")
    assert err <= tol * scale, f"{what}: err {err:.3e} vs scale {scale:.3e}"


def _nan_filled_empty_like(monkeypatch):
    real = torch.empty_like

    def empty_like(t, *args, **kwargs):
        out = real(t, *args, **kwargs)
        if out.is_floating_point():
            out.fill_(math.nan)
        return out

    monkeypatch.setattr(torch, "empty_like", empty_like)


def _run(pr, x_dtype, dev, use_logits=True, use_dist=True, x_grad=True):
    from scaleprotoseg_amd.functional import proto_head_forward

    x = pr["conv"].to(dev, x_dtype).requires_grad_(x_grad)
    pv = pr["bank"].to(dev).requires_grad_(True)
    w = pr["Wl"].to(dev).requires_grad_(True) if use_logits else None
    logits, dist, _ = proto_head_forward(x, pv, w, _layout(pr, K if use_logits else 1), want_distances=True)
    outs, grads = [], []
    if use_logits:
        outs.append(logits)
        grads.append(pr["g_logits"].reshape(-1, K).to(dev))
    if use_dist:
        outs.append(dist)
        grads.append(pr["g_dist"].to(dev))
    torch.autograd.backward(outs, grads)
    torch.cuda.synchronize()
    return x.grad, pv.grad, (w.grad if use_logits else None)


def _check(pr, x_dtype, dev, ref_key, **kw):
    dx_ref, dp_ref, dw_ref = pr["refs"][ref_key]
    first = _run(pr, x_dtype, dev, **kw)
    second = _run(pr, x_dtype, dev, **kw)
    dx, dp, dw = first
    if kw.get("x_grad", True):
        assert dx.dtype == x_dtype and dx.shape == pr["conv"].shape
        assert torch.isfinite(dx).all(), "a dX element inside the image was left unwritten"
        _close(dx, dx_ref, "dX", GRAD_TOL if x_dtype == torch.float32 else BF16_DX_TOL)
    else:
        assert dx is None
    _close(dp, dp_ref, "dPrototypes", GRAD_TOL)
    if dw is not None:
        _close(dw, dw_ref, "dLastLayer", GRAD_TOL)
    for a, b, what in zip(first, second, ("dX", "dPrototypes", "dLastLayer")):
        assert (a is None and b is None) or torch.equal(a, b), f"{what} differs between two runs"


@pytest.mark.parametrize("x_dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_backward_instance(name, x_dtype, monkeypatch):
    """Cases a-f of the table above, both feature types (d: the fp32 instance sums in dX, the bf16 one in the scratch)."""
    dev = gpu_device()
    pr = _problem(name)
    _nan_filled_empty_like(monkeypatch)
    _check(pr, x_dtype, dev, "both")


@pytest.mark.parametrize("variant", ["no_ddist", "no_dlogits", "x_frozen"])
def test_backward_instance_partial_inputs(variant, monkeypatch):
    """Case a with one input of the backward missing: no distance gradient, no logits gradient (no head), features frozen
    (the kernel then writes no dX at all)."""
    dev = gpu_device()
    pr = _problem("a_six_blocks_partial_last")
    _nan_filled_empty_like(monkeypatch)
    if variant == "no_ddist":
        _check(pr, torch.bfloat16, dev, "no_ddist", use_dist=False)
    elif variant == "no_dlogits":
        _check(pr, torch.bfloat16, dev, "no_dlogits", use_logits=False)
    else:
        _check(pr, torch.bfloat16, dev, "both", x_grad=False)
