"""The four device implementations of the pixel-wise cross entropy against float64 OF THE LOGITS THEY RETURN, per pixel:

  1  the stand-alone kernels of csrc/spx_ce.hip (spx_ce_fwd / spx_ce_bwd / spx_ce_finish), through cross_entropy_from_logits
     and through the C ABI;  2  spx_ce_finish alone on crafted pairs;  3  spx_shift_labels alone;
  4  the fused epilogue of csrc/spx_fwd_impl.h (entered through spx_dist_fwd_ce) with the prologue of csrc/spx_bwd_impl.h;
  5  the grouping tail kernel (spx_group_tail_kernel) with the prologue's group-tail branch and d W_g.

Bounds and reference: tests/ce_cases.py (tests/test_ce_inputs_cpu.py holds a plain fp32 restatement to a quarter of each):
pred and count exact, lse to 8 eps32 max(1, |lse64|), loss to 4e-6 max(1, |loss64|) with loss64 >= 0.05, d_logits per element,
rows of ignored pixels exactly 0, NaN loss / zero gradient when every pixel is ignored.  Every test prints error / bound before
it asserts; profiles/ce_float64_summary.md has one run's figures and the arithmetic mutation these tests were tried on.

Every case runs with the float results of torch.empty / torch.empty_like pre-filled with NaN and the int32 ones with a sentinel
(the ``poisoned`` fixture), so an lse, pred, partial pair or d_logits element the kernels leave unwritten is a failure, not a
zero the allocator happened to hand out.

Where the per-pixel lse comes from: the C ABI call's own buffer for the stand-alone kernels; for the fused paths the tuple
``ce_state`` = (labels, lse, pred, partials) the autograd node keeps, reached as ``fce.loss.grad_fn.ce_state``.  The d_logits
buffer the backward prologue writes is the ``torch.empty_like`` of the saved logits inside backward(), caught by the fixture."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import ce_cases as CC
from oracle import ppnet_oracle as O
from support import BF16_DX_TOL, bits_equal, gpu_device, grad_close, GRAD_TOL

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A


@pytest.fixture
def poisoned(monkeypatch):
    """torch.empty / torch.empty_like hand out NaN (float) and SENTINEL (int32); returns the list of empty_like results."""
    made = []
    real_empty, real_like = torch.empty, torch.empty_like

    def poison(t):
        if t.is_floating_point():
            t.fill_(math.nan)
        elif t.dtype == torch.int32:
            t.fill_(SENTINEL)
        return t

    def empty(*args, **kwargs):
        return poison(real_empty(*args, **kwargs))

    def empty_like(*args, **kwargs):
        out = poison(real_like(*args, **kwargs))
        made.append(out)
        return out

    monkeypatch.setattr(torch, "empty", empty)
    monkeypatch.setattr(torch, "empty_like", empty_like)
    return made


def _coef(count):
    """The factor the backward forms on the device: fp32 1 / fp32 count (a gradient of 1 on the loss)."""
    return float(np.float32(1.0) / np.float32(count)) if count else 0.0


def _check_forward(what, ref, lse, pred, count, loss, no_loss=None):
    """pred, count, lse, loss of one launch against the float64 reference of the same logits; returns the ratios."""
    ratios = {"lse": CC.lse_ratio(lse, ref)}
    wrong = CC.pred_mismatches(pred, ref)
    if no_loss is None:
        ratios["loss"] = CC.loss_ratio(loss, ref)
    print(f"CE64 {what}: loss {float(loss):.9g} float64 {ref['loss']:.9g}, count {float(count):.0f}/{ref['count']}, "
          f"pred off on {wrong}; error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert wrong == 0
    assert float(count) == ref["count"]
    if no_loss == "nan":
        assert math.isnan(float(loss)) and ref["count"] == 0
    elif no_loss == "zero":
        assert abs(float(loss)) <= CC.LOSS_TOL and ref["loss"] == 0.0
    else:
        assert ref["loss"] >= CC.MIN_LOSS                               # the value assertion is live
    failed = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not failed, failed
    return ratios


def _check_dlogits(what, d, logits, labels, count):
    ref = CC.reference(logits, labels, coef=_coef(count))
    worst, ignored = CC.dlogits_ratio(d, ref)
    print(f"CE64 {what}: d_logits error / bound {worst:.3f}, largest |d| on an ignored row {ignored:g}")
    assert ignored == 0.0
    assert worst <= 1.0
    if count == 0:
        assert not d.any()                                              # every element exactly 0 (NaN would be "any")
        assert not torch.isnan(d).any()
    return worst


# ------------------------------------------------------------------------------------------------------------------
# 1  stand-alone kernels
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case_reference(name):
    c = CC.case(name)
    return CC.reference(c.logits, c.labels)


def _abi_run(lg, lab):
    """spx_ce_fwd + spx_ce_finish + spx_ce_bwd through the C ABI on buffers of this test's own (NaN / sentinel filled)."""
    from scaleprotoseg_amd import _lib

    lib = _lib.load()
    M, K = lg.shape
    dev = lg.device
    s = _lib.stream_ptr()
    lse = torch.full((M,), math.nan, device=dev)
    pred = torch.full((M,), SENTINEL, dtype=torch.int32, device=dev)
    n = int(lib.spx_ce_partials_flat(M))
    assert n == 4 * ((M + 255) // 256)
    partials = torch.full((n, 2), math.nan, device=dev)
    _lib.check(lib.spx_ce_fwd(_lib.ptr(lg), _lib.ptr(lab), M, K, _lib.ptr(lse), _lib.ptr(pred), _lib.ptr(partials), s))
    loss = torch.full((), math.nan, device=dev)
    aux = torch.full((2,), math.nan, device=dev)
    _lib.check(lib.spx_ce_finish(_lib.ptr(partials), n, _lib.ptr(loss), _lib.ptr(aux), s))
    coef = (torch.ones((), device=dev) / aux[0]).reshape(1).contiguous()
    d = torch.full((M, K), math.nan, device=dev)
    _lib.check(lib.spx_ce_bwd(_lib.ptr(lg), _lib.ptr(lse), _lib.ptr(lab), _lib.ptr(coef), M, K, _lib.ptr(d), s))
    torch.cuda.synchronize()
    return lse, pred, partials, loss, aux, d


def _module_run(lg, lab):
    from scaleprotoseg_amd.functional import cross_entropy_from_logits

    x = lg.clone().requires_grad_(True)
    out = cross_entropy_from_logits(x, lab)
    out.loss.backward()
    torch.cuda.synchronize()
    return out.loss.detach(), out.pred, x.grad


@pytest.mark.parametrize("name", CC.CASE_NAMES)
def test_standalone_kernels_against_float64(name, poisoned):
    dev = gpu_device()
    c = CC.case(name)
    ref = _case_reference(name)
    lg, lab = c.logits.to(dev).contiguous(), c.labels.to(dev).contiguous()
    lse, pred, partials, loss, aux, d = _abi_run(lg, lab)
    assert not torch.isnan(partials).any(), "a partial pair was left unwritten"
    assert float(partials[:, 1].sum()) == ref["count"]
    _check_forward(f"{name} C ABI", ref, lse, pred, aux[0], loss, c.no_loss)
    if c.no_loss != "nan":
        assert float(loss) == float(np.float32(aux[1].item()) / np.float32(aux[0].item()))
    _check_dlogits(f"{name} C ABI", d, lg, lab, ref["count"])
    m_loss, m_pred, m_grad = _module_run(lg, lab)
    _check_forward(f"{name} module", ref, lse, m_pred, ref["count"], m_loss, c.no_loss)
    _check_dlogits(f"{name} module", m_grad, lg, lab, ref["count"])
    # the two routes are the same kernels on the same inputs, and a second run of either changes nothing
    assert bits_equal(m_loss, loss) and torch.equal(m_pred, pred) and bits_equal(m_grad, d)
    again = _abi_run(lg, lab)
    for a, b in zip((lse, pred, partials, loss, aux, d), again):
        assert bits_equal(a, b)
    m_again = _module_run(lg, lab)
    assert bits_equal(m_again[0], m_loss) and torch.equal(m_again[1], m_pred) and bits_equal(m_again[2], m_grad)


# ------------------------------------------------------------------------------------------------------------------
# 2  spx_ce_finish alone   3  spx_shift_labels alone
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", CC.FINISH_SIZES)
def test_finish_kernel_on_crafted_pairs(n, poisoned):
    from scaleprotoseg_amd.functional import _ce_finish

    dev = gpu_device()
    pairs, count, total = CC.finish_pairs(n)
    loss, aux = _ce_finish(pairs.to(dev))                               # its outputs come from the poisoned torch.empty
    torch.cuda.synchronize()
    r_sum = abs(aux[1].item() - total) / (CC.LOSS_TOL * max(1.0, abs(total)))
    r_loss = abs(loss.item() - total / count) / (CC.LOSS_TOL * max(1.0, abs(total / count)))
    print(f"CE64 finish n={n}: count {aux[0].item():.0f}/{count}, error / bound: sum {r_sum:.3f}, loss {r_loss:.3f}")
    assert total / count >= CC.MIN_LOSS
    assert aux[0].item() == count
    assert r_sum <= 1.0 and r_loss <= 1.0
    assert loss.item() == float(np.float32(aux[1].item()) / np.float32(aux[0].item()))


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32], ids=["int64", "int32"])
@pytest.mark.parametrize("n", CC.SHIFT_SIZES)
def test_shift_labels_kernel(n, dtype, poisoned):
    from scaleprotoseg_amd.functional import shifted_labels_i32

    dev = gpu_device()
    K = 19
    v = CC.shift_values(n, K, dtype)
    out = shifted_labels_i32(v.to(dev), dev)                             # on the device: the kernel
    torch.cuda.synchronize()
    assert out.dtype == torch.int32 and out.is_cuda and tuple(out.shape) == (n,)
    got = out.cpu().long()
    exact, want = CC.shift_expected(v)
    print(f"CE64 shift_labels n={n} {dtype}: {int((got != want)[exact].sum())} of {int(exact.sum())} exact values off, "
          f"{int((got[~exact] >= 0).sum())} of {int((~exact).sum())} out-of-range values not negative")
    assert torch.equal(got[exact], want[exact])
    assert bool((got[~exact] < 0).all())                                # SENTINEL (unwritten) is positive too
    is_class = (want >= 0) & (want < K)
    assert torch.equal((got >= 0) & (got < K), is_class)                # no aliased low word becomes a class
    cpu = shifted_labels_i32(v, "cpu")                                  # off the device: the fallback
    assert cpu.dtype == torch.int32 and torch.equal(cpu, out.cpu())


# ------------------------------------------------------------------------------------------------------------------
# 4  fused epilogue + backward prologue
# ------------------------------------------------------------------------------------------------------------------
FUSED_K = (5, 19, 33, 64, 65, 150, 160)                                # one, two, three (strided stores from 65 up) and five class blocks
FUSED_GRIDS = {"16x16": (1, 16, 16), "17x19": (1, 17, 19), "1x37": (1, 1, 37), "3x8x16": (3, 8, 16)}
FUSED_RUNS = [(K, g, torch.float32) for K in FUSED_K for g in FUSED_GRIDS] + [(K, g, torch.bfloat16) for K in (19, 65) for g in FUSED_GRIDS]


def _fused_inputs(B, S, Cs, P, K, H, W, seed, head=None):
    gen = torch.Generator().manual_seed(seed)
    conv = O.bf16_representable(torch.sigmoid(torch.randn(B, S * Cs, H, W, generator=gen)))
    bank = O.bf16_representable(torch.rand(P, Cs, 1, 1, generator=gen))
    if head is None:
        head = torch.randn(K, P, generator=gen) * 0.3
    lab = CC.mixed_labels(B * H * W, K, gen).reshape(B, H * W)
    return conv, bank, head, lab


def _fused_run(conv, bank, head, lab, S, x_dtype, dev, made, gather=None, g_cls=None, backward=True, split=False):
    """proto_head_forward(..., ce_labels=) and the backward of the loss alone.  Returns a dict of what the kernels left."""
    from scaleprotoseg_amd import _lib
    from scaleprotoseg_amd.functional import BankLayout, proto_head_forward

    B, _, H, W = conv.shape
    K, P = head.shape
    Cs = bank.shape[1]
    ranges = O.default_scale_ranges(P, S)
    lay = BankLayout(P, K, S, Cs, tuple(tuple(ranges[s]) for s in range(S)))
    # the epilogue, not the stand-alone kernel behind a scale-parallel forward (``split``: that one, on purpose)
    assert (_lib.load().spx_fwd_split_workspace_bytes(C.byref(lay.plan()), B, H * W) != 0) == split
    x = conv.to(dev, x_dtype).requires_grad_(True)
    pv = bank.to(dev).requires_grad_(True)
    w = head.to(dev).requires_grad_(True)
    labd = lab.to(dev).contiguous()
    if gather is not None:
        gather = gather(lay, dev)
    out = proto_head_forward(x, pv, w, lay, want_distances=False, class_gather=gather, ce_labels=labd)
    logits, cd, fce = out[0], out[1], out[3]
    state = fce.loss.grad_fn.ce_state
    assert state[0] is not None and state[2] is fce.pred
    res = {"logits": logits.detach(), "lse": state[1], "pred": fce.pred, "partials": state[3], "loss": fce.loss.detach(),
           "count": fce.loss.grad_fn.ce_count, "x": x, "pv": pv, "w": w, "ranges": ranges}
    if backward:
        before = len(made)
        total = fce.loss if g_cls is None else fce.loss + (cd * g_cls.to(dev)).sum()
        total.backward()
        torch.cuda.synchronize()
        mine = [t for t in made[before:] if t.shape == logits.shape and t.dtype == torch.float32]
        assert len(mine) == 1, "the prologue's d_logits buffer was not allocated"
        res["d_logits"] = mine[0]
    torch.cuda.synchronize()
    return res


def _fused_check(what, res, lab, no_loss=None):
    ref = CC.reference(res["logits"], lab.reshape(-1))
    assert not torch.isnan(res["partials"]).any(), "a partial pair was left unwritten"
    assert float(res["partials"][:, 1].sum()) == ref["count"]
    _check_forward(what, ref, res["lse"], res["pred"], res["count"], res["loss"], no_loss)
    if "d_logits" in res:
        _check_dlogits(what, res["d_logits"], res["logits"], lab.reshape(-1), ref["count"])
    return ref


def _oracle_grads(conv, bank, head, lab, ranges, S, extra=None):
    c0, p0, w0 = conv.clone().requires_grad_(True), bank.clone().requires_grad_(True), head.clone().requires_grad_(True)
    rl, rd, _ = O.forward_from_conv_features(c0, p0, ranges, S, w0)
    K = head.shape[0]
    flat = lab.reshape(-1).long()
    tl = torch.where((flat >= 0) & (flat < K), flat, torch.full_like(flat, -1))
    loss = torch.nn.functional.cross_entropy(rl.reshape(-1, K), tl, ignore_index=-1)
    if extra is not None:
        loss = loss + extra(rd)
    loss.backward()
    return c0.grad, p0.grad, w0.grad


def _check_oracle(what, res, conv, bank, head, lab, S, x_dtype, extra=None):
    dx, dp, dw = _oracle_grads(conv, bank, head, lab, res["ranges"], S, extra)
    grad_close(res["w"].grad, dw, f"{what} dLastLayer", report="CE64")
    grad_close(res["x"].grad, dx, f"{what} dX", tol=GRAD_TOL if x_dtype == torch.float32 else BF16_DX_TOL, report="CE64")
    grad_close(res["pv"].grad, dp, f"{what} dPrototypes", report="CE64")


@pytest.mark.parametrize("K,grid,x_dtype", FUSED_RUNS, ids=[f"K{K}-{g}-{'bf16' if t == torch.bfloat16 else 'fp32'}" for K, g, t in FUSED_RUNS])
def test_fused_epilogue_and_prologue_against_float64(K, grid, x_dtype, poisoned):
    dev = gpu_device()
    B, H, W = FUSED_GRIDS[grid]
    S, Cs, P = 1, 32, 48
    conv, bank, head, lab = _fused_inputs(B, S, Cs, P, K, H, W, seed=1000 * K + H * W)
    res = _fused_run(conv, bank, head, lab, S, x_dtype, dev, poisoned)
    what = f"fused K={K} {grid} {str(x_dtype)[6:]}"
    if grid == "1x37":                                                  # pixel groups 1 - 3 of the only tile: partly empty, empty, empty
        assert tuple(res["partials"].shape) == (4, 2) and not res["partials"][2:].any()
    _fused_check(what, res, lab)
    _check_oracle(what, res, conv, bank, head, lab, S, x_dtype)


def test_fused_epilogue_class_gathered(poisoned):
    """class_gather= and ce_labels= together (the training step's launch); the slot planes carry a gradient of their own, the
    logits none, so d_logits still comes from the prologue."""
    from scaleprotoseg_amd.functional import ClassGather, class_gather_table

    dev = gpu_device()
    B, S, Cs, P, K, H, W = 2, 1, 32, 40, 5, 9, 11
    conv, bank, head, _ = _fused_inputs(B, S, Cs, P, K, H, W, seed=5911)
    gen = torch.Generator().manual_seed(5912)
    lab = torch.randint(-1, K, (B, H * W), generator=gen, dtype=torch.int32)
    ident = O.default_class_identity(P, K, S)
    width = {}

    def gather(lay, dev_):
        keys, J, table = class_gather_table(lay, ident, dev_)
        width["J"] = J
        return ClassGather(labels=lab.to(dev_).contiguous(), keys=keys, width=J, table=table)

    J = int(O.class_slot_table(ident).shape[1])
    g_cls = torch.randn(B, H * W, J, generator=gen) * 1e-3               # oracle layout [B, HW, J]; the kernels' is [B, J, HW]
    res = _fused_run(conv, bank, head, lab, S, torch.float32, dev, poisoned, gather=gather, g_cls=g_cls.permute(0, 2, 1).contiguous())
    assert width["J"] == J
    _fused_check("fused class-gathered", res, lab)
    _check_oracle("fused class-gathered", res, conv, bank, head, lab, S, torch.float32,
                  extra=lambda rd: (O.gather_class_distances(rd, lab.long(), ident) * g_cls).sum())


@pytest.mark.parametrize("K", [3, 19])
def test_fused_epilogue_two_scales_above_the_split_limit(K, poisoned):
    """S = 2 takes the epilogue only past 1024 tiles of 128 pixels: 257 x 511 px are 1026.  (K = 3 keeps every class in one
    lane half of the accumulator layout - rows 0 - 3 - so the sums across the halves only matter with K = 19.)"""
    dev = gpu_device()
    B, S, Cs, P, H, W = 1, 2, 16, 16, 257, 511
    assert (H * W + 127) // 128 == 1026
    conv, bank, head, lab = _fused_inputs(B, S, Cs, P, K, H, W, seed=257511 + K)
    res = _fused_run(conv, bank, head, lab, S, torch.float32, dev, poisoned)
    _fused_check(f"fused S=2 K={K} 257x511", res, lab)
    _check_oracle(f"fused S=2 K={K} 257x511", res, conv, bank, head, lab, S, torch.float32)


@pytest.mark.parametrize("K", [19, 65])
def test_standalone_forward_behind_a_scale_parallel_launch(K, poisoned):
    """Two scales on a small grid (the training crops' launch): the forward runs scale-parallel, spx_ce_fwd takes the summed
    logits, and the backward's prologue reads the lse that kernel left."""
    dev = gpu_device()
    B, S, Cs, P, H, W = 2, 2, 32, 48, 17, 19
    conv, bank, head, lab = _fused_inputs(B, S, Cs, P, K, H, W, seed=2200 + K)
    res = _fused_run(conv, bank, head, lab, S, torch.float32, dev, poisoned, split=True)
    assert tuple(res["partials"].shape) == (4 * ((B * H * W + 255) // 256), 2)
    _fused_check(f"scale-parallel S=2 K={K}", res, lab)
    _check_oracle(f"scale-parallel S=2 K={K}", res, conv, bank, head, lab, S, torch.float32)


@pytest.mark.parametrize("K,lo,hi", [(19, 1, 5), (65, 2, 40)])
def test_fused_epilogue_breaks_ties_to_the_lower_class(K, lo, hi, poisoned):
    """Two identical positive head rows, every other row zero: the two logit columns are bit-equal and the largest, and
    sit in different lane halves / class blocks of the accumulator layout."""
    dev = gpu_device()
    B, S, Cs, P, H, W = 1, 1, 32, 48, 17, 19
    gen = torch.Generator().manual_seed(K)
    head = torch.zeros(K, P)
    head[lo] = head[hi] = torch.rand(P, generator=gen) * 0.3 + 0.05
    conv, bank, head, lab = _fused_inputs(B, S, Cs, P, K, H, W, seed=77 + K, head=head)
    res = _fused_run(conv, bank, head, lab, S, torch.float32, dev, poisoned)
    lg = res["logits"]
    assert bits_equal(lg[:, lo].contiguous(), lg[:, hi].contiguous()) and bool((lg[:, lo] > 0).all())
    others = torch.ones(K, dtype=torch.bool)
    others[[lo, hi]] = False
    assert not lg[:, others.to(dev)].any()
    assert bool((res["pred"] == lo).all())
    _fused_check(f"fused tie K={K}", res, lab)


@pytest.mark.parametrize("K", [19, 65])
def test_fused_epilogue_on_an_all_zero_head(K, poisoned):
    dev = gpu_device()
    B, S, Cs, P, H, W = 1, 1, 32, 48, 17, 19
    conv, bank, head, lab = _fused_inputs(B, S, Cs, P, K, H, W, seed=99 + K, head=torch.zeros(K, P))
    res = _fused_run(conv, bank, head, lab, S, torch.float32, dev, poisoned)
    assert not res["logits"].any() and bool((res["pred"] == 0).all())
    ref = _fused_check(f"fused zero head K={K}", res, lab)
    assert abs(ref["loss"] - math.log(K)) <= 1e-12
    worst = float((res["lse"].double() - math.log(K)).abs().max()) / (CC.LSE_ULPS * CC.EPS32 * math.log(K))
    r_loss = abs(float(res["loss"]) - math.log(K)) / (CC.LOSS_TOL * math.log(K))
    print(f"CE64 fused zero head K={K}: against log K, error / bound: lse {worst:.3f}, loss {r_loss:.3f}")
    assert worst <= 1.0 and r_loss <= 1.0


def test_fused_epilogue_with_every_pixel_ignored(poisoned):
    dev = gpu_device()
    B, S, Cs, P, K, H, W = 1, 1, 32, 48, 19, 17, 19
    conv, bank, head, _ = _fused_inputs(B, S, Cs, P, K, H, W, seed=4242)
    bad = torch.tensor([-1, -2, K, K + 7, CC.INT32_MIN, CC.INT32_MAX])
    lab = bad[torch.arange(H * W) % 6].to(torch.int32).reshape(B, H * W)
    res = _fused_run(conv, bank, head, lab, S, torch.float32, dev, poisoned)
    _fused_check("fused all ignored", res, lab, no_loss="nan")
    assert not res["d_logits"].any() and not torch.isnan(res["d_logits"]).any()
    assert not res["w"].grad.any() and not torch.isnan(res["w"].grad).any()


# ------------------------------------------------------------------------------------------------------------------
# 5  grouping tail
# ------------------------------------------------------------------------------------------------------------------
# (U, K2, B, H, W): M = B H W with ceil(M / 64) % 4 = 0, 2, 1, 3 and M % 64 = 0, 1, 63, 63
TAIL_RUNS = [(15, 5, 2, 8, 16), (57, 19, 1, 5, 13), (63, 21, 1, 7, 9), (160, 32, 1, 1, 191)]


def _tail_run(U, K2, B, H, W, dev, made, wg=None, lab=None, seed=0):
    from scaleprotoseg_amd.functional import BankLayout, proto_head_forward

    S, Cs, P = 1, 32, 64
    M = B * H * W
    gen = torch.Generator().manual_seed(seed + 31 * U + M)
    x = torch.sigmoid(torch.randn(B, S * Cs, H, W, generator=gen)).bfloat16().to(dev).requires_grad_(True)
    bank = torch.rand(P, Cs, 1, 1, generator=gen).bfloat16().float().to(dev).requires_grad_(True)
    wd = (torch.rand(U, P, generator=gen) * 0.02).to(dev).requires_grad_(True)
    if wg is None:
        wg = torch.randn(K2, U, generator=gen) * 0.1
    wg = wg.to(dev).requires_grad_(True)
    if lab is None:
        lab = CC.mixed_labels(M, K2, gen)
    labd = lab.reshape(B, H * W).to(dev).contiguous()
    lay = BankLayout(P, U, S, Cs, ((0, P),))
    out = proto_head_forward(x, bank, wd, lay, want_distances=True, group_tail=wg, ce_labels=labd)
    logits, fce, gact = out[0], out[3], out[4]
    state = fce.loss.grad_fn.ce_state
    before = len(made)
    fce.loss.backward()
    torch.cuda.synchronize()
    mine = [t for t in made[before:] if t.shape == logits.shape and t.dtype == torch.float32]
    assert len(mine) == 1, "the prologue's d_logits buffer was not allocated"
    return {"logits": logits.detach(), "gact": gact.detach(), "lse": state[1], "pred": fce.pred, "partials": state[3],
            "loss": fce.loss.detach(), "count": fce.loss.grad_fn.ce_count, "d_logits": mine[0], "wg": wg, "lab": lab}


@pytest.mark.parametrize("U,K2,B,H,W", TAIL_RUNS)
def test_group_tail_against_float64(U, K2, B, H, W, poisoned):
    dev = gpu_device()
    M = B * H * W
    res = _tail_run(U, K2, B, H, W, dev, poisoned)
    what = f"tail U={U} K2={K2} M={M}"
    assert tuple(res["partials"].shape) == (4 * ((M + 255) // 256), 2)
    assert not res["partials"][(M + 63) // 64:].any()                  # the padding pairs: cleared by the last workgroup
    ref = _fused_check(what, res, res["lab"])
    refc = CC.reference(res["logits"], res["lab"], coef=_coef(ref["count"]))
    r = CC.dw_ratio(res["wg"].grad, refc["d"], res["gact"])
    print(f"CE64 {what}: d W_g error / bound {r:.3f}")
    assert r <= 1.0


def test_group_tail_breaks_ties_across_class_quarters(poisoned):
    """Classes 3 and 19 (class quarters 0 and 2) with identical positive rows of W_g, every other row zero."""
    dev = gpu_device()
    U, K2, B, H, W = 63, 21, 1, 7, 9
    gen = torch.Generator().manual_seed(319)
    wg = torch.zeros(K2, U)
    wg[3] = wg[19] = torch.rand(U, generator=gen) * 0.1 + 0.01
    res = _tail_run(U, K2, B, H, W, dev, poisoned, wg=wg, seed=1)
    lg = res["logits"]
    assert bits_equal(lg[:, 3].contiguous(), lg[:, 19].contiguous()) and bool((lg[:, 3] > 0).all())
    assert bool((res["pred"] == 3).all())
    _fused_check("tail tie 3 / 19", res, res["lab"])
