"""The segmented cross entropy on the GPU (csrc/spx_ce.hip: spx_ce_seg_fwd / spx_ce_seg_finish / spx_ce_seg_bwd;
``segmented_cross_entropy``, ``SegmentedCrossEntropy``) on the cases of tests/ce_segment_cases.py.

The rule held for every segment of every case: the loss, the lse and pred rows, the counts and d_logits - through ``losses`` alone,
through ``mean`` alone and through both - are BIT FOR BIT what the stand-alone kernels (spx_ce_fwd / spx_ce_finish / spx_ce_bwd,
the path of ``cross_entropy_from_logits``) give on the contiguous slice with coef = g_k / count_k, and lie within the float64
bounds of tests/ce_cases.py.  ``valid`` and ``correct`` are exact against NumPy, ``mean`` is the left-to-right fp32 sum over S, two
runs agree bit for bit, and every output sits in a guarded buffer at an odd element offset.  Then the module: the zero-copy route
(segments of one packed forward) against the concatenating one, its voiding by an in-place edit, ``PixelWiseCrossEntropyLoss`` per
segment, and a replay inside ``graphs.capture_step``."""
import ctypes as C
import functools
import gc
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ce_cases as CC
import ce_segment_cases as SC
import msc_pack_cases as PC
import parity_cases as PAR
from support import Guarded, bits_equal, gpu_device, proto_net, release_cached_blocks  # noqa: F401

import scaleprotoseg_amd as spx

MODES = ("losses", "mean", "both")


def _guarded(n, dtype, dev, fill):
    """n elements of ``dtype`` one element into a guarded buffer (an odd element offset), filled with ``fill``."""
    g = Guarded((n + 2) * 4, dev)
    body = g.body(dtype)
    body.fill_(fill)
    return g, body[1:1 + n]


def _segmented_abi(c, dev, g_losses, g_mean):
    """The three launches through the C ABI on guarded buffers; one backward per mode.  Returns a dict of what they left."""
    from scaleprotoseg_amd import _lib
    from scaleprotoseg_amd.functional import ce_segment_table

    lib = _lib.load()
    lg, lab = c.logits.to(dev).contiguous(), c.labels.to(dev).contiguous()
    M, K, S = lg.shape[0], c.K, c.S
    seg = ce_segment_table(c.offsets, M)
    n_tr = int(lib.spx_ce_seg_partials(C.byref(seg)))
    assert n_tr == 4 * sum((n + 255) // 256 for n in c.sizes)
    s = _lib.stream_ptr()
    nan, sent = math.nan, 0x5A5A5A5A
    guards, out = [], {}
    for name, n, dtype, fill in (("lse", M, torch.float32, nan), ("pred", M, torch.int32, sent), ("partials", 3 * n_tr, torch.float32, nan),
                                 ("losses", S, torch.float32, nan), ("mean", 1, torch.float32, nan), ("count", S, torch.float32, nan),
                                 ("valid", S, torch.int32, sent), ("correct", S, torch.int32, sent)):
        g, out[name] = _guarded(n, dtype, dev, fill)
        guards.append(g)
    p = lambda t: t.data_ptr()
    _lib.check(lib.spx_ce_seg_fwd(p(lg), p(lab), C.byref(seg), K, p(out["lse"]), p(out["pred"]), p(out["partials"]), s))
    _lib.check(lib.spx_ce_seg_finish(p(out["partials"]), C.byref(seg), p(out["losses"]), p(out["mean"]), p(out["count"]),
                                     p(out["valid"]), p(out["correct"]), s))
    gl, gm = g_losses.to(dev).contiguous(), g_mean.to(dev).reshape(1).contiguous()
    for mode in MODES:
        g, d = _guarded(M * K, torch.float32, dev, nan)
        guards.append(g)
        _lib.check(lib.spx_ce_seg_bwd(p(lg), p(out["lse"]), p(lab), C.byref(seg), p(out["count"]), p(gl) if mode != "mean" else None,
                                      p(gm) if mode != "losses" else None, K, p(d), s))
        out["d_" + mode] = d.view(M, K)
    torch.cuda.synchronize()
    assert all(g.intact() for g in guards), "a kernel wrote outside its buffer"
    assert not torch.isnan(out["partials"]).any(), "a partial triple was left unwritten"
    return {k: v.clone() for k, v in out.items()}


def _slice_upstream(g_losses, g_mean, S, mode):
    """The fp32 gradient that reaches segment k's loss: g_losses[k], fp32(g_mean / S), or their fp32 sum."""
    gm = (g_mean.float() / torch.tensor(float(S))).float()
    if mode == "losses":
        return g_losses.clone()
    if mode == "mean":
        return gm.expand(S).clone()
    return g_losses + gm


def _standalone_abi(lg, lab, gs):
    """spx_ce_fwd + spx_ce_finish on one contiguous slice, and one spx_ce_bwd per upstream gradient in ``gs`` with
    coef = g / count formed as ``cross_entropy_from_logits`` forms it (one fp32 division on the device)."""
    from scaleprotoseg_amd import _lib

    lib = _lib.load()
    M, K = lg.shape
    dev = lg.device
    s = _lib.stream_ptr()
    lse = torch.full((M,), math.nan, device=dev)
    pred = torch.full((M,), -7, dtype=torch.int32, device=dev)
    n = int(lib.spx_ce_partials_flat(M))
    partials = torch.full((n, 2), math.nan, device=dev)
    _lib.check(lib.spx_ce_fwd(_lib.ptr(lg), _lib.ptr(lab), M, K, _lib.ptr(lse), _lib.ptr(pred), _lib.ptr(partials), s))
    loss, aux = torch.full((), math.nan, device=dev), torch.full((2,), math.nan, device=dev)
    _lib.check(lib.spx_ce_finish(_lib.ptr(partials), n, _lib.ptr(loss), _lib.ptr(aux), s))
    ds = []
    for g in gs:
        coef = (g.to(dev).float() / aux[0]).reshape(1).contiguous()
        d = torch.full((M, K), math.nan, device=dev)
        _lib.check(lib.spx_ce_bwd(_lib.ptr(lg), _lib.ptr(lse), _lib.ptr(lab), _lib.ptr(coef), M, K, _lib.ptr(d), s))
        ds.append(d)
    return lse, pred, loss, aux, ds


@functools.lru_cache(maxsize=None)
def _runs(name):
    """One segmented run and the stand-alone run of every slice, shared by the tests below (never modified)."""
    dev = gpu_device()
    c = SC.case(name)
    gl, gm = SC.upstream(c.S, seed=len(name))
    seg = _segmented_abi(c, dev, gl, gm)
    ups = {m: _slice_upstream(gl, gm, c.S, m) for m in MODES}
    alone = []
    for k, lg, lab in c.slices():
        alone.append(_standalone_abi(lg.to(dev).contiguous(), lab.to(dev).contiguous(), [ups[m][k] for m in MODES]))
    torch.cuda.synchronize()
    return c, seg, alone, ups


@pytest.mark.parametrize("name", SC.CASE_NAMES)
def test_every_segment_carries_the_standalone_bits(name):
    c, seg, alone, _ = _runs(name)
    o = c.offsets
    for k in range(c.S):
        lse, pred, loss, aux, ds = alone[k]
        rows = slice(o[k], o[k + 1])
        assert bits_equal(seg["lse"][rows], lse), (name, k, "lse")
        assert torch.equal(seg["pred"][rows], pred), (name, k, "pred")
        assert bits_equal(seg["losses"][k], loss), (name, k, "loss", float(seg["losses"][k]), float(loss))
        assert bits_equal(seg["count"][k], aux[0]), (name, k, "count")
        for mode, d in zip(MODES, ds):
            assert bits_equal(seg["d_" + mode][rows], d), (name, k, mode)
    print(f"CESEG {name}: {c.S} segments bit-equal to the stand-alone kernels (lse, pred, loss, count, d_logits x {len(MODES)})")


@pytest.mark.parametrize("name", SC.CASE_NAMES)
def test_every_segment_against_float64_and_numpy(name):
    c, seg, _, ups = _runs(name)
    refs = SC.references(name)
    o = c.offsets
    worst = {"lse": 0.0, "loss": 0.0, "d_logits": 0.0}
    losses = seg["losses"].cpu().numpy()
    for (k, lg, lab), ref in zip(c.slices(), refs):
        rows = slice(o[k], o[k + 1])
        # counts, exact
        labn, predn = lab.numpy().astype(np.int64), seg["pred"][rows].cpu().numpy().astype(np.int64)
        validn = (labn >= 0) & (labn < c.K)
        assert int(seg["valid"][k]) == int(validn.sum()) == ref["count"] and float(seg["count"][k]) == ref["count"]
        assert int(seg["correct"][k]) == int((validn & (predn == labn)).sum())
        assert CC.pred_mismatches(seg["pred"][rows], ref) == 0
        worst["lse"] = max(worst["lse"], CC.lse_ratio(seg["lse"][rows], ref))
        if k == c.nan_segment:
            assert math.isnan(losses[k]) and ref["count"] == 0
        elif c.zero_loss:
            assert abs(losses[k]) <= CC.LOSS_TOL and ref["loss"] == 0.0
        else:
            assert ref["loss"] >= CC.MIN_LOSS
            worst["loss"] = max(worst["loss"], CC.loss_ratio(losses[k], ref))
        for mode in MODES:
            d = seg["d_" + mode][rows]
            coef = float(np.float32(ups[mode][k].item()) / np.float32(ref["count"])) if ref["count"] else 0.0
            r, ignored = CC.dlogits_ratio(d, CC.reference(lg, lab, coef=coef))
            assert ignored == 0.0
            worst["d_logits"] = max(worst["d_logits"], r)
            if k == c.nan_segment:
                assert not d.any() and not torch.isnan(d).any()        # exactly 0, and the neighbours are untouched (above)
    # mean: the left-to-right fp32 sum over S
    acc = np.float32(losses[0])
    for v in losses[1:]:
        acc = np.float32(acc + np.float32(v))
    want = np.float32(acc / np.float32(c.S))
    got = seg["mean"].cpu().numpy()[0]
    assert (math.isnan(want) and math.isnan(got)) or got == want, (got, want)
    assert math.isnan(want) == (c.nan_segment is not None)
    print(f"CESEG {name}: error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f"; mean {got:.9g}")
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("name", ["mixed5_k21", "sixteen_k33", "no_valid_k4"])
def test_two_runs_agree_and_the_operator_is_the_same_launches(name):
    dev = gpu_device()
    c, seg, _, ups = _runs(name)
    gl, gm = SC.upstream(c.S, seed=len(name))
    again = _segmented_abi(c, dev, gl, gm)
    for k in seg:
        a, b = seg[k], again[k]
        assert torch.equal(a, b) if a.dtype == torch.int32 else bits_equal(a, b), k
    lab = c.labels.to(dev)
    for mode in MODES:
        x = c.logits.to(dev).requires_grad_(True)
        r = spx.segmented_cross_entropy(x, lab, c.offsets)
        assert r.losses.shape == (c.S,) and r.mean.shape == () and r.valid.dtype == r.correct.dtype == r.pred.dtype == torch.int32
        outs, grads = [], []                      # the upstream gradients handed over as they are (a NaN loss times g would poison a sum)
        if mode != "mean":
            outs.append(r.losses)
            grads.append(gl.to(dev))
        if mode != "losses":
            outs.append(r.mean)
            grads.append(gm.to(dev))
        torch.autograd.backward(outs, grads)
        assert bits_equal(r.losses.detach(), seg["losses"]) and bits_equal(r.mean.detach().reshape(1), seg["mean"])
        assert torch.equal(r.valid, seg["valid"]) and torch.equal(r.correct, seg["correct"]) and torch.equal(r.pred, seg["pred"])
        assert bits_equal(x.grad, seg["d_" + mode]), mode


# ---- the module ---------------------------------------------------------------------------------------------------------------
def _packed_forward(dev):
    c = PC.recorded()
    B, S, Cs, P, K = (int(v) for v in c["shape"])

    def init(net):
        net.prototype_vectors.copy_(torch.from_numpy(c["bank"]))
        net.last_layer.weight.copy_(torch.from_numpy(c["head"]))

    net = proto_net(P, K, S, Cs, init=init, device=dev)
    pk = spx.msc_pack([torch.from_numpy(m).to(dev) for m in c["conv"]], "none", torch.bfloat16, with_max=False)
    targets = [PAR.gather_labels(B, h, w, K, seed=60 + k).to(dev) for k, (h, w) in enumerate(pk.layout.grids)]
    return net, pk, targets, K


def test_zero_copy_route_equals_the_concatenating_route():
    dev = gpu_device()
    net, pk, targets, K = _packed_forward(dev)
    ce = spx.SegmentedCrossEntropy(ignore_index=-1)
    w = torch.tensor([1.0, 0.5, 2.0, 0.25], device=dev)
    outs = net.forward_from_conv_features(pk)
    seg_logits = [o[0] for o in outs]
    base = seg_logits[0].spx_packed[0]
    assert tuple(base.shape) == (pk.layout.M, K) and [l.spx_packed[2] for l in seg_logits] == [0, 1, 2, 3]
    assert ce._packed_base(seg_logits) is not None
    base.retain_grad()
    r = ce(seg_logits, targets)
    ((r.losses * w).sum() + r.mean).backward()
    # the concatenating route: the same values as leaves of their own
    leaves = [l.detach().clone().requires_grad_(True) for l in seg_logits]
    assert ce._packed_base(leaves) is None
    r2 = ce(leaves, targets)
    ((r2.losses * w).sum() + r2.mean).backward()
    assert bits_equal(r.losses.detach(), r2.losses.detach()) and bits_equal(r.mean.detach(), r2.mean.detach())
    for a, b in ((r.valid, r2.valid), (r.correct, r2.correct), (r.pred, r2.pred), (r.labels, r2.labels)):
        assert torch.equal(a, b)
    assert bits_equal(base.grad, torch.cat([l.grad.reshape(-1, K) for l in leaves]))
    assert net.prototype_vectors.grad is not None and float(net.prototype_vectors.grad.abs().max()) > 0
    # PixelWiseCrossEntropyLoss per segment: the same loss bits and the same counts
    pw = spx.PixelWiseCrossEntropyLoss(ignore_index=-1, return_correct=True)
    for k, (l, t) in enumerate(zip(leaves, targets)):
        loss, correct = pw(l.detach(), t)
        assert bits_equal(loss, r.losses[k].detach()), k
        assert int(correct.sum()) == int(r.correct[k]) and int(correct.shape[0]) == int(r.valid[k])
    # an ignore_index inside 0..K-1 is mapped to -1, as there
    ce2, pw2 = spx.SegmentedCrossEntropy(ignore_index=2), spx.PixelWiseCrossEntropyLoss(ignore_index=2)
    r3 = ce2(seg_logits, targets)
    for k, (l, t) in enumerate(zip(leaves, targets)):
        assert bits_equal(pw2(l.detach(), t), r3.losses[k].detach()), k
    # an in-place edit of the packed logits voids the zero-copy route (the values are then read from the segments)
    # (on a forward without a graph: autograd itself refuses views of an edited base that carry one)
    with torch.no_grad():
        plain = [o[0] for o in net.forward_from_conv_features(pk)]
        assert ce._packed_base(plain) is not None
        plain[0].spx_packed[0].add_(0)
        assert ce._packed_base(plain) is None
        r4 = ce(plain, targets)
    assert bits_equal(r4.losses, r.losses.detach())
    # a list that is not the whole forward in order takes the concatenating route too
    assert ce._packed_base(seg_logits[:3]) is None and ce._packed_base(seg_logits[::-1]) is None
    # refusals that need a device
    with pytest.raises(spx.SpxError, match="targets\\[1\\]"):
        ce(seg_logits, [targets[0], targets[1][:, :-1], targets[2], targets[3]])
    with pytest.raises(spx.SpxError, match="empty"):
        ce([seg_logits[0], seg_logits[1][:0]], [targets[0], targets[1][:0]])
    with pytest.raises(spx.SpxError, match="fp32"):
        ce([l.double() for l in seg_logits], targets)


def test_inside_capture_step():
    from scaleprotoseg_amd.graphs import capture_step

    dev = gpu_device()
    K, shapes = 5, ((2, 7, 9), (2, 4, 5), (2, 6, 7))
    leaves = [torch.zeros(*s, K, device=dev).requires_grad_(True) for s in shapes]
    gen = torch.Generator().manual_seed(77)
    targets = [torch.randint(0, K + 1, s, generator=gen).to(dev) for s in shapes]
    ce = spx.SegmentedCrossEntropy(ignore_index=-1)
    w = torch.tensor([1.0, 0.5, 2.0], device=dev)
    s = torch.cuda.Stream()

    def step():
        for t in leaves:
            t.grad = None
        r = ce(leaves, targets)
        ((r.losses * w).sum() + r.mean).backward()
        return r.losses.detach(), r.mean.detach(), r.valid, r.correct

    def refill(seed):
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for t in leaves:
                t.copy_(torch.randn(t.shape, generator=g) * 3.0)

    eager = {}
    for seed in (1, 2):
        refill(seed)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            out = step()
        torch.cuda.synchronize()
        eager[seed] = [o.clone() for o in out] + [t.grad.clone() for t in leaves]
        del out
    gc.collect()
    graph, captured = capture_step(step, warmup=1, stream=s)
    for seed in (1, 2):
        refill(seed)
        for o in captured:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got = list(captured) + [t.grad for t in leaves]
        for i, (a, b) in enumerate(zip(got, eager[seed])):
            assert torch.equal(a, b) if a.dtype == torch.int32 else bits_equal(a, b), (seed, i)
    assert int(eager[1][2].sum()) > 0 and not bits_equal(eager[1][0], eager[2][0])
