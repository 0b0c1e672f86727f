"""GPU checks of the cross-scale aggregation (csrc/spx_scale_agg.hip, functional.scale_aggregate, scale_head.WeightedAgg and the
scale_head_type of both PPNetMultiScale classes).

The op is held to float64 on the same fp32 inputs (tests/scale_head_restatement.py):
  forward   |out - out64| <= |d out / d s| E_s + 2^-22 |out64|,
            E_s = sum_p |p_pc| 2^-21 (1 + |a_p|) + (Pn + 2) 2^-24 sum_p |p_pc a_p|
            (first term: act_log's one-ulp reciprocal and logarithm - the claim of csrc/spx_common.h - with a factor 2 of headroom;
            second: the fp32 accumulation chain of the fp32-input MFMA).  The worst error-to-bound ratio is printed per case.
  backward  grad_close (GRAD_TOL; dx of bf16 x: BF16_DX_TOL) against float64 autograd; dproto of two runs is bit-identical.
The modules are held link by link (tests/test_scale_head_cpu.py says why): every chained scale's distances to the oracle at
(bf16(x'), bf16(p)) with x' from the public op on the module's own distances of the scale above, the last scale to the
reference-recorded fixture; gradients to the composed restatement (scale_head_restatement.chain_gradients)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

import offgrid_restatement as R
import scale_head_restatement as SH
from parity_cases import assert_fwd
from support import (BF16_DX_TOL, EPS, GRAD_TOL, HERE, Guarded, ListData, bits_equal, gpu_device, grad_close, group_net, proto_net,
                     release_cached_blocks)  # noqa: F401

GOLDEN = os.path.join(HERE, "golden")

# id -> (B, Cs, Pn, H, W, channels of the tensor x is a slice of, first channel of the slice)
OP_SHAPES = {
    "G1": (2, 16, 8, 5, 7, 16, 0),
    "A2-13": (1, 64, 13, 9, 13, 64, 0),          # scale ranges (0,7),(7,20),(20,21): the aggregated scales have 13 and 1 rows
    "A2-1": (1, 64, 1, 9, 13, 64, 0),            # Pn = 1: the k tail of the MFMA alone
    "A3": (2, 48, 190, 33, 33, 144, 48),         # Cs % 32 = 16, several panels, ragged last pixel tile, x a slice of 3 scales
    "A4": (1, 256, 200, 8, 8, 256, 0),           # four channel chunks, half a pixel tile
}
MODES = ("none", "sum", "mult")
SOURCES = ("log", "linear", "activations")
KIND = {"activations": 0, "log": 1, "linear": 2}
DTYPES = (torch.float32, torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _inputs(shape, mode, source, dtype):
    """CPU inputs: x values (bf16-representable when ``dtype`` is bf16) inside their parent tensor, the fp32 source, the bank.
    x . s > 0 in mode "mult" (the region the formula is defined on): the bank is negative under the linear similarity."""
    B, Cs, Pn, H, W, Cp, c0 = OP_SHAPES[shape]
    g = torch.Generator().manual_seed(1000 * len(shape) + 10 * MODES.index(mode) + SOURCES.index(source) + B * Cs + Pn)
    parent = torch.sigmoid(torch.randn(B, Cp, H, W, generator=g))
    if dtype == torch.bfloat16:
        parent = R.bf16_rne(parent)
    src = torch.rand(B, Pn, H, W, generator=g) * (5.0 if source == "activations" else 4.0)
    if source == "log":
        src[0, 0, 0, 0] = 0.0                                                  # the largest activation: log(1 / eps) = 9.2
    proto = torch.rand(Pn, Cs, generator=g)
    if source == "linear" and mode == "mult":
        proto = -proto
    gout = torch.randn(B, Cs, H, W, generator=g)
    return parent, src, proto, gout


def _kwargs(source):
    return dict(source_kind="activations") if source == "activations" else dict(source_kind="distances", activation=source)


def _reference(shape, mode, source, dtype, grads=False):
    B, Cs, Pn, H, W, Cp, c0 = OP_SHAPES[shape]
    parent, src, proto, gout = _inputs(shape, mode, source, dtype)
    x = parent[:, c0:c0 + Cs].double().requires_grad_(grads)
    s64, p64 = src.double().requires_grad_(grads), proto.double().requires_grad_(grads)
    out = SH.aggregate(x, s64, p64, mode, eps=EPS, **_kwargs(source))
    if not grads:
        return x, s64, p64, out
    out.backward(gout.double())
    return (x.grad if mode != "none" else None), s64.grad, p64.grad


def _device_inputs(shape, mode, source, dtype, dev, grads=False):
    B, Cs, Pn, H, W, Cp, c0 = OP_SHAPES[shape]
    parent, src, proto, gout = _inputs(shape, mode, source, dtype)
    parent = parent.to(dev).to(dtype)
    if grads:
        parent.requires_grad_(True)
    x = parent[:, c0:c0 + Cs]
    return parent, x, src.to(dev).requires_grad_(grads), proto.to(dev).requires_grad_(grads), gout.to(dev)


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", list(OP_SHAPES))
def test_op_forward(shape, mode, source, dtype):
    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd import _lib

    dev = gpu_device()
    B, Cs, Pn, H, W, Cp, c0 = OP_SHAPES[shape]
    parent, x, src, proto, _ = _device_inputs(shape, mode, source, dtype, dev)
    assert Cp == Cs or not x.is_contiguous()
    # the C entry point on a guarded output
    lib = _lib.load()
    out_g = Guarded(B * Cs * H * W * 4, dev)
    _lib.check(lib.spx_scale_agg_fwd(x.data_ptr(), 0 if dtype == torch.bfloat16 else 1, x.stride(0), src.data_ptr(), KIND[source],
                                     proto.data_ptr(), out_g.ptr, B, Cs, Pn, H * W, MODES.index(mode), EPS, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert out_g.intact(), "write outside the output"
    out = out_g.body(torch.float32).reshape(B, Cs, H, W).clone()
    # the public op: the same bits, x read in place
    pub = spx.scale_aggregate(x, src, proto, mode=mode, epsilon=EPS, **_kwargs(source))
    assert pub.shape == (B, Cs, H, W) and pub.dtype == torch.float32 and pub.is_contiguous()
    assert bits_equal(pub, out)

    x64, s64, p64, out64 = _reference(shape, mode, source, dtype)
    a64 = SH.similarity(s64, source, EPS) if source != "activations" else s64
    E_s = SH.s_error_bound(a64, p64)
    bound = SH.out_error_bound(mode, x64, SH.weighted_sum(a64, p64), out64, E_s)
    err = (out.double().cpu() - out64).abs()
    assert torch.isfinite(out).all()
    ratio = (err / bound).max().item()
    print(f"scale_aggregate forward {shape} {mode} {source} {dtype}: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0, f"error exceeds the derived bound: worst ratio {ratio:.3f}"


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", list(OP_SHAPES))
def test_op_backward(shape, mode, source, dtype):
    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd import _lib

    dev = gpu_device()
    B, Cs, Pn, H, W, Cp, c0 = OP_SHAPES[shape]
    parent, x, src, proto, gout = _device_inputs(shape, mode, source, dtype, dev, grads=True)
    runs = []
    for _ in range(2):
        out = spx.scale_aggregate(x, src, proto, mode=mode, epsilon=EPS, **_kwargs(source))
        runs.append(torch.autograd.grad(out, (parent, src, proto), gout, allow_unused=True))
    dpar, dsrc, dproto = runs[0]
    assert bits_equal(dproto, runs[1][2]), "dproto differs between two runs"
    assert bits_equal(dsrc, runs[1][1])
    rx, rs, rp = _reference(shape, mode, source, dtype, grads=True)
    grad_close(dsrc, rs, "d source")
    grad_close(dproto, rp, "d proto")
    if mode == "none":
        assert dpar is None
    else:
        assert dpar.dtype == dtype
        grad_close(dpar[:, c0:c0 + Cs], rx, "d x", tol=BF16_DX_TOL if dtype == torch.bfloat16 else GRAD_TOL)
        if Cp != Cs:
            assert not dpar[:, :c0].any() and not dpar[:, c0 + Cs:].any()

    # the C entry point on guarded outputs: nothing outside them, the bits of the public op
    lib = _lib.load()
    esz = 2 if dtype == torch.bfloat16 else 4
    n = B * H * W
    bufs = dict(dx=Guarded(n * Cs * esz, dev), dsrc=Guarded(n * Pn * 4, dev), dproto=Guarded(Pn * Cs * 4, dev),
                ws=Guarded(lib.spx_scale_agg_workspace_bytes(B, Cs, Pn, H * W), dev))
    xd = x.detach()
    _lib.check(lib.spx_scale_agg_bwd(xd.data_ptr(), 0 if dtype == torch.bfloat16 else 1, xd.stride(0), src.data_ptr(), KIND[source],
                                     proto.data_ptr(), gout.data_ptr(), bufs["dx"].ptr if mode != "none" else None, bufs["dsrc"].ptr,
                                     bufs["dproto"].ptr, bufs["ws"].ptr, B, Cs, Pn, H * W, MODES.index(mode), EPS, _lib.stream_ptr()))
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert b.intact(), f"write outside {k}"
    assert bits_equal(bufs["dsrc"].body(torch.float32).reshape(dsrc.shape), dsrc)
    assert bits_equal(bufs["dproto"].body(torch.float32).reshape(dproto.shape), dproto)
    if mode != "none":
        assert torch.equal(bufs["dx"].body(dtype).reshape(B, Cs, H, W), dpar[:, c0:c0 + Cs])


def test_memory_is_outputs_plus_workspace():
    """One forward + backward at A3 allocates the returned tensors and the declared workspace, nothing of size B Pn Cs HW."""
    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd import _lib

    dev = gpu_device()
    shape, mode, source = "A3", "mult", "log"
    B, Cs, Pn, H, W, Cp, c0 = OP_SHAPES[shape]
    parent, x, src, proto, gout = _device_inputs(shape, mode, source, torch.float32, dev, grads=True)
    spx.scale_aggregate(x, src, proto, mode=mode, epsilon=EPS, **_kwargs(source))          # library loaded, kernels resident
    up = lambda nbytes: -(-int(nbytes) // 512) * 512
    n = B * H * W
    allowed = (up(n * Cs * 4)            # out
               + up(n * Cs * 4)          # dx
               + up(n * Pn * 4)          # dsource
               + up(Pn * Cs * 4)         # dproto
               + up(_lib.load().spx_scale_agg_workspace_bytes(B, Cs, Pn, H * W)))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = spx.scale_aggregate(x, src, proto, mode=mode, epsilon=EPS, **_kwargs(source))
    dx, dsrc, dproto = torch.autograd.grad(out, (x, src, proto), gout)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"scale_aggregate A3 forward + backward: peak rise {rise} bytes, allowed {allowed}; the broadcast product would be "
          f"{n * Pn * Cs * 4}")
    assert rise <= allowed
    assert allowed < n * Pn * Cs * 4


def test_op_refusals():
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    x, src, p = torch.rand(1, 16, 3, 3, device=dev), torch.rand(1, 5, 3, 3, device=dev), torch.rand(5, 16, device=dev)
    ok = spx.scale_aggregate(x, src, p, mode="sum")
    assert ok.shape == (1, 16, 3, 3)
    bad = [
        (dict(x=x.cpu()), "no CPU fallback"), (dict(source=src.cpu()), "no CPU fallback"), (dict(prototypes=p.cpu()), "no CPU fallback"),
        (dict(x=x[:, :8]), "x must be"), (dict(source=src[0]), "source must be"), (dict(source=src.double()), "source must be"),
        (dict(prototypes=p[:4]), "rows"), (dict(source=src[:, :0], prototypes=p[:0]), "empty scale"),
        (dict(x=torch.rand(1, 24, 3, 3, device=dev), prototypes=torch.rand(5, 24, device=dev)), "multiple of 16"),
        (dict(mode="max"), "unknown mode"), (dict(x=None), "combines with x"), (dict(x=x.half()), "bfloat16 or float32"),
    ]
    for change, msg in bad:
        kw = dict(x=x, source=src, prototypes=p, mode="sum")
        kw.update(change)
        with pytest.raises(spx.SpxError, match=msg):
            spx.scale_aggregate(kw.pop("x"), kw.pop("source"), kw.pop("prototypes"), **kw)


def test_weighted_agg_drop_in():
    """WeightedAgg.forward(x, activations, prototypes) with the reference's shapes, all three types; Pn = 1 works (the reference's
    squeeze(dim=0) drops the prototype axis there)."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    g = torch.Generator().manual_seed(5)
    for Pn in (6, 1):
        x = torch.sigmoid(torch.randn(2, 16, 5, 7, generator=g))
        act = torch.rand(2, Pn, 5, 7, generator=g) * 5
        protos = torch.rand(Pn, 16, 1, 1, generator=g)
        for head in SH.HEADS:
            torch.manual_seed(7)
            agg = spx.WeightedAgg(output_type=head, channel_dim=16).to(dev)
            out = agg(x.to(dev), act.to(dev), protos.to(dev))
            lin = None
            if head == "concat":
                l0 = agg.output_layer.linear_block[0]
                lin = (l0.weight.detach().double().cpu(), l0.bias.detach().double().cpu())
            ref = SH.aggregate(x.double(), act.double(), protos.double(), head, source_kind="activations", linear=lin)
            assert out.shape == ref.shape
            assert (out.double().cpu() - ref).abs().max().item() <= 2e-6 * (1 + ref.abs().max().item()), (head, Pn)


# ---- the modules, link by link ---------------------------------------------------------------------------------------------
def _module(fx, head, phase, dev):
    import scaleprotoseg_amd as spx

    d = fx["dims"]
    net = (proto_net(d.P, d.K, d.S, d.Cs, scale_head_type=head) if phase == "proto"
           else group_net(d.P, d.K, d.S, d.Cs, d.G, scale_head_type=head))
    spx.load_reference_state_dict(net, {k: fx["sd." + k] for k in fx["state_keys"]})
    spx.functional.invalidate_pack_cache()
    return net.to(dev)


def _device_x_primes(net, conv, dist, fx):
    """x' of every chained scale from the public op on the module's own distances of the scale above (fp32, on the CPU)."""
    d = fx["dims"]
    out = {}
    with torch.no_grad():
        for i in range(d.S - 1):
            lo1, hi1 = fx["ranges"][i + 1]
            xs = conv.detach()[:, i * d.Cs:(i + 1) * d.Cs]
            xp = net.scale_head.from_distances(xs, dist.detach()[:, lo1:hi1].contiguous(), net.prototype_vectors[lo1:hi1], "log", net.epsilon)
            out[i] = xp.float().cpu()
    return out


@pytest.mark.parametrize("phase", SH.PHASES)
@pytest.mark.parametrize("head", SH.HEADS)
@pytest.mark.parametrize("gid", ("G1", "G2"))
def test_module_link_by_link(gid, head, phase):
    dev = gpu_device()
    fx = SH.fixture(gid, head, phase, GOLDEN)
    d = fx["dims"]
    net = _module(fx, head, phase, dev)
    conv = fx["conv"].to(dev).requires_grad_(True)
    logits, dist, act = net.forward_from_conv_features(conv, return_activations=True, return_distances=True)
    assert logits.shape == (d.B, d.H, d.W, d.K) and dist.shape == (d.B, d.P, d.H, d.W) and act.shape == (d.B * d.H * d.W, d.P)
    xps = _device_x_primes(net, conv, dist, fx)
    bank = fx["sd.prototype_vectors"]
    rdist, _ = SH.chain(fx["conv"], bank, fx["ranges"], d.S, head, linear=fx["linear"], rounding=R.bf16_rne, x_primes=xps)
    got = dist.detach().double().cpu()
    for s in range(d.S):
        lo, hi = fx["ranges"][s]
        ref = fx["distances"][:, lo:hi].double() if s == d.S - 1 else rdist[:, lo:hi]
        ratio = R.distance_ratio(got[:, lo:hi], ref)
        print(f"{gid} {head} {phase} scale {s}: worst |d - ref| / (1e-4 (1 + d)) = {ratio:.3f}"
              + (" (fixture)" if s == d.S - 1 else " (oracle at bf16(x'), bf16(p))"))
        assert ratio <= 1.0, f"scale {s}"
    params = SH.head_params(fx, phase)
    _, rlogits, ract = SH.head_loss(fx, phase, rdist, params)
    assert_fwd(logits.detach(), None, act.detach(), rlogits.detach().float(), None, ract.detach().float())

    # gradients of the fixture's loss against the composed restatement at the device's x'
    loss = (logits * fx["g_logits"].to(dev)).sum() + (dist * fx["g_dist"].to(dev)).sum() + (act * fx["g_act"].to(dev)).sum()
    net.zero_grad()
    loss.backward()
    leaves = SH.head_params(fx, phase)
    ref = SH.chain_gradients(fx["conv"], bank, fx["ranges"], d.S, head, lambda dd: SH.head_loss(fx, phase, dd, leaves)[0],
                             linear=fx["linear"], x_primes=xps)
    tag = f"{gid} {head} {phase}"
    grad_close(conv.grad, ref.conv, "d conv", report=tag)
    grad_close(net.prototype_vectors.grad, ref.bank, "d prototype_vectors", report=tag)
    if phase == "proto":
        grad_close(net.last_layer.weight.grad, leaves["last_layer.weight"].grad, "d last_layer", report=tag)
    else:
        grad_close(net.last_layer_group.weight.grad, leaves["last_layer_group.weight"].grad, "d last_layer_group", report=tag)
        for j, gp in enumerate(net.group_projection):
            grad_close(gp.weight.grad, leaves[f"group_projection.{j}.weight"].grad, f"d group_projection.{j}", report=tag)
    if head == "concat":
        l0 = net.scale_head.output_layer.linear_block[0]
        grad_close(l0.weight.grad, ref.linear[0], "d concat weight", report=tag)
        grad_close(l0.bias.grad, ref.linear[1], "d concat bias", report=tag)


@pytest.mark.parametrize("phase", SH.PHASES)
def test_tuple_modes_and_list_recursion(phase):
    dev = gpu_device()
    fx = SH.fixture("G1", "sum", phase, GOLDEN)
    d = fx["dims"]
    net = _module(fx, "sum", phase, dev)
    conv = fx["conv"].to(dev)
    with torch.no_grad():
        o_default = net.forward_from_conv_features(conv)
        o_act = net.forward_from_conv_features(conv, return_activations=True)
        o_both = net.forward_from_conv_features(conv, return_activations=True, return_distances=True)
        o_list = net.forward_from_conv_features([conv, conv[..., ::2, ::2].contiguous()])
        pd = net._scale_l2_convolution(conv)
    assert len(o_default) == 2 and len(o_act) == 2 and len(o_both) == 3
    M = d.B * d.H * d.W
    assert o_default[0].shape == (d.B, d.H, d.W, d.K) and o_default[1].shape == (d.B, d.P, d.H, d.W)
    assert o_act[1].shape == (M, d.P) and o_both[1].shape == (d.B, d.P, d.H, d.W) and o_both[2].shape == (M, d.P)
    assert bits_equal(o_default[1], o_both[1]) and bits_equal(o_act[1], o_both[2]) and bits_equal(pd, o_both[1])
    assert isinstance(o_list, list) and len(o_list) == 2 and all(len(o) == 2 for o in o_list)
    assert o_list[1][1].shape == (d.B, d.P, (d.H + 1) // 2, (d.W + 1) // 2)
    assert bits_equal(o_list[0][1], o_both[1])


def test_callable_similarity_runs_the_chain():
    """A user-supplied similarity under a scale head: the chain hands the kernel ready activations."""
    dev = gpu_device()
    fx = SH.fixture("G1", "mult", "proto", GOLDEN)
    d = fx["dims"]
    net = _module(fx, "mult", "proto", dev)
    conv = fx["conv"].to(dev)
    with torch.no_grad():
        ref = net._scale_l2_convolution(conv)
        net.prototype_activation_function = lambda dist: torch.log((dist + 1) / (dist + net.epsilon))
        got = net._scale_l2_convolution(conv)
    assert R.distance_ratio(got.cpu(), ref.cpu()) <= 1.0


def test_capture_replays_eager_bit_for_bit():
    import gc

    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd.graphs import capture_step

    dev = gpu_device()
    shape, mode, source = "G1", "mult", "log"
    B, Cs, Pn, H, W, Cp, c0 = OP_SHAPES[shape]
    parent, _, src, proto, gout = _device_inputs(shape, mode, source, torch.float32, dev)
    leaves = (parent, src, proto)
    for t in leaves:
        t.requires_grad_(True)
    s = torch.cuda.Stream()

    def step():
        # every node of the autograd graph - the slice of x included - is made inside the step, on the stream it runs on: a
        # graph made eagerly on the default stream and still alive would pull that stream into the capture (graphs.py)
        for t in leaves:
            t.grad = None
        out = spx.scale_aggregate(parent[:, c0:c0 + Cs], src, proto, mode=mode, epsilon=EPS, **_kwargs(source))
        out.backward(gout)
        return out.detach()

    with torch.cuda.stream(s):             # eager reference on the capture's side stream
        step()
        out = step()
    torch.cuda.synchronize()
    eager = [out.clone()] + [t.grad.clone() for t in leaves]
    del out
    gc.collect()
    graph, captured = capture_step(step, warmup=1, stream=s)
    captured.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for what, a, b in zip(("out", "dx", "dsource", "dproto"), [captured] + [t.grad for t in leaves], eager):
        assert bits_equal(a, b), what


def test_refusals_of_the_fused_paths():
    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd import push as push_mod

    dev = gpu_device()
    for phase in SH.PHASES:
        fx = SH.fixture("G1", "sum", phase, GOLDEN)
        d = fx["dims"]
        net = _module(fx, "sum", phase, dev)
        net.add_on_layers = nn.Identity()
        conv = fx["conv"].to(dev)
        lab = torch.ones(d.B, d.H, d.W, dtype=torch.long, device=dev)
        with pytest.raises(spx.SpxError, match="scale_head"):
            net.forward_from_conv_features(conv, ce_target=lab)
        if phase == "proto":
            with pytest.raises(spx.SpxError, match="scale_head"):
                net.forward_from_conv_features(conv, target_labels=lab)
        assert net.push_min_from_conv(conv, lambda hw: lab, void_class=0) is None
        with torch.no_grad():
            pconv, pdist = net.push_forward(conv)
            assert bits_equal(pconv, conv) and bits_equal(pdist, net._scale_l2_convolution(conv))
            assert bits_equal(net.prototype_distances(conv), pdist)
        data = ListData([(fx["conv"][0], np.ones((8 * d.H, 8 * d.W), np.int64))])
        with pytest.raises(spx.SpxError, match="scale_head"):
            push_mod.push_prototypes_multiscale(data, net, None, log=lambda *_: None, batch_size=2)
        with pytest.raises(spx.SpxError, match="scale_head"):
            spx.push_single_pass(data, net, batch_size=1)
        with pytest.raises(spx.SpxError, match="scale_head"):
            spx.nearest_images_to_prototypes(data, net, n=1)
        with pytest.raises(spx.SpxError, match="scale_head"):
            spx.find_k_nearest_patches_to_prototypes(data, net, k=1)


def test_two_pass_push_reduces_the_written_map():
    """The default push under a scale head: push_min_distances declines, compute_distances reduces the chain's map."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    fx = SH.fixture("G1", "sum", "proto", GOLDEN)
    d = fx["dims"]
    net = _module(fx, "sum", "proto", dev)
    net.add_on_layers = nn.Identity()
    g = torch.Generator().manual_seed(11)
    target = torch.randint(0, d.K + 1, (d.H, d.W), generator=g).repeat_interleave(8, 0).repeat_interleave(8, 1).numpy().astype(np.int64)
    img = fx["conv"][0]
    idx, val = spx.compute_distances(net, ListData(), img, target, d.K, void_class=0)
    with torch.no_grad():
        dist = net._scale_l2_convolution(img[None].to(dev))
    lab = spx.resize_label(target, (d.W, d.H)).unsqueeze(0)
    ridx, rval = spx.push_masked_argmin(dist, lab, net.prototype_class_identity, void_class=0)
    assert torch.equal(idx.cpu(), ridx.cpu()) and bits_equal(val, rval)
