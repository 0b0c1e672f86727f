"""GPU checks of the multi-scale input fusion (csrc/spx_msc.hip, scaleprotoseg_amd/msc.py, the model hook), at B = 2, C = 5 (a
channel count no vector width divides) on the fixture's five shape sets: odd widths, a 1 x 1 source, a source larger than the
target and the Pascal grids 41 <- {21, 31} and 65 <- {33, 49}.

* forward: every element within the float64 restatement's bound (tests/msc_restatement.py); the index legitimate everywhere,
  equal to the float64 argmax wherever the gap exceeds the bounds, at most 0.1 % of the pixels left out that way; the exact tie
  returns the lowest k, a NaN wins with the first NaN's index;
* sigmoid within 4 . 2^-24 of float64 sigma of the kernel's own "none" output (expf's 2 ulp passed through y (1 - y) <= 1/4, plus
  the add and the divide; inputs within [-12, 12]); the bf16 output is the rounding of the fp32-mode output and bf16 inputs give
  what the same values give as fp32 inputs, bit for bit;
* backward: with the kernel's own index every map's gradient within the restatement's gradient bound (fp32 g without and with
  the sigmoid; the bf16-output case against the float64 formula at the bf16 y); a map that needs no gradient gets none and
  leaves the others unchanged; two runs agree bit for bit;
* eight maps, as many as the kernels' unrolled loops take: forward with the float64 argmax on every pixel, backward with gaps in
  the set of maps that need a gradient;
* memory: ``out``, the index and the gradient buffers inside guard bands, poisoned with NaN, at offsets no vector width
  divides, from a channel slice of a wider tensor: every element inside written, nothing outside;
* the module on the device is ``msc_max`` of its own base outputs; ``fuse_feature_epilogue`` on a small net; one forward +
  backward inside ``graphs.capture_step`` (both launches on the capture's one stream: a linear graph), replayed with new inputs."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import msc_cases as MC
import msc_restatement as MR
from support import Backbone, Guarded, bits_equal, gpu_device, proto_net, release_cached_blocks  # noqa: F401

import scaleprotoseg_amd as spx

U = 2.0 ** -24


def _maps(name, dev, dtype=torch.float32):
    return [torch.from_numpy(m).to(dev).to(dtype) for m in MC.case(name)["maps"]]


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("name", MC.SHAPE_SETS)
def test_forward_values_and_index(name):
    dev = gpu_device()
    y, index = spx.msc_max(_maps(name, dev), return_index=True)
    assert y.dtype == torch.float32 and index.dtype == torch.uint8 and y.is_contiguous() and y.shape == index.shape
    z, idx64, zb, u, b = MC.restated(name)
    got, gi = y.cpu().numpy().astype(np.float64), index.cpu().numpy()
    err = np.abs(got - z)
    print(f"msc_max forward {name}: worst error / bound {np.max(err[zb > 0] / zb[zb > 0]):.3f}")
    assert (err <= zb).all()
    assert gi.max() < len(MC.case(name)["maps"])
    pick = lambda t: np.take_along_axis(t, gi[None].astype(np.int64), 0)[0]
    best = np.take_along_axis(u, idx64[None].astype(np.int64), 0)[0]
    best_b = np.take_along_axis(b, idx64[None].astype(np.int64), 0)[0]
    assert (pick(u) >= best - (pick(b) + best_b)).all()                 # legitimate everywhere
    sure = MR.decided(u, b)
    print(f"msc_max forward {name}: {100.0 * (1.0 - sure.mean()):.4f} % of the pixels undecided in float64")
    assert 1.0 - sure.mean() <= 1e-3
    assert np.array_equal(gi[sure], idx64[sure])


def test_tie_and_nan():
    dev = gpu_device()
    c = MC.case("tie")
    y, index = spx.msc_max(_maps("tie", dev), return_index=True)
    tied = torch.from_numpy(c["maps"][0] == 0.5)
    assert int(tied.sum()) >= 100 and bool((index.cpu()[tied] == 0).all()) and bool((y.cpu()[tied] == 0.5).all())
    assert np.array_equal(index.cpu().numpy(), c["index"])             # map 1 wins exactly where map 0 is below 0.5
    c = MC.case("nan")
    z, idx64 = MC.restated("nan")[:2]
    y, index = spx.msc_max(_maps("nan", dev), return_index=True)
    nan = np.isnan(z)
    assert nan.sum() >= 3 and np.array_equal(np.isnan(y.cpu().numpy()), nan)
    assert np.array_equal(index.cpu().numpy()[nan], idx64[nan]) and np.array_equal(idx64[nan], c["index"][nan])
    ys = spx.msc_max(_maps("nan", dev), activation="sigmoid", dtype=torch.bfloat16)
    assert np.array_equal(torch.isnan(ys).cpu().numpy(), nan)


@pytest.mark.parametrize("name", MC.SHAPE_SETS)
def test_sigmoid_and_bf16(name):
    dev = gpu_device()
    maps = _maps(name, dev)
    assert max(float(m.abs().max()) for m in maps) <= 12.0
    z = spx.msc_max(maps)
    y = spx.msc_max(maps, activation="sigmoid")
    err = np.abs(y.cpu().numpy().astype(np.float64) - MR.sigmoid(z.cpu().numpy()))
    print(f"msc_max sigmoid {name}: worst error {err.max() / U:.2f} x 2^-24 (bound 4)")
    assert err.max() <= 4 * U
    y16 = spx.msc_max(maps, activation="sigmoid", dtype=torch.bfloat16)
    assert y16.dtype == torch.bfloat16 and _same_bits(y16, y.to(torch.bfloat16))
    assert _same_bits(spx.msc_max(maps, dtype=torch.bfloat16), z.to(torch.bfloat16))
    # bf16 inputs: what the same values give as fp32 inputs
    low = [m.to(torch.bfloat16) for m in maps]
    wide = [m.float() for m in low]
    for act in ("none", "sigmoid"):
        a, ia = spx.msc_max(low, activation=act, dtype=torch.float32, return_index=True)
        b_, ib = spx.msc_max(wide, activation=act, return_index=True)
        assert _same_bits(a, b_) and torch.equal(ia, ib)
        assert _same_bits(spx.msc_max(low, activation=act), b_.to(torch.bfloat16))          # the inputs' dtype by default


def _backward(maps, g, activation, dtype, needs=None):
    leaves = [m.clone().requires_grad_(needs is None or needs[k]) for k, m in enumerate(maps)]
    y, index = spx.msc_max(leaves, activation=activation, dtype=dtype, return_index=True)
    y.backward(g.to(y.dtype))
    return y.detach(), index, [l.grad for l in leaves]


@pytest.mark.parametrize("activation,dtype", [("none", torch.float32), ("sigmoid", torch.float32), ("sigmoid", torch.bfloat16)])
@pytest.mark.parametrize("name", MC.SHAPE_SETS)
def test_backward(name, activation, dtype):
    dev = gpu_device()
    c = MC.case(name)
    maps = _maps(name, dev)
    g = torch.from_numpy(c["g"]).to(dev)
    if dtype == torch.bfloat16:
        g = g.to(torch.bfloat16).float()                               # the upstream gradient arrives in the output's dtype
    y, index, grads = _backward(maps, g, activation, dtype)
    y64, g64 = y.float().cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64)
    gprime = g64 * y64 * (1.0 - y64) if activation == "sigmoid" else g64          # at the SAVED y, in its own dtype
    ref, bounds = MR.gradients([m.shape[2:] for m in maps], index.cpu().numpy(), gprime, derivative=activation == "sigmoid")
    for k, (got, want, bound) in enumerate(zip(grads, ref, bounds)):
        assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        worst = np.max(err[bound > 0] / bound[bound > 0]) if (bound > 0).any() else 0.0
        print(f"msc_max backward {name} {activation} {dtype} map {k}: worst error / bound {worst:.3f}")
        assert (err <= bound).all(), k
        assert k == 0 or float(got.abs().max()) > 0 or name == "one_up"
    # two runs agree bit for bit
    _, index2, again = _backward(maps, g, activation, dtype)
    assert torch.equal(index, index2) and all(bits_equal(a, b) for a, b in zip(grads, again))
    # a map that needs no gradient gets none; the others are unchanged
    _, _, part = _backward(maps, g, activation, dtype, needs=(True, False, True))
    assert part[1] is None and bits_equal(part[0], grads[0]) and bits_equal(part[2], grads[2])


def test_eight_maps_forward():
    """As many maps as the kernels' unrolled loops take (tests/msc_cases.py): float64 decides every pixel of this case, so the
    index is the float64 argmax everywhere."""
    dev = gpu_device()
    y, index = spx.msc_max(_maps("eight", dev), return_index=True)
    z, idx64, zb, u, b = MC.restated("eight")
    assert MR.decided(u, b).all()
    err = np.abs(y.cpu().numpy().astype(np.float64) - z)
    print(f"msc_max forward eight: worst error / bound {np.max(err[zb > 0] / zb[zb > 0]):.3f}")
    assert (err <= zb).all()
    assert np.array_equal(index.cpu().numpy(), idx64)


@pytest.mark.parametrize("activation,dtype", [("none", torch.float32), ("sigmoid", torch.bfloat16)])
def test_eight_maps_backward(activation, dtype):
    """``test_backward``'s measure on eight maps, then with ``MC.EIGHT_NEEDS``: empty ranges of the prefix sums at the front, in
    the middle and next to the end."""
    dev = gpu_device()
    maps = _maps("eight", dev)
    g = torch.from_numpy(MC.case("eight")["g"]).to(dev)
    if dtype == torch.bfloat16:
        g = g.to(torch.bfloat16).float()
    y, index, grads = _backward(maps, g, activation, dtype)
    y64, g64 = y.float().cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64)
    gprime = g64 * y64 * (1.0 - y64) if activation == "sigmoid" else g64
    ref, bounds = MR.gradients([m.shape[2:] for m in maps], index.cpu().numpy(), gprime, derivative=activation == "sigmoid")
    for k, (got, want, bound) in enumerate(zip(grads, ref, bounds)):
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        worst = np.max(err[bound > 0] / bound[bound > 0]) if (bound > 0).any() else 0.0
        print(f"msc_max backward eight {activation} {dtype} map {k}: worst error / bound {worst:.3f}")
        assert tuple(got.shape) == want.shape and (err <= bound).all(), k
        assert float(got.abs().max()) > 0
    _, index2, part = _backward(maps, g, activation, dtype, needs=MC.EIGHT_NEEDS)
    assert torch.equal(index, index2)
    for k, need in enumerate(MC.EIGHT_NEEDS):
        assert (bits_equal(part[k], grads[k]) if need else part[k] is None), k


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["odd", "pascal41", "wide"])
def test_single_map(name, dtype):
    """K = 1 (its own kernel: a plane is one row, four channels per step where every group is a whole vector, else element by
    element - C = 5 takes both paths): the activation and the cast alone, from a channel slice, into a guarded ``out``."""
    dev = gpu_device()
    c = MC.case(name)
    m = torch.from_numpy(c["maps"][0]).to(dev)
    B, Cc, H, W = m.shape
    parent = torch.full((B, Cc + 3, H, W), float("nan"), device=dev)
    parent[:, 2:2 + Cc] = m
    view = parent[:, 2:2 + Cc]
    y, index = spx.msc_max([view], return_index=True)
    assert bits_equal(y, m) and index.shape == y.shape and not bool(index.any())
    ys = spx.msc_max([view], activation="sigmoid")
    assert np.abs(ys.cpu().numpy().astype(np.float64) - MR.sigmoid(c["maps"][0])).max() <= 4 * U
    n = m.numel()
    for off in (1, 2, 3):
        og = Guarded((n + 4) * (2 if dtype == torch.bfloat16 else 4), dev)
        body = og.body(dtype)
        body.fill_(float("nan"))
        out = body[off:off + n].view(m.shape)
        spx.msc_max([view], activation="sigmoid", dtype=dtype, out=out)
        assert _same_bits(out, ys.to(dtype)) and og.intact()
        assert bool(torch.isnan(body[:off]).all()) and bool(torch.isnan(body[off + n:]).all())
    low = view.to(torch.bfloat16)
    assert _same_bits(spx.msc_max([low], activation="sigmoid", dtype=torch.float32), spx.msc_max([low.float()], activation="sigmoid"))
    # backward: g y (1 - y) at the saved y
    g = torch.from_numpy(c["g"]).to(dev)
    yk, _, (grad,) = _backward([m], g, "sigmoid", dtype)
    y64, g64 = yk.float().cpu().numpy().astype(np.float64), g.to(dtype).float().cpu().numpy().astype(np.float64)
    want = g64 * y64 * (1.0 - y64)
    assert (np.abs(grad.cpu().numpy() - want) <= 3 * U * np.abs(want)).all()


def test_bf16_maps_get_bf16_gradients():
    dev = gpu_device()
    c = MC.case("odd")
    maps = _maps("odd", dev, torch.bfloat16)
    g = torch.from_numpy(c["g"]).to(dev)
    y, index, grads = _backward(maps, g, "sigmoid", torch.float32)
    _, index32, wide = _backward([m.float() for m in maps], g, "sigmoid", torch.float32)
    assert torch.equal(index, index32)
    for a, b in zip(grads, wide):
        assert a.dtype == torch.bfloat16 and _same_bits(a, b.to(torch.bfloat16))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["odd", "one_up", "pascal41"])
def test_memory_hygiene(name, dtype):
    """Channel-slice inputs with non-trivial batch and channel strides, every output inside guard bands at an element offset
    that no vector width divides, poisoned with NaN."""
    from scaleprotoseg_amd import _lib

    dev = gpu_device()
    lib = _lib.load()
    c = MC.case(name)
    esz = 2 if dtype == torch.bfloat16 else 4
    dense = _maps(name, dev, dtype)
    maps = []
    for k, m in enumerate(dense):                 # planes 1 + 2 c of a [B + 1, 2 C + 3] parent, batches 1..: strides of their own
        B, Cc, h, w = m.shape
        parent = torch.full((B + 1, 2 * Cc + 3, h, w), float("nan"), dtype=dtype, device=dev)
        view = parent[1:, 1:1 + 2 * Cc:2]
        view.copy_(m)
        assert view.stride(0) != Cc * h * w and view.stride(1) != h * w
        maps.append(view)
    B, Cc, H, W = maps[0].shape
    n = B * Cc * H * W
    want, want_index = spx.msc_max(dense, activation="sigmoid", return_index=True)

    # forward through the public call, out= one element into a guarded buffer
    og = Guarded((n + 2) * esz, dev)
    body = og.body(dtype)
    body.fill_(float("nan"))
    out = body[1:1 + n].view(B, Cc, H, W)
    got = spx.msc_max(maps, activation="sigmoid", out=out)
    assert got.data_ptr() == out.data_ptr() and _same_bits(out, want)
    assert og.intact() and bool(torch.isnan(body[0])) and bool(torch.isnan(body[n + 1]))

    # forward with the index and backward through the C entry points, every buffer guarded at an odd element offset
    ig = Guarded(n + 6, dev)
    ig.body(torch.uint8).fill_(0xEE)
    g = torch.from_numpy(c["g"]).to(dev).to(dtype)
    bufs = [Guarded((m.numel() + 2) * esz, dev) for m in maps]
    for bg in bufs:
        bg.body(dtype).fill_(float("nan"))
    a = _lib.SpxMsc()
    a.K, a.B, a.C = len(maps), B, Cc
    a.in_dtype = a.out_dtype = a.g_dtype = 0 if dtype == torch.bfloat16 else 1
    a.activation = 1
    for k, m in enumerate(maps):
        d = a.maps[k]
        d.data, d.batch_stride, d.channel_stride, d.h, d.w = m.data_ptr(), m.stride(0), m.stride(1), m.shape[2], m.shape[3]
        a.grads[k] = bufs[k].ptr + esz
    body.fill_(float("nan"))
    a.out, a.index, a.g = og.ptr + esz, ig.ptr + 3, g.data_ptr()
    _lib.check(lib.spx_msc_max_fwd(C.byref(a), _lib.stream_ptr()))
    _lib.check(lib.spx_msc_max_bwd(C.byref(a), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert og.intact() and ig.intact() and all(bg.intact() for bg in bufs)
    assert _same_bits(out, want) and bool(torch.isnan(body[0])) and bool(torch.isnan(body[n + 1]))
    ib = ig.body(torch.uint8)
    assert torch.equal(ib[3:3 + n].view(B, Cc, H, W), want_index) and bool((ib[:3] == 0xEE).all()) and bool((ib[3 + n:] == 0xEE).all())
    _, _, ref = _backward(dense, g, "sigmoid", dtype)
    for k, (bg, m) in enumerate(zip(bufs, maps)):
        gb = bg.body(dtype)
        inner = gb[1:1 + m.numel()].view(m.shape)
        assert not bool(torch.isnan(inner).any()) and _same_bits(inner, ref[k]), k        # every element inside is written
        assert bool(torch.isnan(gb[0])) and bool(torch.isnan(gb[1 + m.numel()]))


class _Recorder(torch.nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner = inner
        self.seen = []

    def forward(self, x):
        out = self.inner(x)
        self.seen.append(out)
        return out


def test_module_on_the_device():
    dev = gpu_device()
    torch.manual_seed(3)
    base = _Recorder(Backbone(16, "pool", stride=2)).to(dev)
    msc = spx.MSC(base)
    x = torch.randn(2, 3, 26, 34, device=dev)
    with torch.no_grad():
        for training in (False, True):
            msc.train(training)
            base.seen.clear()
            out = msc(x)
            outs = list(base.seen)
            assert [tuple(t.shape[2:]) for t in outs] == [(13, 17), (6, 8), (9, 12)]
            want = spx.msc_max(outs)
            base.seen.clear()
            fused = msc.fused(x, "sigmoid", torch.bfloat16)
            want16 = spx.msc_max(outs, activation="sigmoid", dtype=torch.bfloat16)
            if training:
                assert isinstance(out, list) and len(out) == 4 and all(a is b for a, b in zip(out[:3], outs))
                assert bits_equal(out[3], want)
                assert len(fused) == 4 and _same_bits(fused[3], want16)
                for f, o in zip(fused[:3], outs):
                    assert _same_bits(f, spx.msc_max([o], "sigmoid", torch.bfloat16))
            else:
                assert bits_equal(out, want) and _same_bits(fused, want16)
    # the gradient reaches the base's parameters through every scale
    msc.train(False)
    msc(x).square().sum().backward()
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in base.inner.base.parameters())


def test_fused_feature_epilogue_on_a_small_net():
    dev = gpu_device()
    net = proto_net(40, 5, 4, 16, seed=11, device=dev, backbone="pool", stride=2)
    net.features = spx.MSC(net.features)
    net.eval()
    x = torch.randn(2, 3, 26, 34, device=dev)
    with torch.no_grad():
        before = net.forward(x)
        net.fuse_feature_epilogue(torch.bfloat16)
        logits, dist = net.forward(x)
        feats = net.conv_features(x)
        feats32 = net.features.fused(x, "sigmoid", torch.float32)
        assert feats.dtype == torch.bfloat16 and _same_bits(feats, net.features.fused(x, "sigmoid", torch.bfloat16))
        assert _same_bits(feats, feats32.to(torch.bfloat16))
        l2, d2 = net.forward_from_conv_features(feats)
        assert bits_equal(logits, l2) and bits_equal(dist, d2)
        # the distance kernel rounds fp32 features to bf16 once, to nearest even, and uses the rounded value
        l3, d3 = net.forward_from_conv_features(feats32)
        assert bits_equal(dist, d3) and bits_equal(logits, l3)
        pf, pd = net.push_forward(x)
        assert _same_bits(pf, feats) and bits_equal(pd, net.prototype_distances(x))
        net.fuse_feature_epilogue(None)
        after = net.forward(x)
        assert bits_equal(after[0], before[0]) and bits_equal(after[1], before[1])
        assert net.conv_features(x).dtype == torch.float32


def test_capture_forward_and_backward():
    from scaleprotoseg_amd.graphs import capture_step

    dev = gpu_device()
    c = MC.case("odd")
    leaves = [m.requires_grad_(True) for m in _maps("odd", dev)]
    gout = torch.from_numpy(c["g"]).to(dev)
    s = torch.cuda.Stream()

    def step():
        for t in leaves:
            t.grad = None
        out = spx.msc_max(leaves, activation="sigmoid", dtype=torch.bfloat16)
        out.backward(gout.to(torch.bfloat16))
        return out.detach()

    def refill(seed):
        gen = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for t in leaves:
                t.copy_(torch.randn(t.shape, generator=gen))

    eager = {}
    for seed in (1, 2):
        refill(seed)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):         # eager reference on the capture's side stream
            out = step()
        torch.cuda.synchronize()
        eager[seed] = [out.clone()] + [t.grad.clone() for t in leaves]
        del out
    gc.collect()
    graph, captured = capture_step(step, warmup=1, stream=s)
    for seed in (1, 2):
        refill(seed)
        captured.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for what, a, b in zip(("out", "d0", "d1", "d2"), [captured] + [t.grad for t in leaves], eager[seed]):
            assert _same_bits(a, b), (seed, what)
