"""GPU checks of the packed training maps (csrc/spx_msc.hip: spx_msc_pack_fwd / _bwd; scaleprotoseg_amd/msc.py; the model's packed
path), on the recorded MSC cases at B = 2, C = 5 (tests/msc_cases.py) and on the reference's recorded training forward
(tests/golden/msc_packed_forward.npz):

1. values: every segment view bit-equal to what ``msc_max`` returns for that segment (``[m]`` for the plain ones, all maps for
   the maximum), the index too; every segment within the float64 bounds of tests/test_gpu_msc.py; ``with_max=False``; K = 1;
2. backward: every gradient within the bound of tests/msc_pack_cases.py; bf16 maps get bf16 gradients; two runs bit-identical;
   a map that needs no gradient gets no buffer; 1. and 2. on eight maps too (nine segments, gaps in the set of gradients);
3. the distance path on the packed axis against the fixture / the oracle (``parity_cases.close_fwd``, ``grad_close``) in the
   three tuple modes, with a loss that weights the segments differently; bit-equality with the list path is measured and
   printed (distances and activations: asserted, as the MI355X run showed it; logits: reported only - they were bit-equal on
   these shapes too, but the list path may take the scale-parallel launch on a small grid, which sums in another order);
4. ``target_labels=`` as a list: ``ClassDistances`` per segment, ``KLDLoss``, gradients, the fast path per segment;
5. the module: ``fuse_feature_epilogue(dtype, packed=True)`` in training, eval / ``packed=False`` / ``None`` unchanged, refusals;
6. pack + distance forward + backward + pack backward inside ``graphs.capture_step``;
7. memory hygiene: guarded buffers at odd offsets, nothing allocated beyond the outputs."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import msc_cases as MC
import msc_pack_cases as PC
import msc_restatement as MR
import parity_cases as PAR
from oracle import ppnet_oracle as O
from support import GRAD_TOL, Guarded, bits_equal, gpu_device, grad_close, proto_net, release_cached_blocks  # noqa: F401

import scaleprotoseg_amd as spx
from scaleprotoseg_amd import _gathered

U = 2.0 ** -24
MODES = (dict(), dict(return_activations=True), dict(return_activations=True, return_distances=True))


def _maps(name, dev, dtype=torch.float32):
    return [torch.from_numpy(m).to(dev).to(dtype) for m in MC.case(name)["maps"]]


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- 1. values -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("activation", ["none", "sigmoid"])
@pytest.mark.parametrize("in_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", PC.CASES)
def test_pack_is_msc_max_per_segment(name, in_dtype, activation, out_dtype):
    dev = gpu_device()
    maps = _maps(name, dev, in_dtype)
    pk = spx.msc_pack(maps, activation=activation, dtype=out_dtype)
    lay = PC.layout(name)
    B, Cc = maps[0].shape[:2]
    assert tuple(pk.features.shape) == (1, Cc, 1, lay.M) and pk.features.is_contiguous() and pk.features.dtype == out_dtype
    assert pk.segments == lay.segments and pk.index.dtype == torch.uint8 and pk.index.shape == maps[0].shape
    views = pk.views()
    assert [v.stride() for v in views] == [lay.view_strides(k) for k in range(len(lay))]
    for k, m in enumerate(maps):
        assert _same_bits(views[k], spx.msc_max([m], activation=activation, dtype=out_dtype)), k
    want, index = spx.msc_max(maps, activation=activation, dtype=out_dtype, return_index=True)
    assert _same_bits(views[-1], want) and torch.equal(pk.index, index)
    # the ragged form: the same plain segments, no maximum, no index
    rg = spx.msc_pack(maps, activation=activation, dtype=out_dtype, with_max=False)
    assert rg.index is None and rg.M == lay.M - lay.sizes[-1] and len(rg.views()) == len(maps)
    assert all(_same_bits(a, b) for a, b in zip(rg.views(), views))
    # K = 1, with and without the maximum's segment (which is then the map again)
    one = spx.msc_pack(maps[:1], activation=activation, dtype=out_dtype)
    assert one.M == 2 * lay.sizes[0] and _same_bits(one.views()[0], views[0]) and _same_bits(one.views()[1], views[0])
    assert not bool(one.index.any())
    alone = spx.msc_pack(maps[:1], activation=activation, dtype=out_dtype, with_max=False)
    assert alone.M == lay.sizes[0] and _same_bits(alone.views()[0], views[0])


@pytest.mark.parametrize("name", MC.SHAPE_SETS)
def test_pack_within_the_float64_bounds(name):
    """The measures of tests/test_gpu_msc.py, per segment: the fp32 output within the restatement's bound, the index legitimate
    and decided as there, the sigmoid within 4 . 2^-24 of float64 sigma of the kernel's own "none" output."""
    dev = gpu_device()
    maps = _maps(name, dev)
    lay = PC.layout(name)
    pk = spx.msc_pack(maps)
    z, zb, idx64 = PC.restated(name)
    got = pk.features.reshape(-1, lay.M).cpu().numpy().astype(np.float64)
    err = np.abs(got - z)
    assert (err <= zb).all()
    assert (err[:, :lay.offsets[-1]] == 0).all()                       # the plain segments are copies
    _, _, _, u, b = MC.restated(name)
    gi = pk.index.cpu().numpy()
    pick = lambda t: np.take_along_axis(t, gi[None].astype(np.int64), 0)[0]
    best = np.take_along_axis(u, idx64[None].astype(np.int64), 0)[0]
    best_b = np.take_along_axis(b, idx64[None].astype(np.int64), 0)[0]
    assert (pick(u) >= best - (pick(b) + best_b)).all()
    sure = MR.decided(u, b)
    print(f"msc_pack forward {name}: worst error / bound {np.max(err[zb > 0] / zb[zb > 0]):.3f}, "
          f"{100.0 * (1.0 - sure.mean()):.4f} % undecided")
    assert 1.0 - sure.mean() <= 1e-3 and np.array_equal(gi[sure], idx64[sure])
    assert max(float(m.abs().max()) for m in maps) <= 12.0
    ys = spx.msc_pack(maps, activation="sigmoid").features.reshape(-1, lay.M).cpu().numpy().astype(np.float64)
    serr = np.abs(ys - MR.sigmoid(got))
    print(f"msc_pack sigmoid {name}: worst error {serr.max() / U:.2f} x 2^-24 (bound 4)")
    assert serr.max() <= 4 * U


# ---- 2. backward -----------------------------------------------------------------------------------------------------------------
def _backward(maps, g, activation, dtype, needs=None, with_max=True):
    leaves = [m.clone().requires_grad_(needs is None or needs[k]) for k, m in enumerate(maps)]
    pk = spx.msc_pack(leaves, activation=activation, dtype=dtype, with_max=with_max)
    pk.features.backward(g.to(pk.features.dtype).view_as(pk.features))
    return pk.features.detach(), pk.index, [l.grad for l in leaves]


def _upstream(lay, Cc, dev, dtype, seed=17):
    g = torch.round(torch.randn(Cc, lay.M, generator=torch.Generator().manual_seed(seed)) * 2.0 ** 10) / 2.0 ** 10
    if dtype == torch.bfloat16:
        g = g.to(torch.bfloat16).float()                               # the upstream gradient arrives in the output's dtype
    return g.to(dev)


@pytest.mark.parametrize("activation,dtype", [("none", torch.float32), ("sigmoid", torch.float32), ("sigmoid", torch.bfloat16)])
@pytest.mark.parametrize("name", MC.SHAPE_SETS)
def test_backward(name, activation, dtype):
    dev = gpu_device()
    maps = _maps(name, dev)
    lay = PC.layout(name)
    B, Cc = maps[0].shape[:2]
    shapes = [tuple(m.shape[2:]) for m in maps]
    g = _upstream(lay, Cc, dev, dtype)
    y, index, grads = _backward(maps, g, activation, dtype)
    y64 = y.float().reshape(Cc, lay.M).cpu().numpy() if activation == "sigmoid" else None      # the SAVED y, in its own dtype
    ref, bounds = PC.gradients(shapes, B, index.cpu().numpy(), g.cpu().numpy(), y64)
    for k, (got, want, bound) in enumerate(zip(grads, ref, bounds)):
        assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        worst = np.max(err[bound > 0] / bound[bound > 0]) if (bound > 0).any() else 0.0
        print(f"msc_pack backward {name} {activation} {dtype} map {k}: worst error / bound {worst:.3f}")
        assert (err <= bound).all(), k
        assert float(got.abs().max()) > 0
    # two runs agree bit for bit
    _, index2, again = _backward(maps, g, activation, dtype)
    assert torch.equal(index, index2) and all(bits_equal(a, b) for a, b in zip(grads, again))
    # a map that needs no gradient gets no buffer; the others are unchanged
    _, _, part = _backward(maps, g, activation, dtype, needs=(True, False, True))
    assert part[1] is None and bits_equal(part[0], grads[0]) and bits_equal(part[2], grads[2])
    # without the maximum's segment: the own term alone
    rl = PC.layout(name, with_max=False)
    g0 = g[:, :rl.M].contiguous()
    y0, none, own = _backward(maps, g0, activation, dtype, with_max=False)
    y064 = y0.float().reshape(Cc, rl.M).cpu().numpy() if activation == "sigmoid" else None
    ref0, bounds0 = PC.gradients(shapes, B, None, g0.cpu().numpy(), y064, with_max=False)
    assert none is None
    for got, want, bound in zip(own, ref0, bounds0):
        assert (np.abs(got.cpu().numpy().astype(np.float64) - want) <= bound).all()


@pytest.mark.parametrize("activation,dtype", [("none", torch.float32), ("sigmoid", torch.bfloat16)])
@pytest.mark.parametrize("with_max", [True, False])
def test_eight_maps_pack_is_msc_max_per_segment(with_max, activation, dtype):
    """As many maps as the kernels' unrolled decode loops take (tests/msc_cases.py): M = 880 with the maximum's segment (vector
    stores), 754 without (element stores)."""
    dev = gpu_device()
    maps = _maps("eight", dev)
    lay = PC.layout("eight", with_max)
    pk = spx.msc_pack(maps, activation=activation, dtype=dtype, with_max=with_max)
    assert lay.M == (880 if with_max else 754) and pk.segments == lay.segments and len(pk.views()) == 8 + with_max
    views = pk.views()
    for k, m in enumerate(maps):
        assert _same_bits(views[k], spx.msc_max([m], activation=activation, dtype=dtype)), k
    if with_max:
        want, index = spx.msc_max(maps, activation=activation, dtype=dtype, return_index=True)
        assert _same_bits(views[8], want) and torch.equal(pk.index, index)
    else:
        assert pk.index is None


@pytest.mark.parametrize("activation,dtype", [("none", torch.float32), ("sigmoid", torch.bfloat16)])
def test_eight_maps_backward(activation, dtype):
    """``test_backward``'s measure on eight maps, then with ``MC.EIGHT_NEEDS``: empty ranges of the prefix sums at the front, in
    the middle and next to the end."""
    dev = gpu_device()
    maps = _maps("eight", dev)
    lay = PC.layout("eight")
    B, Cc = maps[0].shape[:2]
    g = _upstream(lay, Cc, dev, dtype)
    y, index, grads = _backward(maps, g, activation, dtype)
    y64 = y.float().reshape(Cc, lay.M).cpu().numpy() if activation == "sigmoid" else None
    ref, bounds = PC.gradients([tuple(m.shape[2:]) for m in maps], B, index.cpu().numpy(), g.cpu().numpy(), y64)
    for k, (got, want, bound) in enumerate(zip(grads, ref, bounds)):
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        worst = np.max(err[bound > 0] / bound[bound > 0]) if (bound > 0).any() else 0.0
        print(f"msc_pack backward eight {activation} {dtype} map {k}: worst error / bound {worst:.3f}")
        assert tuple(got.shape) == want.shape and (err <= bound).all(), k
    _, index2, part = _backward(maps, g, activation, dtype, needs=MC.EIGHT_NEEDS)
    assert torch.equal(index, index2)
    for k, need in enumerate(MC.EIGHT_NEEDS):
        assert (bits_equal(part[k], grads[k]) if need else part[k] is None), k


def test_bf16_maps_get_bf16_gradients():
    dev = gpu_device()
    maps = _maps("odd", dev, torch.bfloat16)
    lay = PC.layout("odd")
    g = _upstream(lay, maps[0].shape[1], dev, torch.float32)
    y, index, grads = _backward(maps, g, "sigmoid", torch.float32)
    _, index32, wide = _backward([m.float() for m in maps], g, "sigmoid", torch.float32)
    assert torch.equal(index, index32)
    for a, b in zip(grads, wide):
        assert a.dtype == torch.bfloat16 and _same_bits(a, b.to(torch.bfloat16))


# ---- 3. the distance path on the packed axis ---------------------------------------------------------------------------------------
def _recorded_net(dev):
    c = PC.recorded()
    B, S, Cs, P, K = (int(v) for v in c["shape"])

    def init(net):
        net.prototype_vectors.copy_(torch.from_numpy(c["bank"]))
        net.last_layer.weight.copy_(torch.from_numpy(c["head"]))

    return c, proto_net(P, K, S, Cs, init=init, device=dev)


def _coarse(shape, gen, scale=1e-3):
    return torch.round(torch.randn(shape, generator=gen) * scale * 2.0 ** 20) / 2.0 ** 20


def _segment_upstreams(lay, P, K, seed):
    gen = torch.Generator().manual_seed(seed)
    return [(_coarse((lay.B, h, w, K), gen), _coarse((lay.B, P, h, w), gen), _coarse((lay.B * h * w, P), gen)) for h, w in lay.grids]


def _weighted_loss(outs, ups, dev=None):
    move = (lambda t: t.to(dev)) if dev is not None else (lambda t: t)
    return sum(wk * ((l * move(gl)).sum() + (d * move(gd)).sum() + (a * move(ga)).sum())
               for wk, (l, d, a), (gl, gd, ga) in zip(PC.SEGMENT_WEIGHTS, outs, ups))


def _oracle_step(convs, bank, head, ranges, S, ups):
    """The oracle on every segment's own feature values, one shared bank and head: outputs and the autograd gradients of the
    weighted loss."""
    xs = [c.clone().requires_grad_(True) for c in convs]
    p0, w0 = bank.clone().requires_grad_(True), head.clone().requires_grad_(True)
    outs = [O.forward_from_conv_features(x, p0, ranges, S, w0) for x in xs]
    _weighted_loss(outs, ups).backward()
    return [tuple(t.detach() for t in o) for o in outs], [x.grad for x in xs], p0.grad, w0.grad


def _check_modes(net, pk, want, tag):
    """The three tuple modes against ``want`` (one (logits, distances, activations) per segment)."""
    with torch.no_grad():
        for mode in MODES:
            out = net.forward_from_conv_features(pk, **mode)
            assert isinstance(out, list) and len(out) == len(want)
            for k, (o, (l, d, a)) in enumerate(zip(out, want)):
                names = ("logits", "distances", "activations") if len(mode) == 2 else (("logits", "activations") if mode else ("logits", "distances"))
                assert len(o) == len(names), (tag, mode, k)
                for t, kind in zip(o, names):
                    PAR.close_fwd(t, {"logits": l, "distances": d, "activations": a}[kind], kind)


def _list_path_bits(net, pk, tag):
    """Bit-equality of the packed outputs with the list path (one launch per segment on a contiguous copy of its view)."""
    with torch.no_grad():
        packed = net.forward_from_conv_features(pk, return_activations=True, return_distances=True)
        eq = {"logits": True, "distances": True, "activations": True}
        for v, (l, d, a) in zip(pk.views(), packed):
            l1, d1, a1 = net.forward_from_conv_features(v.contiguous(), return_activations=True, return_distances=True)
            eq["logits"] &= bits_equal(l, l1)
            eq["distances"] &= bits_equal(d, d1)
            eq["activations"] &= bits_equal(a, a1)
    print(f"packed against list path, {tag}: bit-equal " + ", ".join(f"{k} {v}" for k, v in eq.items()))
    return eq


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_distance_path_on_the_recorded_forward(dtype):
    """The reference's own training forward on four maps (a ragged batch: ``with_max=False``, the fourth map is the recorded
    one): values in the three tuple modes, gradients of a loss that weights the segments differently, through the pack's
    backward down to the maps."""
    dev = gpu_device()
    c, net = _recorded_net(dev)
    B, S, Cs, P, K = (int(v) for v in c["shape"])
    convs = [torch.from_numpy(m) for m in c["conv"]]
    leaves = [m.to(dev).requires_grad_(True) for m in convs]
    pk = spx.msc_pack(leaves, "none", dtype, with_max=False)
    lay = pk.layout
    assert lay.M == 376 and pk.index is None
    want = [(torch.from_numpy(c["logits"][k]), torch.from_numpy(c["distances"][k]), torch.from_numpy(c["activations"][k])) for k in range(4)]
    _check_modes(net, pk, want, "recorded")
    eq = _list_path_bits(net, pk, f"recorded {dtype}")
    assert eq["distances"] and eq["activations"]
    ups = _segment_upstreams(lay, P, K, seed=3)
    outs = net.forward_from_conv_features(pk, return_activations=True, return_distances=True)
    assert [tuple(o[1].shape) for o in outs] == [(B, P, h, w) for h, w in lay.grids]
    assert [o[1].stride() for o in outs] == [lay.view_strides(k) for k in range(4)]         # views of ONE map, nothing copied
    _weighted_loss(outs, ups, dev).backward()
    _, dxs, dp, dw = _oracle_step(convs, torch.from_numpy(c["bank"]), torch.from_numpy(c["head"]), c["ranges"], S, ups)
    for k, (leaf, dx) in enumerate(zip(leaves, dxs)):
        grad_close(leaf.grad, dx, f"dX map {k} {dtype}", tol=PAR.dx_tolerance(dtype))
    grad_close(net.prototype_vectors.grad, dp, f"dPrototypes {dtype}")
    grad_close(net.last_layer.weight.grad, dw, f"dLastLayer {dtype}")


def test_distance_path_on_the_pascal_grids():
    """41 x 41 <- {21 x 21, 31 x 31} at B = 2 with the maximum: M = 9 528, 75 tiles, every boundary inside a tile.  No fixture:
    the oracle at each segment's own feature values (the pack's bf16 output)."""
    dev = gpu_device()
    p = PC.PASCAL
    B, S, Cs, P, K = p["B"], p["S"], p["Cs"], p["P"], p["K"]
    gen = torch.Generator().manual_seed(41)
    raw = [torch.randn(B, S * Cs, h, w, generator=gen).to(dev) for h, w in p["grids"]]
    bank = O.bf16_representable(torch.rand(P, Cs, 1, 1, generator=gen))
    head = O.last_layer_init(O.default_class_identity(P, K, S)) + 0.05 * torch.randn(K, P, generator=gen)

    def init(net):
        net.prototype_vectors.copy_(bank)
        net.last_layer.weight.copy_(head)

    net = proto_net(P, K, S, Cs, init=init, device=dev)
    pk = spx.msc_pack(raw, "sigmoid", torch.bfloat16)
    lay = pk.layout
    assert lay.M == 9528 and (lay.M + 127) // 128 == 75 and all(o % 128 for o in lay.offsets[1:])
    feats = pk.features.detach().requires_grad_(True)                   # dX at the packed features themselves
    pk2 = spx.PackedMaps(features=feats, layout=lay, index=pk.index)
    convs = [v.detach().float().cpu().contiguous() for v in pk.views()]
    ranges = O.default_scale_ranges(P, S)
    ups = _segment_upstreams(lay, P, K, seed=5)
    want, dxs, dp, dw = _oracle_step(convs, bank, head, ranges, S, ups)
    _check_modes(net, pk2, want, "pascal41")
    eq = _list_path_bits(net, pk, "pascal41 bf16")
    assert eq["distances"] and eq["activations"]
    outs = net.forward_from_conv_features(pk2, return_activations=True, return_distances=True)
    _weighted_loss(outs, ups, dev).backward()
    for k, dx in enumerate(dxs):
        grad_close(lay.view(feats.grad, k), dx, f"dX segment {k}", tol=PAR.dx_tolerance(torch.bfloat16))
    grad_close(net.prototype_vectors.grad, dp, "dPrototypes")
    grad_close(net.last_layer.weight.grad, dw, "dLastLayer")


# ---- 4. target_labels as a list -----------------------------------------------------------------------------------------------------
def test_target_labels_per_segment():
    import kld_cases as KC

    dev = gpu_device()
    c, net = _recorded_net(dev)
    B, S, Cs, P, K = (int(v) for v in c["shape"])
    leaves = [torch.from_numpy(m).to(dev).requires_grad_(True) for m in c["conv"]]
    pk = spx.msc_pack(leaves, "none", torch.bfloat16, with_max=False)
    pk.features.retain_grad()
    lay = pk.layout
    targets = [PAR.gather_labels(B, h, w, K, seed=30 + k).to(dev) for k, (h, w) in enumerate(lay.grids)]
    with torch.no_grad():
        wide = net.forward_from_conv_features(pk, return_distances=True)
    out = net.forward_from_conv_features(pk, return_distances=True, target_labels=targets)
    kld = spx.KLDLoss(net.prototype_class_identity, S, net.scale_num_prototypes)
    table = out[0][1].table
    fast, slow = 0.0, 0.0
    for k, ((logits, cd), (wl, wd), t) in enumerate(zip(out, wide, targets)):
        h, w = lay.grids[k]
        assert isinstance(cd, spx.ClassDistances) and cd.grid == (h, w) and cd.target is t and cd.target_version == t._version
        assert tuple(cd.values.shape) == (B, table.shape[1], h * w) and tuple(cd.labels.shape) == (B, h * w)
        assert torch.equal(cd.labels.long(), t.reshape(B, -1) - 1)
        want = _gathered.gather_class_distances(wd, cd.labels, table).permute(0, 2, 1)
        assert bits_equal(cd.values.detach().contiguous(), want.contiguous()), k
        assert bits_equal(logits, wl)
        assert _gathered.from_class_distances(cd, t).poison is None                     # the fast path: no compare launch
        fast = fast + kld(cd, t)
        slow = slow + kld(wd, t)
    f, s_ = float(fast.detach()), float(slow.detach())
    print(f"KLD on the four segments: class-gathered {f:.6e}, P-wide {s_:.6e}")
    assert abs(f - s_) <= KC.LOSS_TOL * max(1.0, abs(s_))
    fast.backward()
    g = pk.features.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    assert all(l.grad is not None and float(l.grad.abs().max()) > 0 for l in leaves)
    # an in-place edit of ONE label map voids that segment's fast path only
    targets[1].add_(0)
    voided = [_gathered.from_class_distances(o[1], t).poison is not None for o, t in zip(out, targets)]
    assert voided == [False, True, False, False]
    assert float(_gathered.from_class_distances(out[1][1], targets[1]).poison) == 1.0     # the same classes: still valid
    # a wrong list raises before any launch
    for bad in (targets[:3], targets[0], targets[:3] + [targets[3][:, :-1]], [targets[1]] + targets[1:]):
        with pytest.raises(spx.SpxError, match="target_labels"):
            net.forward_from_conv_features(pk, return_distances=True, target_labels=bad)


# ---- 5. the module ---------------------------------------------------------------------------------------------------------------
def test_module_packed_training():
    dev = gpu_device()
    net = proto_net(40, 5, 4, 16, seed=11, device=dev, backbone="pool", stride=2)
    net.features = spx.MSC(net.features)
    x = torch.randn(2, 3, 26, 34, device=dev)
    flags = dict(return_activations=True, return_distances=True)
    with torch.no_grad():
        net.train()
        stock_train = net(x, **flags)
        net.eval()
        stock_eval = net(x, **flags)
        net.fuse_feature_epilogue(torch.bfloat16)
        fused_eval = net(x, **flags)
        net.train()
        fused_train = net(x, **flags)

        net.fuse_feature_epilogue(torch.bfloat16, packed=True)
        conv = net.conv_features(x)
        assert isinstance(conv, spx.PackedMaps) and conv.features.dtype == torch.bfloat16
        assert [g for g in conv.layout.grids] == [(13, 17), (6, 8), (9, 12), (13, 17)]
        for v, f in zip(conv.views(), net.features.fused(x, "sigmoid", torch.bfloat16)):
            assert _same_bits(v, f)
        for mode in MODES:
            out = net(x, **mode)
            ref = [net.forward_from_conv_features(v.contiguous(), **mode) for v in conv.views()]
            assert isinstance(out, list) and len(out) == 4 and all(len(o) == len(r) for o, r in zip(out, ref))
            names = ("logits", "distances", "activations") if len(mode) == 2 else (("logits", "activations") if mode else ("logits", "distances"))
            for o, r in zip(out, ref):
                for t, u, kind in zip(o, r, names):
                    assert t.shape == u.shape
                    PAR.close_fwd(t, u.cpu(), kind)
        out = net(x, **flags)
        assert [tuple(o[0].shape) for o in out] == [(2, 13, 17, 5), (2, 6, 8, 5), (2, 9, 12, 5), (2, 13, 17, 5)]
        assert [tuple(o[1].shape) for o in out] == [(2, 40, 13, 17), (2, 40, 6, 8), (2, 40, 9, 12), (2, 40, 13, 17)]
        assert [tuple(o[2].shape) for o in out] == [(442, 40), (96, 40), (216, 40), (442, 40)]
        for o, r in zip(out, fused_train):
            for t, u, kind in zip(o, r, ("logits", "distances", "activations")):
                PAR.close_fwd(t, u.cpu(), kind)
        # eval is untouched by packed=True; packed=False and None are what they were, bit for bit
        net.eval()
        packed_eval = net(x, **flags)
        assert all(bits_equal(a, b) for a, b in zip(packed_eval, fused_eval))
        net.train()
        net.fuse_feature_epilogue(torch.bfloat16, packed=False)
        again = net(x, **flags)
        assert all(bits_equal(a, b) for o, r in zip(again, fused_train) for a, b in zip(o, r))
        net.fuse_feature_epilogue(None)
        assert all(bits_equal(a, b) for o, r in zip(net(x, **flags), stock_train) for a, b in zip(o, r))
        net.eval()
        assert all(bits_equal(a, b) for a, b in zip(net(x, **flags), stock_eval))


def test_module_refusals():
    dev = gpu_device()
    net = proto_net(40, 5, 4, 16, seed=11, device=dev, backbone="pool", stride=2)
    net.features = spx.MSC(net.features)
    net.fuse_feature_epilogue(torch.bfloat16, packed=True)
    net.train()
    x = torch.randn(2, 3, 26, 34, device=dev)
    with torch.no_grad():
        pk = net.conv_features(x)
        t = [torch.ones(2, h, w, dtype=torch.long, device=dev) for h, w in pk.layout.grids]
        with pytest.raises(spx.SpxError, match="ce_target"):
            net.forward_from_conv_features(pk, ce_target=t)
        with pytest.raises(spx.SpxError, match="ce_target"):
            net(x, ce_target=t)
        with pytest.raises(spx.SpxError, match="push"):
            net.push_forward(x)
        with pytest.raises(spx.SpxError, match="push"):
            net.push_min_from_conv(pk, lambda grid: None)
        with pytest.raises(spx.SpxError, match="target_labels"):
            net(x, return_distances=True, target_labels=t[0])
        net.prototype_activation_function = lambda d: -d
        with pytest.raises(spx.SpxError, match="callable"):
            net.forward_from_conv_features(pk)
        net.prototype_activation_function = "log"
        headed = proto_net(40, 5, 4, 16, seed=11, device=dev, backbone="pool", stride=2, scale_head_type="sum")
        with pytest.raises(spx.SpxError, match="scale_head"):
            headed.train().forward_from_conv_features(pk)


# ---- 6. capture ------------------------------------------------------------------------------------------------------------------
def test_capture_pack_distance_forward_and_backward():
    from scaleprotoseg_amd.graphs import capture_step

    dev = gpu_device()
    c, net = _recorded_net(dev)
    B, S, Cs, P, K = (int(v) for v in c["shape"])
    raw = [torch.zeros(B, S * Cs, h, w, device=dev).requires_grad_(True) for h, w in ((7, 9), (4, 5), (6, 7))]
    lay = PC.layout("odd")
    ups = [tuple(t.to(dev) for t in u) for u in _segment_upstreams(lay, P, K, seed=9)]
    leaves = raw + [net.prototype_vectors, net.last_layer.weight]
    s = torch.cuda.Stream()

    def step():
        for t in leaves:
            t.grad = None
        pk = spx.msc_pack(raw, "sigmoid", torch.bfloat16)
        outs = net.forward_from_conv_features(pk, return_activations=True, return_distances=True)
        _weighted_loss(outs, ups).backward()
        return pk.features.detach(), outs[3][0].detach()

    def refill(seed):
        gen = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for t in raw:
                t.copy_(torch.randn(t.shape, generator=gen))

    eager = {}
    for seed in (1, 2):
        refill(seed)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):         # eager reference on the capture's side stream
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
        for what, a, b in zip(("features", "logits", "d0", "d1", "d2", "dP", "dW"), got, eager[seed]):
            assert _same_bits(a, b), (seed, what)


# ---- 7. memory hygiene -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["odd", "one_up", "pascal41"])
def test_memory_hygiene(name, dtype):
    """Channel-slice inputs with strides of their own; ``out``, the index and the gradient buffers inside guard bands at
    element offsets no vector width divides, poisoned: every element inside written, nothing outside.  ``out=`` at any element
    offset is handled (element stores), as documented.  The public call allocates the outputs and nothing else."""
    from scaleprotoseg_amd import _lib

    dev = gpu_device()
    lib = _lib.load()
    esz = 2 if dtype == torch.bfloat16 else 4
    dense = _maps(name, dev, dtype)
    lay = PC.layout(name)
    maps = []
    for m in dense:
        B, Cc, h, w = m.shape
        parent = torch.full((B + 1, 2 * Cc + 3, h, w), float("nan"), dtype=dtype, device=dev)
        view = parent[1:, 1:1 + 2 * Cc:2]
        view.copy_(m)
        maps.append(view)
    B, Cc, H, W = maps[0].shape
    n = Cc * lay.M
    want = spx.msc_pack(dense, activation="sigmoid")
    want_bits, want_index = want.features.reshape(Cc, lay.M), want.index

    # the public call: out= at element offsets 0..3 of a guarded buffer
    for off in (0, 1, 2, 3):
        og = Guarded((n + 4) * esz, dev)
        body = og.body(dtype)
        body.fill_(float("nan"))
        out = body[off:off + n].view(Cc, lay.M)
        got = spx.msc_pack(maps, activation="sigmoid", out=out)
        assert got.features.data_ptr() == out.data_ptr() and _same_bits(out, want_bits) and torch.equal(got.index, want_index)
        assert og.intact() and bool(torch.isnan(body[:off]).all()) and bool(torch.isnan(body[off + n:]).all())

    # nothing allocated beyond the outputs (the caching allocator hands out multiples of 512 bytes)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    with torch.no_grad():
        held = spx.msc_pack(dense, activation="sigmoid")
    torch.cuda.synchronize()
    r512 = lambda v: (v + 511) // 512 * 512
    assert torch.cuda.memory_allocated(dev) - before == r512(n * esz) + r512(B * Cc * H * W)
    del held

    # forward and backward through the C entry points, every buffer guarded at an odd element offset
    og = Guarded((n + 2) * esz, dev)
    body = og.body(dtype)
    body.fill_(float("nan"))
    ig = Guarded(B * Cc * H * W + 6, dev)
    ig.body(torch.uint8).fill_(0xEE)
    g = _upstream(lay, Cc, dev, dtype).to(dtype)
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
    a.out, a.index, a.g = og.ptr + esz, ig.ptr + 3, g.data_ptr()
    _lib.check(lib.spx_msc_pack_fwd(C.byref(a), 1, _lib.stream_ptr()))
    _lib.check(lib.spx_msc_pack_bwd(C.byref(a), 1, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert og.intact() and ig.intact() and all(bg.intact() for bg in bufs)
    assert _same_bits(body[1:1 + n].view(Cc, lay.M), want_bits) and bool(torch.isnan(body[0])) and bool(torch.isnan(body[n + 1]))
    ib = ig.body(torch.uint8)
    ni = B * Cc * H * W
    assert torch.equal(ib[3:3 + ni].view(B, Cc, H, W), want_index) and bool((ib[:3] == 0xEE).all()) and bool((ib[3 + ni:] == 0xEE).all())
    _, _, ref = _backward(dense, g, "sigmoid", dtype)
    for k, (bg, m) in enumerate(zip(bufs, maps)):
        gb = bg.body(dtype)
        inner = gb[1:1 + m.numel()].view(m.shape)
        assert not bool(torch.isnan(inner).any()) and _same_bits(inner, ref[k]), k
        assert bool(torch.isnan(gb[0])) and bool(torch.isnan(gb[1 + m.numel()]))
