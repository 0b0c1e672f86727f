"""GPU checks of the activation losses (csrc/spx_actloss.hip through EntropySpatLoss, EntropySamplLoss, NormLoss and
ActivationRegularizers): against the reference-recorded fixture (tests/golden/activation_losses.npz) and the float64
restatement of tests/activation_loss_cases.py.  Tolerances are those of the KLD kernels' tests for the same comparisons."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from activation_loss_cases import (CASES, EPS, TERMS, W3, check_against_reference64, identity, load_case, log_activation, reference64,
                                   restate_term)
from support import gpu_device, proto_net


def _patchy_target(B, H, W, K, gen, salt=0.03):
    """8 x 16 blocks of one label (0 = void .. K) with salt (single pixels of any label 0 .. K + 1, K + 1 = out of range)."""
    blocks = torch.randint(0, K + 1, (B, (H + 7) // 8, (W + 15) // 16), generator=gen)
    t = blocks.repeat_interleave(8, 1).repeat_interleave(16, 2)[:, :H, :W].contiguous()
    m = torch.rand(B, H, W, generator=gen) < salt
    t[m] = torch.randint(0, K + 2, (int(m.sum()),), generator=gen)
    return t


def _class_distances(d_map, target, ident, dev, grid=None):
    """ClassDistances of the [B, P, H, W] map ``d_map`` (a leaf on ``dev``: the gather is differentiable to it)."""
    from scaleprotoseg_amd.loss import ClassDistances, class_slot_table, gather_class_distances

    B = d_map.shape[0]
    table = class_slot_table(ident).to(dev)
    labels0 = (target.reshape(B, -1).long() - 1).to(dev)
    planes = gather_class_distances(d_map, labels0, table).permute(0, 2, 1).contiguous()
    tgt = target.to(dev)
    grid = grid or tuple(d_map.shape[-2:])
    return ClassDistances(values=planes, labels=labels0.to(torch.int32), table=table, grid=grid, target=tgt,
                          target_version=tgt._version), tgt


def _to_map(flat, B, H, W):
    """[B * H * W, P] -> [B, P, H, W]"""
    return flat.reshape(B, H * W, -1).permute(0, 2, 1).reshape(B, -1, H, W).contiguous()


def _from_map(m):
    """[B, P, H, W] -> [B * H * W, P]"""
    B, P = m.shape[:2]
    return m.reshape(B, P, -1).permute(0, 2, 1).reshape(-1, P)


def _drop_in(spx, term, ident, S, ranges):
    if term == "spat":
        return spx.EntropySpatLoss(ident)
    if term == "sampl":
        return spx.EntropySamplLoss(ident, S, ranges)
    return spx.NormLoss(ident, term)


@pytest.mark.parametrize("name", CASES)
def test_fixture_parity(name):
    """1: every term alone through its drop-in and all three through ActivationRegularizers, fed the [M, P] activations (gradient to
    act) and a ClassDistances built from d (gradient to d); |value - ref| <= 2e-6, gradient <= 2e-5 max|ref| + 1e-9; two runs
    bit-identical.

    The recorded gradients are the reference's own fp32 autograd.  For one array that is itself further from the exact gradient
    than the bound: `ties`, sample entropy, gradient to d - at the five pixels with d = 0 one slot holds nearly all of the softmax,
    log_softmax's backward subtracts two numbers that agree to 1.7e-3, and a'(0) = -9999 carries the rounding into d.  Measured on
    the CPU: fixture against the float64 restatement 5.44e-6 = 2.55e-5 of max|grad| 0.214 (bound 4.27e-6); every other array
    <= 2.9e-7 of its maximum.  The kernels measured 5.45e-6 against that fixture array and agree with float64.  So the gradient
    is held to the bound against the float64 restatement of the same inputs, and against the fixture to the bound plus the
    fixture's own distance from that restatement, computed here (not a constant)."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    c = load_case(name)
    ident, target = c["ident"], c["target"]
    B, H, W = target.shape
    S = len(c["ranges"])
    ranges = {s: r for s, r in enumerate(c["ranges"])}

    def run(make_loss, form):
        if form == "act":
            x = c["act"].to(dev).requires_grad_(True)
            v = make_loss()(x, target.to(dev))
        else:
            x = _to_map(c["d"], B, H, W).to(dev).requires_grad_(True)
            cd, tgt = _class_distances(x, target, ident, dev)
            v = make_loss()(cd, tgt)
        tot = v[0] if isinstance(v, tuple) else v
        tot.backward()
        g = x.grad if form == "act" else _from_map(x.grad)
        return v, g

    exact = {}                                  # float64 restatement of the recorded gradients, per (term, form)
    for term in TERMS:
        d64 = c["d"].double().clone().requires_grad_(True)
        a64 = log_activation(d64)
        a64.retain_grad()
        restate_term(term, a64, target, ident, c["ranges"])[0].backward()
        exact[term, "act"], exact[term, "d"] = a64.grad, d64.grad

    def check(v, g, ref_v, ref_g, ex_g, what):
        g = g.double().cpu()
        err, gerr, gmax = abs(v.item() - ref_v), (g - ref_g).abs().max().item(), ref_g.abs().max().item()
        own, exerr = (ref_g.double() - ex_g).abs().max().item(), (g - ex_g).abs().max().item()
        print(f"{name} {what}: value {v.item():.9g} ref {ref_v:.9g} err {err:.3g}; gradient err {gerr:.3g} of max {gmax:.3g} "
              f"(fixture to float64 {own:.3g}, kernels to float64 {exerr:.3g})")
        assert err <= 2e-6, what
        assert exerr <= 2e-5 * gmax + 1e-9, what
        assert gerr <= 2e-5 * gmax + 1e-9 + own, what

    for form in ("act", "d"):
        for term in TERMS:
            mk = lambda: _drop_in(spx, term, ident, S, ranges)
            v, g = run(mk, form)
            assert v.is_cuda and v.dim() == 0
            check(v, g, c[term].item(), c[f"d_{term}_{form}"], exact[term, form], f"{term} / {form}")
            v2, g2 = run(mk, form)
            assert torch.equal(v, v2) and torch.equal(g, g2)
        for nt in ("l1", "linf"):
            mk = lambda: spx.ActivationRegularizers(ident, S, ranges, *W3, norm_type=nt)
            (tot, terms), g = run(mk, form)
            keys = ("spat", "sampl", nt)
            ref_g = sum(w * c[f"d_{k}_{form}"] for w, k in zip(W3, keys))
            for i, k in enumerate(keys):
                assert abs(terms[i].item() - c[k].item()) <= 2e-6, (k, form)
            ex_g = sum(w * exact[k, form] for w, k in zip(W3, keys))
            check(tot, g, sum(w * c[k].item() for w, k in zip(W3, keys)), ref_g, ex_g, f"fused {nt} / {form}")
            (tot2, terms2), g2 = run(mk, form)
            assert torch.equal(tot, tot2) and torch.equal(terms, terms2) and torch.equal(g, g2)


EDGE_COUNTS = [[2, 1, 0, 3, 2, 2], [2, 2, 0, 1, 3, 2]]      # class 1: one prototype in scale 0, class 3: one in scale 1, class 2: none


@pytest.mark.parametrize("grid", [(5, 64), (67, 333), (1, 1000)])
@pytest.mark.parametrize("linear_walk", [False, True])
def test_edges_against_the_float64_restatement(grid, linear_walk):
    """2: the column walk, partial tiles and the linear walk; ragged per-class counts with ns = 1 and a class without prototypes."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    H, W = grid
    B, K = 2, 6
    gen = torch.Generator().manual_seed(1000 * H + W)
    ident, rl = identity(EDGE_COUNTS)
    ranges = {s: r for s, r in enumerate(rl)}
    target = _patchy_target(B, H, W, K, gen)
    d = torch.rand(B * H * W, ident.shape[0], generator=gen) * 2.0
    for nt in ("l1", "linf"):
        ref = reference64(d, target, ident, rl, nt, W3, log_activation)
        x = _to_map(d, B, H, W).to(dev).requires_grad_(True)
        cd, tgt = _class_distances(x, target, ident, dev, grid=(1, H * W) if linear_walk else (H, W))
        tot, terms = spx.ActivationRegularizers(ident, 2, ranges, *W3, norm_type=nt)(cd, tgt)
        tot.backward()
        check_against_reference64(tot, terms, _from_map(x.grad), ref, f"{grid} linear={linear_walk} {nt}")


def test_slot_limit():
    """3: sixteen slots per class run; seventeen are refused."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    B, H, W, K = 2, 9, 33, 3
    gen = torch.Generator().manual_seed(16)
    ident, rl = identity([[4, 4, 4]] * 4)
    ranges = {s: r for s, r in enumerate(rl)}
    target = _patchy_target(B, H, W, K, gen, salt=0.1)
    d = torch.rand(B * H * W, ident.shape[0], generator=gen) * 2.0
    ref = reference64(d, target, ident, rl, "l1", W3, log_activation)
    x = _to_map(d, B, H, W).to(dev).requires_grad_(True)
    cd, tgt = _class_distances(x, target, ident, dev)
    assert cd.values.shape[1] == 16
    tot, terms = spx.ActivationRegularizers(ident, 4, ranges, *W3)(cd, tgt)
    tot.backward()
    check_against_reference64(tot, terms, _from_map(x.grad), ref, "J = 16")
    ident17, rl17 = identity([[17, 2, 2]])
    act = torch.rand(B * H * W, 21, generator=gen).to(dev)
    with pytest.raises(spx.SpxError):
        spx.NormLoss(ident17, "l1")(act, target.to(dev))
    with pytest.raises(spx.SpxError):
        spx.ActivationRegularizers(ident17, 1, {0: rl17[0]}, *W3)(act, target.to(dev))


def test_large_class_count():
    """4: 150 classes x 12 slots: the per-class tables of the sums and gradient passes span several class blocks."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    B, H, W, K = 2, 33, 65, 150
    gen = torch.Generator().manual_seed(150)
    ident, rl = identity([[3] * K] * 4)
    ranges = {s: r for s, r in enumerate(rl)}
    target = _patchy_target(B, H, W, K, gen, salt=0.3)
    d = torch.rand(B * H * W, ident.shape[0], generator=gen) * 2.0
    ref = reference64(d, target, ident, rl, "l1", W3, log_activation)
    x = _to_map(d, B, H, W).to(dev).requires_grad_(True)
    cd, tgt = _class_distances(x, target, ident, dev)
    assert cd.values.shape[1] == 12
    tot, terms = spx.ActivationRegularizers(ident, 4, ranges, *W3)(cd, tgt)
    tot.backward()
    check_against_reference64(tot, terms, _from_map(x.grad), ref, "K = 150")


def test_linf_ties():
    """5: exactly five pixels of one segment at d = 0 in one slot share the linf gradient evenly, the slot's other pixels get 0;
    the same on equal activations (mode 0)."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    B, H, W, K = 2, 7, 9, 3
    gen = torch.Generator().manual_seed(5)
    ident, rl = identity([[2, 2, 2], [2, 2, 2]])
    target = torch.randint(0, K + 1, (B, H, W), generator=gen)
    seg = torch.nonzero(target[1].reshape(-1) == 2).flatten() + H * W          # rows of segment (image 1, class 1) in [B*HW, P]
    assert len(seg) >= 8
    p = int(torch.nonzero(ident[:, 1]).flatten()[2])                           # the class's third slot
    nseg = sum(1 for b in range(B) for k in range(K) if (target[b] == k + 1).any())
    coef = 1.0 / (nseg * 4)                                                    # mean over segments, mean over the Jc = 4 slots
    loss = spx.NormLoss(ident, "linf")

    d = torch.rand(B * H * W, 12, generator=gen) * 2.0 + 0.01
    d[seg[:5], p] = 0.0
    x = _to_map(d, B, H, W).to(dev).requires_grad_(True)
    cd, tgt = _class_distances(x, target, ident, dev)
    loss(cd, tgt).backward()
    g = _from_map(x.grad).cpu()
    want = coef / 5 * (1.0 - 1.0 / EPS)                                        # a'(0) = 1/(0+1) - 1/(0+eps)
    print("ties, distances: got", g[seg[:5], p].tolist(), "want", want)
    assert (g[seg[:5], p] - want).abs().max().item() <= 1e-5 * abs(want)
    assert (g[seg[5:], p] == 0).all()

    act = torch.rand(B * H * W, 12, generator=gen) * 2.0
    act[seg[:5], p] = 3.0
    a = act.to(dev).requires_grad_(True)
    loss(a, target.to(dev)).backward()
    g = a.grad.cpu()
    print("ties, activations: got", g[seg[:5], p].tolist(), "want", coef / 5)
    assert (g[seg[:5], p] - coef / 5).abs().max().item() <= 1e-6 * coef
    assert (g[seg[5:], p] == 0).all()


def test_empty():
    """6: no labelled pixel: every term is exactly 0 on the device, the gradient is all zero."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    B, H, W = 2, 7, 9
    ident, rl = identity([[2, 2, 2], [2, 2, 2]])
    ranges = {s: r for s, r in enumerate(rl)}
    gen = torch.Generator().manual_seed(6)
    target = torch.zeros(B, H, W, dtype=torch.long)
    target[0, 0, 0] = 5                                                        # out of range: no class either
    a = torch.rand(B * H * W, 12, generator=gen).to(dev).requires_grad_(True)
    tot, terms = spx.ActivationRegularizers(ident, 2, ranges, *W3)(a, target.to(dev))
    tot.backward()
    assert tot.is_cuda and tot.item() == 0.0 and (terms == 0).all() and (a.grad == 0).all()
    x = torch.rand(B, 12, H, W, generator=gen).to(dev).requires_grad_(True)
    cd, tgt = _class_distances(x, target, ident, dev)
    for term in TERMS:
        v = _drop_in(spx, term, ident, 2, ranges)(cd, tgt)
        assert v.is_cuda and v.item() == 0.0
    spx.NormLoss(ident, "linf")(cd, tgt).backward()
    assert (x.grad == 0).all()


def test_linear_activation():
    """7: activation = "linear" (a = -d) against the restatement."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    B, H, W, K = 2, 19, 37, 6
    gen = torch.Generator().manual_seed(7)
    ident, rl = identity(EDGE_COUNTS)
    ranges = {s: r for s, r in enumerate(rl)}
    target = _patchy_target(B, H, W, K, gen, salt=0.1)
    d = torch.rand(B * H * W, ident.shape[0], generator=gen) * 2.0
    for nt in ("l1", "linf"):
        ref = reference64(d, target, ident, rl, nt, W3, lambda t: -t)
        x = _to_map(d, B, H, W).to(dev).requires_grad_(True)
        cd, tgt = _class_distances(x, target, ident, dev)
        tot, terms = spx.ActivationRegularizers(ident, 2, ranges, *W3, norm_type=nt, activation="linear")(cd, tgt)
        tot.backward()
        check_against_reference64(tot, terms, _from_map(x.grad), ref, f"linear {nt}")


def test_fused_equals_separate_terms():
    """8: ActivationRegularizers(w1, w2, w3) = sum of w_i x drop-in i, value and gradient."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    B, H, W, K = 2, 19, 37, 6
    gen = torch.Generator().manual_seed(8)
    ident, rl = identity(EDGE_COUNTS)
    ranges = {s: r for s, r in enumerate(rl)}
    target = _patchy_target(B, H, W, K, gen, salt=0.1)
    d = _to_map(torch.rand(B * H * W, ident.shape[0], generator=gen) * 2.0, B, H, W)
    for nt in ("l1", "linf"):
        x = d.to(dev).requires_grad_(True)
        cd, tgt = _class_distances(x, target, ident, dev)
        tot, terms = spx.ActivationRegularizers(ident, 2, ranges, *W3, norm_type=nt)(cd, tgt)
        tot.backward()
        y = d.to(dev).requires_grad_(True)
        cd2, tgt2 = _class_distances(y, target, ident, dev)
        parts = [_drop_in(spx, t, ident, 2, ranges)(cd2, tgt2) for t in ("spat", "sampl", nt)]
        sep = sum(w * v for w, v in zip(W3, parts))
        sep.backward()
        for i in range(3):
            assert abs(terms[i].item() - parts[i].item()) <= 1e-6 * max(1.0, abs(parts[i].item()))
        assert abs(tot.item() - sep.item()) <= 1e-6 * max(1.0, abs(sep.item()))
        gmax = y.grad.abs().max().item()
        assert gmax > 0 and (x.grad - y.grad).abs().max().item() <= 1e-6 * gmax


def _regs(spx, net, **kw):
    return spx.ActivationRegularizers(net.prototype_class_identity, net.num_scales, net.scale_num_prototypes, *W3,
                                      epsilon=net.epsilon, **kw)


def test_through_the_module():
    """9: the loss on the ClassDistances of forward_from_conv_features(target_labels=...) against the same loss on the
    return_activations=True activations: value and the gradients to the prototypes and the features."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    B, H, W, K, S, Cs = 2, 9, 9, 3, 2, 16
    net = proto_net(24, 3, 2, 16, seed=9, device=dev)
    gen = torch.Generator().manual_seed(9)
    conv = torch.sigmoid(torch.randn(B, S * Cs, H, W, generator=gen)).to(torch.bfloat16).float()
    target = torch.randint(0, K + 1, (B, H, W), generator=gen).to(dev)
    reg = _regs(spx, net)
    out = []
    for route in ("gathered", "activations"):
        net.zero_grad(set_to_none=True)
        x = conv.to(dev).requires_grad_(True)
        if route == "gathered":
            _, cd = net.forward_from_conv_features(x, target_labels=target)
            assert isinstance(cd, spx.ClassDistances)
            tot, terms = reg(cd, target)
        else:
            _, act = net.forward_from_conv_features(x, return_activations=True)
            tot, terms = reg(act, target)
        tot.backward()
        out.append((tot.item(), terms.cpu(), net.prototype_vectors.grad.clone(), x.grad.clone()))
    (v0, t0, gp0, gx0), (v1, t1, gp1, gx1) = out
    print("module: gathered", v0, "activations", v1, "terms", t0.tolist(), t1.tolist())
    assert (t1 > 0).all()
    assert abs(v0 - v1) <= 1e-5 * max(1.0, abs(v1))
    for a, b, what in ((gp0, gp1, "prototypes"), (gx0, gx1, "features")):
        scale = b.abs().max().item()
        err = (a - b).abs().max().item()
        print(f"module: d {what} err {err:.3g} of max {scale:.3g}")
        assert scale > 0 and err <= 1e-4 * scale, what


def test_no_host_synchronisation():
    """10: after a first call (caches), forward and backward run without a host synchronisation, in both input forms."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    B, H, W, K, S, Cs = 2, 9, 9, 3, 2, 16
    net = proto_net(24, 3, 2, 16, seed=10, device=dev)
    gen = torch.Generator().manual_seed(10)
    x = torch.sigmoid(torch.randn(B, S * Cs, H, W, generator=gen)).to(dev)
    target = torch.randint(0, K + 1, (B, H, W), generator=gen).to(dev)
    reg = _regs(spx, net)

    def step():
        net.zero_grad(set_to_none=True)
        _, cd = net.forward_from_conv_features(x, target_labels=target)
        tot, terms = reg(cd, target)
        _, act = net.forward_from_conv_features(x, return_activations=True)
        tot2, _ = reg(act, target)
        (tot + tot2).backward()
        return terms

    step()
    torch.cuda.synchronize()
    mode_works = True
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            torch.zeros(1, device=dev).item()
            mode_works = False
        except RuntimeError:
            pass
        terms = step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.isfinite(terms).all() and (terms > 0).all()
    print("sync debug mode effective:", mode_works)


def test_captured_step_replays_eager_bit_for_bit():
    """11: forward with target_labels, CE + KLD + ActivationRegularizers, backward: a captured step replays equal to eager."""
    import gc

    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd.graphs import capture_step

    dev = gpu_device()
    B, H, W, K, S, Cs = 2, 9, 9, 3, 2, 16
    net = proto_net(24, 3, 2, 16, seed=11, device=dev)
    gen = torch.Generator().manual_seed(11)
    x = torch.sigmoid(torch.randn(B, S * Cs, H, W, generator=gen)).to(dev)
    target = torch.randint(0, K + 1, (B, H, W), generator=gen).to(dev)
    reg = _regs(spx, net)
    ce = spx.PixelWiseCrossEntropyLoss(ignore_index=-1)
    kld = spx.KLDLoss(net.prototype_class_identity, net.num_scales, net.scale_num_prototypes)
    s = torch.cuda.Stream()

    def step():
        net.zero_grad(set_to_none=True)
        logits, cd = net.forward_from_conv_features(x, target_labels=target, ce_target=target)
        tot, terms = reg(cd, target)
        loss = ce(logits, target) + 0.25 * kld(cd, target) + tot
        loss.backward()
        return loss.detach(), terms.detach()

    with torch.cuda.stream(s):             # eager reference on the capture's side stream
        step()
        loss, terms = step()
    torch.cuda.synchronize()
    eager = [loss.clone(), terms.clone()] + [p.grad.clone() for p in net.parameters() if p.grad is not None]
    del loss, terms
    gc.collect()
    graph, out = capture_step(step, warmup=1, stream=s)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    got = [out[0], out[1]] + [p.grad for p in net.parameters() if p.grad is not None]
    assert len(got) == len(eager) and len(got) >= 3
    for a, b in zip(got, eager):
        assert torch.equal(a, b)
    assert torch.isfinite(eager[1]).all() and (eager[1] > 0).all()
