"""The weight-side regularisers on the MI355X (csrc/spx_reg.hip through scaleprotoseg_amd.loss): EntropyGroup,
CrossEntropyGroup, ScaleMax (segmentation/model/loss.py:351-464), the masked L1 of both heads and GroupRegularizers against
the reference's recorded values and gradients, a float64 restatement, the tie and clamp rules, determinism, the gradient
route through the forward's dense group matrix and graph capture."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from regularizer_cases import CASES, case_inputs, check_against_f64, close, flat_grads, flat_weights, restate, zero_grads
from support import gpu_device, group_net, proto_net

pytestmark = pytest.mark.gpu


def _group_net(P, K, S, G=3, seed=0):
    return group_net(P, K, S, 16, G, seed=seed, add_on=nn.Sequential())


def _net_from_case(z, name, dev):
    """A group net (and a prototype-phase net) carrying the fixture case's tables and weights."""
    ident, scales, G, eps, w, hg, hp = case_inputs(z, name)
    P, K = ident.shape
    S = len(scales)
    net = _group_net(P, K, S, G=G)
    net.prototype_class_identity = ident.clone()
    net.scale_num_prototypes = dict(scales)
    net._initialize_groups()
    net = net.to(dev)
    off = 0
    for gp in net.group_projection:
        n = gp.weight.numel()
        gp.weight.data.copy_(torch.from_numpy(w[off:off + n]).view_as(gp.weight))
        off += n
    net.last_layer_group.weight.data.copy_(torch.from_numpy(hg))
    proto = proto_net(P, K, S, 16, add_on=nn.Sequential())
    proto.prototype_class_identity = ident.clone()
    proto.scale_num_prototypes = dict(scales)
    proto = proto.to(dev)
    proto.last_layer.weight.data.copy_(torch.from_numpy(hp))
    return net, proto, eps


@pytest.mark.parametrize("name", CASES)
def test_terms_match_reference_fixture(golden, name):
    import scaleprotoseg_amd as spx

    dev = gpu_device(required=True)
    z = golden("group_regularizers")
    net, proto, eps = _net_from_case(z, name, dev)
    for key, mod in (("ent", spx.EntropyGroup(net, epsilon=eps)), ("ceg", spx.CrossEntropyGroup(net, epsilon=eps)),
                     ("sm", spx.ScaleMax(net))):
        zero_grads(net)
        v = mod()
        assert v.shape == () and v.is_cuda
        v.backward()
        assert close(v.cpu(), z[f"{name}__{key}"], 1e-5), (name, key, v.item(), z[f"{name}__{key}"])
        assert close(flat_grads(net).cpu(), z[f"{name}__d_{key}"], 1e-5), (name, "d_" + key)
    for key, m in (("l1_group", net), ("l1_proto", proto)):
        zero_grads(m)
        v = spx.head_l1(m)
        v.backward()
        W = m.last_layer_group.weight if key == "l1_group" else m.last_layer.weight
        assert close(v.cpu(), z[f"{name}__{key}"], 1e-5), (name, key)
        assert close(W.grad.cpu(), z[f"{name}__d_{key}"], 1e-5), (name, "d_" + key)


@pytest.mark.parametrize("P,K,prune,eps", [(228, 19, (), 1e-5), (252, 21, (), 1e-5), (1800, 150, (), 1e-5), (2054, 182, (), 1e-5),
                                           (24, 2, (), 1e-5), (228, 19, (0, 1, 2, 5, 60, 61, 62, 100, 227), 1e-5),
                                           (2054, 182, tuple(range(0, 2054, 7)), 1e-5), (228, 19, (), 1e-3)])
def test_group_regularizers_match_float64(P, K, prune, eps):
    import scaleprotoseg_amd as spx

    dev = gpu_device(required=True)
    net = _group_net(P, K, 4, seed=P + K)
    if prune:
        net.prune_prototypes(list(prune))
        net._initialize_weights()
    net = net.to(dev)
    g = torch.Generator().manual_seed(P)
    for gp in net.group_projection:            # simplex rows with a few raw entries (values in (0, eps) and above)
        w = gp.weight.data.cpu()
        m = torch.rand(w.shape, generator=g)
        w[m < 0.1] = 3e-6
        gp.weight.data.copy_(w)
    net.last_layer_group.weight.data.add_(0.01 * torch.randn(net.last_layer_group.weight.shape, generator=g).to(dev))
    weights = (0.25, 0.1, 0.3, 1e-3)
    reg = spx.GroupRegularizers(net, group_ent=weights[0], crs_ent_group=weights[1], scale_max=weights[2], l1=weights[3], epsilon=eps)
    check_against_f64(net, reg, weights, eps)


@pytest.mark.parametrize("P,K", [(228, 19), (1800, 150), (2054, 182)])
def test_prototype_head_l1_matches_float64(P, K):
    import scaleprotoseg_amd as spx

    dev = gpu_device(required=True)
    net = proto_net(P, K, 4, 16, add_on=nn.Sequential(), device=dev)
    g = torch.Generator().manual_seed(K)
    W = torch.randn(K, P, generator=g)
    W[torch.rand(K, P, generator=g) < 0.1] = 0.0
    net.last_layer.weight.data.copy_(W)
    reg = spx.GroupRegularizers(net, l1=1e-4)
    total, terms = reg()
    total.backward()
    m = 1 - net.prototype_class_identity.double().t()
    ref = (W.double() * m).abs().sum()
    assert abs(terms[3].item() - ref.item()) <= 1e-6 * max(1.0, ref.item())
    assert terms[:3].abs().sum().item() == 0
    assert abs(total.item() - 1e-4 * ref.item()) <= 1e-6 * max(1.0, 1e-4 * ref.item())
    dref = 1e-4 * torch.sign(W.double() * m) * m
    assert (net.last_layer.weight.grad.cpu().double() - dref).abs().max() <= 1e-6 * dref.abs().max()


def test_scale_max_gradient_goes_to_first_maximum_under_ties():
    import scaleprotoseg_amd as spx

    dev = gpu_device(required=True)
    net = _group_net(48, 4, 4).to(dev)          # 12 prototypes per class, 3 per scale: spans [0,3) [3,6) [6,9) [9,12)
    for gp in net.group_projection:
        w = torch.zeros(3, 12)
        w[0, 3:6] = 0.5                          # tie at columns 3, 4, 5
        w[1, 7] = 0.25
        w[1, 8] = 0.25                           # tie at 7, 8 (the zeros of the span tie elsewhere)
        gp.weight.data.copy_(w)
    sm = spx.ScaleMax(net)
    v = sm()
    v.backward()
    nspans = 4 * 4
    unit = np.float32(np.float32(-1.0) / np.float32(nspans)) / np.float32(3)
    for gp in net.group_projection:
        d = gp.weight.grad.cpu().numpy()
        expect = np.zeros((3, 12), np.float32)
        for g in range(3):
            for c0 in (0, 3, 6, 9):
                row = gp.weight.data.cpu().numpy()[g, c0:c0 + 3]
                expect[g, c0 + int(np.argmax(row))] = unit          # np.argmax: first maximal index
        assert np.array_equal(d, expect), (d, expect)


def test_cross_entropy_clamp_mask_at_epsilon():
    import scaleprotoseg_amd as spx

    dev = gpu_device(required=True)
    net = _group_net(48, 4, 4).to(dev)
    eps = float(np.float32(1e-5))
    for gp in net.group_projection:
        w = torch.full((3, 12), 0.05)
        w[1, 0] = eps                            # exactly eps: the clamp passes the gradient
        w[1, 1] = float(np.nextafter(np.float32(eps), np.float32(0)))      # just below: it does not
        w[2, 2] = 3e-6
        gp.weight.data.copy_(w)
    ceg = spx.CrossEntropyGroup(net, epsilon=1e-5)
    v = ceg()
    v.backward()
    r = restate(net.prototype_class_identity.cpu(), net.scale_num_prototypes, 3, 1e-5, flat_weights(net).cpu().numpy(),
                np.zeros((4, 12), np.float32), np.zeros((4, 48), np.float32), dtype=torch.float32)
    got = flat_grads(net).cpu()
    assert close(got, r["d_ceg"], 1e-5)
    # the element at eps gets the clamp term (q * w_other / eps, large); the one just below only its row-i terms
    assert got[12 + 0].abs() > 100 * got[12 + 1].abs()


def test_repeated_calls_are_bit_identical():
    import scaleprotoseg_amd as spx

    dev = gpu_device(required=True)
    net = _group_net(1800, 150, 4, seed=3).to(dev)
    reg = spx.GroupRegularizers(net, group_ent=0.25, crs_ent_group=0.1, scale_max=0.3, l1=1e-4)
    outs = []
    for _ in range(3):
        zero_grads(net)
        total, terms = reg()
        total.backward()
        outs.append((total.clone(), terms.clone(), flat_grads(net).clone(), net.last_layer_group.weight.grad.clone()))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert torch.equal(a, b)


def _group_step_inputs(net, dev, B=2, H=9, W=9, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, net.num_scales * 16, H, W, generator=g).to(dev)
    target = torch.randint(0, net.num_classes + 1, (B, H, W), generator=g).to(dev)
    return x, target


def test_gradients_through_logits_route_equal_standalone_terms():
    import scaleprotoseg_amd as spx

    dev = gpu_device(required=True)
    for P, K in ((228, 19), (1800, 150)):
        net = _group_net(P, K, 4, seed=K).to(dev)
        x, target = _group_step_inputs(net, dev, seed=K)
        wts = (0.25, 0.1, 0.3, 1e-3)
        reg = spx.GroupRegularizers(net, *wts)
        ce = spx.PixelWiseCrossEntropyLoss(ignore_index=-1)

        zero_grads(net)
        logits, _ = net.forward_from_conv_features(x, ce_target=target)
        total, _ = reg(logits)
        (ce(logits, target) + total).backward()
        fused = (flat_grads(net).clone(), net.last_layer_group.weight.grad.clone(), net.prototype_vectors.grad.clone())

        zero_grads(net)
        logits, _ = net.forward_from_conv_features(x, ce_target=target)
        terms = (spx.EntropyGroup(net)(), spx.CrossEntropyGroup(net)(), spx.ScaleMax(net)(), spx.head_l1(net))
        loss = ce(logits, target) + wts[3] * terms[3] + wts[1] * terms[1] + wts[2] * terms[2] + wts[0] * terms[0]
        loss.backward()
        alone = (flat_grads(net), net.last_layer_group.weight.grad, net.prototype_vectors.grad)
        for a, b in zip(fused, alone):
            assert (a - b).abs().max() <= 1e-6 * b.abs().max(), (P, (a - b).abs().max())


def test_captured_group_step_replays_eager_bit_for_bit():
    import gc

    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd.graphs import capture_step

    dev = gpu_device(required=True)
    net = _group_net(228, 19, 4, seed=7).to(dev)
    x, target = _group_step_inputs(net, dev, seed=7)
    reg = spx.GroupRegularizers(net, group_ent=0.05, crs_ent_group=0.0, scale_max=0.0, l1=1e-3)
    ce = spx.PixelWiseCrossEntropyLoss(ignore_index=-1)
    s = torch.cuda.Stream()

    def step():
        zero_grads(net)
        logits, _ = net.forward_from_conv_features(x, ce_target=target)
        total, terms = reg(logits)
        loss = ce(logits, target) + total
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
    assert len(got) == len(eager)
    for a, b in zip(got, eager):
        assert torch.equal(a, b)
    assert torch.isfinite(eager[1]).all() and eager[1][0] > 0


def test_regularizers_do_not_synchronise():
    import scaleprotoseg_amd as spx

    dev = gpu_device(required=True)
    net = _group_net(228, 19, 4, seed=9).to(dev)
    reg = spx.GroupRegularizers(net, group_ent=0.05, l1=1e-3)
    total, _ = reg()                        # build the caches (host work) first
    total.backward()
    torch.cuda.synchronize()
    mode_works = True
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            torch.zeros(1, device=dev).item()
            mode_works = False
        except RuntimeError:
            pass
        zero_grads(net)
        total, terms = reg()
        total.backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.isfinite(terms).all()
    print("sync debug mode effective:", mode_works)
