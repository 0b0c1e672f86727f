"""The group model on the packed MSC training maps (``PPNetMultiScaleGroup.forward_from_conv_features(PackedMaps)``,
``forward_packed``) with ``SegmentedCrossEntropy``, on the GPU:

1. the reference's own group-phase training step on four maps (tests/golden/msc_group_packed_step.npz,
   tools/gen_msc_group_packed_golden.py) with the tolerances of tests/test_gpu_modules.py's group step: group activations
   2e-4 (1 + |ref|), CE 1e-5, KLD 2e-4, ``grad_close`` / GRAD_TOL for every gradient, ``PAR.dx_tolerance`` for the maps, the
   counts exactly; the three tuple modes;
2. against the list path (one launch per contiguous segment): distances and activations bit-equal, group activations and
   logits within ``PAR.close_fwd`` with the equality printed;
3. the Pascal grids at B = 2 (M = 9 528, every boundary inside a tile) against the oracle at the pack's own bf16 values, on
   each of the three head branches (the module's width limits lowered for the test);
4. ``compute_group`` returns views of the one [M, U] tensor, ``GroupRegularizers(logits=...)`` per segment, ``forward_packed`` in
   train and in eval, the refusals, and the whole step inside ``graphs.capture_step``."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import msc_pack_cases as PC
import parity_cases as PAR
from oracle import ppnet_oracle as O
from support import GRAD_TOL, bits_equal, gpu_device, grad_close, group_net, load_cases, release_cached_blocks  # noqa: F401

import scaleprotoseg_amd as spx
import scaleprotoseg_amd.model_multiscale_group as MG

MODES = (dict(), dict(return_activations=True), dict(return_activations=True, return_distances=True))
FULL = MODES[2]


def _names(mode):
    return ("logits", "distances", "activations") if len(mode) == 2 else (("logits", "activations") if mode else ("logits", "distances"))


def _recorded():
    c = dict(load_cases("msc_group_packed_step")["step"])
    c["n"] = len(c["grids"])
    return c


def _recorded_net(c, dev):
    B, S, Cs, P, K, G = (int(v) for v in c["shape"])

    def init(net):
        net.prototype_vectors.copy_(torch.from_numpy(c["bank"]))
        for i, gp in enumerate(net.group_projection):
            gp.weight.copy_(torch.from_numpy(c[f"group_w_{i}"]))
        net.last_layer_group.weight.copy_(torch.from_numpy(c["last_layer_group"]))

    return group_net(P, K, S, Cs, G, init=init, device=dev)


# ---- 1. the recorded step ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_recorded_training_step(dtype):
    dev = gpu_device()
    c = _recorded()
    net = _recorded_net(c, dev)
    B, S, Cs, P, K, G = (int(v) for v in c["shape"])
    n = c["n"]
    leaves = [torch.from_numpy(c[f"conv{k}"]).to(dev).requires_grad_(True) for k in range(n)]
    pk = spx.msc_pack(leaves, "none", dtype, with_max=False)
    targets = [torch.from_numpy(c[f"target{k}"]).to(dev) for k in range(n)]
    outs = net.forward_from_conv_features(pk, **FULL)
    assert isinstance(outs, list) and len(outs) == n and all(len(o) == 3 for o in outs)
    kld_fn = spx.KLDLossGroup(net.prototype_class_identity, net.group_class_identity, G)
    ce = spx.SegmentedCrossEntropy(ignore_index=-1)([o[0] for o in outs], targets)
    assert torch.equal(ce.correct.cpu().long(), torch.from_numpy(c["n_correct"]))
    assert torch.equal(ce.valid.cpu().long(), torch.from_numpy(c["n_valid"]))
    rest = 0.0
    for k, (logits, dist, act) in enumerate(outs):
        PAR.close_fwd(logits, c[f"logits{k}"], "logits")
        PAR.close_fwd(dist, c[f"distances{k}"], "distances")
        PAR.close_fwd(act, c[f"activations{k}"], "activations")
        groups = net.compute_group(act)
        assert len(groups) == len(net.group_projection) and all(t.shape == (act.shape[0], G) for t in groups)
        ref_cat = torch.from_numpy(c[f"group_cat{k}"])
        assert ((torch.cat(groups, dim=-1).detach().cpu() - ref_cat).abs() <= 2e-4 * (1 + ref_cat.abs())).all(), k
        kld = kld_fn(list_group_activation=groups, target_labels=targets[k])
        want_ce, want_kld = float(c["ce"][k]), float(c["kld"][k])
        got_ce, got_kld = ce.losses[k].item(), kld.item()
        print(f"GROUPPACK {dtype} segment {k}: CE {got_ce:.7f} (reference {want_ce:.7f}), KLD {got_kld:.7f} "
              f"(reference {want_kld:.7f})")
        assert abs(got_ce - want_ce) <= 1e-5 * max(1.0, abs(want_ce))
        assert abs(got_kld - want_kld) <= 2e-4 * max(1.0, abs(want_kld))
        rest = rest + float(c["w_kld"]) * kld + (dist * torch.from_numpy(c[f"g_dist{k}"]).to(dev)).sum()
    loss = ce.mean + rest / n                                              # the mean over the segments (:300)
    want = float(c["loss"])
    assert abs(loss.item() - want) <= 2e-4 * max(1.0, abs(want))
    loss.backward()
    for k, leaf in enumerate(leaves):
        grad_close(leaf.grad, c[f"d_conv{k}"], f"dX map {k} {dtype}", tol=PAR.dx_tolerance(dtype), report="GROUPPACK")
    grad_close(net.prototype_vectors.grad, c["d_bank"], "dPrototypes", report="GROUPPACK")
    grad_close(net.last_layer_group.weight.grad, c["d_last_layer_group"], "dLastLayerGroup", report="GROUPPACK")
    scale = max(np.abs(c[f"d_group_w_{i}"]).max() for i in range(len(net.group_projection)))
    for i, gp in enumerate(net.group_projection):
        err = (gp.weight.grad.cpu() - torch.from_numpy(c[f"d_group_w_{i}"])).abs().max().item()
        assert err <= GRAD_TOL * scale, f"d group_projection[{i}]: {err:.3e} vs {scale:.3e}"


def test_tuple_modes_views_and_the_list_path():
    dev = gpu_device()
    c = _recorded()
    net = _recorded_net(c, dev)
    B, S, Cs, P, K, G = (int(v) for v in c["shape"])
    U = G * K
    pk = spx.msc_pack([torch.from_numpy(c[f"conv{k}"]).to(dev) for k in range(c["n"])], "none", torch.bfloat16, with_max=False)
    lay = pk.layout
    with torch.no_grad():
        for mode in MODES:
            out = net.forward_from_conv_features(pk, **mode)
            assert isinstance(out, list) and len(out) == c["n"]
            for k, o in enumerate(out):
                assert len(o) == len(_names(mode)), (mode, k)
                for t, kind in zip(o, _names(mode)):
                    PAR.close_fwd(t, c[f"{kind}{k}"], kind)
        packed = net.forward_from_conv_features(pk, **FULL)
        assert [tuple(o[0].shape) for o in packed] == [(B, h, w, K) for h, w in lay.grids]
        assert [o[1].stride() for o in packed] == [lay.view_strides(k) for k in range(c["n"])]      # views of ONE distance map
        # compute_group hands out views of the ONE [M, U] tensor the kernel wrote; run_last_layer is the segment's product
        g0 = packed[0][2].spx_group[2]
        for k, (logits, _, act) in enumerate(packed):
            ver, units, gk = act.spx_group
            assert ver == act._version and units is None and tuple(gk.shape) == (lay.sizes[k], U)
            assert gk.data_ptr() == g0.data_ptr() + 4 * U * lay.offsets[k]
            groups = net.compute_group(act)
            assert [t.data_ptr() for t in groups] == [gk.data_ptr() + 4 * G * j for j in range(len(groups))]
            PAR.close_fwd(net.run_last_layer(act).reshape(logits.shape), logits.cpu(), "logits")
            assert logits.spx_group_wd[1] is net and logits.spx_packed[2] == k and logits.spx_packed[1] is lay
        # the list path: one launch per contiguous segment
        eq = {"logits": True, "distances": True, "activations": True, "groups": True}
        for v, (l, d, a) in zip(pk.views(), packed):
            l1, d1, a1 = net.forward_from_conv_features(v.contiguous(), **FULL)
            gp, g1 = torch.cat(net.compute_group(a), dim=-1), torch.cat(net.compute_group(a1), dim=-1)
            PAR.close_fwd(l, l1.cpu(), "logits")
            PAR.close_fwd(gp, g1.cpu(), "activations")
            eq["logits"] &= bits_equal(l, l1)
            eq["distances"] &= bits_equal(d, d1)
            eq["activations"] &= bits_equal(a, a1)
            eq["groups"] &= bits_equal(gp, g1)
    print("GROUPPACK packed against list path: bit-equal " + ", ".join(f"{k} {v}" for k, v in eq.items()))
    assert eq["distances"] and eq["activations"]
    # GroupRegularizers per segment: the dense matrix of this very forward
    outs = net.forward_from_conv_features(pk)
    reg = spx.GroupRegularizers(net, group_ent=0.5, crs_ent_group=0.25, scale_max=0.125, l1=1e-3)
    plain_total, plain_terms = reg()
    for k, o in enumerate(outs):
        total, terms = reg(logits=o[0])
        assert bits_equal(total.detach(), plain_total.detach()) and bits_equal(terms.detach(), plain_terms.detach()), k
    wd = outs[2][0].spx_group_wd[0]
    assert all(o[0].spx_group_wd[0] is wd for o in outs)
    (total + outs[2][0].sum() * 1e-3).backward()
    assert all(gp.weight.grad is not None and bool(torch.isfinite(gp.weight.grad).all()) for gp in net.group_projection)


# ---- 3. the Pascal grids on the three head branches ---------------------------------------------------------------------------
def _coarse(shape, gen, scale=1e-3):
    return torch.round(torch.randn(shape, generator=gen) * scale * 2.0 ** 20) / 2.0 ** 20


def _weighted_loss(outs, ups, dev=None):
    move = (lambda t: t.to(dev)) if dev is not None else (lambda t: t)
    return sum(wk * ((l * move(gl)).sum() + (d * move(gd)).sum() + (a * move(ga)).sum())
               for wk, (l, d, a), (gl, gd, ga) in zip(PC.SEGMENT_WEIGHTS, outs, ups))


@pytest.mark.parametrize("branch", ["fused_tail", "wide_tail", "product_kernels"])
def test_pascal_grids_on_every_head_branch(branch, monkeypatch):
    dev = gpu_device()
    p = PC.PASCAL
    B, S, Cs, P, K, G = p["B"], p["S"], p["Cs"], p["P"], p["K"], 3
    if branch == "wide_tail":                                  # units in the distance kernel, the tail in the product kernel
        monkeypatch.setattr(MG, "MAX_FUSED_TAIL_CLASSES", K - 1)
    elif branch == "product_kernels":                          # both products on the activations (the ADE / COCO widths)
        monkeypatch.setattr(MG, "MAX_FUSED_HEAD_ROWS", G * K - 1)
    gen = torch.Generator().manual_seed(43)
    raw = [torch.randn(B, S * Cs, h, w, generator=gen).to(dev) for h, w in p["grids"]]
    bank = O.bf16_representable(torch.rand(P, Cs, 1, 1, generator=gen))
    torch.manual_seed(7)
    net = group_net(P, K, S, Cs, G, init=lambda n: n.prototype_vectors.copy_(bank), device=dev)
    with torch.no_grad():
        net.last_layer_group.weight.add_(0.05 * torch.randn(K, G * K, generator=gen).to(dev))
    pk = spx.msc_pack(raw, "sigmoid", torch.bfloat16)
    lay = pk.layout
    assert lay.M == 9528 and all(o % 128 for o in lay.offsets[1:])
    feats = pk.features.detach().requires_grad_(True)
    pk2 = spx.PackedMaps(features=feats, layout=lay, index=pk.index)
    # the oracle at every segment's own (bf16) feature values, one shared bank and head
    ident = net.prototype_class_identity.cpu()
    ranges = {s: tuple(net.scale_num_prototypes[s]) for s in range(S)}
    xs = [v.detach().float().cpu().contiguous().requires_grad_(True) for v in pk.views()]
    p0 = bank.clone().requires_grad_(True)
    gw = [gp.weight.detach().cpu().clone().requires_grad_(True) for gp in net.group_projection]
    wg = net.last_layer_group.weight.detach().cpu().clone().requires_grad_(True)
    want = [O.forward_from_conv_features(x, p0, ranges, S, None, class_identity=ident, group_weights=gw, last_layer_group_weight=wg)
            for x in xs]
    ups = [(_coarse((B, h, w, K), gen), _coarse((B, P, h, w), gen), _coarse((B * h * w, P), gen)) for h, w in lay.grids]
    _weighted_loss(want, ups).backward()
    outs = net.forward_from_conv_features(pk2, **FULL)
    # the fused tail leaves exp(units), the other two branches the units themselves
    assert all((o[2].spx_group[1] is None) == (branch == "fused_tail") and (o[2].spx_group[2] is None) == (branch != "fused_tail")
               for o in outs)
    for k, ((l, d, a), (rl, rd, ra)) in enumerate(zip(outs, want)):
        PAR.close_fwd(l, rl.detach(), "logits")
        PAR.close_fwd(d, rd.detach(), "distances")
        PAR.close_fwd(a, ra.detach(), "activations")
        rg = torch.cat(O.compute_group(ra.detach(), ident, [w.detach() for w in gw]), dim=-1)
        PAR.close_fwd(torch.cat(net.compute_group(a), dim=-1), rg, "activations")
    _weighted_loss(outs, ups, dev).backward()
    for k, x in enumerate(xs):
        grad_close(lay.view(feats.grad, k), x.grad, f"{branch} dX segment {k}", tol=PAR.dx_tolerance(torch.bfloat16), report="GROUPPACK")
    grad_close(net.prototype_vectors.grad, p0.grad, f"{branch} dPrototypes", report="GROUPPACK")
    grad_close(net.last_layer_group.weight.grad, wg.grad, f"{branch} dLastLayerGroup", report="GROUPPACK")
    scale = max(w.grad.abs().max().item() for w in gw)
    for i, gp in enumerate(net.group_projection):
        err = (gp.weight.grad.cpu() - gw[i].grad).abs().max().item()
        assert err <= GRAD_TOL * scale, f"{branch} d group_projection[{i}]: {err:.3e} vs {scale:.3e}"


# ---- 4. the module -----------------------------------------------------------------------------------------------------------
def _msc_net(dev, **kw):
    net = group_net(40, 5, 4, 16, 3, seed=11, device=dev, **kw)
    net.features = spx.MSC(net.features)                        # the stand-in backbone is the identity: the images ARE the features
    return net


def test_forward_packed_in_train_and_eval():
    dev = gpu_device()
    net = _msc_net(dev)
    x = torch.randn(2, 64, 13, 17, device=dev)
    with pytest.raises(spx.SpxError, match="fuse_feature_epilogue"):
        net.forward_packed(x)
    net.fuse_feature_epilogue(torch.bfloat16)
    with pytest.raises(spx.SpxError, match="packed=True"):
        net.fuse_feature_epilogue(torch.bfloat16, packed=True)          # the switch itself stays refused for this class
    with torch.no_grad():
        net.train()
        for mode in MODES:
            out, ref = net.forward_packed(x, **mode), net(x, **mode)
            assert isinstance(out, list) and len(out) == len(ref) == 4
            for o, r in zip(out, ref):
                assert len(o) == len(r)
                for t, u, kind in zip(o, r, _names(mode)):
                    assert t.shape == u.shape
                    PAR.close_fwd(t, u.cpu(), kind)
                    if kind != "logits":
                        assert bits_equal(t, u), kind
        assert [tuple(o[0].shape) for o in net.forward_packed(x)] == [(2, 13, 17, 5), (2, 6, 8, 5), (2, 9, 12, 5), (2, 13, 17, 5)]
        net.eval()
        for a, b in zip(net.forward_packed(x, **FULL), net(x, **FULL)):
            assert bits_equal(a, b)
        net.train()
        net.features.scales = []
        for a, b in zip(net.forward_packed(x, **FULL), net(x, **FULL)):
            assert bits_equal(a, b)


def test_refusals():
    dev = gpu_device()
    c = _recorded()
    net = _recorded_net(c, dev)
    pk = spx.msc_pack([torch.from_numpy(c[f"conv{k}"]).to(dev) for k in range(c["n"])], "none", torch.bfloat16, with_max=False)
    t = [torch.from_numpy(c[f"target{k}"]).to(dev) for k in range(c["n"])]
    with torch.no_grad():
        with pytest.raises(spx.SpxError, match="SegmentedCrossEntropy"):
            net.forward_from_conv_features(pk, ce_target=t)
        net.prototype_activation_function = lambda d: -d
        with pytest.raises(spx.SpxError, match="callable"):
            net.forward_from_conv_features(pk)
        net.prototype_activation_function = "log"
        B, S, Cs, P, K, G = (int(v) for v in c["shape"])
        headed = group_net(P, K, S, Cs, G, seed=3, device=dev, scale_head_type="sum")
        with pytest.raises(spx.SpxError, match="scale_head"):
            headed.forward_from_conv_features(pk)
        ce = spx.SegmentedCrossEntropy(ignore_index=-1)
        logits = [o[0] for o in net.forward_from_conv_features(pk)]
        with pytest.raises(spx.SpxError, match="target maps"):
            ce(logits, t[:3])
        with pytest.raises(spx.SpxError, match="targets\\[2\\]"):
            ce(logits, t[:2] + [t[2][:, 1:]] + t[3:])


def test_whole_step_inside_capture_step():
    from scaleprotoseg_amd.graphs import capture_step

    dev = gpu_device()
    c = _recorded()
    net = _recorded_net(c, dev)
    B, S, Cs, P, K, G = (int(v) for v in c["shape"])
    raw = [torch.zeros(B, S * Cs, h, w, device=dev).requires_grad_(True) for h, w in ((7, 9), (4, 5), (6, 7))]
    grids = ((7, 9), (4, 5), (6, 7), (7, 9))
    targets = [PAR.gather_labels(B, h, w, K, seed=80 + k).to(dev) for k, (h, w) in enumerate(grids)]
    params = [net.prototype_vectors, net.last_layer_group.weight] + [gp.weight for gp in net.group_projection]
    leaves = raw + params
    ce_fn = spx.SegmentedCrossEntropy(ignore_index=-1)
    kld_fn = spx.KLDLossGroup(net.prototype_class_identity, net.group_class_identity, G)
    s = torch.cuda.Stream()

    def step():
        for t in leaves:
            t.grad = None
        pk = spx.msc_pack(raw, "sigmoid", torch.bfloat16)
        outs = net.forward_from_conv_features(pk, **FULL)
        ce = ce_fn([o[0] for o in outs], targets)
        kld = sum(kld_fn(net.compute_group(o[2]), t) for o, t in zip(outs, targets))
        (ce.mean + 0.25 * kld / len(outs)).backward()
        return ce.losses.detach(), ce.mean.detach(), ce.valid, ce.correct, kld.detach()

    def refill(seed):
        gen = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for t in raw:
                t.copy_(torch.randn(t.shape, generator=gen))

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
    assert not bits_equal(eager[1][0], eager[2][0]) and int(eager[1][2].sum()) > 0
