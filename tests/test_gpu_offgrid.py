"""GPU parity for inputs OFF the bf16 grid: unrounded fp32 features and bank (what a backbone emitting fp32 and an fp32 bank after
one optimizer step or one push hand the kernels), and bf16 features with an unrounded bank (autocast).

The contract (DESIGN.md 4 "operand sites", restated in float64 by tests/offgrid_restatement.py), with x~ = bf16_rne(x), p~ = bf16_rne(p):
  forward    every output equals the oracle at (x~, p~), within the on-grid tolerances of parity_cases.assert_fwd
  backward   dX and dPrototypes equal the per-site restatement (G at (x~, p~); 2 rs x with the caller's x, P^T G with p~, G^T X with
             x~, p colsum(G) with the fp32 p), head / grouping gradients float64 autograd at (x~, p~); GRAD_TOL / BF16_DX_TOL under
             grad_close's max-normalised measure
tests/test_offgrid_cpu.py shows on the CPU that the references this file tells apart lie further apart than these tolerances.
Every check prints its worst error / tolerance ratio before asserting (profiles/offgrid_summary.md records them)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import offgrid_restatement as R  # noqa: E402
from oracle import ppnet_oracle as O  # noqa: E402
from parity_cases import PUSH_FUSED_SHAPES, assert_fwd, bank_layout, dx_tolerance, gather_labels  # noqa: E402
from support import gpu_device, grad_close, GRAD_TOL, ListData, proto_net  # noqa: E402

pytestmark = pytest.mark.gpu

FP32 = [(c, torch.float32) for c in R.FP32_CASES]
BF16 = [(c, torch.bfloat16) for c in R.BF16_CASES]


def _id(v):
    return v if isinstance(v, str) else str(v).replace("torch.", "")


# (local: an off-grid case of offgrid_restatement with its oracle forward; parity_cases.problem draws on-grid inputs)
@functools.lru_cache(maxsize=None)
def _problem(case, x_dtype, signed=False):
    """(inputs, fp32 oracle forward at (x~, p~)): computed once, shared, never written to."""
    pb = R.build(case, x_dtype, signed=signed)
    return pb, R.forward_reference(pb)


@functools.lru_cache(maxsize=None)
def _restated(case, x_dtype):
    return R.restated_gradients(_problem(case, x_dtype)[0])


def _report(tag, **ratios):
    print(f"offgrid {tag}: " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))


def forward_ratios(logits, dist, act, ref_logits, ref_dist, ref_act):
    """Worst error / tolerance of each bound in assert_fwd."""
    out = {}
    if dist is not None:
        out["dist"] = R.distance_ratio(dist.detach().cpu(), ref_dist)
    if act is not None:
        out["act"] = ((act.detach().cpu() - ref_act).abs() / (2e-4 * (1 + ref_act.abs()))).max().item()
    if logits is not None:
        rl = ref_logits.reshape(-1, ref_logits.shape[-1])
        e = (logits.detach().cpu().reshape(rl.shape) - rl).abs()
        top = max(1.0, rl.abs().max().item())
        out["logits"] = e.max().item() / (1e-4 * top)
        out["logits_elem"] = (e / (1.1e-4 * (rl.abs() + 0.2 * top))).max().item()
    return out


def run_forward(pb, dev, **kw):
    from scaleprotoseg_amd.functional import proto_head_forward

    B, S, Cs, P, K, H, W = pb.shape
    out = proto_head_forward(pb.conv.to(dev, pb.x_dtype), pb.bank.to(dev), pb.Wl.to(dev), bank_layout(P, K, S, Cs, pb.ranges),
                             want_distances=True, want_activations=True, **kw)
    torch.cuda.synchronize()
    return out


def run_backward(pb, dev):
    """(dX, dP, dW) of the test loss through the kernels."""
    from scaleprotoseg_amd.functional import proto_head_forward

    B, S, Cs, P, K, H, W = pb.shape
    x = pb.conv.to(dev, pb.x_dtype).requires_grad_(True)
    pv = pb.bank.to(dev).requires_grad_(True)
    w = pb.Wl.to(dev).requires_grad_(True)
    logits, dist, act = proto_head_forward(x, pv, w, bank_layout(P, K, S, Cs, pb.ranges), want_distances=True, want_activations=True)
    ((logits * pb.g_logits.reshape(-1, K).to(dev)).sum() + (dist * pb.g_dist.to(dev)).sum() + (act * pb.g_act.to(dev)).sum()).backward()
    torch.cuda.synchronize()
    assert x.grad.dtype == pb.x_dtype and x.grad.shape == x.shape
    return x.grad, pv.grad, w.grad


@pytest.mark.parametrize("case,x_dtype", FP32 + BF16, ids=_id)
def test_forward_off_grid(case, x_dtype):
    dev = gpu_device()
    pb, (rl, rd, ra) = _problem(case, x_dtype)
    logits, dist, act = run_forward(pb, dev)
    _report(f"forward {case} {_id(x_dtype)}", **forward_ratios(logits, dist, act, rl, rd, ra))
    assert_fwd(logits, dist, act, rl, rd, ra)


def test_forward_off_grid_signed_features():
    """3 randn features against a randn bank: the kernels document no sign assumption (functional.proto_head_forward: "any
    bf16 / fp32 values are accepted") and take none."""
    dev = gpu_device()
    pb, (rl, rd, ra) = _problem("F1", torch.float32, True)
    assert (pb.conv < 0).any() and (pb.bank < 0).any() and pb.conv.abs().max() > 8
    logits, dist, act = run_forward(pb, dev)
    _report("forward F1 signed", **forward_ratios(logits, dist, act, rl, rd, ra))
    assert_fwd(logits, dist, act, rl, rd, ra)


@pytest.mark.parametrize("case,x_dtype", FP32 + BF16, ids=_id)
def test_backward_off_grid(case, x_dtype):
    dev = gpu_device()
    pb, _ = _problem(case, x_dtype)
    dx_ref, dp_ref, dw_ref = _restated(case, x_dtype)
    dx, dp, dw = run_backward(pb, dev)
    tol = dx_tolerance(x_dtype, pb.ranges)
    _report(f"backward {case} {_id(x_dtype)}", dX=R.max_normalised(dx.float().cpu(), dx_ref) / tol,
            dP=R.max_normalised(dp.cpu(), dp_ref) / GRAD_TOL, dW=R.max_normalised(dw.cpu(), dw_ref) / GRAD_TOL)
    grad_close(dx, dx_ref, "dX", tol=tol)
    grad_close(dp, dp_ref, "dPrototypes")
    grad_close(dw, dw_ref, "dLastLayer")


@pytest.mark.parametrize("case,x_dtype", [("F1", torch.float32), ("F3", torch.float32), ("F1", torch.bfloat16)], ids=_id)
def test_gathered_and_tail_off_grid(case, x_dtype):
    """The class-gathered planes and the fused grouping tail (spx_dist_fwd_cls / _group and their backwards) at (x~, p~), with
    the tolerances of test_random_gather_and_tail (group activations: test_fused_group_tail's); dX / dPrototypes against the
    per-site restatement of each loss, head / projection / grouping-head gradients against float64 autograd at (x~, p~)."""
    from scaleprotoseg_amd.functional import ClassGather, class_gather_table, proto_head_forward

    dev = gpu_device()
    pb, (rl, rd, _) = _problem(case, x_dtype)
    B, S, Cs, P, K, H, W = pb.shape
    ident, ranges = pb.ident, pb.ranges
    g = torch.Generator().manual_seed(41)
    g_logits = pb.g_logits
    dx_tol = dx_tolerance(x_dtype, ranges)
    tag = f"{case} {_id(x_dtype)}"

    # ---- class gather
    lay = bank_layout(P, K, S, Cs, ranges)
    lab0 = gather_labels(B, H, W, K, seed=5).reshape(B, -1) - 1
    keys, J, table = class_gather_table(lay, ident, dev)
    gather = ClassGather(labels=lab0.to(dev, torch.int32).contiguous(), keys=keys, width=J, table=table)
    g_cls = torch.randn(B, H * W, J, generator=g) * 1e-3
    cd_ref = O.gather_class_distances(rd, lab0, ident)
    w0 = pb.Wl.double().requires_grad_(True)

    def gather_loss(d):
        act = O.distance_2_similarity(d.permute(0, 2, 3, 1).reshape(-1, P))
        return (torch.nn.functional.linear(act, w0) * g_logits.double().reshape(-1, K)).sum() \
            + (O.gather_class_distances(d, lab0, ident) * g_cls.double()).sum()

    dx_ref, dp_ref, _ = R.restated_gradients(pb, loss_fn=gather_loss)
    x = pb.conv.to(dev, x_dtype).requires_grad_(True)
    pv = pb.bank.to(dev).requires_grad_(True)
    w = pb.Wl.to(dev).requires_grad_(True)
    logits, cd, _ = proto_head_forward(x, pv, w, lay, class_gather=gather)
    got = cd.detach().cpu().permute(0, 2, 1)
    ((logits * g_logits.reshape(-1, K).to(dev)).sum() + (cd * g_cls.permute(0, 2, 1).contiguous().to(dev)).sum()).backward()
    torch.cuda.synchronize()
    _report(f"gather {tag}", cls_dist=R.distance_ratio(got, cd_ref), **forward_ratios(logits, None, None, rl, None, None),
            dX=R.max_normalised(x.grad.float().cpu(), dx_ref) / dx_tol, dP=R.max_normalised(pv.grad.cpu(), dp_ref) / GRAD_TOL,
            dW=R.max_normalised(w.grad.cpu(), w0.grad) / GRAD_TOL)
    assert ((got - cd_ref).abs() <= 1e-4 * (1 + cd_ref)).all()
    assert (got[cd_ref == 0] == 0).all()
    assert_fwd(logits, None, None, rl, None, None)
    grad_close(x.grad, dx_ref, "dX (gather)", tol=dx_tol)
    grad_close(pv.grad, dp_ref, "dPrototypes (gather)")
    grad_close(w.grad, w0.grad, "dLastLayer (gather)")

    # ---- fused grouping tail
    G = 3
    idx = [i for i in O.class_prototype_index(ident) if len(i) > 0]
    gw = [O.projection_simplex_sort(torch.rand(G, len(i), generator=g)) for i in idx]
    U = G * len(idx)
    wg = torch.randn(K, U, generator=g) * 0.5
    gw0 = [t.double().requires_grad_(True) for t in gw]
    wg0 = wg.double().requires_grad_(True)

    def units_of(d, weights):
        act = O.distance_2_similarity(d).permute(0, 2, 3, 1).reshape(-1, P)
        return torch.cat(O.compute_group(act, ident, weights), dim=-1)

    def tail_loss(d):
        return (torch.nn.functional.linear(units_of(d, gw0), wg0) * g_logits.double().reshape(-1, K)).sum() + (d * pb.g_dist.double()).sum()

    dx_ref, dp_ref, _ = R.restated_gradients(pb, loss_fn=tail_loss)
    units_ref = units_of(rd, gw)                                      # fp32 oracle, as the on-grid tests
    l_ref = torch.nn.functional.linear(units_ref, wg)
    wd = torch.zeros(U, P)
    mask = torch.zeros(U, P, dtype=torch.bool)
    dwd_ref = torch.zeros(U, P, dtype=torch.float64)
    for k, i in enumerate(idx):
        wd[k * G:(k + 1) * G, i] = gw[k]
        mask[k * G:(k + 1) * G, i] = True
        dwd_ref[k * G:(k + 1) * G, i] = gw0[k].grad
    x = pb.conv.to(dev, x_dtype).requires_grad_(True)
    pv = pb.bank.to(dev).requires_grad_(True)
    wdd = wd.to(dev).requires_grad_(True)
    wgd = wg.to(dev).requires_grad_(True)
    logits, dist, _, gact = proto_head_forward(x, pv, wdd, bank_layout(P, U, S, Cs, ranges), group_tail=wgd)
    ((logits * g_logits.reshape(-1, K).to(dev)).sum() + (dist * pb.g_dist.to(dev)).sum()).backward()
    torch.cuda.synchronize()
    top = max(1.0, l_ref.abs().max().item())
    _report(f"tail {tag}", group_logits=(logits.detach().cpu() - l_ref).abs().max().item() / (1e-4 * top),
            group_act=((gact.detach().cpu() - units_ref).abs() / (2e-4 * (1 + units_ref.abs()))).max().item(),
            dist=R.distance_ratio(dist.detach().cpu(), rd), dX=R.max_normalised(x.grad.float().cpu(), dx_ref) / dx_tol,
            dP=R.max_normalised(pv.grad.cpu(), dp_ref) / GRAD_TOL, dWg=R.max_normalised(wgd.grad.cpu(), wg0.grad) / GRAD_TOL,
            dProj=R.max_normalised(wdd.grad.cpu() * mask, dwd_ref) / GRAD_TOL)
    assert (logits.detach().cpu() - l_ref).abs().max().item() <= 1e-4 * top
    assert ((gact.detach().cpu() - units_ref).abs() <= 2e-4 * (1 + units_ref.abs())).all()
    assert ((dist.detach().cpu() - rd).abs() <= 1e-4 * (1 + rd)).all()
    grad_close(x.grad, dx_ref, "dX (tail)", tol=dx_tol)
    grad_close(pv.grad, dp_ref, "dPrototypes (tail)")
    grad_close(wgd.grad, wg0.grad, "dLastLayerGroup")
    grad_close(wdd.grad.cpu() * mask, dwd_ref, "dGroupProjection")


def test_prototype_equal_to_an_off_grid_pixel():
    """After a push with fp32 features a prototype IS an unrounded latent pixel.  The three terms of |x|^2 - 2 x.p + |p|^2 then
    have to come from the same rounded values, or d sits near 2^-9 |x|^2 where it should be ~0 (and the activation falls from
    9.2 to about 3.5).  The argmin lands on the planted pixel, or on an EARLIER pixel with the same x~ (one is planted)."""
    from scaleprotoseg_amd.functional import proto_head_forward, push_masked_argmin

    dev = gpu_device()
    B, S, Cs, P, K, H, W = shape = (1, 4, 64, 228, 19, 12, 16)
    pb = R.build(shape, seed=4)
    conv, bank, ident, ranges = pb.conv.clone(), pb.bank.clone(), pb.ident, pb.ranges
    flat = conv.view(S, Cs, H * W)
    planted = {p: (p * 11) % (H * W) for p in range(0, P, 7)}              # 77 and 192 are coprime: 33 distinct pixels
    assert len(set(planted.values())) == len(planted) and min(planted.values()) == 0
    twin_p = max(planted, key=planted.get)                                 # its pixel gets a twin: same x~, other x, earlier
    twin_q = next(q for q in range(H * W) if q not in planted.values())
    assert twin_q < planted[twin_p]
    flat[:, :, twin_q] = R.bf16_rne(flat[:, :, planted[twin_p]])
    target = torch.randint(0, K + 1, (H * W,), generator=torch.Generator().manual_seed(8))
    for p, q in planted.items():
        bank[p, :, 0, 0] = flat[p // (P // S), :, q]
        target[q] = int(ident[p].argmax()) + 1
    target[twin_q] = target[planted[twin_p]]
    assert not torch.equal(R.bf16_rne(bank), bank) and not torch.equal(flat[:, :, twin_q], flat[:, :, planted[twin_p]])
    xt = R.bf16_rne(conv).view(S, Cs, H * W)

    _, dist, _ = proto_head_forward(conv.to(dev), bank.to(dev), None, bank_layout(P, 1, S, Cs, ranges))
    idx, val = push_masked_argmin(dist, target.view(1, H, W).to(dev), ident, void_class=0)
    dist, idx = dist.cpu().view(P, H * W), idx.cpu()
    ref = O.scale_l2_convolution(R.bf16_rne(conv), R.bf16_rne(bank), ranges, S).view(P, H * W)
    _report("planted pixel", d_at_pixel=max(dist[p, q].item() for p, q in planted.items()) / 1e-4, dist=R.distance_ratio(dist, ref))
    for p, q in planted.items():
        assert dist[p, q].item() <= 1e-4, (p, q, dist[p, q].item())
        s = p // (P // S)
        same = (xt[s] == xt[s][:, q:q + 1]).all(dim=0) & (target == target[q])
        allowed = [r for r in range(q + 1) if bool(same[r])]
        assert int(idx[0, p]) in allowed, (p, q, int(idx[0, p]), allowed)
        if p == twin_p:
            assert allowed == [twin_q, q]
    assert ((dist - ref).abs() <= 1e-4 * (1 + ref)).all()


def test_fused_push_minimum_off_grid():
    """test_fused_push_minimum_equals_the_two_step_push at its smallest shape, features and bank left unrounded: the fused
    minimum, the two-step path and the oracle's push on the written map agree bit for bit, distance ~0 at the copied pixel."""
    from scaleprotoseg_amd.functional import proto_head_forward, push_masked_argmin, push_min_from_features

    dev = gpu_device()
    B, S, Cs, P, K, H, W = shape = PUSH_FUSED_SHAPES[2]
    pb = R.build(shape, seed=31)
    conv, bank, ident, ranges = pb.conv.clone(), pb.bank.clone(), pb.ident, pb.ranges
    conv[:, :, 2:4, :] = conv[:, :, 0:2, :]                # repeated rows of pixels: exact ties along a prototype row
    cv = conv[0].view(S, Cs, H, W)
    p_sel = next(p for p in range(P // S) if int(ident[p].argmax()) != 2)
    bank[p_sel, :, 0, 0] = cv[0, :, 1, 2]                  # a pushed prototype: an UNROUNDED pixel, distance ~0 at (1, 2) and (3, 2)
    bank[p_sel + 2] = bank[p_sel + 1]
    assert not torch.equal(R.bf16_rne(conv), conv) and not torch.equal(R.bf16_rne(bank[p_sel]), bank[p_sel])
    g = torch.Generator().manual_seed(32)
    target = torch.randint(0, K + 1, (B, H, W), generator=g)
    target[target == 3] = 1                                # class 2 absent everywhere
    target[0, 1, 2] = target[0, 3, 2] = int(ident[p_sel].argmax()) + 1
    layout = bank_layout(P, 1, S, Cs, ranges)
    x = conv.to(dev)
    _, dist, _ = proto_head_forward(x, bank.to(dev), None, layout)
    idx2, val2 = push_masked_argmin(dist, target.to(dev), ident, void_class=0)
    idx, val = push_min_from_features(x, bank.to(dev), layout, target.to(dev), ident, void_class=0)
    ref = O.scale_l2_convolution(R.bf16_rne(conv), R.bf16_rne(bank), ranges, S)
    _report("fused push", dist=R.distance_ratio(dist.cpu(), ref), d_at_copy=val[0, p_sel].item() / 1e-4)
    np.testing.assert_array_equal(idx.cpu().numpy(), idx2.cpu().numpy())
    np.testing.assert_array_equal(val.cpu().numpy(), val2.cpu().numpy())
    ref_idx, ref_val = O.push_masked_argmin(dist.cpu(), target, ident, K, void_class=0)
    np.testing.assert_array_equal(idx.cpu().numpy(), ref_idx.numpy())
    np.testing.assert_array_equal(val.cpu().numpy(), ref_val.numpy())
    assert (ref_val == 1e10).any()
    assert val[0, p_sel].item() <= 1e-4 and int(idx[0, p_sel]) == 1 * W + 2
    assert ((dist.cpu() - ref).abs() <= 1e-4 * (1 + ref)).all()


def test_push_is_a_fixed_point_off_grid():
    """push_prototypes_multiscale twice on 3 in-memory images (F3-sized bank, 8 x 12 latent grid, unrounded fp32 features).
    After the first push every surviving prototype lies within 1e-4 of its source pixel; the second push leaves bf16(bank)
    bit-identical and drops nothing.  The fp32 bank itself may move to another pixel with the same x~ - an exact tie of the
    distances, broken towards the lowest image and flat index as everywhere: the tie rule, not an error."""
    from scaleprotoseg_amd.push import push_prototypes_multiscale

    dev = gpu_device()
    _, S, Cs, P, K, _, _ = R.CASES["F3"]
    # the pooling stand-in with a bare Sigmoid behind it: the module hands the kernels unrounded fp32 features
    net = proto_net(P, K, S, Cs, seed=5, backbone="pool", add_on=nn.Sequential(nn.Sigmoid()), device=dev)
    gen = torch.Generator().manual_seed(6)

    data = ListData()
    for _ in range(3):
        t = torch.randint(0, K + 1, (4, 6), generator=gen).repeat_interleave(8, 0).repeat_interleave(8, 1)
        data.append((torch.randn(3, 32, 48, generator=gen), t.numpy().astype(np.int64)))
    with torch.no_grad():
        feats = [net.conv_features(img.unsqueeze(0).to(dev)) for img, _ in data]
    assert tuple(feats[0].shape) == (1, S * Cs, 8, 12) and feats[0].dtype == torch.float32
    assert not torch.equal(R.bf16_rne(feats[0].cpu()), feats[0].cpu())

    best, tot_idx, dup = push_prototypes_multiscale(data, net, log=lambda *_: None)
    keep = [p for p in range(P) if p not in set(dup)]
    assert net.num_prototypes == len(keep) >= S * K
    bank1 = net.prototype_vectors.detach().cpu().clone()
    assert not torch.equal(R.bf16_rne(bank1), bank1)                                   # the bank holds unrounded pixels
    worst = 0.0
    with torch.no_grad():
        for j, p in enumerate(keep):
            i = int(best[p])
            _, dist = net.forward_from_conv_features(feats[i])
            d = dist.reshape(len(keep), -1)[j, int(tot_idx[i][0, p])].item()
            worst = max(worst, d)
    _report("push fixed point", d_at_source=worst / 1e-4)
    assert worst <= 1e-4
    _, _, dup2 = push_prototypes_multiscale(data, net, log=lambda *_: None)
    assert dup2 == [] and net.num_prototypes == len(keep)
    assert torch.equal(R.bf16_rne(net.prototype_vectors.detach().cpu()), R.bf16_rne(bank1))
