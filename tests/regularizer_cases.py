"""The weight-side regularisers' cases and checkers, shared by tests/test_regularizers_cpu.py and the GPU suites: the names of
the fixture cases (tests/golden/group_regularizers.npz, tools/gen_regularizer_golden.py), a torch restatement of
segmentation/model/loss.py:351-464 and the training modules' masked L1, the comparison rule, and the check of GroupRegularizers
against the float64 restatement."""
import numpy as np
import torch

CASES = ("city", "ragged", "raw", "raw_eps", "single")


def case_inputs(z, name):
    f = lambda k: z[f"{name}__{k}"]
    ident = torch.from_numpy(f("ident"))
    scales = {s: (int(a), int(b)) for s, (a, b) in enumerate(f("scales"))}
    return ident, scales, int(f("G")), float(f("eps")), f("w"), f("head_group"), f("head_proto")


def present_blocks(ident):
    return [(k, int(torch.count_nonzero(ident[:, k]))) for k in range(ident.shape[1]) if torch.count_nonzero(ident[:, k]) > 0]


def reference_spans(ident, scales, num_scales):
    """The reference's column walk (loss.py:366-390), restated: per present class, per scale, (prev, prev + count)."""
    out = []
    for k, _ in present_blocks(ident):
        prev, row = 0, []
        for s in range(num_scales):
            lo, hi = scales[s]
            cnt = int(torch.count_nonzero(ident[lo:hi, k]))
            row.append((prev, prev + cnt))
            prev += cnt
        out.append(row)
    return out


def restate(ident, scales, G, eps, w_flat, head_group, head_proto, dtype=torch.float64):
    """Values and gradients of the three group terms (to the flat block-order weights) and the two L1s, by torch autograd
    of per-block loops written from the reference's definitions.  ``eps`` is taken in fp32 as the fp32 reference uses it."""
    eps = float(np.float32(eps))
    blocks = present_blocks(ident)
    w = torch.tensor(np.asarray(w_flat), dtype=dtype).requires_grad_(True)
    parts, off = [], 0
    for _, n in blocks:
        parts.append(w[off:off + G * n].view(G, n))
        off += G * n
    ent = torch.stack([-(b[g] * torch.log(b[g] + eps)).sum() / torch.log(torch.tensor(float(b.shape[1]), dtype=dtype))
                       for b in parts for g in range(G)]).mean()
    ceg = -torch.stack([-(b[i] * torch.log(torch.clamp(b[l], eps))).sum() for b in parts for i in range(G) for l in range(G)
                        if i != l]).mean()
    spans = reference_spans(ident, scales, len(scales))
    sm = -torch.stack([b[:, c0:c1].max(dim=1).values.mean() for b, row in zip(parts, spans) for c0, c1 in row if c1 > c0]).mean()
    out = {}
    for key, v in (("ent", ent), ("ceg", ceg), ("sm", sm)):
        (d,) = torch.autograd.grad(v, [w], retain_graph=True)
        out[key], out["d_" + key] = v.detach(), d
    U = G * len(blocks)
    gci = torch.zeros(U, ident.shape[1], dtype=dtype)
    for j, (k, _) in enumerate(blocks):
        gci[j * G:(j + 1) * G, k] = 1
    for key, W, I in (("l1_group", head_group, gci), ("l1_proto", head_proto, ident.to(dtype))):
        Wt = torch.tensor(np.asarray(W), dtype=dtype).requires_grad_(True)
        v = (Wt * (1 - I.t())).abs().sum()
        (d,) = torch.autograd.grad(v, [Wt])
        out[key], out["d_" + key] = v.detach(), d
    return out


def close(got, ref, rtol):
    """Same finiteness pattern (NaN where NaN, the same infinities) and |got - ref| <= rtol * max(1, |ref|) elsewhere."""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    fin = torch.isfinite(ref)
    if not torch.equal(torch.isfinite(got), fin) or not torch.equal(torch.isnan(got), torch.isnan(ref)):
        return False
    if not torch.equal(got[torch.isinf(ref)], ref[torch.isinf(ref)]):
        return False
    return bool(((got[fin] - ref[fin]).abs() <= rtol * ref[fin].abs().clamp_min(1.0)).all())


def flat_weights(net):
    return torch.cat([gp.weight.detach().reshape(-1) for gp in net.group_projection])


def flat_grads(net):
    return torch.cat([gp.weight.grad.reshape(-1) for gp in net.group_projection])


def zero_grads(net):
    for p in net.parameters():
        p.grad = None


def check_against_f64(net, reg, weights, eps):
    """GroupRegularizers' total, terms and gradients against the float64 restatement: values within 1e-6 max(1, |ref|),
    gradients within 1e-6 max|g|."""
    zero_grads(net)
    total, terms = reg()
    total.backward()
    torch.cuda.synchronize()
    ident = net.prototype_class_identity.cpu()
    hg = net.last_layer_group.weight.detach().cpu().numpy()
    r = restate(ident, net.scale_num_prototypes, net.num_groups, eps, flat_weights(net).cpu().numpy(), hg,
                np.zeros((ident.shape[1], ident.shape[0]), np.float32))
    ref_terms = [r["ent"], r["ceg"], r["sm"], r["l1_group"]]
    for i in range(4):
        assert close(terms[i].cpu(), ref_terms[i], 1e-6), (i, terms[i].item(), ref_terms[i].item())
    ref_total = ((weights[3] * ref_terms[3] + weights[1] * ref_terms[1]) + weights[2] * ref_terms[2]) + weights[0] * ref_terms[0]
    assert close(total.cpu(), ref_total, 1e-6), ("total", total.item(), ref_total.item())
    d_ref = sum(wt * r["d_" + k] for wt, k in zip(weights[:3], ("ent", "ceg", "sm")))
    d_got = flat_grads(net).cpu().double()
    assert (d_got - d_ref).abs().max() <= 1e-6 * d_ref.abs().max(), (d_got - d_ref).abs().max()
    dh_ref = weights[3] * r["d_l1_group"]
    dh = net.last_layer_group.weight.grad.cpu().double()
    assert (dh - dh_ref).abs().max() <= 1e-6 * dh_ref.abs().max(), (dh - dh_ref).abs().max()
