"""CPU checks of the weight-side regularisers (scaleprotoseg_amd/loss.py, csrc/spx_reg.hip): a torch restatement of
segmentation/model/loss.py:351-464 and the training modules' masked L1 against the fixture recorded from the reference's own
classes (tests/golden/group_regularizers.npz, tools/gen_regularizer_golden.py), the ScaleMax span tables of every group
config and of pruned layouts, and the refusal of CPU models (there is no CPU fallback)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

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


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_reference_fixture(golden, name):
    z = golden("group_regularizers")
    ident, scales, G, eps, w, hg, hp = case_inputs(z, name)
    r = restate(ident, scales, G, eps, w, hg, hp, dtype=torch.float32)
    for key in ("ent", "ceg", "sm", "l1_group", "l1_proto"):
        assert close(r[key], z[f"{name}__{key}"], 1e-5), (name, key, r[key], z[f"{name}__{key}"])
        assert close(r["d_" + key], z[f"{name}__d_{key}"], 1e-5), (name, "d_" + key)


def test_fixture_covers_the_edge_cases(golden):
    z = golden("group_regularizers")
    assert np.isnan(z["single__ent"]) and not np.isfinite(z["single__d_ent"]).all()       # log(1) = 0, w < -eps
    w = z["raw__w"]
    assert ((w > 0) & (w < np.float32(1e-5))).any() and (w == np.float32(1e-5)).any()
    assert (z["city__w"] == 0).any()                                                       # simplex zeros: ScaleMax ties
    ident = torch.from_numpy(z["ragged__ident"])
    assert (ident.sum(0) == 0).any() and (ident.sum(1) == 0).any()                         # absent class, class-less rows


def _group_net(P, K, S, G=3, Cs=16):
    from scaleprotoseg_amd.model_multiscale_group import PPNetMultiScale as GroupNet

    class _Features(nn.Module):
        def __init__(self, ch):
            super().__init__()
            self.base = nn.Sequential(nn.Conv2d(3, ch, 1), nn.Conv2d(ch, ch, 1))

        def __str__(self):
            return "MSC(stand-in)"

    net = GroupNet(_Features(S * Cs), 64, (P, Cs, 1, 1), [], K, add_on_layers_type="deeplab_simple", patch_classification=True,
                   num_scales=S, num_groups=G)
    return net


@pytest.mark.parametrize("P,K,S,prune", [(228, 19, 4, ()), (252, 21, 4, ()), (1800, 150, 4, ()), (2054, 182, 4, ()),
                                         (24, 2, 4, ()), (228, 19, 4, (0, 1, 2, 5, 60, 61, 62, 100, 227)),
                                         (2054, 182, 4, tuple(range(0, 2054, 7)))])
def test_span_tables(P, K, S, prune):
    from scaleprotoseg_amd.model_multiscale_group import group_scale_spans

    net = _group_net(P, K, S)
    if prune:
        net.prune_prototypes(list(prune))
    ident, scales = net.prototype_class_identity, net.scale_num_prototypes
    info, spans, nspans = group_scale_spans(ident, scales, S, 3)
    ref = reference_spans(ident, scales, S)
    blocks = present_blocks(ident)
    assert spans.dtype == torch.int32 and info.shape == (len(blocks), 4) and spans.shape == (len(blocks), S, 2)
    assert spans.tolist() == [[list(p) for p in row] for row in ref]
    assert nspans == sum(c1 > c0 for row in ref for c0, c1 in row)
    off = 0
    for j, (k, n) in enumerate(blocks):
        assert info[j].tolist() == [off, n, 3 * j, 0]
        assert int(spans[j, -1, 1]) == n            # the spans cover the class's columns (no prototype outside the scales)
        off += 3 * n
    # the flat block order of the dense group tables (rows, cols) matches block_info
    rows, cols, U, _ = net._group_index(torch.device("cpu"))
    assert U == 3 * len(blocks) and rows.numel() == off
    for j, (k, n) in enumerate(blocks):
        o = int(info[j, 0])
        assert int(rows[o]) == 3 * j and torch.equal(ident[cols[o:o + n], k], torch.ones(n))


def test_regularizers_refuse_cpu_models():
    import scaleprotoseg_amd as spx

    net = _group_net(24, 2, 4)
    for make in (lambda: spx.EntropyGroup(net), lambda: spx.CrossEntropyGroup(net), lambda: spx.ScaleMax(net),
                 lambda: spx.GroupRegularizers(net, group_ent=0.05, l1=1e-3)):
        with pytest.raises(spx.SpxError):
            make()()
    with pytest.raises(spx.SpxError):
        spx.head_l1(net)


def test_regularizers_refuse_wrong_models():
    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd.model_multiscale import PPNetMultiScale

    proto = PPNetMultiScale(_group_net(24, 2, 4).features, 64, (24, 16, 1, 1), [], 2, add_on_layers_type="deeplab_simple",
                            patch_classification=True, num_scales=4)
    with pytest.raises(spx.SpxError):
        spx.EntropyGroup(proto)
    with pytest.raises(spx.SpxError):
        spx.GroupRegularizers(proto, group_ent=0.05)
    with pytest.raises(spx.SpxError):
        spx.GroupRegularizers(proto, l1=1e-4)()                    # L1 only is allowed, but the weights are on the CPU
