"""CPU checks of the weight-side regularisers (scaleprotoseg_amd/loss.py, csrc/spx_reg.hip): a torch restatement of
segmentation/model/loss.py:351-464 and the training modules' masked L1 against the fixture recorded from the reference's own
classes (tests/golden/group_regularizers.npz, tools/gen_regularizer_golden.py), the ScaleMax span tables of every group
config and of pruned layouts, and the refusal of CPU models (there is no CPU fallback)."""
import numpy as np
import pytest
import torch

from regularizer_cases import CASES, case_inputs, close, present_blocks, reference_spans, restate
from support import group_net


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


@pytest.mark.parametrize("P,K,S,prune", [(228, 19, 4, ()), (252, 21, 4, ()), (1800, 150, 4, ()), (2054, 182, 4, ()),
                                         (24, 2, 4, ()), (228, 19, 4, (0, 1, 2, 5, 60, 61, 62, 100, 227)),
                                         (2054, 182, 4, tuple(range(0, 2054, 7)))])
def test_span_tables(P, K, S, prune):
    from scaleprotoseg_amd.model_multiscale_group import group_scale_spans

    net = group_net(P, K, S, 16, 3)
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

    net = group_net(24, 2, 4, 16, 3)
    for make in (lambda: spx.EntropyGroup(net), lambda: spx.CrossEntropyGroup(net), lambda: spx.ScaleMax(net),
                 lambda: spx.GroupRegularizers(net, group_ent=0.05, l1=1e-3)):
        with pytest.raises(spx.SpxError):
            make()()
    with pytest.raises(spx.SpxError):
        spx.head_l1(net)


def test_regularizers_refuse_wrong_models():
    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd.model_multiscale import PPNetMultiScale

    proto = PPNetMultiScale(group_net(24, 2, 4, 16, 3).features, 64, (24, 16, 1, 1), [], 2, add_on_layers_type="deeplab_simple",
                            patch_classification=True, num_scales=4)
    with pytest.raises(spx.SpxError):
        spx.EntropyGroup(proto)
    with pytest.raises(spx.SpxError):
        spx.GroupRegularizers(proto, group_ent=0.05)
    with pytest.raises(spx.SpxError):
        spx.GroupRegularizers(proto, l1=1e-4)()                    # L1 only is allowed, but the weights are on the CPU
