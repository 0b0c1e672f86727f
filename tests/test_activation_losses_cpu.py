"""CPU checks of the activation losses (EntropySpatLoss, EntropySamplLoss, NormLoss, ActivationRegularizers): a torch restatement
of their definitions, held against the fixture recorded from the reference (tools/gen_activation_loss_golden.py), and the
package's refusal of anything but the GPU kernels.  The restatement is what the GPU tests hold the kernels against."""
import math

import pytest
import torch

from activation_loss_cases import CASES, TERMS, load_case, log_activation, restate, restate_term
from regularizer_cases import close


@pytest.mark.parametrize("name", CASES)
def test_fixture_preconditions(name):
    c = load_case(name)
    K = c["ident"].shape[1]
    t = c["target"]
    assert (t == 0).any() and (t == K + 1).any()
    assert any(int((t[b] == k + 1).sum()) == 1 for b in range(t.shape[0]) for k in range(K) if c["ident"][:, k].sum() > 0)
    for term in TERMS:
        assert torch.isfinite(c[term]).all() and torch.isfinite(c[f"d_{term}_act"]).all() and torch.isfinite(c[f"d_{term}_d"]).all()
    if name == "ties":
        assert int((c["d"] == 0).sum()) == 5 and (c["d"][c["d"] != 0] >= 0.01).all()


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("term", TERMS)
def test_fp32_restatement_equals_the_reference_fixture(name, term):
    c = load_case(name)
    d = c["d"].clone().requires_grad_(True)
    act = log_activation(d)
    act.retain_grad()
    v, n = restate_term(term, act, c["target"], c["ident"], c["ranges"])
    assert n > 0
    v.backward()
    assert close(v.detach(), c[term], 1e-5)
    assert close(act.grad, c[f"d_{term}_act"], 1e-5)
    assert close(d.grad, c[f"d_{term}_d"], 1e-5)


def test_linf_ties_share_the_gradient_evenly():
    c = load_case("ties")
    act = c["act"].clone().requires_grad_(True)
    v, _ = restate_term("linf", act, c["target"], c["ident"], c["ranges"])
    v.backward()
    tied = c["d"] == 0
    g = act.grad[tied]
    assert len(g) == 5 and (g > 0).all() and torch.equal(g, g[0].expand(5))
    col = int(torch.nonzero(tied.any(0)).flatten()[0])
    hw = c["target"][0].numel()
    seg = c["target"][0].reshape(-1) == 2                      # the tied pixels' segment: image 0 = the first hw rows
    assert tied[:hw, col].sum() == 5 and (tied[:hw, col] <= seg).all()
    assert (act.grad[:hw][seg & ~tied[:hw, col], col] == 0).all()


def test_a_single_prototype_scale_is_skipped():
    """One (class, scale) with a single prototype: the restatement stays finite and equals the mean over the other items."""
    g = torch.Generator().manual_seed(5)
    # class 0: scale 0 has ONE prototype (index 0), scale 1 two; class 1: two and two
    ident = torch.zeros(7, 2)
    ident[[0, 3, 4], 0] = 1
    ident[[1, 2, 5, 6], 1] = 1
    ranges = [(0, 3), (3, 7)]
    target = torch.randint(0, 3, (2, 4, 5), generator=g)
    act = torch.randn(2 * 20, 7, generator=g, dtype=torch.float64)
    vals, counts = restate(act, target, ident, ranges)
    assert torch.isfinite(vals["sampl"])
    lab = target.reshape(2, -1) - 1
    items = []
    for b in range(2):
        for c, groups in ((0, [[3, 4]]), (1, [[1, 2], [5, 6]])):
            m = lab[b] == c
            if m.sum() == 0:
                continue
            for cols in groups:
                p = torch.softmax(act.reshape(2, 20, 7)[b][m][:, cols], dim=1)
                items.append((-(p * p.log()).sum(1) / math.log(len(cols))).mean())
    assert counts["sampl"] == len(items) > 0
    assert abs(vals["sampl"].item() - torch.stack(items).mean().item()) <= 1e-12


def test_cpu_tensors_and_bad_norm_type_are_refused():
    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd.loss import ClassDistances, class_slot_table

    c = load_case("even")
    ident, ranges = c["ident"], {s: r for s, r in enumerate(c["ranges"])}
    mods = [spx.EntropySpatLoss(ident), spx.EntropySamplLoss(ident, 2, ranges), spx.NormLoss(ident, "l1"), spx.NormLoss(ident, "linf"),
            spx.ActivationRegularizers(ident, 2, ranges, ent_spat=1.0, ent_sampl=1.0, norm=1.0)]
    B = c["target"].shape[0]
    cd = ClassDistances(values=torch.zeros(B, 4, 63), labels=torch.zeros(B, 63, dtype=torch.int32), table=class_slot_table(ident), grid=(7, 9))
    for m in mods:
        with pytest.raises(spx.SpxError):
            m(c["act"], c["target"])
        with pytest.raises(spx.SpxError):
            m(cd, c["target"])
    for bad in ("l2", "", None):
        with pytest.raises(ValueError):
            spx.NormLoss(ident, bad)
        with pytest.raises(ValueError):
            spx.ActivationRegularizers(ident, 2, ranges, norm=1.0, norm_type=bad)


def test_new_symbols_are_exported_and_bound():
    import ctypes as C

    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd import _lib

    for name in ("EntropySpatLoss", "EntropySamplLoss", "NormLoss", "ActivationRegularizers"):
        assert hasattr(spx, name)
    lib = _lib.load()
    for name in ("spx_actloss_workspace_bytes", "spx_actloss_segment_max", "spx_actloss_segment_sums", "spx_actloss_finish",
                 "spx_actloss_backward"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.spx_version() == 17
    d = _lib.SpxActLoss()
    assert lib.spx_actloss_workspace_bytes(C.byref(d)) == 0 and b"NULL" in lib.spx_last_error()
    assert lib.spx_actloss_segment_max(None, None, None) != 0
    sid = (C.c_int32 * 8)(*([0] * 8))
    d.slot_scale = C.cast(sid, C.c_void_p)
    d.B, d.J, d.HW, d.W, d.K, d.mode, d.terms, d.norm_type = 2, 4, 63, 9, 2, 1, 7, 0
    assert lib.spx_actloss_workspace_bytes(C.byref(d)) == 4 * 16 * 8 + 216      # four 64-bit and three 32-bit tables of B*K*J, counts, one key; 8-byte padded
    d.J = 17
    assert lib.spx_actloss_workspace_bytes(C.byref(d)) == 0 and b"J <= 16" in lib.spx_last_error()
    d.J, d.mode = 4, 3
    assert lib.spx_actloss_workspace_bytes(C.byref(d)) == 0 and b"mode" in lib.spx_last_error()
