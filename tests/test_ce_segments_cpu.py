"""CPU checks of the segmented cross entropy: are the cases of tests/ce_segment_cases.py sound (against float64, with the bounds
of tests/ce_cases.py), do the entry points exist in the built library and refuse bad arguments, and do the Python entry points
refuse what they document - all before any launch."""
import ctypes as C
import math
import os

import pytest
import torch

import ce_cases as CC
import ce_segment_cases as SC


@pytest.fixture(scope="module")
def lib():
    from scaleprotoseg_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        from scaleprotoseg_amd.build import build

        build()
    return _lib.load()


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def test_cases_hold_what_they_say():
    kinds = set()
    for name in SC.CASE_NAMES:
        c = SC.case(name)
        assert c.logits.shape == (sum(c.sizes), c.K) and c.labels.shape == (sum(c.sizes),) and c.labels.dtype == torch.int32
        assert 1 <= c.S <= SC.MAX_SEGMENTS and all(n >= 1 for n in c.sizes) and c.offsets[-1] == c.logits.shape[0]
        for k, _, lab in c.slices():
            has_valid = bool(((lab >= 0) & (lab < c.K)).any())
            assert has_valid == (k != c.nan_segment), (name, k)
        for o in c.offsets[1:-1]:
            kinds.add(("wave", o % 64 == 0))
            kinds.add(("block", o % 256 == 0))
    assert kinds == {("wave", True), ("wave", False), ("block", True), ("block", False)}
    assert {SC.case(n).K for n in SC.CASE_NAMES} == {1, 4, 21, 33}
    assert SC.case("mixed5_k21").sizes == (63, 1, 257, 64, 320) and SC.case("one_row_k4").sizes == (1,)
    assert SC.case("two_blocks_k1").sizes == (256, 256) and SC.case("sixteen_k33").S == 16
    assert SC.case("pascal_k21").sizes == (3362, 882, 1922, 3362) and sum(SC.PASCAL_SIZES) == 9528
    nv = SC.case("no_valid_k4")
    assert nv.nan_segment == 2 and nv.sizes[2] == 257
    assert sum(1 for n in SC.CASE_NAMES if SC.case(n).S == 1) == 2
    g, gm = SC.upstream(16, 1)
    assert bool((g > 0).all()) and bool((g * 64 == (g * 64).round()).all()) and float(gm) == 1.75


@pytest.mark.parametrize("name", SC.CASE_NAMES)
def test_every_segment_against_float64(name):
    """Per slice: the float64 reference is torch's cross entropy, has a loss of at least 0.05 where it has one, and the kernels'
    formula restated in fp32 keeps a quarter of every bound of tests/ce_cases.py."""
    c = SC.case(name)
    refs = SC.references(name)
    for (k, lg, lab), ref in zip(c.slices(), refs):
        r32 = CC.restatement(lg, lab)
        tl = torch.where((lab.long() >= 0) & (lab.long() < c.K), lab.long(), torch.full_like(lab.long(), -1))
        want = torch.nn.functional.cross_entropy(lg.double(), tl, ignore_index=-1).item()
        assert CC.pred_mismatches(r32["pred"], ref) == 0 and r32["count"] == ref["count"] == int((tl >= 0).sum())
        rc = CC.reference(lg, lab, coef=r32["coef"])
        d, ignored = CC.dlogits_ratio(r32["d"], rc)
        ratios = {"lse": CC.lse_ratio(r32["lse"], ref), "d_logits": d}
        assert ignored == 0.0
        if k == c.nan_segment:
            assert math.isnan(ref["loss"]) and math.isnan(want) and math.isnan(r32["loss"]) and not r32["d"].any()
        elif c.zero_loss:
            assert ref["loss"] == 0.0 and r32["loss"] == 0.0
        else:
            assert abs(ref["loss"] - want) <= 1e-12 * max(1.0, abs(want))
            assert ref["loss"] >= CC.MIN_LOSS, (name, k, ref["loss"])
            ratios["loss"] = CC.loss_ratio(r32["loss"], ref)
        assert all(v <= CC.QUARTER for v in ratios.values()), (name, k, ratios)
    worst = max(r["count"] for r in refs)
    print(f"{name}: {c.S} segments, K = {c.K}, counts up to {worst}")


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def _table(offsets):
    from scaleprotoseg_amd import _lib

    seg = _lib.SpxCeSegments()
    seg.S = len(offsets) - 1
    for k, o in enumerate(offsets[:17]):
        seg.off[k] = o
    return seg


def test_entry_points_exist_and_refuse_bad_arguments(lib):
    from scaleprotoseg_amd import _lib

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spx_hip.h")).read()
    for name in ("spx_ce_seg_partials", "spx_ce_seg_fwd", "spx_ce_seg_finish", "spx_ce_seg_bwd"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name in header
    assert C.sizeof(_lib.SpxCeSegments) == 8 + 17 * 8 and _lib.SPX_CE_MAX_SEGMENTS == 16
    good = _table((0, 63, 64, 321, 385, 705))
    assert lib.spx_ce_seg_partials(C.byref(good)) == 4 * (1 + 1 + 2 + 1 + 2)
    assert lib.spx_ce_seg_partials(C.byref(_table((0, 256, 512)))) == 8
    assert lib.spx_ce_seg_partials(C.byref(_table((0, 1)))) == 4
    p = 4096                                                # any non-NULL address: every call below fails before a launch
    calls = {
        "spx_ce_seg_fwd": lambda s, **kw: lib.spx_ce_seg_fwd(kw.get("a", p), p, s, kw.get("K", 4), p, None, p, None),
        "spx_ce_seg_finish": lambda s, **kw: lib.spx_ce_seg_finish(kw.get("a", p), s, p, p, p, p, p, None),
        "spx_ce_seg_bwd": lambda s, **kw: lib.spx_ce_seg_bwd(kw.get("a", p), p, p, s, p, None, None, kw.get("K", 4), p, None),
    }
    bad_tables = {
        "1..16": [_table((0,)), _table(tuple(range(18)))],               # S = 0, S = 17
        "empty": [_table((0, 5, 5, 9))],
        "increasing": [_table((0, 9, 5, 12))],
        "off[0]": [_table((1, 5, 9))],
    }
    for who, call in calls.items():
        assert call(None) != 0 and b"NULL" in lib.spx_last_error() and who.encode() in lib.spx_last_error()
        assert call(C.byref(good), a=None) != 0 and b"NULL" in lib.spx_last_error()
        for word, tables in bad_tables.items():
            for t in tables:
                assert call(C.byref(t)) != 0, (who, word)
                assert word.encode() in lib.spx_last_error(), (who, word, lib.spx_last_error())
    for t in sum(bad_tables.values(), []):
        assert lib.spx_ce_seg_partials(C.byref(t)) == 0
    assert lib.spx_ce_seg_partials(None) == 0 and b"NULL" in lib.spx_last_error()
    assert calls["spx_ce_seg_fwd"](C.byref(good), K=0) != 0 and calls["spx_ce_seg_bwd"](C.byref(good), K=0) != 0
    assert lib.spx_ce_seg_finish(p, C.byref(good), p, None, p, p, p, None) != 0 and b"NULL" in lib.spx_last_error()


# ---- the Python entry points: refusals before any launch --------------------------------------------------------------------
def test_python_entry_points_refuse_before_any_launch(lib):
    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd.functional import ce_segment_table

    lg, lab = torch.zeros(10, 4), torch.zeros(10, dtype=torch.int32)
    with pytest.raises(spx.SpxError, match="no CPU fallback"):
        spx.segmented_cross_entropy(lg, lab, (0, 4, 10))
    t = ce_segment_table((0, 4, 10), 10)
    assert t.S == 2 and [t.off[k] for k in range(3)] == [0, 4, 10]
    for offs, word in (((0, 10, 10), "empty"), ((0, 7, 4, 10), "empty or out of order"), ((0, 4, 9), "0 to the 10"),
                       ((1, 10), "0 to the 10"), (tuple(range(18)), "17 segments"), ((0,), "0 segments")):
        with pytest.raises(spx.SpxError, match=word):
            ce_segment_table(offs, 10 if len(offs) < 18 else 17)
    ce = spx.SegmentedCrossEntropy(ignore_index=-1)
    seg = [torch.zeros(2, 3, 5, 4), torch.zeros(2, 2, 2, 4)]
    tg = [torch.zeros(2, 3, 5, dtype=torch.long), torch.zeros(2, 2, 2, dtype=torch.long)]
    with pytest.raises(spx.SpxError, match="no CPU fallback"):
        ce(seg, tg)
    with pytest.raises(spx.SpxError, match="1 target maps for 2"):
        ce(seg, tg[:1])
    with pytest.raises(spx.SpxError, match="18 segments"):
        ce(seg * 9, tg * 9)
    with pytest.raises(spx.SpxError, match="list"):
        ce(seg[0], tg[0])
