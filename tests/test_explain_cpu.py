"""Explanation maps, CPU side: the NumPy restatement (tests/explain_restatement.py) against the fixture recorded from the
reference's own plot_activation_proto / plot_activation_group (tools/gen_explain_golden.py), the exported symbols, their argument
validation and the host-side checks of the Python surface.  No kernel runs here."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import explain_restatement as E  # noqa: E402
from map_cases import EXPLAIN_CASES as CASES, class_planes, planes_of, weights_of  # noqa: E402
from support import EPS  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "explanation_maps.npz")
SYMBOLS = ("spx_explain_range", "spx_explain_heat", "spx_explain_dominant")


def test_fixture_holds_the_cases_of_the_issue():
    assert os.path.getsize(GOLDEN) <= max(os.path.getsize(os.path.join(HERE, "golden", f)) for f in os.listdir(os.path.join(HERE, "golden"))
                                          if f != "explanation_maps.npz")
    shapes = set()
    for name, c in CASES.items():
        planes, lab, table = planes_of(c), c["labels"], c["table"]
        N, _, h, w = planes.shape
        H, W = lab.shape[1:]
        shapes.add((h, w, H, W))
        assert (N, table.shape) == (2, (3, 3)) and lab.dtype == np.uint8
        assert (lab == table.shape[0] + 2).sum() == N                                  # one label outside 0..K per image
        present = {(n, k) for n in range(N) for k in range(3) if (lab[n] == k + 1).any()}
        assert len(present) == 5                                                       # one class is absent from one image
        assert {tuple(r) for r in c["dom_rows"]} == present
        assert [tuple(r) for r in c["heat_rows"]] == [(n, k, j) for n, k in sorted(present) for j in range(3) if table[k, j] >= 0]
        R, R2 = len(c["heat_rows"]), len(c["dom_rows"])
        assert c["heat"].shape == c["heat_ambiguous"].shape == (R, H, W) and c["heat"].dtype == np.uint8
        assert c["ranges"].shape == (R, 2) and c["ranges"].dtype == np.float32
        assert c["ref_argmax"].shape == c["dom_ambiguous"].shape == (R2, H, W) and c["ref_argmax"].dtype == np.uint8
        cap = 4 + H * W / 50
        assert (c["heat_ambiguous"].reshape(R, -1).sum(1) <= cap).all()
        assert (c["dom_ambiguous"].reshape(R2, -1).sum(1)[~c["tied"]] <= cap).all()
        t = torch.from_numpy(c["distances"] if str(c["kind"]) == "proto" else c["activations"])
        assert torch.equal(t.to(torch.bfloat16).float(), t)
        if str(c["kind"]) == "proto":
            assert (table == -1).sum() == 1 and not c["degenerate"].any()
        else:
            # the constant plane: hi == lo, all zeros
            flat = [i for i, (n, k, j) in enumerate(c["heat_rows"]) if (planes[n, table[k, j]] == 0).all()]
            assert flat and c["degenerate"].tolist() == [i in flat for i in range(R)]
            assert not c["heat"][flat].any() and (c["ranges"][flat] == 0).all()
            assert c["head"][0, 0] < 0 and (c["head"] != 1).all()
    assert shapes == {(5, 7, 33, 41), (3, 3, 17, 19)}
    assert {str(c["kind"]) for c in CASES.values()} == {"proto", "group"}
    tied = CASES["proto_3x3_17x19_tied"]
    assert tied["tied"].sum() == 2 and np.array_equal(tied["distances"][:, 7], tied["distances"][:, 5])
    rows = [i for i in range(len(tied["tied"])) if tied["tied"][i]]
    assert all(tied["dom_ambiguous"][i].sum() > 20 and not (tied["ref_argmax"][i] == 2).any() for i in rows)   # first maximum wins


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_the_reference_driven_fixture(name):
    """Exactly, every byte: the restatement is the arithmetic the reference ran on the same float32 maps."""
    c = CASES[name]
    planes, lab, table, wgt = planes_of(c), c["labels"], c["table"], weights_of(c)
    for i, (n, k, j) in enumerate(c["heat_rows"]):
        heat, lo, hi = E.heat_map(planes[n, table[k, j]], lab[n], k)
        assert heat.dtype == np.uint8 and np.array_equal(heat, c["heat"][i]), (name, i)
        assert (lo, hi) == tuple(c["ranges"][i]) and bool(hi == lo) == bool(c["degenerate"][i])
        assert np.array_equal(E.heat_ambiguous(planes[n, table[k, j]], lab[n], k), c["heat_ambiguous"][i])
    for i, (n, k) in enumerate(c["dom_rows"]):
        on = lab[n] == k + 1
        dom = E.dominant(class_planes(c, n, k), wgt[k], lab[n], k)
        assert np.array_equal(dom, np.where(on, c["ref_argmax"][i], E.OFF)), (name, i)
        amb, first, second = E.dominant_top2(class_planes(c, n, k), wgt[k], lab[n], k)
        assert np.array_equal(amb, c["dom_ambiguous"][i])
        clear = on & ~amb
        assert np.array_equal(first[clear], dom[clear])


def test_restatement_on_hand_made_maps():
    lab = np.array([[1, 1, 0], [2, 1, 7]], np.uint8)
    plane = np.array([[1.0, 3.0, 5.0], [7.0, 9.0, 11.0]], np.float32)            # identity resampling: u = the plane
    heat, lo, hi = E.heat_map(plane, lab, 0)
    assert (lo, hi) == (0.0, 9.0) and heat.tolist() == [[28, 85, 0], [0, 255, 0]]  # trunc(255 * 1 / 9), trunc(255 * 3 / 9)
    heat, lo, hi = E.heat_map(-plane, lab, 0)
    assert (lo, hi) == (-9.0, 0.0) and heat.tolist() == [[226, 170, 255], [255, 0, 255]]
    assert not E.heat_map(plane, lab, 2)[0].any() and not E.heat_map(0 * plane, lab, 0)[0].any()      # absent class, constant plane
    dom = E.dominant([plane, None, 10 - plane], [1.0, 1.0, 1.0], lab, 0)
    assert dom.tolist() == [[2, 2, 255], [255, 0, 255]]
    assert E.dominant([plane, None, 10 - plane], [1.0, 1.0, -1.0], lab, 0).tolist() == [[0, 0, 255], [255, 0, 255]]
    assert E.dominant([plane, plane, None], [1.0, 1.0, 1.0], lab, 0).tolist() == [[0, 0, 255], [255, 0, 255]]      # ties: the first
    assert (E.dominant([None, None], [1.0, 1.0], lab, 0) == 255).all()


def test_symbols_are_declared_bound_and_exported_at_abi_17():
    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd import _lib, explain

    assert spx.ExplanationMaps is explain.ExplanationMaps and spx.activation_heat_maps is explain.activation_heat_maps
    assert spx.dominant_slot_maps is explain.dominant_slot_maps
    header = open(os.path.join(HERE, "..", "include", "spx_hip.h")).read()
    assert int(re.search(r"#define SPX_ABI_VERSION (\d+)", header).group(1)) == 17 == _lib.ABI_VERSION
    lib = _lib.load()
    assert lib.spx_version() == 17
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SIGNATURES and hasattr(lib, name), name
        declared = re.search(r"\bint %s\((.*?)\);" % name, header, re.S).group(1)
        assert len(declared.split(",")) == len(_lib.SIGNATURES[name][1]), name


def _heat_args(**kw):
    a = dict(planes=16, st=(C.c_int64 * 4)(1000, 100, 10, 1), labels=16, lb=1, rows=16, host=(C.c_int32 * 6)(0, 1, 2, 0, 3, 0), R=2, N=1,
             C=4, h=5, w=7, H=33, W=41, ws=16)
    a.update(kw)
    return [a[k] for k in ("planes", "st", "labels", "lb", "rows", "host", "R", "N", "C", "h", "w", "H", "W", "ws")]


def _dom_args(**kw):
    a = dict(planes=16, st=(C.c_int64 * 4)(1000, 100, 10, 1), labels=16, lb=1, rows=16, host=(C.c_int32 * 4)(0, 1, 0, 2), table=16,
             wgt=None, R=2, N=1, C=4, K=3, J=3, h=5, w=7, H=33, W=41, dom=16)
    a.update(kw)
    return [a[k] for k in ("planes", "st", "labels", "lb", "rows", "host", "table", "wgt", "R", "N", "C", "K", "J", "h", "w", "H", "W", "dom")]


def test_argument_validation_messages():
    """Every refusal happens on the host, before any launch (the device pointers above are never dereferenced)."""
    from scaleprotoseg_amd import _lib

    lib = _lib.load()
    err = lambda: lib.spx_last_error().decode()
    rows = lambda *v: (C.c_int32 * 6)(0, 1, 2, *v)
    shared = ((dict(planes=None), "NULL"), (dict(st=None), "NULL"), (dict(labels=None), "NULL"), (dict(rows=None), "NULL"),
              (dict(host=None), "NULL"), (dict(lb=2), "label byte code"), (dict(R=0), "rows"), (dict(R=65536), "rows"),
              (dict(C=4097), "C <= 4096"), (dict(N=0), "empty"), (dict(H=65536, W=32768), "H*W < 2^31"), (dict(H=40000), "too large"),
              (dict(W=32769), "too large"), (dict(h=16385), "latent grid"), (dict(w=2000), "latent grid"),
              (dict(st=(C.c_int64 * 4)(1000, -1, 10, 1)), "negative stride"), (dict(st=(C.c_int64 * 4)(0, 2 ** 30, 10, 1)), "2^31 elements"))
    heat_only = ((dict(ws=None), "NULL"), (dict(host=rows(1, 0, 0)), "row 1"), (dict(host=rows(-1, 0, 0)), "row 1"),
                 (dict(host=rows(0, 4, 0)), "row 1"), (dict(host=rows(0, -1, 0)), "row 1"), (dict(host=rows(0, 0, -1)), "row 1"))
    for kw, msg in shared + heat_only:
        assert lib.spx_explain_range(*_heat_args(**kw), None) != 0, kw
        assert err().startswith("spx_explain_range") and msg in err(), (kw, err())
        assert lib.spx_explain_heat(*_heat_args(**kw), 16, 16, None) != 0, kw
        assert err().startswith("spx_explain_heat") and msg in err(), (kw, err())
    assert lib.spx_explain_heat(*_heat_args(), None, 16, None) != 0 and "NULL" in err()
    assert lib.spx_explain_heat(*_heat_args(), 16, None, None) != 0 and "NULL" in err()
    pair = lambda *v: (C.c_int32 * 4)(0, 1, *v)
    dom_only = ((dict(table=None), "NULL"), (dict(dom=None), "NULL"), (dict(J=33), "J <= 32"), (dict(J=0), "J <= 32"), (dict(K=0), "K <="),
                (dict(K=1025), "K <="), (dict(host=pair(1, 0)), "row 1"), (dict(host=pair(-1, 0)), "row 1"),
                (dict(host=pair(0, 3)), "row 1"), (dict(host=pair(0, -1)), "row 1"))
    for kw, msg in shared + dom_only:
        assert lib.spx_explain_dominant(*_dom_args(**kw), None) != 0, kw
        assert err().startswith("spx_explain_dominant") and msg in err(), (kw, err())


def test_python_surface_refuses_on_the_host():
    """Bad rows, too many slots, a wrong label type and mismatched N raise SpxError before anything needs a device."""
    import scaleprotoseg_amd as spx

    act = torch.zeros(2, 8, 5, 7)
    lab = torch.zeros(2, 33, 41, dtype=torch.long)
    table = torch.tensor([[0, 1, 2], [3, 4, -1], [5, 6, 7]])
    ok3, ok2 = [[0, 1, 1]], [[1, 2]]
    for rows, msg in (([[2, 0, 0]], "row 0"), ([[0, 0, 0], [-1, 0, 0]], "row 1"), ([[0, 3, 0]], "row 0"), ([[0, 0, 3]], "row 0"),
                      ([[0, 0, -1]], "row 0"), ([[0, 1, 2]], "no such slot"), ([[0, 1]], r"\[R, 3\]"), ([[0.0, 1.0, 1.0]], "integer"),
                      (torch.zeros(0, 3, dtype=torch.long), "R >= 1")):
        with pytest.raises(spx.SpxError, match=msg):
            spx.activation_heat_maps(act, lab, rows, table)
    for rows, msg in (([[2, 0]], "row 0"), ([[0, 0], [0, 3]], "row 1"), ([[0, -1]], "row 0"), ([[0, 1, 1]], r"\[R, 2\]")):
        with pytest.raises(spx.SpxError, match=msg):
            spx.dominant_slot_maps(act, lab, rows, table)
    wide = torch.arange(66).reshape(2, 33)
    with pytest.raises(spx.SpxError, match="at most 32"):
        spx.activation_heat_maps(torch.zeros(2, 66, 5, 7), lab, ok3, wide)
    with pytest.raises(spx.SpxError, match="at most 32"):
        spx.dominant_slot_maps(torch.zeros(2, 66, 5, 7), lab, ok2, wide)
    with pytest.raises(spx.SpxError, match="at most 32"):
        spx.ExplanationMaps(2, wide)
    for call, rows in ((spx.activation_heat_maps, ok3), (spx.dominant_slot_maps, ok2)):
        with pytest.raises(spx.SpxError, match="labels must be uint8, int32 or int64"):
            call(act, lab.to(torch.int16), rows, table)
        with pytest.raises(spx.SpxError, match="labels must be uint8, int32 or int64"):
            call(act, lab.float(), rows, table)
        with pytest.raises(spx.SpxError, match="labels hold 3 images, activations 2"):
            call(act, torch.zeros(3, 33, 41, dtype=torch.long), rows, table)
        with pytest.raises(spx.SpxError, match="fp32"):
            call(act.double(), lab, rows, table)
        with pytest.raises(spx.SpxError, match="names channel 7"):
            call(act[:, :7], lab, rows, table)
        with pytest.raises(spx.SpxError, match="no CPU fallback"):                 # everything fits: only the device is missing
            call(act, lab, rows, table)
    with pytest.raises(spx.SpxError, match=r"weights must be fp32 \[3, 3\]"):
        spx.dominant_slot_maps(act, lab, ok2, table, weights=torch.ones(3, 2))
    ex = spx.ExplanationMaps(3, table)
    with pytest.raises(spx.SpxError, match="labels are required"):
        ex.heat_maps(ok3, act)
    with pytest.raises(spx.SpxError, match="pass either"):
        ex.dominant_slots(ok2, labels=lab)
    with pytest.raises(spx.SpxError, match="needs ExplanationMaps.for_prototypes"):
        ex.heat_maps(ok3, labels=lab, distances=act)
    with pytest.raises(spx.SpxError, match="row 0"):
        ex.heat_maps([[0, 1, 2]], act, lab)


def _enumerate(lab, table):
    rows, rows2 = [], []
    for n in range(lab.shape[0]):
        for k in range(table.shape[0]):
            if (lab[n] == k + 1).any():
                slots = [j for j in range(table.shape[1]) if table[k, j] >= 0]
                rows += [(n, k, j) for j in slots]
                rows2 += [(n, k)] if slots else []
    return rows, rows2


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32, torch.int64])
def test_rows_for_against_an_enumeration(dtype):
    import scaleprotoseg_amd as spx

    table = np.array([[0, 1, 2], [3, 4, -1], [-1, -1, -1], [5, -1, 6]])              # a class without a slot, a hole
    ex = spx.ExplanationMaps(4, torch.from_numpy(table))
    g = np.random.default_rng(5)
    lab = g.integers(0, 7, (3, 9, 11))                                                # labels 5, 6: no class
    lab[1][lab[1] == 2] = 0                                                           # class 1 absent from image 1
    lab[2] = 0                                                                        # an image of void
    if dtype != torch.uint8:
        lab[0, 0, 0] = -3
    rows, rows2 = ex.rows_for(torch.from_numpy(lab).to(dtype))
    want, want2 = _enumerate(lab, table)
    assert rows.dtype == rows2.dtype == torch.int64 and not rows.is_cuda
    assert [tuple(r) for r in rows.tolist()] == want and [tuple(r) for r in rows2.tolist()] == want2
    assert want2 and all(k != 2 for _, k in want2) and (1, 1) not in want2
    for name, c in CASES.items():                                                     # the reference's own order of visits
        ex = spx.ExplanationMaps(3, torch.from_numpy(c["table"]))
        rows, rows2 = ex.rows_for(torch.from_numpy(c["labels"]).to(dtype))
        assert np.array_equal(rows.numpy(), c["heat_rows"]) and np.array_equal(rows2.numpy(), c["dom_rows"]), name


def test_model_constructors_on_the_host():
    import scaleprotoseg_amd as spx

    c = CASES["proto_5x7_33x41"]

    class Net:
        num_classes = 3
        prototype_class_identity = torch.from_numpy(c["ident"])
        distance_2_similarity = staticmethod(lambda d: torch.log((d + 1) / (d + EPS)))

    ex = spx.ExplanationMaps.for_prototypes(Net())
    assert np.array_equal(ex.slot_table.numpy(), c["table"]) and ex.num_slots == 3
