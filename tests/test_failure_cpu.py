"""Failure cases, CPU side: the NumPy restatement (tests/failure_restatement.py) against the fixture recorded from the
reference's own failure_cases.py and eval_test.py (tools/gen_failure_golden.py), the exported symbols, their argument validation
and the host-side checks of the Python surface.  No kernel runs here."""
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
import failure_restatement as FR  # noqa: E402
from failure_cases_data import CASES, activations_of, as_batch, net_tables  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "failure_cases.npz")
SYMBOLS = ("spx_predict_accumulate", "spx_failure_table", "spx_paired_range", "spx_paired_heat")


def test_fixture_holds_the_cases_of_the_issue():
    assert os.path.getsize(GOLDEN) <= 64 * 1024
    assert sorted(CASES) == ["group", "proto"] and {str(c["kind"]) for c in CASES.values()} == {"group", "proto"}
    for name, c in CASES.items():
        K = c["table"].shape[0]
        assert c["labels"].dtype == np.uint8 and c["labels"].max() <= K and (c["labels"] == 0).any()
        for key in ("logits", "distances", "activations", "head", "test_logits"):
            if key in c:
                t = torch.from_numpy(c[key])
                assert torch.equal(t.to(torch.bfloat16).float(), t), (name, key)
        conf = FR.confusion(FR.argmax_map(c["logits"], c["labels"].shape[1:]), c["labels"], K)
        _, _, fail = FR.failure_table(conf, float(c["threshold"]))
        for n, a in np.argwhere(fail):                                   # no ties, no failing class without a misprediction
            others = np.delete(conf[n, a], a)
            assert others.max() > 0 and (others == others.max()).sum() == 1
        present = sum(int((c["labels"][n] == k + 1).any()) for n in range(len(conf)) for k in range(K))
        assert 0 < len(c["cases"]) < present and len(set(c["cases"][:, 2])) > 1
        kind = str(c["kind"])
        rows, (H, W) = c[kind + "_rows"], c["labels"].shape[1:]
        Q = int(rows[:, 3].max()) + 1
        amb = FR.paired_ambiguous(activations_of(c), c["labels"], rows, Q)
        assert (amb.reshape(len(rows), -1).sum(1) <= 4 + H * W / 50).all()
        assert (Q == len(rows)) == (kind == "proto")
    assert CASES["group"]["group_flagged"].any() and (CASES["group"]["group_ranges"][:, 0] < 0).any()


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_the_reference_driven_fixture(name):
    c = CASES[name]
    kind, K, thr = str(c["kind"]), c["table"].shape[0], float(c["threshold"])
    k_star = FR.argmax_map(c["logits"], c["labels"].shape[1:])
    conf = FR.confusion(k_star, c["labels"], K)
    assert np.array_equal(conf.sum(0), FR.aggregate(k_star, c["labels"], K))
    iou, miss, fail = FR.failure_table(conf, thr)
    cases, rows = FR.cases_and_rows(fail, miss, c["table"], kind == "group")
    assert np.array_equal(cases, c["cases"]) and np.array_equal(rows, c[kind + "_rows"])
    assert [f"{iou[n, a]:.4f}" for n, a, _ in cases] == [str(s) for s in c["logged_iou"]]
    # the reference's own CLS_I and CLS_U: the counters and the float64 quotient are exact
    for (n, a, _), (I, U) in zip(cases, c["counts"]):
        assert conf[n, a, a] == I and conf[n, a].sum() + conf[n, :, a].sum() - conf[n, a, a] == U
        assert iou[n, a] == int(I) / int(U)
    planes, Q = activations_of(c), int(rows[:, 3].max()) + 1
    heat, ranges, flagged = FR.paired_heat(planes, c["labels"], rows, Q)
    amb = FR.paired_ambiguous(planes, c["labels"], rows, Q)
    assert np.array_equal(flagged, c[kind + "_flagged"])
    loose = flagged | amb
    diff = np.abs(heat.astype(np.int64) - c[kind + "_heat"])
    assert (diff[~loose] == 0).all() and (diff[amb & ~flagged] <= 1).all()
    m0 = FR.slot_margin(planes, rows, Q)
    assert (np.abs(ranges - c[kind + "_ranges"]).max(1) <= m0).all()


def test_restatement_of_the_label_maps_matches_eval_test():
    c = CASES["proto"]
    lut = c["test_lut"]
    assert lut.dtype == np.uint8 and lut.shape == (19,) and len(set(lut.tolist())) == 19 and lut.max() > 19      # the data set's own ids
    pred = FR.predict(c["test_logits"], c["test_pred"].shape[1:], lut)
    assert pred.dtype == np.uint8 and np.array_equal(pred, c["test_pred"])


def test_restatement_on_hand_made_counters():
    """What the fixture must not hold: ties (the lowest class), a failing class without a misprediction (-1), an absent class, a
    label outside 1..K counted in the union, and the strict comparison."""
    K = 4
    conf = np.zeros((2, K + 1, K), np.int64)
    conf[0, 0] = [1, 1, 0, 0]
    conf[0, 2] = [0, 3, 5, 3]
    conf[0, 3] = [0, 0, 0, 4]
    conf[0, 4] = [0, 0, 0, 10]
    iou, miss, fail = FR.failure_table(conf, 0.5)
    assert iou[0].tolist()[0] == 0.5 and fail[0].tolist() == [0, 0, 1, 1] and miss[0].tolist() == [1, -1, 1, -1]
    assert np.isnan(iou[0, 1]) and iou[0, 2] == 5 / 11 and iou[0, 3] == 4 / 17 and np.isnan(iou[1]).all() and not fail[1].any()
    assert FR.failure_table(conf, np.nextafter(0.5, 1.0))[2][0, 0] == 1
    table = np.array([[0, 1], [2, -1], [3, 4], [5, 6]])
    cases, rows = FR.cases_and_rows(fail, miss, table, shared=False)
    assert cases.tolist() == [[0, 2, 1]]                                            # the case without a miss has no rows
    assert rows.tolist() == [[0, 3, 2, 0], [0, 4, 2, 1], [0, 2, 2, 2]]
    assert FR.cases_and_rows(fail, miss, table, shared=True)[1].tolist() == [[0, 3, 2, 0], [0, 4, 2, 1], [0, 2, 2, 0]]
    assert len(FR.cases_and_rows(fail, miss, table, False, ignore_miss=1)[0]) == 0
    # a byte above 255 saturates, a dead slot gives zeros
    lab = np.array([[[1, 1, 0], [2, 1, 7]]], np.uint8)
    plane = np.array([[[[1.0, 3.0, 5.0], [7.0, 9.0, 11.0]], [[-4.0, -4.0, 0.0], [0.0, -4.0, 0.0]]]], np.float32)
    heat, ranges, flagged = FR.paired_heat(plane, lab, np.array([(0, 0, 0, 0), (0, 1, 0, 0), (0, 1, 0, 1)]), 2)
    assert ranges.tolist() == [[-4.0, 9.0], [-4.0, 0.0]]
    assert heat[0].tolist() == [[141, 198, 113], [113, 255, 113]] and flagged[0].tolist() == [[False, False, False], [False, True, False]]
    assert heat[1].tolist() == [[0, 0, 113], [113, 0, 113]] and not heat[2].any() and flagged[2].all()


def test_symbols_are_declared_bound_and_exported():
    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd import _lib, failures

    assert spx.FailureCases is failures.FailureCases and spx.predict_label_maps is failures.predict_label_maps
    assert spx.failure_table is failures.failure_table and spx.paired_heat_maps is failures.paired_heat_maps
    header = open(os.path.join(HERE, "..", "include", "spx_hip.h")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SIGNATURES and hasattr(lib, name), name
        declared = re.search(r"\bint %s\((.*?)\);" % name, header, re.S).group(1)
        assert len(declared.split(",")) == len(_lib.SIGNATURES[name][1]), name


def _st(*v):
    return (C.c_int64 * 4)(*v)


def test_c_entry_points_refuse_without_a_device():
    """NULL, sizes and K are refused on the host (the device pointers below are never dereferenced)."""
    from scaleprotoseg_amd import _lib

    lib = _lib.load()
    err = lambda: lib.spx_last_error().decode()

    def predict(**kw):
        a = dict(logits=16, st=_st(1000, 1, 100, 10), labels=16, lb=1, idm=None, N=1, K=3, h=5, w=7, H=33, W=41, pred=16, conf=16)
        a.update(kw)
        return lib.spx_predict_accumulate(*[a[k] for k in ("logits", "st", "labels", "lb", "idm", "N", "K", "h", "w", "H", "W", "pred", "conf")], None)

    for kw, msg in ((dict(logits=None), "NULL"), (dict(st=None), "NULL"), (dict(pred=None, conf=None), "NULL"), (dict(labels=None), "NULL labels"),
                    (dict(lb=2), "label byte code"), (dict(K=257), "at most 256"), (dict(K=0), "empty"), (dict(N=0), "empty"), (dict(H=0), "empty"),
                    (dict(N=64, H=8192, W=8192), "too large"), (dict(st=_st(1000, -1, 100, 10)), "negative"),
                    (dict(st=_st(0, 2 ** 30, 100, 10)), "2^31 elements")):
        assert predict(**kw) != 0, kw
        assert err().startswith("spx_predict_accumulate") and msg in err(), (kw, err())

    def table(**kw):
        a = dict(conf=16, N=2, K=3, thr=0.5, iou=16, miss=16, fail=16)
        a.update(kw)
        return lib.spx_failure_table(*[a[k] for k in ("conf", "N", "K", "thr", "iou", "miss", "fail")], None)

    for kw, msg in ((dict(conf=None), "NULL"), (dict(iou=None), "NULL"), (dict(miss=None), "NULL"), (dict(fail=None), "NULL"), (dict(N=0), "empty"),
                    (dict(K=0), "empty"), (dict(K=1025), "K <="), (dict(thr=float("nan")), "NaN")):
        assert table(**kw) != 0, kw
        assert err().startswith("spx_failure_table") and msg in err(), (kw, err())

    rows = lambda *v: (C.c_int32 * 8)(0, 1, 2, 0, *v)

    def paired(fn, extra, **kw):
        a = dict(planes=16, st=_st(1000, 100, 10, 1), labels=16, lb=1, rows=16, host=rows(0, 3, 2, 1), R=2, Q=2, N=1, C=4, h=5, w=7, H=33, W=41,
                 ws=16)
        a.update(kw)
        return fn(*[a[k] for k in ("planes", "st", "labels", "lb", "rows", "host", "R", "Q", "N", "C", "h", "w", "H", "W", "ws")], *extra, None)

    bad = ((dict(planes=None), "NULL"), (dict(st=None), "NULL"), (dict(labels=None), "NULL"), (dict(rows=None), "NULL"), (dict(host=None), "NULL"),
           (dict(ws=None), "NULL"), (dict(lb=3), "label byte code"), (dict(R=0), "rows"), (dict(R=65536), "rows"), (dict(Q=0), "range slots"),
           (dict(Q=3), "range slots"), (dict(N=0), "empty"), (dict(C=4097), "C <= 4096"), (dict(H=40000), "too large"), (dict(w=2000), "latent grid"),
           (dict(host=rows(1, 0, 0, 1)), "row 1"), (dict(host=rows(0, 4, 0, 1)), "row 1"), (dict(host=rows(0, 0, -1, 1)), "row 1"),
           (dict(host=rows(0, 0, 0, 2)), "row 1"), (dict(host=rows(0, 0, 0, -1)), "row 1"), (dict(host=rows(0, 3, 2, 0)), "no row names range slot 1"),
           (dict(host=rows(0, 3, 1, 0), Q=1), "shares slot 0"))
    for kw, msg in bad:
        assert paired(lib.spx_paired_range, (), **kw) != 0, kw
        assert err().startswith("spx_paired_range") and msg in err(), (kw, err())
        assert paired(lib.spx_paired_heat, (16, 16), **kw) != 0, kw
        assert err().startswith("spx_paired_heat") and msg in err(), (kw, err())
    assert paired(lib.spx_paired_heat, (None, 16)) != 0 and "NULL" in err()
    assert paired(lib.spx_paired_heat, (16, None)) != 0 and "NULL" in err()


def test_python_surface_refuses_on_the_host():
    """Wrong types and shapes, K > 256 and bad rows raise SpxError before anything needs a device; CPU tensors raise last."""
    import scaleprotoseg_amd as spx

    lg = torch.zeros(2, 5, 7, 3)
    lab = torch.zeros(2, 33, 41, dtype=torch.long)
    for call, msg in ((lambda: spx.predict_label_maps(lg.double(), (33, 41)), "fp32"), (lambda: spx.predict_label_maps(lg[0], (33, 41)), "fp32"),
                      (lambda: spx.predict_label_maps(torch.zeros(1, 2, 2, 257), (4, 4)), "257 classes"),
                      (lambda: spx.predict_label_maps(lg), "size"), (lambda: spx.predict_label_maps(lg, (0, 4)), "positive"),
                      (lambda: spx.predict_label_maps(lg, (33, 40), labels=lab), "is not the labels'"),
                      (lambda: spx.predict_label_maps(lg, labels=lab.float()), "labels must be uint8, int32 or int64"),
                      (lambda: spx.predict_label_maps(lg, labels=lab[:1]), "labels hold 1 images, logits 2"),
                      (lambda: spx.predict_label_maps(lg, (33, 41), want_pred=False), "need labels"),
                      (lambda: spx.predict_label_maps(lg, (33, 41), id_map=torch.zeros(3, dtype=torch.long)), r"id_map must be uint8 \[3\]"),
                      (lambda: spx.predict_label_maps(lg, (33, 41), id_map=torch.zeros(4, dtype=torch.uint8)), r"id_map must be uint8 \[3\]"),
                      (lambda: spx.predict_label_maps(lg, labels=lab, conf=torch.zeros(2, 3, 3, dtype=torch.long)), "conf must be"),
                      (lambda: spx.predict_label_maps(lg, (33, 41)), "no CPU fallback"),
                      (lambda: spx.predict_label_maps(lg, labels=lab), "no CPU fallback"),
                      (lambda: spx.failure_table(torch.zeros(2, 4, 4, dtype=torch.long), 0.5), r"int64 \[N, K\+1, K\]"),
                      (lambda: spx.failure_table(torch.zeros(2, 4, 3), 0.5), r"int64 \[N, K\+1, K\]"),
                      (lambda: spx.failure_table(torch.zeros(2, 4, 3, dtype=torch.long), float("nan")), "NaN"),
                      (lambda: spx.failure_table(torch.zeros(2, 4, 3, dtype=torch.long), 0.5), "no CPU fallback")):
        with pytest.raises(spx.SpxError, match=msg):
            call()
    act = torch.zeros(2, 8, 5, 7)
    ok = [[0, 1, 0, 0], [0, 2, 0, 0], [1, 3, 2, 1]]
    for rows, Q, msg in (([[2, 0, 0, 0]], 1, "row 0"), ([[0, 8, 0, 0]], 1, "row 0"), ([[0, 0, -1, 0]], 1, "row 0"), ([[0, 0, 0, 1]], 1, "row 0"),
                         ([[0, 0, 0, 0], [0, 0, 0, -1]], 1, "row 1"), ([[0, 0, 0, 0], [0, 1, 0, 2]], 3, "no row names range slot 1"),
                         ([[0, 0, 0, 0], [1, 1, 0, 0]], 1, "row 1 .*shares its range slot"), ([[0, 0, 0, 0], [0, 1, 1, 0]], 1, "row 1 .*shares"),
                         ([[0, 1, 0]], 1, r"\[R, 4\]"), ([[0.0, 1.0, 0.0, 0.0]], 1, "integer"), (torch.zeros(0, 4, dtype=torch.long), 1, "R >= 1"),
                         (ok, 0, "num_ranges")):
        with pytest.raises(spx.SpxError, match=msg):
            spx.paired_heat_maps(act, lab, rows, Q)
    with pytest.raises(spx.SpxError, match="fp32"):
        spx.paired_heat_maps(act.double(), lab, ok, 2)
    with pytest.raises(spx.SpxError, match="labels hold 3 images"):
        spx.paired_heat_maps(act, torch.zeros(3, 33, 41, dtype=torch.long), ok, 2)
    with pytest.raises(spx.SpxError, match="no CPU fallback"):                      # everything fits: only the device is missing
        spx.paired_heat_maps(act, lab, ok, 2)
    table = torch.tensor([[0, 1, 2], [3, 4, -1], [5, 6, 7]])
    with pytest.raises(spx.SpxError, match="257 classes"):
        spx.FailureCases(257, torch.zeros(257, 1, dtype=torch.long), 0.5)
    with pytest.raises(spx.SpxError, match=r"slot_table must be \[2, J\]"):
        spx.FailureCases(2, table, 0.5)
    fc = spx.FailureCases(3, table, 0.5)
    with pytest.raises(spx.SpxError, match=r"logits must be \[N, h, w, 3\]"):
        fc.update(torch.zeros(2, 5, 7, 4), lab)
    with pytest.raises(spx.SpxError, match="labels are required"):
        fc.heat_maps(ok, act)
    with pytest.raises(spx.SpxError, match="needs FailureCases.for_prototypes"):
        fc.heat_maps(ok, labels=lab, distances=act)
    with pytest.raises(spx.SpxError, match="no batch"):
        fc.compute()


@pytest.mark.parametrize("name", sorted(CASES))
def test_rows_for_orders_the_rows_as_the_reference_does(name):
    """From the restatement's table on the host, with the slot tables of a real module: the recorded triples and rows, and the
    Pascal rule."""
    import scaleprotoseg_amd as spx

    c = CASES[name]
    kind = str(c["kind"])
    net, make = net_tables(c)
    fc = make(spx.FailureCases, net, float(c["threshold"]))
    assert np.array_equal(fc.slot_table.numpy(), c["table"]) and fc.shared_ranges == (kind == "group")
    b = as_batch(c, spx.BatchFailures, FR)
    cases, rows = fc.rows_for(b)
    assert cases.dtype == rows.dtype == torch.int64 and not rows.is_cuda
    assert np.array_equal(cases.numpy(), c["cases"]) and np.array_equal(rows.numpy(), c[kind + "_rows"])
    drop = int(c["cases"][0, 2])
    kept, kept_rows = make(spx.FailureCases, net, float(c["threshold"]), ignore_miss=drop).rows_for(b)
    want = FR.cases_and_rows(b.fail.numpy(), b.miss.numpy(), c["table"], kind == "group", ignore_miss=drop)
    assert np.array_equal(kept.numpy(), want[0]) and np.array_equal(kept_rows.numpy(), want[1]) and 0 < len(kept) < len(cases)
    # a failing class without a misprediction is reported by the table and has no rows; no case at all gives empty tables
    miss = b.miss.clone()
    n, a = (int(v) for v in c["cases"][0, :2])
    miss[n, a] = -1
    fewer = fc.rows_for(b._replace(miss=miss))[0]
    assert np.array_equal(fewer.numpy(), c["cases"][1:])
    none = fc.rows_for(b._replace(fail=torch.zeros_like(b.fail)))
    assert tuple(none[0].shape) == (0, 3) and tuple(none[1].shape) == (0, 4)
