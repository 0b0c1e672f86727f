"""CPU checks of the part consistency / stability definition: tests/consistency_restatement.py against the rows and aggregates
that tools/gen_parts_golden.py recorded from the reference's own ``consistency.part_intersect`` (tests/golden/
part_consistency.npz), its labelling on hand-written masks, and the argument errors of scaleprotoseg_amd.parts, which need no GPU."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import consistency_restatement as CR  # noqa: E402

CASES = ("nonzero", "image", "explicit", "filtered")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(HERE, "golden", "part_consistency.npz")))


def case_args(fx, name):
    """(mode, explicit, include, skip_classes) of a recorded case."""
    mode = "image" if name == "image" else "nonzero"
    explicit = fx["explicit"] if name == "explicit" else None
    include = fx["include"].tolist() if name == "filtered" else None
    skip = tuple(fx["skip"].tolist()) if name == "filtered" else ()
    return mode, explicit, include, skip


@pytest.fixture(scope="module")
def restated(fx):
    out = {}
    for name in CASES:
        mode, explicit, include, skip = case_args(fx, name)
        out[name] = CR.presence(fx["activations"], fx["labels"], fx["parts"], fx["slot_table"], int(fx["max_parts"]), float(fx["q"]),
                                mode, explicit, include, skip)
    return out


@pytest.mark.parametrize("name", CASES)
def test_presence_rows_equal_the_reference(fx, restated, name):
    M, N = int(fx["max_parts"]), fx["labels"].shape[0]
    want_tab, want_valid = CR.rows_to_table(fx[f"rows__{name}"], fx["slot_table"], N, M)
    tab, valid = restated[name]
    assert tab.dtype == np.uint8 and np.array_equal(tab, want_tab)          # byte for byte: 255 = the reference's NaN
    # the reference returns no row for a class none of whose prototypes is kept: its flag cannot be read off the rows
    has_slot = CR.existing(fx["slot_table"], fx["activations"].shape[1], case_args(fx, name)[2]).any(1)
    assert np.array_equal(valid * has_slot[None], want_valid)
    assert int(valid.sum()) * fx["slot_table"].shape[1] >= len(fx[f"rows__{name}"]) > 0


def test_fixture_holds_the_cases_it_is_for(fx):
    M = int(fx["max_parts"])
    body = fx["rows__nonzero"][:, :M + 1]
    assert (body == 0).any() and (body == 1).any() and np.isnan(body).any() and np.isnan(body[:, 0]).all()
    assert (fx["rows__image"][:, :M + 1] == 0).any()                       # a class covers more than q of an image
    assert len(fx["rows__filtered"]) < len(fx["rows__nonzero"])
    assert (fx["labels"] > fx["slot_table"].shape[0]).any() and (fx["parts"] < 0).any() and fx["parts"].max() <= M


@pytest.mark.parametrize("name", CASES)
def test_aggregate_equals_pandas(fx, restated, name):
    _, _, include, _ = case_args(fx, name)
    table = fx["slot_table"]
    tab, valid = restated[name]
    ok = CR.existing(table, fx["activations"].shape[1], include)
    # two batches give what one gives
    agg = CR.consistency([tab[:2], tab[2:]], [valid[:2], valid[2:]], ok)
    mean, cons = fx[f"mean__{name}"], fx[f"cons__{name}"]
    assert int((agg["rows"] > 0).sum()) == len(cons)
    for r in range(len(cons)):
        k, c = int(mean[r, 0]), int(mean[r, 1])
        j = list(table[k]).index(c)
        assert np.array_equal(agg["mean"][k, j], mean[r, 2:], equal_nan=True)
        assert agg["is_consistent"][k, j] == cons[r]
    assert agg["score"] == float(fx[f"score__{name}"])


def test_labelling_on_hand_written_masks():
    diag = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], bool)
    assert CR.components(diag) == [(3, 3, 3)]                              # diagonal-only contact joins
    anti = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0]], bool)
    assert CR.components(anti) == [(3, 3, 3)]
    ring = np.zeros((7, 7), bool)
    ring[1:6, 1:6] = True
    ring[2:5, 2:5] = False
    ring[3, 3] = True                                                      # an island inside the ring, not touching it
    assert sorted(CR.components(ring)) == [(1, 3, 3), (16, 48, 48)]
    one = np.zeros((4, 5), bool)
    one[2, 4] = True
    assert CR.components(one) == [(1, 4, 2)]
    assert CR.components(np.zeros((3, 3), bool)) == []
    split = np.array([[1, 0, 1], [0, 0, 0], [1, 0, 1]], bool)
    assert len(CR.components(split)) == 4


def test_centroids_include_the_complement_and_round_half_to_even():
    b = np.zeros((4, 4), bool)
    b[0, 0:2] = True                                                       # x mean 0.5 -> 0 (half to even), y 0
    pts = CR.centroids(b)
    assert pts[0] == (0, 0) and len(pts) == 2
    rest = ~b
    ys, xs = np.nonzero(rest)
    assert pts[1] == (int(np.round(xs.mean())), int(np.round(ys.mean())))
    assert CR.centroids(np.ones((3, 3), bool)) == [(1, 1)]                 # the whole image: no complement


def test_source_index_is_the_float64_expression():
    assert CR.source_index(56, 7).tolist() == [int(min(np.floor(x * (1.0 / (56 / 7))), 6)) for x in range(56)]
    s = CR.source_index(53, 7)
    assert s[0] == 0 and s[-1] == 6 and (np.diff(s) >= 0).all()


def test_argument_errors_need_no_gpu():
    import scaleprotoseg_amd as spx

    act = torch.zeros(2, 6, 5, 7)
    lab = torch.zeros(2, 37, 53, dtype=torch.uint8)
    par = torch.zeros(2, 37, 53, dtype=torch.int32)
    table = torch.tensor([[0, 3], [1, 4], [2, 5]])
    for bad in (0, 255, -1):
        with pytest.raises(spx.SpxError, match="max_parts"):
            spx.part_presence(act, lab, par, table, bad)
        with pytest.raises(spx.SpxError, match="max_parts"):
            spx.part_components(lab, par, bad)
    for q in (0.0, 1.0, 1.5):
        with pytest.raises(spx.SpxError, match="quantile"):
            spx.part_presence(act, lab, par, table, 4, q=q)
    with pytest.raises(spx.SpxError, match="threshold must be"):
        spx.part_presence(act, lab, par, table, 4, threshold="median")
    with pytest.raises(spx.SpxError, match="parts must be"):
        spx.part_presence(act, lab, par[:, :36], table, 4)
    with pytest.raises(spx.SpxError, match="parts must be"):
        spx.part_presence(act, lab, par.float(), table, 4)
    with pytest.raises(spx.SpxError, match="labels hold"):
        spx.part_presence(act, lab[:1], par[:1], table, 4)
    with pytest.raises(spx.SpxError, match="fp32"):
        spx.part_presence(act.double(), lab, par, table, 4)
    with pytest.raises(spx.SpxError, match="thresholds must be"):
        spx.part_presence(act, lab, par, table, 4, thresholds=torch.zeros(5))
    with pytest.raises(spx.SpxError, match="skip_classes"):
        spx.part_presence(act, lab, par, table, 4, skip_classes=(3,))
    # well-formed CPU tensors: refused, not computed elsewhere
    with pytest.raises(spx.SpxError, match="no CPU fallback"):
        spx.part_presence(act, lab, par, table, 4)
    with pytest.raises(spx.SpxError, match="no CPU fallback"):
        spx.part_thresholds(act, lab, table)
    with pytest.raises(spx.SpxError, match="no CPU fallback"):
        spx.part_components(lab, par, 4)
    with pytest.raises(spx.SpxError, match="max_parts"):
        spx.PartConsistency(3, table, 300, "cuda")
    with pytest.raises(spx.SpxError, match="no CPU fallback"):
        spx.PartConsistency(3, table, 4, "cpu")
    with pytest.raises(spx.SpxError, match="no CPU fallback"):
        spx.PartStability(3, table, 4, "cpu")
