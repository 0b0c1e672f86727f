"""Push bounding boxes, CPU side: the NumPy restatement (tests/push_boxes_restatement.py) against the fixture recorded from the
reference's own update_prototypes_on_image / find_continuous_high_activation_crop (tools/gen_push_boxes_golden.py), the patch-box
arithmetic, the exported symbol and its argument validation.  No kernel runs here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import push_boxes_restatement as PB  # noqa: E402
from map_cases import PUSH_BOX_CASES as CASES, classes_of, planes_of  # noqa: E402


def test_fixture_holds_the_cases_of_the_issue():
    shapes = {(5, 7, 33, 50), (9, 11, 70, 85), (17, 17, 129, 129), (33, 65, 257, 513)}
    seen, feats = set(), set()
    for name, c in CASES.items():
        planes, lab = planes_of(c), c["labels"]
        h, w = planes.shape[2:]
        H, W = lab.shape[1:]
        P = planes.shape[1]
        assert c["ref_rf"].shape == c["ref_box"].shape == (P, 6) and c["ref_rf"].dtype == np.int64
        assert (c["ref_rf"] >= 0).all() and (c["ref_box"] >= 0).all()
        assert int((~c["robust"]).sum()) <= (0 if name.startswith("exact") else P // 8)
        if str(c["kind"]) == "log":
            seen.add((h, w, H, W))
            d = torch.from_numpy(c["distances"])
            assert torch.equal(d.to(torch.bfloat16).float(), d)
        cls = classes_of(c)
        for p in range(P):
            r, b = c["ref_rf"][p], c["ref_box"][p]
            feats |= {n for n, hit in (("top", b[1] == 0), ("bottom", b[2] == H), ("left", b[3] == 0), ("right", b[4] == W)) if hit}
            if c["flat"][p] == h * w - 1:
                assert r[2] > H and r[4] > W                                  # the patch box ends beyond the image
                feats.add("last")
            still = [max(r[1] - 5, 0), min(r[2] + 5, H - 1) + 1, max(r[3] - 5, 0), min(r[4] + 5, W - 1) + 1]
            absent = not (lab[c["img"][p]] == cls[p] + 1).any()
            if list(b[1:5]) == still:
                feats.add("no_growth")
            if absent and c["thresholds"][p] > 0:
                assert list(b[1:5]) == still
                feats.add("absent")
            if c["thresholds"][p] <= 0:
                feats.add("T<=0")
                assert planes[c["img"][p], p].max() < 0
    assert seen == shapes
    assert feats == {"top", "bottom", "left", "right", "last", "no_growth", "absent", "T<=0"}
    ex = CASES["exact_70x85"]
    a = planes_of(ex)
    assert a.shape[2:] == ex["labels"].shape[1:] and np.array_equal(a * 4, np.round(a * 4))
    assert sum(int((a[ex["img"][p], p] == ex["thresholds"][p]).sum()) for p in range(a.shape[1])) > 0     # ties under >=
    # crops really grow: at the two larger sizes by tens of pixels
    big = CASES["log_s33x65"]
    grow = (big["ref_box"][:, 2] - big["ref_box"][:, 1]) - (big["ref_rf"][:, 2] - big["ref_rf"][:, 1])
    assert (grow > 40).sum() >= 4


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_the_reference_driven_fixture(name):
    """Every row, robust or not: both walk the same float32 map with numpy's threshold."""
    c = CASES[name]
    planes, cls = planes_of(c), classes_of(c)
    for p in range(planes.shape[1]):
        n = int(c["img"][p])
        got = PB.boxes(planes[n, p], c["labels"][n], int(cls[p]), int(c["flat"][p]))
        assert [n, *got["rf"], cls[p]] == c["ref_rf"][p].tolist(), p
        assert [n, *got["box"], cls[p]] == c["ref_box"][p].tolist(), p
        assert got["threshold"] == c["thresholds"][p] and got["robust"] == bool(c["robust"][p])


def test_rf_arithmetic_on_odd_ratios():
    # 129 x 257 -> 1024 x 2048 (Cityscapes): ph = 7.937..., pw = 7.968...
    assert PB.rf_box(0, 129, 257, 1024, 2048) == [0, 8, 0, 8]
    assert PB.rf_box(128 * 257 + 256, 129, 257, 1024, 2048) == [1016, 1025, 2040, 2049]
    assert PB.rf_box(64 * 257 + 100, 129, 257, 1024, 2048) == [int(64 * (1024 / 129)), int(64 * (1024 / 129) + 1024 / 129) + 1,
                                                               int(100 * (2048 / 257)), int(100 * (2048 / 257) + 2048 / 257) + 1]
    # 5 x 7 -> 33 x 50: ph = 6.6, pw = 7.142857...
    assert PB.rf_box(0, 5, 7, 33, 50) == [0, 7, 0, 8]
    assert PB.rf_box(4 * 7 + 6, 5, 7, 33, 50) == [26, 34, 42, 51]
    assert PB.rf_box(2 * 7 + 3, 5, 7, 33, 50) == [13, 20, 21, 29]
    # the sum i * ph + ph is not (i + 1) * ph in float64: 3 x 3 -> 10 x 10 row 2: 2 * (10 / 3) + 10 / 3
    assert PB.rf_box(8, 3, 3, 10, 10) == [6, int(2 * (10 / 3) + 10 / 3) + 1, 6, int(2 * (10 / 3) + 10 / 3) + 1]
    # identity and downsampling
    assert PB.rf_box(70 * 85 - 1, 70, 85, 70, 85) == [69, 71, 84, 86]
    assert PB.rf_box(5, 4, 4, 2, 2) == [0, 2, 0, 2]


def test_walk_on_hand_made_maps():
    hit = np.zeros((20, 30), bool)
    hit[5:12, 8:20] = True
    assert PB.walk(hit, [8, 9, 10, 11], add_margin=0)[0] == (5, 12, 8, 20)
    assert PB.walk(hit, [8, 9, 10, 11], add_margin=5)[0] == (0, 17, 3, 25)
    assert PB.walk(np.zeros((20, 30), bool), [8, 9, 10, 11])[0] == (3, 15, 5, 17)
    assert PB.walk(np.ones((20, 30), bool), [8, 9, 10, 11])[0] == (0, 20, 0, 30)
    # sticky flags: the first pass finds nothing above (columns 10..11), stops there, and the later widening that would
    # expose the hit at column 14 of row 7 does not reopen it
    hit = np.zeros((20, 30), bool)
    hit[8:10, 10:16] = True
    hit[7, 14] = True
    assert PB.walk(hit, [8, 9, 10, 11], add_margin=0)[0] == (8, 10, 10, 16)
    # a patch box that ends beyond the image: the clipped segments, then the clip of the result
    hit = np.zeros((10, 10), bool)
    hit[4:, 6:] = True
    assert PB.walk(hit, [8, 11, 8, 11], add_margin=1)[0] == (3, 10, 5, 10)


def test_symbol_is_exported():
    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd import _lib, pushbox

    assert spx.push_bounding_boxes is pushbox.push_bounding_boxes
    lib = _lib.load()
    assert hasattr(lib, "spx_push_boxes") and "spx_push_boxes" in _lib.SIGNATURES
    assert lib.spx_version() == 17


def _call(lib, **kw):
    host = (C.c_int32 * 8)(0, 1, 2, 3, 0, 3, 0, 34)
    a = dict(planes=16, st=(C.c_int64 * 4)(1000, 100, 10, 1), labels=16, lb=1, rows=16, host=host, thr=16, R=2, N=1, C=4, h=5, w=7,
             H=33, W=50, margin=5, rf=16, box=16)
    a.update(kw)
    return lib.spx_push_boxes(a["planes"], a["st"], a["labels"], a["lb"], a["rows"], a["host"], a["thr"], a["R"], a["N"], a["C"],
                              a["h"], a["w"], a["H"], a["W"], a["margin"], a["rf"], a["box"], None)


def test_argument_validation_messages():
    """Every refusal happens on the host, before any launch (the device pointers above are never dereferenced)."""
    from scaleprotoseg_amd import _lib

    lib = _lib.load()
    err = lambda: lib.spx_last_error().decode()
    rows = lambda *v: (C.c_int32 * 8)(0, 1, 2, 3, *v)
    for kw, msg in ((dict(planes=None), "NULL"), (dict(st=None), "NULL"), (dict(labels=None), "NULL"), (dict(rows=None), "NULL"),
                    (dict(thr=None), "NULL"), (dict(rf=None), "NULL"), (dict(box=None), "NULL"), (dict(lb=2), "label byte code"),
                    (dict(R=0), "rows"), (dict(R=-3), "rows"), (dict(margin=-1), "add_margin"), (dict(C=4097), "C <= 4096"),
                    (dict(N=0), "empty"), (dict(H=65536, W=32768), "H*W < 2^31"), (dict(H=40000), "too large"),
                    (dict(w=2000), "latent grid"), (dict(st=(C.c_int64 * 4)(1000, -1, 10, 1)), "negative stride"),
                    (dict(st=(C.c_int64 * 4)(0, 2 ** 30, 10, 1)), "2^31 elements"),
                    (dict(host=rows(1, 0, 0, 0)), "row 1"), (dict(host=rows(-1, 0, 0, 0)), "row 1"),
                    (dict(host=rows(0, 4, 0, 0)), "row 1"), (dict(host=rows(0, -1, 0, 0)), "row 1"),
                    (dict(host=rows(0, 0, -1, 0)), "row 1"), (dict(host=rows(0, 0, 0, 35)), "row 1"),
                    (dict(host=rows(0, 0, 0, -1)), "row 1")):
        assert _call(lib, **kw) != 0, kw
        assert err().startswith("spx_push_boxes") and msg in err(), (kw, err())


def test_cpu_tensors_are_refused():
    import scaleprotoseg_amd as spx

    rows = torch.tensor([[0, 1, 2, 3]])
    with pytest.raises(spx.SpxError, match="no CPU fallback"):
        spx.push_bounding_boxes(torch.zeros(1, 2, 5, 7), torch.zeros(1, 33, 50, dtype=torch.long), rows)
    with pytest.raises(spx.SpxError, match="0 < q < 1"):
        spx.push_bounding_boxes(torch.zeros(1, 2, 5, 7), torch.zeros(1, 33, 50, dtype=torch.long), rows, q=1.0)
    with pytest.raises(spx.SpxError, match="fp32"):
        spx.push_bounding_boxes(torch.zeros(1, 2, 5, 7, dtype=torch.float64), torch.zeros(1, 33, 50, dtype=torch.long), rows)


def test_sharded_push_refuses_boxes(monkeypatch):
    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd import push

    class Net:
        num_classes = 2
        prototype_vectors = torch.zeros(2, 4, 1, 1)

        def eval(self):
            return self

    monkeypatch.setattr(push, "_dp_world", lambda group: (0, 2))
    with pytest.raises(spx.SpxError, match="sharded"):
        push.push_prototypes_multiscale([], Net(), boxes=True, log=lambda *_: None)
    with pytest.raises(spx.SpxError, match="sharded"):
        push.push_prototypes_multiscale([], Net(), proto_bound_boxes_filename_prefix="bb", log=lambda *_: None)
