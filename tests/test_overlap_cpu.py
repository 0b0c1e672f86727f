"""Activation-overlap metrics, CPU side: the float64 restatement (tests/overlap_restatement.py) against the fixture recorded
from the reference's own prototype_overlap / group_overlap (tools/gen_overlap_golden.py), the exported symbols, argument
validation, the workspace query and the float64 finalisation.  No kernel runs here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import overlap_restatement as R  # noqa: E402
from map_cases import OVERLAP_CASES as CASES, planes_of  # noqa: E402


def test_fixture_holds_the_cases_of_the_issue():
    shapes = {(5, 7, 33, 50), (9, 11, 70, 85), (17, 17, 129, 129), (33, 65, 257, 513)}
    seen = set()
    for name, c in CASES.items():
        if str(c["kind"]) == "proto":
            seen.add((tuple(c["distances"].shape[2:]) + tuple(c["labels"].shape[1:]), float(c["q"])))
            lab = c["labels"]
            assert lab.shape[0] == 2 and (lab == 0).any() and (lab > c["ident"].shape[1]).any()
            present = [set(np.unique(l)) for l in lab]
            assert present[0] != present[1]                                  # different class presence
            assert not (lab == 5).any()                                      # an absent class that owns prototypes
            per_class = c["ident"].sum(0)
            assert 1 in per_class and 0 in per_class                         # a class with one slot, a class with none
            assert np.array_equal(c["distances"][:, 2], c["distances"][:, 0])  # a duplicated channel
            assert c["ref_inter"][0, 0, 2] == c["ref_union"][0, 0, 2] == c["area"][0, 0] > 0
    assert seen == {(s, q) for s in shapes for q in (0.95, 0.8)}
    ex = CASES["exact_70x85_q95"]
    assert ex["activations"].shape[2:] == ex["labels"].shape[1:]
    assert np.array_equal(ex["activations"] * 4, np.round(ex["activations"] * 4))
    assert (ex["activations"][:, 5] == ex["activations"][0, 5, 0, 0]).all()  # the constant plane


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_the_reference_driven_fixture(name):
    c = CASES[name]
    planes, q = planes_of(c), float(c["q"])
    got = R.overlap_counts(planes, c["labels"], c["table"], q)
    union = got["area"][:, :, None] + got["area"][:, None, :] - got["inter"]
    pair = c["ref_union"] > 0
    assert np.array_equal(got["inter"], c["ref_inter"])
    assert np.array_equal(union * pair, c["ref_union"])
    assert np.array_equal(got["area"], c["area"])
    used = ~np.isnan(got["thresholds"])
    assert used.any()
    for n, ch in zip(*np.nonzero(used)):
        assert abs(float(got["thresholds"][n, ch]) - float(c["thresholds"][n, ch])) <= R.margin(planes[n, ch])
    ci, total = R.finalize(got["inter"], got["area"], c["table"])
    assert total == int(c["ref_total_inter"]) / int(c["ref_total_union"])
    for k, v in ci.items():
        assert v == c["ref_inter"][k].sum() / c["ref_union"][k].sum()
    if not name.startswith("exact"):
        # correlated channels: independent masks would overlap by (1 - q) / (1 + q) = 0.026 (q = 0.95) or 0.11 (q = 0.8)
        assert 0.2 < total < 1.0


@pytest.mark.parametrize("name", sorted(n for n in CASES if not n.startswith("exact")))
def test_few_pixels_are_ambiguous(name):
    """A_c <= 4 + |mask_c| / 1000 with |mask_c| the plane's own mask at the recorded threshold: what lets the GPU counters be
    held to the fixture within A."""
    c = CASES[name]
    planes = planes_of(c)
    H, W = c["labels"].shape[1:]
    for n in range(planes.shape[0]):
        for ch in range(planes.shape[1]):
            mask = int((R.upsample(planes[n, ch], (H, W)).astype(np.float32) > c["thresholds"][n, ch]).sum())
            assert mask > 0 and c["ambiguous"][n, ch] <= 4 + mask / 1000, (n, ch, int(c["ambiguous"][n, ch]), mask)


def test_restatement_agrees_with_torch_bicubic():
    g = torch.Generator().manual_seed(3)
    a = torch.randn(1, 1, 9, 11, generator=g)
    t = torch.nn.functional.interpolate(a, size=(70, 85), mode="bicubic", align_corners=False)[0, 0].numpy()
    u = R.upsample(a[0, 0].numpy(), (70, 85))
    assert np.abs(u - t).max() <= R.margin(a.numpy())


def test_symbols_are_exported():
    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd import _lib, overlap

    for n in ("ActivationOverlap", "OverlapResult", "high_activation_threshold"):
        assert hasattr(spx, n) and getattr(spx, n) is getattr(overlap, n)
    lib = _lib.load()
    for n in ("spx_overlap_workspace_bytes", "spx_overlap_thresholds", "spx_overlap_accumulate"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert lib.spx_version() == 17


def test_workspace_does_not_depend_on_the_image_size():
    from scaleprotoseg_amd import _lib

    lib = _lib.load()
    base = lib.spx_overlap_workspace_bytes(1, 228, 19)
    assert base > 0
    assert lib.spx_overlap_workspace_bytes.argtypes == [C.c_int32] * 3          # no H, W to depend on
    assert lib.spx_overlap_workspace_bytes(2, 228, 19) > base
    assert lib.spx_overlap_workspace_bytes(1, 456, 19) > base
    assert lib.spx_overlap_workspace_bytes(2, 228, 19) - base == lib.spx_overlap_workspace_bytes(3, 228, 19) - lib.spx_overlap_workspace_bytes(2, 228, 19)
    assert lib.spx_overlap_workspace_bytes(1, 228, 1024) >= base
    assert lib.spx_overlap_workspace_bytes(1, 4097, 19) == 0 and b"C <= 4096" in lib.spx_last_error()
    assert lib.spx_overlap_workspace_bytes(1, 228, 1025) == 0 and b"K <= 1024" in lib.spx_last_error()


def _thr(lib, **kw):
    a = dict(planes=16, st=(C.c_int64 * 4)(1000, 100, 10, 1), N=1, C=4, h=5, w=7, H=33, W=50, k=10, gamma=0.5, ws=16, out=16)
    a.update(kw)
    return lib.spx_overlap_thresholds(a["planes"], a["st"], a["N"], a["C"], a["h"], a["w"], a["H"], a["W"], a["k"], a["gamma"],
                                      a["ws"], a["out"], None)


def _acc(lib, **kw):
    a = dict(planes=16, st=(C.c_int64 * 4)(1000, 100, 10, 1), thr=16, labels=16, lb=1, table=16, N=1, C=4, K=3, J=2, h=5, w=7,
             H=33, W=50, inter=16, area=16, images=16, ws=16)
    a.update(kw)
    return lib.spx_overlap_accumulate(a["planes"], a["st"], a["thr"], a["labels"], a["lb"], a["table"], a["N"], a["C"], a["K"],
                                      a["J"], a["h"], a["w"], a["H"], a["W"], a["inter"], a["area"], a["images"], a["ws"], None)


def test_argument_validation_messages():
    """Every refusal happens on the host, before any launch (the pointers above are never dereferenced)."""
    from scaleprotoseg_amd import _lib

    lib = _lib.load()
    err = lambda: lib.spx_last_error().decode()
    for kw, msg in ((dict(planes=None), "NULL"), (dict(ws=None), "NULL"), (dict(out=None), "NULL thresholds"),
                    (dict(C=4097), "C <= 4096"), (dict(C=0), "empty"), (dict(H=65536, W=32768), "H*W < 2^31"),
                    (dict(H=40000), "too large"), (dict(w=2000), "latent grid"), (dict(k=33 * 50 - 1), "0 < q < 1"),
                    (dict(k=-1), "0 < q < 1"), (dict(gamma=1.0), "0 < q < 1"), (dict(gamma=-0.1), "0 < q < 1"),
                    (dict(st=(C.c_int64 * 4)(1000, -1, 10, 1)), "negative stride"),
                    (dict(st=(C.c_int64 * 4)(0, 2 ** 30, 10, 1)), "2^31 elements")):
        assert _thr(lib, **kw) != 0, kw
        assert err().startswith("spx_overlap_thresholds") and msg in err(), (kw, err())
    for kw, msg in ((dict(thr=None), "NULL"), (dict(labels=None), "NULL"), (dict(table=None), "NULL"), (dict(inter=None), "NULL"),
                    (dict(area=None), "NULL"), (dict(images=None), "NULL"), (dict(ws=None), "NULL"), (dict(lb=2), "label byte code"),
                    (dict(J=33), "J <= 32"), (dict(J=0), "J <= 32"), (dict(K=1025), "K <= 1024"), (dict(C=4097), "C <= 4096"),
                    (dict(H=65536, W=32768), "H*W < 2^31")):
        assert _acc(lib, **kw) != 0, kw
        assert err().startswith("spx_overlap_accumulate") and msg in err(), (kw, err())


def test_cpu_tensors_are_refused():
    import scaleprotoseg_amd as spx

    with pytest.raises(spx.SpxError, match="no CPU fallback"):
        spx.high_activation_threshold(torch.zeros(1, 2, 5, 7), (33, 50))
    with pytest.raises(spx.SpxError, match="no CPU fallback"):
        spx.ActivationOverlap(3, torch.zeros(3, 2, dtype=torch.long), "cpu")
    with pytest.raises(spx.SpxError, match="0 < q < 1"):
        spx.high_activation_threshold(torch.zeros(1, 2, 5, 7), (33, 50), q=1.0)
    with pytest.raises(spx.SpxError, match="fp32"):
        spx.high_activation_threshold(torch.zeros(1, 2, 5, 7, dtype=torch.float64), (33, 50))


def test_compute_arithmetic_on_hand_made_counters():
    from scaleprotoseg_amd.overlap import finalize

    table = torch.tensor([[0, 1, 2], [3, 4, -1], [5, -1, -1], [-1, -1, -1]])
    area = torch.tensor([[10, 20, 30], [8, 8, 0], [7, 0, 0], [0, 0, 0]])
    inter = torch.zeros(4, 3, 3, dtype=torch.int64)
    inter[0, 0, 1], inter[0, 0, 2], inter[0, 1, 2] = 5, 0, 20
    inter[1, 0, 1] = 8
    res = finalize(inter, area, torch.tensor([2, 1, 1, 0]), table)
    u0 = (10 + 20 - 5) + (10 + 30 - 0) + (20 + 30 - 20)
    assert res.class_iou == {0: 25 / u0, 1: 1.0}                 # one slot / no slot: no pair, no entry
    assert res.total == (25 + 8) / (u0 + 8)
    assert res.images.tolist() == [2, 1, 1, 0] and res.inter.dtype == torch.int64
    empty = finalize(torch.zeros(4, 3, 3, dtype=torch.int64), torch.zeros(4, 3, dtype=torch.int64), torch.zeros(4), table)
    assert empty.class_iou == {} and np.isnan(empty.total)
    ci, total = R.finalize(inter.numpy(), area.numpy(), table.numpy())
    assert ci == res.class_iou and total == res.total
