"""predict_label_maps / failure_table / paired_heat_maps / FailureCases on the GPU against upsample_argext (itself pinned to
F.interpolate operation by operation), SegmentationMetrics, the NumPy restatement (tests/failure_restatement.py) and the fixture
recorded from the reference's own failure_cases.py and eval_test.py (tests/golden/failure_cases.npz).

Bounds.  Predictions, counters and the failure table are exact: integers, and a float64 quotient of two of them.  The heat maps
are bytes: the kernel's fp32 sample lies within m0 = 64 * 2^-23 * max|a| of the float64 restatement, so a byte can differ from
the restatement's only at the "ambiguous" pixels of failure_restatement (the float64 value 255 x within 255 (2 + x) m0 / hi of an
integer), and there by one; ``ranges`` are within m0; rows of a slot with hi <= 0 are all zeros."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import failure_restatement as FR  # noqa: E402
from failure_cases_data import CASES, activations_of, net_tables  # noqa: E402
from map_cases import EXPLAIN_CASES, band_edge_case, planes_of  # noqa: E402
from support import gpu_device  # noqa: E402
from support import release_cached_blocks  # noqa: E402,F401  (a module-scoped autouse fixture, taken by importing its name)

pytestmark = pytest.mark.gpu

LABEL_TYPES = [torch.uint8, torch.int32, torch.int64]
# 5x7 -> 37x53 (odd H*W), 3x2 -> 9x3 (a row is narrower than a dword), 6x20 -> 40x150 (crosses a tile in both axes), 4x6 -> 3x5 (down)
PREDICT_SHAPES = [(5, 7, 37, 53), (3, 2, 9, 3), (6, 20, 40, 150), (4, 6, 3, 5)]
# 90 is the largest K whose (K+1) K matrix fits the workgroup's LDS beside the staging area, 91 the first on the diagonal-only path
PREDICT_CLASSES = [1, 3, 19, 90, 91, 256]


def _labels(g, N, H, W, K, dtype):
    """Void pixels, every class, and values above K (row K); a negative one where the type has them."""
    top = min(K + 3, 255) if dtype == torch.uint8 else K + 3
    lab = torch.randint(0, top + 1, (N, H, W), generator=g)
    lab[:, 0, 0] = 0
    lab[1, 0, 1] = top
    if dtype != torch.uint8:
        lab[0, H - 1, W - 1] = -2
    return lab.to(dtype)


def _bincount(k_star, lab, K):
    """int64 [N, K+1, K] on the CPU from the class map and the labels."""
    N = lab.shape[0]
    lab = lab.to(torch.int64).reshape(N, -1)
    row = torch.where((lab >= 1) & (lab <= K), lab - 1, torch.full_like(lab, K))
    flat = row * K + k_star.reshape(N, -1)
    return torch.stack([torch.bincount(flat[n][lab[n] != 0], minlength=(K + 1) * K).view(K + 1, K) for n in range(N)])


@pytest.mark.parametrize("K", PREDICT_CLASSES)
@pytest.mark.parametrize("shape", PREDICT_SHAPES, ids=lambda s: "%dx%d_%dx%d" % s)
def test_predict_and_count_exactly(shape, K):
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    h, w, H, W = shape
    N = 3
    g = torch.Generator().manual_seed(1000 * K + H)
    logits = torch.randn(N, h, w, K, generator=g).to(torch.bfloat16).float()
    if K >= 3:
        logits[..., 2] = logits[..., 1]                                  # two classes equal everywhere: the first wins
    lg = logits.to(dev)
    k_star = spx.upsample_argext(lg.permute(0, 3, 1, 2), (H, W), largest=True)[0]
    assert K < 3 or not (k_star == 2).any()
    id_map = torch.randperm(256, generator=g)[:K].to(torch.uint8).to(dev)
    want_ids = id_map[k_star]
    size = N * H * W
    for dtype in LABEL_TYPES:
        lab = _labels(g, N, H, W, K, dtype)
        want_conf = _bincount(k_star.cpu(), lab, K)
        assert want_conf[:, K].sum() > 0 or K == 256 and dtype == torch.uint8
        buf = torch.full((size + 13,), 0xA5, dtype=torch.uint8, device=dev)
        out = buf[5:5 + size].view(N, H, W)                               # one byte off a dword: images straddle dwords
        assert out.data_ptr() % 4 == 1
        pred, conf = spx.predict_label_maps(lg, labels=lab.to(dev), id_map=id_map, out=out)
        assert pred.data_ptr() == out.data_ptr() and (buf[:5] == 0xA5).all() and (buf[5 + size:] == 0xA5).all()
        assert torch.equal(pred, want_ids)
        assert conf.dtype == torch.int64 and torch.equal(conf.cpu(), want_conf)
        m = spx.SegmentationMetrics(K, None, dev)
        m.update(lg, lab.to(dev))
        assert torch.equal(conf.sum(0), m.conf)
        # counters only, added to what is there
        none, again = spx.predict_label_maps(lg, labels=lab.to(dev), conf=conf, want_pred=False)
        assert none is None and again.data_ptr() == conf.data_ptr() and torch.equal(conf.cpu(), 2 * want_conf)
    # bytes only, without a map; the size given or taken from labels
    pred = spx.predict_label_maps(lg, (H, W))
    assert pred.dtype == torch.uint8 and torch.equal(pred.to(torch.int64), k_star)
    # the same logits as a permuted [N, K, h, w] tensor and as a slice of a longer batch
    cm = lg.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    wide = torch.zeros(N + 2, h, w, K, device=dev)
    wide[1:N + 1] = lg
    lab = _labels(g, N, H, W, K, torch.int64).to(dev)
    base = spx.predict_label_maps(lg, labels=lab, id_map=id_map)
    for view in (cm, wide[1:N + 1]):
        assert view.stride() != lg.stride() or view.data_ptr() != lg.data_ptr() or K == 1
        got = spx.predict_label_maps(view, labels=lab, id_map=id_map)
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    assert torch.equal(base[0], want_ids)


@pytest.mark.parametrize("K", [19, 91])
def test_predict_when_a_workgroup_walks_several_tiles_across_images(K):
    """8x8 -> 496x1030 is 31 x 17 = 527 tiles of 64 x 16 pixels per image, 1581 for N = 3: more than the workgroups the device
    holds at once (one or two of 1024 threads per CU), so every workgroup walks a run of 2 .. 16 tiles, and since no such
    length divides 527 = 17 * 31 the boundary between two images falls inside a run.  That exercises what the small shapes
    cannot: the flush and re-zero of the LDS counters when the image changes, into the image they were counted for; counters
    carried over the tiles of one image; the staging area reused by the next tile; and for K = 91 (only the diagonal in LDS)
    the global off-diagonal atomics of the image after the change.  The logits follow the labels loosely, so diagonal and
    off-diagonal cells are both busy; every image has its own labels, so counts flushed into the wrong image show."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    N, h, w, H, W = 3, 8, 8, 496, 1030
    props = torch.cuda.get_device_properties(dev)
    tiles = N * ((H + 15) // 16) * ((W + 63) // 64)
    assert tiles == 3 * 527 and tiles > 2 * props.multi_processor_count        # at most 2 workgroups of 1024 threads per CU
    g = torch.Generator().manual_seed(50 + K)
    cells = torch.randint(0, K + 2, (N, h, w), generator=g)                          # 0 = void, K + 1 = no class
    onehot = torch.nn.functional.one_hot(cells.clamp(1, K) - 1, K).float()
    logits = (2.5 * onehot + torch.randn(N, h, w, K, generator=g)).to(torch.bfloat16).float()
    lab = torch.nn.functional.interpolate(cells[:, None].float(), size=(H, W), mode="nearest")[:, 0].to(torch.uint8)
    lg, ld = logits.to(dev), lab.to(dev)
    k_star = spx.upsample_argext(lg.permute(0, 3, 1, 2), (H, W), largest=True)[0]
    want = _bincount(k_star.cpu(), lab, K)
    diag = torch.diagonal(want[:, :K], dim1=1, dim2=2).sum()
    assert diag > want.sum() // 8 and want.sum() - diag > want.sum() // 8 and want[:, K].sum() > 0      # both kinds of cell are busy
    assert not torch.equal(want[0], want[1]) and not torch.equal(want[1], want[2])
    id_map = torch.randperm(256, generator=g)[:K].to(torch.uint8).to(dev)
    buf = torch.full((N * H * W + 13,), 0xA5, dtype=torch.uint8, device=dev)
    out = buf[3:3 + N * H * W].view(N, H, W)
    pred, conf = spx.predict_label_maps(lg, labels=ld, id_map=id_map, out=out)
    assert (buf[:3] == 0xA5).all() and (buf[3 + N * H * W:] == 0xA5).all()
    assert torch.equal(pred, id_map[k_star])
    assert torch.equal(conf.cpu(), want)
    m = spx.SegmentationMetrics(K, None, dev)
    m.update(lg, ld)
    assert torch.equal(conf.sum(0), m.conf)
    _, again = spx.predict_label_maps(lg, labels=ld, conf=conf, want_pred=False)      # run-to-run: exactly twice
    assert torch.equal(again.cpu(), 2 * want)


def test_the_module_and_the_paired_maps_do_not_synchronise():
    """paired_heat_maps, FailureCases.update and FailureCases.heat_maps under torch's sync debug mode (the check the other
    modules' tests use): nothing in them waits for the device, and they give what the plain calls give."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    c = CASES["proto"]
    net, make = net_tables(c, dev)
    fc = make(spx.FailureCases, net, float(c["threshold"]))
    lg, lab = torch.from_numpy(c["logits"]).to(dev), torch.from_numpy(c["labels"]).to(dev)
    dist = torch.from_numpy(c["distances"]).to(dev)
    act = torch.from_numpy(activations_of(c)).to(dev)
    rows = torch.from_numpy(c["proto_rows"])
    Q = int(rows[:, 3].max()) + 1
    want_b = fc.update(lg, lab)
    want_heat = fc.heat_maps(rows, labels=lab, distances=dist)
    want_pair = spx.paired_heat_maps(act, lab, rows, Q)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        b = fc.update(lg, lab)
        heat = fc.heat_maps(rows, labels=lab, distances=dist)
        pair = spx.paired_heat_maps(act, lab, rows, Q)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert all(torch.equal(x, y) for x, y in zip(b[:2] + b[3:], want_b[:2] + want_b[3:]))
    assert torch.equal(b.iou.view(torch.int64), want_b.iou.view(torch.int64))
    assert torch.equal(heat[0], want_heat[0]) and torch.equal(heat[1], want_heat[1])
    assert torch.equal(pair[0], want_pair[0]) and torch.equal(pair[1], want_pair[1])
    # what update returned is the caller's: adding to it does not reach the module's own counters
    spx.predict_label_maps(lg, labels=lab, conf=b.conf, want_pred=False)
    report = fc.compute()
    assert torch.equal(report.image_confusion, torch.cat([want_b.conf, want_b.conf]).cpu())


def test_predict_against_the_restatement_and_without_synchronisation():
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    h, w, H, W, K, N = 5, 7, 37, 53, 19, 2
    g = torch.Generator().manual_seed(7)
    logits = torch.randn(N, h, w, K, generator=g).to(torch.bfloat16).float()
    lab = _labels(g, N, H, W, K, torch.uint8)
    lut = np.arange(K, dtype=np.uint8)[::-1].copy()
    k_star = FR.argmax_map(logits.numpy(), (H, W))
    lg, ld, idm = logits.to(dev), lab.to(dev), torch.from_numpy(lut).to(dev)
    spx.predict_label_maps(lg, labels=ld, id_map=idm)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        pred, conf = spx.predict_label_maps(lg, labels=ld, id_map=idm)
        iou, miss, fail = spx.failure_table(conf, 0.5)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert np.array_equal(pred.cpu().numpy(), FR.predict(logits.numpy(), (H, W), lut))
    want = FR.confusion(k_star, lab.numpy(), K)
    assert np.array_equal(conf.cpu().numpy(), want) and np.array_equal(want.sum(0), FR.aggregate(k_star, lab.numpy(), K))
    _check_table((iou, miss, fail), FR.failure_table(want, 0.5))


def _check_table(got, want):
    iou, miss, fail = (t.cpu().numpy() for t in got)
    assert iou.dtype == np.float64 and miss.dtype == np.int32 and fail.dtype == np.uint8
    assert np.array_equal(iou, want[0], equal_nan=True) and np.array_equal(miss, want[1]) and np.array_equal(fail, want[2])


def test_failure_table_by_hand():
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    K = 4
    conf = np.zeros((3, K + 1, K), np.int64)
    conf[0, 0] = [1, 1, 0, 0]                   # I = 1, U = 2: iou == threshold is not a failure; class 1 absent but predicted
    conf[0, 2] = [0, 3, 5, 3]                   # a tie between classes 1 and 3: the lowest
    conf[0, 3] = [0, 0, 0, 4]                   # all of its pixels right ...
    conf[0, 4] = [0, 0, 0, 10]                  # ... but labels outside 1..K predicted as 3 inflate the union: fails without a miss
    conf[2] = np.random.default_rng(3).integers(0, 50, (K + 1, K))
    conf[2, 1, 0] = conf[2, 1, 2] = 49          # another tie
    want = FR.failure_table(conf, 0.5)
    assert want[0][0, 0] == 0.5 and want[2][0, 0] == 0 and want[1][0, 0] == 1
    assert np.isnan(want[0][0, 1]) and want[1][0, 1] == -1 and want[2][0, 1] == 0
    assert want[1][0, 2] == 1 and want[2][0, 2] == 1 and want[0][0, 2] == 5 / 11
    assert want[0][0, 3] == 4 / 17 and want[2][0, 3] == 1 and want[1][0, 3] == -1
    assert np.isnan(want[0][1]).all() and want[1][2, 1] == 0
    _check_table(spx.failure_table(torch.from_numpy(conf).to(dev), 0.5), want)
    for thr in (0.0, 1.0, 5 / 11, np.nextafter(5 / 11, 1.0)):
        _check_table(spx.failure_table(torch.from_numpy(conf).to(dev), thr), FR.failure_table(conf, thr))


# ---- paired heat maps ------------------------------------------------------------------------------------------------------
def _strided(planes, dev):
    N, C, h, w = planes.shape
    view = torch.zeros(N, C + 2, h + 1, w + 3, device=dev)[:, 1:C + 1, :h, 2:w + 2]
    view.copy_(torch.from_numpy(planes))
    assert not view.is_contiguous()
    return view


def _check_heat(tag, heat, ranges, planes, labels, rows, Q, want=None, want_ranges=None):
    """Bytes and ranges from the device against the restatement (or the recorded ``want``) under the ambiguity rule."""
    heat, ranges = heat.cpu().numpy(), ranges.cpu().numpy()
    ref, ref_ranges, flagged = FR.paired_heat(planes, labels, rows, Q)
    amb = FR.paired_ambiguous(planes, labels, rows, Q)
    m0 = FR.slot_margin(planes, rows, Q)
    if want is not None:                                                  # recorded bytes hold off the flagged pixels
        assert np.array_equal(want[~flagged], ref[~flagged])
        ref_ranges = want_ranges
    assert heat.dtype == np.uint8 and heat.shape == ref.shape and ranges.shape == (Q, 2) and ranges.dtype == np.float32
    diff = np.abs(heat.astype(np.int64) - ref.astype(np.int64))
    print(f"{tag}: {len(rows)} rows, {Q} slots, {int(amb.sum())} ambiguous and {int(flagged.sum())} flagged of {amb.size} pixels, "
          f"{int((diff > 0).sum())} bytes differ (all by {int(diff.max())}), ranges off by {np.abs(ranges - ref_ranges).max():.3g} "
          f"(m0 {m0.max():.3g})")
    assert (diff[~amb] == 0).all(), (tag, np.argwhere((diff > 0) & ~amb)[:5])
    assert (diff <= 1).all()
    assert amb.sum() < amb.size / 2                                       # the check is not empty
    for q in range(Q):
        assert np.abs(ranges[q] - ref_ranges[q]).max() <= m0[q], (tag, q, ranges[q], ref_ranges[q])
    for i, r in enumerate(rows):
        if not ref_ranges[r[3], 1] > 0:
            assert not heat[i].any()
    return flagged


def _pair_rows(lab, table, shared):
    """Per image the lowest present class a and the next class b: the slots of a, then of b, over a."""
    cases = []
    for n in range(lab.shape[0]):
        present = [k for k in range(table.shape[0]) if (lab[n] == k + 1).any()]
        cases.append((n, present[0], (present[0] + 1) % table.shape[0]))
    fail = np.zeros((lab.shape[0], table.shape[0]), np.uint8)
    miss = np.full(fail.shape, -1, np.int32)
    for n, a, b in cases:
        fail[n, a], miss[n, a] = 1, b
    return FR.cases_and_rows(fail, miss, table, shared)[1]


@pytest.mark.parametrize("dtype", LABEL_TYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("name", sorted(EXPLAIN_CASES))
def test_paired_heat_on_the_small_grids(name, dtype):
    """The explanation maps' recorded planes and labels: prototypes with a range per plane, groups (which undershoot zero, so
    lo < 0 and bytes saturate) with a range shared by two rows; strided planes, out= at every alignment."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    c = EXPLAIN_CASES[name]
    planes, lab, table = planes_of(c).astype(np.float32), c["labels"], c["table"]
    shared = str(c["kind"]) == "group"
    rows = _pair_rows(lab, table, shared)
    Q = int(rows[:, 3].max()) + 1
    assert (Q < len(rows)) == shared
    act, ld = _strided(planes, dev), torch.from_numpy(lab).to(dtype).to(dev)
    heat, ranges = spx.paired_heat_maps(act, ld, torch.from_numpy(rows), Q)
    flagged = _check_heat(name, heat, ranges, planes, lab, rows, Q)
    if shared:
        assert (ranges[:, 0] < 0).any() and flagged.any() and (heat.cpu().numpy()[flagged] == 255).all()
    again = spx.paired_heat_maps(torch.from_numpy(planes).to(dev), ld, torch.from_numpy(rows), Q)
    assert torch.equal(again[0], heat) and torch.equal(again[1].view(torch.int32), ranges.view(torch.int32))
    N, C, h, w = planes.shape
    pix = torch.from_numpy(planes).to(dev).permute(0, 2, 3, 1).reshape(N * h * w, C).contiguous()
    assert torch.equal(spx.paired_heat_maps(pix, ld, torch.from_numpy(rows), Q, grid=(h, w))[0], heat)
    H, W = lab.shape[1:]
    size = len(rows) * H * W
    for guard in (64, 61, 62, 63):
        buf = torch.full((guard + size + 67,), 0xA5, dtype=torch.uint8, device=dev)
        out = buf[guard:guard + size].view(len(rows), H, W)
        got = spx.paired_heat_maps(act, ld, torch.from_numpy(rows), Q, out=out)[0]
        assert got.data_ptr() == out.data_ptr() and (buf[:guard] == 0xA5).all() and (buf[guard + size:] == 0xA5).all()
        assert torch.equal(out, heat), guard


@pytest.mark.parametrize("name", ["two_bands_257x50", "partially_staged_129x65"])
def test_paired_heat_across_bands_with_a_dead_slot_and_a_full_class(name):
    """Several bands of the range pass; slot 0 shared by two planes over the wide class (lo < 0: bytes saturate), slot 1 a plane
    that is negative wherever the class is (hi <= 0: all zeros), slot 2 a class that covers its whole image."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    c = band_edge_case(name)
    p = c["planes"]
    planes = np.concatenate([p, -np.abs(p[:, :1]) - 1.0, np.abs(p[:, 1:])], axis=1)
    planes = np.concatenate([planes, planes])                                       # image 1: the same planes
    lab = np.concatenate([c["labels"], np.ones_like(c["labels"])])                  # image 1: one class everywhere
    rows = np.array([(0, 0, 0, 0), (0, 1, 0, 0), (0, 2, 0, 1), (1, 3, 0, 2), (1, 0, 0, 3)], np.int64)
    Q = 4
    heat, ranges = spx.paired_heat_maps(torch.from_numpy(planes).to(dev), torch.from_numpy(lab).to(dev), torch.from_numpy(rows), Q)
    flagged = _check_heat(name, heat, ranges, planes, lab, rows, Q)
    r = ranges.cpu().numpy()
    assert r[0, 0] < 0 < r[0, 1] and flagged[:2].any() and not flagged[:2].all()
    assert r[1, 1] == 0 and r[1, 0] < 0 and flagged[2].all() and not heat[2].any()
    assert r[2, 0] != 0 and not flagged[3].all()                                    # no pixel outside the class: lo is a sample
    assert r[3, 0] < 0 and flagged[4].any()
    heat2, ranges2 = spx.paired_heat_maps(torch.from_numpy(planes).to(dev), torch.from_numpy(lab).to(dev), torch.from_numpy(rows), Q)
    assert torch.equal(heat2, heat) and torch.equal(ranges2.view(torch.int32), ranges.view(torch.int32))


# ---- the fixture and the module ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_failure_cases_end_to_end_against_the_fixture(name):
    """FailureCases over the recorded validation images, one batch: the reference's triples, its logged IoU, its bytes and ranges,
    with the slot tables taken from a real module; the Pascal rule drops exactly the cases it names."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    c = CASES[name]
    kind = str(c["kind"])
    net, make = net_tables(c, dev)
    fc = make(spx.FailureCases, net, float(c["threshold"]))
    lg, lab = torch.from_numpy(c["logits"]).to(dev), torch.from_numpy(c["labels"]).to(dev)
    b = fc.update(lg, lab)
    cases, rows = fc.rows_for(b)
    assert np.array_equal(cases.numpy(), c["cases"])
    iou = b.iou.cpu().numpy()
    assert [f"{iou[n, a]:.4f}" for n, a, _ in c["cases"]] == [str(s) for s in c["logged_iou"]]
    assert [iou[n, a] for n, a, _ in c["cases"]] == [int(I) / int(U) for I, U in c["counts"]]        # the reference's CLS_I / CLS_U
    assert np.array_equal(rows.numpy(), c[kind + "_rows"])
    planes = activations_of(c)
    Q = int(rows[:, 3].max()) + 1
    if kind == "proto":
        heat, ranges = fc.heat_maps(rows, labels=lab, distances=torch.from_numpy(c["distances"]).to(dev))
        # the device's own log differs from NumPy's by an ulp here and there: every byte within one off the flagged pixels
        flagged = FR.paired_heat(planes, c["labels"], rows.numpy(), Q)[2]
        diff = np.abs(heat.cpu().numpy().astype(np.int64) - c["proto_heat"])
        assert (diff[~flagged] <= 1).all()
        heat, ranges = fc.heat_maps(rows, torch.from_numpy(planes).to(dev), lab)
    else:
        N, U, h, w = planes.shape
        G = U // fc.num_classes
        groups = list(torch.split(torch.from_numpy(planes).to(dev).permute(0, 2, 3, 1).reshape(N * h * w, U), G, dim=1))
        heat, ranges = fc.heat_maps(rows, groups, lab, grid=(h, w))
    _check_heat(name, heat, ranges, planes, c["labels"], rows.numpy(), Q, c[kind + "_heat"], c[kind + "_ranges"])
    report = fc.compute()
    assert np.array_equal(np.stack([report.image.numpy(), report.cls.numpy(), report.miss.numpy()], 1), c["cases"])
    assert np.array_equal(report.image_confusion.numpy(), b.conf.cpu().numpy())
    m = spx.SegmentationMetrics(fc.num_classes, None, dev)
    m.update(lg, lab)
    assert torch.equal(report.confusion, m.conf.cpu())
    # the Pascal rule: the cases whose miss is the ignored class are dropped, the others stay in order
    drop = int(c["cases"][0, 2])
    fi = make(spx.FailureCases, net, float(c["threshold"]), ignore_miss=drop)
    kept = fi.rows_for(fi.update(lg, lab))[0].numpy()
    assert np.array_equal(kept, c["cases"][c["cases"][:, 2] != drop]) and len(kept) < len(c["cases"])


def test_label_maps_against_the_recorded_eval_test():
    """eval_test.py's bytes for the Cityscapes mapping: the recorded look-up table as ``id_map``."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    c = CASES["proto"]
    lut = torch.from_numpy(c["test_lut"]).to(dev)
    pred = spx.predict_label_maps(torch.from_numpy(c["test_logits"]).to(dev), c["test_pred"].shape[1:], id_map=lut)
    assert torch.equal(pred.cpu(), torch.from_numpy(c["test_pred"]))
