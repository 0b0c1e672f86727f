"""The nearest-image / nearest-prototype analysis on the GPU (scaleprotoseg_amd/nearest.py) against the fixture recorded from the
reference's own functions (tests/golden/nearest_analysis.npz over the planes of push_boxes.npz) and, for other shapes, against
the NumPy restatement (tests/nearest_restatement.py).

Bounds.  The masked select is exact on the fp32 values the kernel computes, each within m = overlap_restatement.margin(plane) =
64 * 2^-23 * max|a| of the float64 restatement, so |T - numpy| <= m: the bound tests/test_gpu_overlap.py holds the unmasked
select to; with identity resampling T is numpy's bit for bit.  Majorities, nearest prototypes and crops are integers: a crop row
is equal or not, and only a row whose walk holds a query that could change under 2 m ("non-robust", push_boxes_restatement) is
skipped; such rows are at most 1 in 8 per case and masking.  Everything else is an equality."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import nearest_restatement as NR  # noqa: E402
import overlap_restatement as R  # noqa: E402
import push_boxes_restatement as PB  # noqa: E402
from map_cases import BAND_EDGES, band_edge_case  # noqa: E402
from nearest_cases import CROP_CASES, NEAREST, crop_case  # noqa: E402
from support import bits_equal, gpu_device, ListData, proto_net  # noqa: E402
from support import release_cached_blocks  # noqa: E402,F401  (a module-scoped autouse fixture, taken by importing its name)

pytestmark = pytest.mark.gpu


def _bf16(a):
    return torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def _within(tag, got, want, planes_of_rows, exact=False):
    """|got - want| <= margin(plane) per row (inf must meet inf); bit for bit when ``exact``.  Prints the worst ratio."""
    worst = 0.0
    for r, (g, t) in enumerate(zip(got, want)):
        if np.isinf(t) or exact:
            assert np.float32(g).tobytes() == np.float32(t).tobytes(), (tag, r, g, t)
            continue
        m = R.margin(planes_of_rows[r])
        worst = max(worst, abs(float(g) - float(t)) / m)
        assert abs(float(g) - float(t)) <= m, (tag, r, g, t, m)
    print(f"{tag}: {len(got)} thresholds, worst |T - numpy| = {worst:.3f} of the margin")


# ---- masked thresholds ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CROP_CASES)
def test_masked_thresholds_fixture(name):
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    c = crop_case(name)
    rows = c["rows"]
    p, l = torch.from_numpy(c["planes"]).to(dev), torch.from_numpy(c["labels"]).to(dev)
    T = spx.high_activation_threshold_masked(p, l, torch.from_numpy(rows[:, :3]))
    assert T.dtype == torch.float32 and T.is_cuda and tuple(T.shape) == (len(rows),)
    _within(name, T.cpu().numpy(), c["threshold_gt"], [c["planes"][n, ch] for n, ch in rows[:, :2]], exact=c["exact"])
    assert np.isposinf(c["threshold_gt"]).any()                            # an absent class is among the rows: +inf


_WHOLE = {"w50": (5, 7, 33, 50), "w513": (33, 65, 257, 513), "two_bands_257x50": (5, 7, 257, 50),
          "partially_staged_129x65": (129, 65, 140, 70)}


@pytest.mark.parametrize("name", sorted(_WHOLE))
def test_whole_image_mask_equals_the_unmasked_select(name):
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    h, w, H, W = _WHOLE[name]
    g = torch.Generator().manual_seed(len(name))
    p = torch.randn(2, 3, h, w, generator=g).to(dev)
    l = torch.full((2, H, W), 3, dtype=torch.uint8, device=dev)
    rows = torch.tensor([[n, c, 3] for n in range(2) for c in range(3)])
    for q in (0.95, 0.5):
        want = spx.high_activation_threshold(p, (H, W), q)
        assert bits_equal(spx.high_activation_threshold_masked(p, l, rows, q).view(2, 3), want), (name, q)
    assert torch.isposinf(spx.high_activation_threshold_masked(p, l, torch.tensor([[1, 2, 4]]))).all()


def test_counts_of_one_and_two_dtypes_views_and_repeats():
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    h, w, H, W = 9, 11, 70, 85
    g = np.random.default_rng(5)
    planes = _bf16(g.normal(size=(2, 3, h, w)))
    labels = g.integers(0, 3, (2, H, W)).astype(np.int64)
    labels[0, 13, 50] = 5                                                   # label 5: one pixel of image 0
    labels[1, 3, 4] = labels[1, 69, 84] = 6                                 # label 6: two pixels of image 1
    rows = np.array([[0, 0, 5], [1, 2, 6], [0, 1, 6], [1, 1, 5], [0, 2, 1], [1, 0, 0], [1, 1, 2]], np.int64)
    want = np.array([NR.masked_threshold(R.upsample(planes[n, c], (H, W)).astype(np.float32), labels[n] == L) for n, c, L in rows])
    assert np.isposinf(want[2:4]).all() and np.isfinite(want[[0, 1]]).all()
    p, l, r = torch.from_numpy(planes).to(dev), torch.from_numpy(labels).to(dev), torch.from_numpy(rows)
    T = spx.high_activation_threshold_masked(p, l, r)
    _within("small counts", T.cpu().numpy(), want, [planes[n, c] for n, c, _ in rows])
    assert bits_equal(spx.high_activation_threshold_masked(p, l, r), T)                       # twice: identical
    for dt in (torch.uint8, torch.int32):
        assert bits_equal(spx.high_activation_threshold_masked(p, l.to(dt), r), T), dt
    pix = p.permute(0, 2, 3, 1).reshape(2 * h * w, 3).contiguous()                            # the forward's [M, P] layout
    assert bits_equal(spx.high_activation_threshold_masked(pix, l, r, grid=(h, w)), T)
    padded = torch.zeros(2, 5, h, w + 3, device=dev)[:, 1:4, :, 2:w + 2]
    padded.copy_(p)
    assert not padded.is_contiguous() and bits_equal(spx.high_activation_threshold_masked(padded, l, r), T)
    assert bits_equal(spx.high_activation_threshold_masked(p, l, r.to(dev)), T)               # rows the host never reads
    bad = r.clone()
    bad[1, 1] = 3
    bad[4, 2] = -1
    with pytest.raises(spx.SpxError, match="row 1"):
        spx.high_activation_threshold_masked(p, l, bad)
    got = spx.high_activation_threshold_masked(p, l, bad.to(dev))
    keep = torch.ones(len(rows), dtype=torch.bool)
    keep[[1, 4]] = False
    assert torch.isnan(got[~keep.to(dev)]).all() and bits_equal(got[keep.to(dev)], T[keep.to(dev)])


@pytest.mark.parametrize("name", sorted(BAND_EDGES))
def test_classes_at_the_edges_of_the_bands(name):
    """A class whose rows lie in two bands, and classes of one pixel in the last band and on the first and the last row of a
    band: the threshold of a lone pixel is that pixel's value."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    c = band_edge_case(name)
    planes, labels = c["planes"], c["labels"]
    rows = np.array([[0, ch, L] for ch in range(2) for L in [1] + c["lone"]], np.int64)
    up = [R.upsample(planes[0, ch], labels.shape[1:]).astype(np.float32) for ch in range(2)]
    want = np.array([NR.masked_threshold(up[ch], labels[0] == L) for _, ch, L in rows])
    assert all((labels[0] == L).sum() == 1 for L in c["lone"]) and np.isfinite(want).all()
    T = spx.high_activation_threshold_masked(torch.from_numpy(planes).to(dev), torch.from_numpy(labels).to(dev), torch.from_numpy(rows))
    assert torch.isfinite(T).all()
    _within(name, T.cpu().numpy(), want, [planes[0, ch] for _, ch, _ in rows])


# ---- patch majority ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CROP_CASES)
def test_patch_majority_fixture(name):
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    c = crop_case(name)
    rows = c["rows"]
    got = spx.patch_majority(torch.from_numpy(c["labels"]).to(dev), torch.from_numpy(rows[:, [0, 3]]), c["planes"].shape[2:], 4)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), c["majority"])
    H, W = c["labels"].shape[1:]
    h, w = c["planes"].shape[2:]
    if not c["exact"]:
        assert any(PB.rf_box(int(f), h, w, H, W)[1] > H for f in rows[:, 3])                  # a box past the image's edge


def test_patch_majority_tie_edge_and_label_types():
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    lab = np.zeros((2, 6, 8), np.int64)
    lab[0, :, :4], lab[0, :, 4:] = 7, 2                                     # 24 pixels each: the smaller label wins
    lab[1, :3], lab[1, 3:] = 1023, 5
    rows = torch.tensor([[0, 0], [1, 0]])
    for dt in (torch.int64, torch.int32):
        got = spx.patch_majority(torch.from_numpy(lab).to(dev).to(dt), rows, (1, 1), 1023)     # one patch: the box is the image + 1
        assert got.tolist() == [2, 5] == [NR.patch_majority(lab[n], PB.rf_box(0, 1, 1, 6, 8)) for n in range(2)]
    g = np.random.default_rng(2)
    lab = g.integers(0, 20, (3, 37, 41)).astype(np.uint8)
    rows = np.array([[n, f] for n in range(3) for f in range(5 * 6)], np.int64)
    want = [NR.patch_majority(lab[n], PB.rf_box(int(f), 5, 6, 37, 41)) for n, f in rows]
    assert spx.patch_majority(torch.from_numpy(lab).to(dev), torch.from_numpy(rows), (5, 6), 19).tolist() == want
    dev_rows = torch.from_numpy(rows).to(dev)
    dev_rows[3, 1] = 30
    got = spx.patch_majority(torch.from_numpy(lab).to(dev), dev_rows, (5, 6), 19).tolist()
    assert got[3] == -1 and got[:3] + got[4:] == want[:3] + want[4:]


# ---- crops from per-row thresholds ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CROP_CASES)
def test_push_boxes_rows_fixture(name):
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    c = crop_case(name)
    rows = c["rows"]
    p, l = torch.from_numpy(c["planes"]).to(dev), torch.from_numpy(c["labels"]).to(dev)
    h, w = c["planes"].shape[2:]
    H, W = c["labels"].shape[1:]
    table = torch.from_numpy(np.stack([rows[:, 0], rows[:, 1], rows[:, 2] - 1, rows[:, 3]], axis=1))
    assert (table[:, 2] == -1).any()                                        # a void-majority patch: class -1
    thr_gt = spx.high_activation_threshold_masked(p, l, torch.from_numpy(rows[:, :3]))
    thr = spx.high_activation_threshold(p, (H, W))[torch.from_numpy(rows[:, 0]).to(dev), torch.from_numpy(rows[:, 1]).to(dev)]
    want_rf = np.array([PB.rf_box(int(f), h, w, H, W) for f in rows[:, 3]])
    for tag, T, want, robust in (("all-pixel", thr, c["box"], c["robust"]), ("gt", thr_gt, c["box_gt"], c["robust_gt"])):
        rf, box = spx.push_bounding_boxes(p, l, table, row_thresholds=T.contiguous())
        rf, box = rf.cpu().numpy(), box.cpu().numpy()
        assert np.array_equal(rf, want_rf)
        skipped = 0
        for masking in (0, 1):
            sel = rows[:, 4] == masking
            bad = int((~robust[sel]).sum())
            assert bad <= (0 if c["exact"] else int(sel.sum()) // 8)
            skipped += bad
        differ = [r for r in range(len(rows)) if list(box[r]) != list(want[r])]
        print(f"{name} {tag}: {len(rows)} rows, {skipped} non-robust skipped, {len(differ)} differ from the reference ({differ[:8]})")
        for r in range(len(rows)):
            if robust[r] or c["exact"]:
                assert list(box[r]) == list(want[r]), (name, tag, r, list(box[r]), list(want[r]))
    # the void-majority rows and the +inf rows are never ambiguous
    void, absent = table[:, 2].numpy() == -1, np.isposinf(c["threshold_gt"])
    assert void.any() and absent.any() and c["robust_gt"][absent].all()
    still = np.stack([np.maximum(want_rf[:, 0] - 5, 0), np.minimum(want_rf[:, 1] + 5, H - 1) + 1, np.maximum(want_rf[:, 2] - 5, 0),
                      np.minimum(want_rf[:, 3] + 5, W - 1) + 1], axis=1)
    assert np.array_equal(c["box_gt"][absent], still[absent])               # +inf: the patch box plus the margin
    assert torch.isposinf(thr_gt[torch.from_numpy(absent).to(dev)]).all()
    # thresholds gathered from the [N, C] table: the existing call, bit for bit
    own = table[:, 2] >= 0
    full = spx.high_activation_threshold(p, (H, W))
    old = spx.push_bounding_boxes(p, l, table[own], thresholds=full)
    new = spx.push_bounding_boxes(p, l, table[own], row_thresholds=thr[own.to(dev)].contiguous())
    assert torch.equal(old[0], new[0]) and torch.equal(old[1], new[1])
    new = spx.push_bounding_boxes(p, l, table[own].to(dev), row_thresholds=thr[own.to(dev)].contiguous())      # device rows
    assert torch.equal(old[0], new[0]) and torch.equal(old[1], new[1])


# ---- nearest prototypes -----------------------------------------------------------------------------------------------
def test_nearest_prototypes_fixture():
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    c = NEAREST["protos"]
    d = torch.from_numpy(c["distances"]).to(dev)
    for t in (0, 1):
        lists = c[f"lists{t}"]
        n = lists.shape[1]
        idx, val = spx.nearest_prototypes(d, torch.from_numpy(c[f"pixels{t}"]), n, include=c[f"include{t}"].tolist(), window=n + 10)
        assert idx.dtype == torch.int64 and val.dtype == torch.float32 and np.array_equal(idx.cpu().numpy(), lists)
        for (_, y, x), row, v in zip(c[f"pixels{t}"], lists, val.cpu().numpy()):
            assert all(v[j] == (c["distances"][0, row[j], y, x] if row[j] >= 0 else np.inf) for j in range(n))


@pytest.mark.parametrize("P,k", [(228, 13), (7, 1), (2000, 64), (7, 13)], ids=["P228_k13", "P7_k1", "P2000_k64", "P7_k13_pads"])
def test_nearest_prototypes_shapes_masks_and_ties(P, k):
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    g = np.random.default_rng(P + k)
    B, h, w = 2, 3, 5
    d = (g.integers(0, max(8, P // 4), (B, P, h, w)) * 0.25).astype(np.float32)               # quarters: exact ties everywhere
    pixels = np.array([[b, y, x] for b in range(B) for y in range(h) for x in range(w)], np.int64)[::3]
    nearest = [NR.nearest_protos(d[b, :, y, x], 1)[0] for b, y, x in pixels]
    include = np.ones(P, bool)
    include[nearest[0]] = include[nearest[-1]] = False                      # the mask removes a pixel's nearest prototype
    include[g.integers(0, P, P // 3)] = False
    dd = torch.from_numpy(d).to(dev)
    for tag, kw, ref in (("plain", {}, lambda col: NR.nearest_protos(col, k)),
                         ("mask", dict(include=torch.from_numpy(include)), lambda col: NR.nearest_protos(col, k, np.flatnonzero(include))),
                         ("window", dict(include=np.flatnonzero(include).tolist(), window=k + 10),
                          lambda col: NR.nearest_protos(col, k, np.flatnonzero(include), k + 10))):
        idx, val = spx.nearest_prototypes(dd, torch.from_numpy(pixels), k, **kw)
        idx, val = idx.cpu().numpy(), val.cpu().numpy()
        ties = 0
        for (b, y, x), row, v in zip(pixels, idx, val):
            col = d[b, :, y, x]
            want = ref(col)
            assert row[:len(want)].tolist() == want and (row[len(want):] == -1).all() and np.isposinf(v[len(want):]).all(), (tag, b, y, x)
            assert np.array_equal(v[:len(want)], col[want])
            ties += int((np.diff(v[:len(want)]) == 0).sum())
        assert ties > 0 or k == 1, tag                                      # equal distances: the lower prototype first
        if P < k:
            assert (idx[:, P:] == -1).all()
    again = spx.nearest_prototypes(dd, torch.from_numpy(pixels).to(dev), k)                   # device pixels, repeated
    plain = spx.nearest_prototypes(dd, torch.from_numpy(pixels), k)
    assert torch.equal(again[0], plain[0]) and bits_equal(again[1], plain[1])


# ---- inside a captured step ---------------------------------------------------------------------------------------------
def test_masked_select_and_row_crops_inside_a_captured_step():
    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd import graphs

    dev = gpu_device()
    c = crop_case("log_s5x7")
    rows = c["rows"]
    p, l = torch.from_numpy(c["planes"]).to(dev), torch.from_numpy(c["labels"]).to(dev)
    masked = torch.from_numpy(rows[:, :3]).to(torch.int32).to(dev)
    table = torch.from_numpy(np.stack([rows[:, 0], rows[:, 1], rows[:, 2] - 1, rows[:, 3]], axis=1)).to(torch.int32).to(dev)

    def step():
        T = spx.high_activation_threshold_masked(p, l, masked)
        return (T,) + spx.push_bounding_boxes(p, l, table, row_thresholds=T)

    want = step()
    graph, out = graphs.capture_step(step, warmup=1)
    for t in out:
        t.zero_()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert bits_equal(out[0], want[0]) and torch.equal(out[1], want[1]) and torch.equal(out[2], want[2])


# ---- the drivers, end to end --------------------------------------------------------------------------------------------
def _problem(dev):
    S, Cs, K, per = 2, 16, 3, 2
    net = proto_net(S * K * per, K, S, Cs, seed=21, backbone="pool", add_on=nn.Sequential(nn.Sigmoid()), device=dev).eval()
    gen = torch.Generator().manual_seed(22)
    data = ListData()
    for H, W in [(40, 56)] * 3 + [(48, 40)] * 3:                            # two image sizes: latent 10 x 14 and 12 x 10
        t = torch.randint(0, K + 1, (H // 8, W // 8), generator=gen).repeat_interleave(8, 0).repeat_interleave(8, 1)
        img = torch.nn.functional.interpolate(torch.randn(1, 3, H // 8, W // 8, generator=gen), size=(H, W), mode="bicubic")[0]
        data.append((img, t.numpy().astype(np.int64)))
    return net, data, K


def _restated_row(act, lab, f, L=None):
    """(rf, majority - 1, T, T_gt, box dict, box_gt dict) of one plane on one label image; L None = the patch majority."""
    h, w = act.shape
    rf = PB.rf_box(f, h, w, *lab.shape)
    if L is None:
        L = NR.patch_majority(lab, rf)
    u32 = R.upsample(act, lab.shape).astype(np.float32)
    T = R.threshold(u32, 0.95)
    return rf, L - 1, T, NR.masked_threshold(u32, lab == L), NR.gt_boxes(act, lab, L, f, threshold=T, u32=u32), NR.gt_boxes(act, lab, L, f, u32=u32)


def test_nearest_images_to_prototypes_end_to_end():
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    net, data, K = _problem(dev)
    P, n = net.num_prototypes, 3
    with torch.no_grad():
        dist = [net.push_forward(img.unsqueeze(0).to(dev))[1][0] for img, _ in data]
        acts = [net.distance_2_similarity(d).float().cpu().numpy() for d in dist]
    minima = np.stack([d.flatten(1).min(1).values.cpu().numpy() for d in dist])
    flats = np.stack([d.flatten(1).argmin(1).cpu().numpy() for d in dist])
    idx, val = NR.topk_images(minima, n)
    for p in range(P):
        assert len(set(np.sort(minima[:, p])[:n + 1].tolist())) == n + 1    # no tie decides an order
    got = spx.nearest_images_to_prototypes(data, net, n, batch_size=1)        # encoded one by one, as the maps above were
    assert np.array_equal(got.image.numpy(), idx) and np.array_equal(got.distance.numpy(), val)
    assert np.array_equal(got.flat.numpy(), flats[idx, np.arange(P)[:, None]])
    assert len({data[i][1].shape for i in set(idx.ravel().tolist())}) == 2                    # winners of both image sizes
    bad = bad_gt = 0
    for p in range(P):
        for j in range(n):
            i = int(idx[p, j])
            rf, cls, T, T_gt, box, box_gt = _restated_row(acts[i][p], data[i][1], int(got.flat[p, j]))
            assert got.rf_box[p, j].tolist() == rf and int(got.patch_class[p, j]) == cls
            m = R.margin(acts[i][p])
            assert abs(float(got.threshold[p, j]) - float(T)) <= m
            assert (np.isposinf(T_gt) and np.isposinf(float(got.threshold_gt[p, j]))) or abs(float(got.threshold_gt[p, j]) - float(T_gt)) <= m
            bad, bad_gt = bad + (not box["robust"]), bad_gt + (not box_gt["robust"])
            if box["robust"]:
                assert got.bound_box[p, j].tolist() == box["box"], (p, j)
            if box_gt["robust"]:
                assert got.bound_box_gt[p, j].tolist() == box_gt["box"], (p, j)
    print(f"end to end: {P * n} rows, non-robust {bad} (all-pixel) and {bad_gt} (gt)")
    assert bad <= P * n // 8 and bad_gt <= P * n // 8
    # more entries asked for than there are images: padded with -1
    wide = spx.nearest_images_to_prototypes(data, net, len(data) + 2, batch_size=4)
    assert torch.equal(wide.image[:, :n], got.image) and (wide.image[:, len(data):] == -1).all() and (wide.image[:, :len(data)] >= 0).all()
    for t in (wide.flat, wide.distance, wide.rf_box, wide.patch_class, wide.threshold, wide.threshold_gt, wide.bound_box, wide.bound_box_gt):
        assert (t[:, len(data):] == -1).all()
    assert torch.equal(wide.bound_box_gt[:, :n], got.bound_box_gt) and bits_equal(wide.threshold_gt[:, :n].contiguous(), got.threshold_gt)


def test_push_with_gt_boxes():
    from scaleprotoseg_amd.push import push_prototypes_multiscale

    dev = gpu_device()
    net, data, K = _problem(dev)
    P = net.num_prototypes
    with torch.no_grad():
        acts = [net.distance_2_similarity(net.push_forward(img.unsqueeze(0).to(dev))[1][0]).float().cpu().numpy() for img, _ in data]
    cls = net.prototype_class_identity.argmax(1).tolist()
    a, b = copy.deepcopy(net), copy.deepcopy(net)
    with_gt = push_prototypes_multiscale(data, a, log=lambda *_: None, boxes=True, gt_boxes=True)
    plain = push_prototypes_multiscale(data, b, log=lambda *_: None, boxes=True)
    assert len(with_gt) == 6 and len(plain) == 5
    assert torch.equal(with_gt[0], plain[0]) and all(torch.equal(x, y) for x, y in zip(with_gt[1], plain[1])) and with_gt[2] == plain[2]
    assert np.array_equal(with_gt[3], plain[3]) and np.array_equal(with_gt[4], plain[4])
    assert torch.equal(a.prototype_vectors.detach(), b.prototype_vectors.detach())
    gt = with_gt[5]
    assert gt.shape == (P, 6) and gt.dtype == np.int64 and np.array_equal(gt[:, [0, 5]], with_gt[4][:, [0, 5]])
    bad = 0
    for p in range(P):
        i = int(with_gt[0][p])
        want = _restated_row(acts[i][p], data[i][1], int(with_gt[1][i][0, p]), L=cls[p] + 1)[5]
        bad += not want["robust"]
        if want["robust"]:
            assert gt[p, 1:5].tolist() == want["box"], p
    assert bad <= P // 8
    assert (gt[:, 1:5] != with_gt[4][:, 1:5]).any()                         # the class-restricted crop is another crop
