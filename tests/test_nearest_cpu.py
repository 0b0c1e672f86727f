"""Nearest-image tables and class-restricted crops, CPU side: the NumPy restatement (tests/nearest_restatement.py) against the
fixture recorded from the reference's own nearest_img.min_across_dataset, nearest_proto.min_on_sample and
find_continuous_high_activation_crop (tools/gen_nearest_golden.py), what the host refuses before any launch, and the
bookkeeping of ``nearest_images_to_prototypes`` with its device steps replaced by the oracle and the restatement."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import nearest_restatement as NR  # noqa: E402
import overlap_restatement as R  # noqa: E402
import push_boxes_restatement as PB  # noqa: E402
from nearest_cases import CROP_CASES, NEAREST, crop_case  # noqa: E402
from oracle import ppnet_oracle as O  # noqa: E402
from push_cases import MIXED, feature_problem  # noqa: E402


# ---- the restatement against the fixture ----------------------------------------------------------------------------------
def test_topk_images_equals_the_reference():
    c = NEAREST["images"]
    d = c["distances"]
    N, P = d.shape[:2]
    minima = d.reshape(N, P, -1).min(-1)
    n = c["top"].shape[0]
    idx, val = NR.topk_images(minima, n)
    assert np.array_equal(idx, c["top"].T)
    assert np.array_equal(val, np.sort(minima, axis=0)[:n].T)
    assert np.array_equal(c["flat"], d.reshape(N, P, -1).argmin(-1))
    idx, val = NR.topk_images(minima, N + 2)                               # more than there are images: padded
    assert (idx[:, N:] == -1).all() and np.isinf(val[:, N:]).all() and np.array_equal(idx[:, :n], c["top"].T)


def test_nearest_protos_equals_the_reference():
    c = NEAREST["protos"]
    d = c["distances"]
    short = False
    for t in (0, 1):
        include, lists = c[f"include{t}"], c[f"lists{t}"]
        n = lists.shape[1]
        for (_, y, x), want in zip(c[f"pixels{t}"], lists):
            got = NR.nearest_protos(d[0, :, y, x], n, include, n + 10)
            assert got == [int(p) for p in want if p >= 0]
            short |= len(got) < n
            assert NR.nearest_protos(d[0, :, y, x], n, include) == sorted(include, key=lambda p: d[0, p, y, x])[:n]
    assert short                                                           # a window that holds fewer than n included prototypes


@pytest.mark.parametrize("name", CROP_CASES)
def test_crop_chain_equals_the_reference(name):
    c = crop_case(name)
    planes, labels = c["planes"], c["labels"]
    h, w = planes.shape[2:]
    H, W = labels.shape[1:]
    seen = set()
    u32_of = {}
    for r, (n, p, L, f, _) in enumerate(c["rows"]):
        plane, lab = planes[n, p], labels[n]
        if p not in u32_of:
            u32_of[p] = R.upsample(plane, (H, W)).astype(np.float32)
        u32 = u32_of[p]
        rf = PB.rf_box(int(f), h, w, H, W)
        assert NR.patch_majority(lab, rf) == c["majority"][r]
        T = NR.masked_threshold(u32, lab == L)
        count = int((lab == L).sum())
        if count == 0:
            assert np.isposinf(T) and np.isposinf(c["threshold_gt"][r])
        else:                          # numpy forms gamma from a float32 virtual index on float32 input (the tool's note)
            gap = 0.0 if T == c["threshold_gt"][r] else abs(float(T) - float(c["threshold_gt"][r]))
            assert gap <= (0.0 if c["exact"] else R.margin(plane) / 4)
        got = NR.gt_boxes(plane, lab, int(L), int(f), threshold=c["threshold"][r], u32=u32)
        got_gt = NR.gt_boxes(plane, lab, int(L), int(f), threshold=c["threshold_gt"][r], u32=u32)
        assert got["box"] == list(c["box"][r]) and got_gt["box"] == list(c["box_gt"][r]), (name, r)
        assert got["robust"] == c["robust"][r] and got_gt["robust"] == c["robust_gt"][r]
        seen |= {s for s, hit in (("absent", count == 0), ("one_pixel", count == 1), ("void_majority", c["majority"][r] == 0),
                                  ("gt_differs", list(c["box"][r]) != list(c["box_gt"][r]))) if hit}
    assert {"absent", "one_pixel", "void_majority", "gt_differs"} <= seen
    for masking in (0, 1):
        sel = c["rows"][:, 4] == masking
        for flags in (c["robust"][sel], c["robust_gt"][sel]):
            assert int((~flags).sum()) <= (0 if c["exact"] else int(sel.sum()) // 8)


def test_masked_threshold_small_counts():
    u = np.array([[3.0, 1.0, 2.0, 5.0]], np.float32)
    assert np.isposinf(NR.masked_threshold(u, np.zeros((1, 4), bool)))
    assert NR.masked_threshold(u, np.array([[False, False, False, True]])) == np.float32(5.0)           # one value: itself
    two = NR.masked_threshold(u, np.array([[True, False, False, True]]))
    assert two == np.float32(np.percentile(np.array([3.0, 5.0], np.float32), 95))


# ---- what the host refuses ----------------------------------------------------------------------------------------------
def test_host_validation():
    import scaleprotoseg_amd as spx

    act, lab = torch.zeros(1, 2, 5, 7), torch.zeros(1, 33, 50, dtype=torch.long)
    masked = spx.high_activation_threshold_masked
    with pytest.raises(spx.SpxError, match="row 1"):
        masked(act, lab, torch.tensor([[0, 1, 2], [1, 0, 2]]))
    with pytest.raises(spx.SpxError, match="row 0"):
        masked(act, lab, torch.tensor([[0, 2, 2]]))
    with pytest.raises(spx.SpxError, match="not negative"):
        masked(act, lab, torch.tensor([[0, 1, -1]]))
    with pytest.raises(spx.SpxError, match=r"\[R, 3\]"):
        masked(act, lab, torch.tensor([[0, 1, 2, 3]]))
    with pytest.raises(spx.SpxError, match="0 < q < 1"):
        masked(act, lab, torch.tensor([[0, 1, 2]]), q=0.0)
    with pytest.raises(spx.SpxError, match="no CPU fallback"):
        masked(act, lab, torch.tensor([[0, 1, 2]]))
    rows = torch.tensor([[0, 1, -1, 3]])
    with pytest.raises(spx.SpxError, match="row_thresholds"):
        spx.push_bounding_boxes(act, lab, rows)
    with pytest.raises(spx.SpxError, match="row_thresholds"):
        spx.push_bounding_boxes(act, lab, rows, thresholds=torch.zeros(1, 2))
    with pytest.raises(spx.SpxError, match="not both"):
        spx.push_bounding_boxes(act, lab, rows, thresholds=torch.zeros(1, 2), row_thresholds=torch.zeros(1))
    with pytest.raises(spx.SpxError, match="no CPU fallback"):
        spx.push_bounding_boxes(act, lab, rows, row_thresholds=torch.zeros(1))
    dist = torch.zeros(1, 9, 5, 7)
    with pytest.raises(spx.SpxError, match="outside 1..64"):
        spx.nearest_prototypes(dist, torch.tensor([[0, 1, 1]]), n=65)
    with pytest.raises(spx.SpxError, match="row 0"):
        spx.nearest_prototypes(dist, torch.tensor([[0, 5, 1]]))
    with pytest.raises(spx.SpxError, match="outside 0..8"):
        spx.nearest_prototypes(dist, torch.tensor([[0, 1, 1]]), include=[9])
    with pytest.raises(spx.SpxError, match="window"):
        spx.nearest_prototypes(dist, torch.tensor([[0, 1, 1]]), window=0)
    with pytest.raises(spx.SpxError, match="no CPU fallback"):
        spx.nearest_prototypes(dist, torch.tensor([[0, 1, 1]]))
    with pytest.raises(spx.SpxError, match="at most 1024"):
        spx.patch_majority(lab, torch.tensor([[0, 3]]), (5, 7), 1024)
    with pytest.raises(spx.SpxError, match="row 0"):
        spx.patch_majority(lab, torch.tensor([[0, 35]]), (5, 7), 19)
    with pytest.raises(spx.SpxError, match="no CPU fallback"):
        spx.patch_majority(lab, torch.tensor([[0, 3]]), (5, 7), 19)
    with pytest.raises(spx.SpxError, match="outside 1..64"):
        spx.nearest_images_to_prototypes([], None, n=65)


def test_c_entry_points_refuse_bad_sizes():
    from scaleprotoseg_amd import _lib

    lib = _lib.load()
    err = lambda: lib.spx_last_error().decode()  # noqa: E731
    assert lib.spx_masked_workspace_bytes(4096) > lib.spx_masked_workspace_bytes(1) > 2 * 2048 * 4
    assert lib.spx_masked_workspace_bytes(4097) == 0 and "1..4096" in err()
    st = (C.c_int64 * 4)(70, 35, 7, 1)
    host = (C.c_int32 * 3)(0, 1, -1)
    one = 16                                                                # any non-NULL pointer: nothing is launched
    assert lib.spx_masked_thresholds(one, st, one, 1, one, host, 1, 1, 2, 5, 7, 33, 50, 0.95, one, one, None) != 0
    assert err().startswith("spx_masked_thresholds") and "label -1" in err()
    assert lib.spx_masked_thresholds(one, st, one, 1, one, None, 1, 1, 2, 5, 7, 33, 50, 1.0, one, one, None) != 0 and "0 < q < 1" in err()
    assert lib.spx_masked_thresholds(one, st, one, 2, one, None, 1, 1, 2, 5, 7, 33, 50, 0.5, one, one, None) != 0 and "label byte" in err()
    hrow = (C.c_int32 * 4)(0, 1, -2, 3)
    assert lib.spx_push_boxes_rows(one, st, one, 1, one, hrow, one, 1, 1, 2, 5, 7, 33, 50, 5, one, one, None) != 0
    assert err().startswith("spx_push_boxes_rows") and "class >= -1" in err()
    hrow = (C.c_int32 * 4)(0, 1, -1, 3)                                     # spx_push_boxes keeps refusing class -1
    assert lib.spx_push_boxes(one, st, one, 1, one, hrow, one, 1, 1, 2, 5, 7, 33, 50, 5, one, one, None) != 0 and "class >= 0" in err()
    assert lib.spx_patch_majority(one, 1, one, None, 1, 1, 5, 7, 33, 50, 1025, one, None) != 0 and "1024" in err()
    assert lib.spx_nearest_protos(one, one, None, None, 1, 1, 9, 5, 7, 65, 0, one, one, None) != 0 and "1..64" in err()
    q = (C.c_int32 * 3)(0, 5, 0)
    assert lib.spx_nearest_protos(one, one, q, None, 1, 1, 9, 5, 7, 3, 0, one, one, None) != 0 and "query 0" in err()


# ---- the driver's bookkeeping, device steps replaced --------------------------------------------------------------------
def _oracle_distances(net, conv):
    ranges = {s: tuple(net.scale_num_prototypes[s]) for s in range(net.num_scales)}
    return O.scale_l2_convolution(conv, net.prototype_vectors.detach(), ranges, net.num_scales)


@pytest.fixture
def cpu_steps(monkeypatch):
    """The four device steps of scaleprotoseg_amd/nearest.py on the oracle and the restatement (tests only)."""
    from scaleprotoseg_amd import nearest as mod

    def minima(net, conv):                  # image by image: the oracle's convolution of a batch need not give a lone image's bits
        d = torch.cat([_oracle_distances(net, conv[b:b + 1]) for b in range(conv.shape[0])]).flatten(2)
        val, idx = d.min(dim=2)
        return (val.contiguous().view(torch.int32).to(torch.int64) << 32) | idx

    def merge(table, keys, W, image0):
        B, P = keys.shape
        for b in range(B):
            for p in range(P):
                have = [(int(table.key[p, j]), int(table.image[p, j]), table.cell[p, j].tolist()) for j in range(table.k)
                        if int(table.image[p, j]) >= 0]
                f = int(keys[b, p]) & 0xFFFFFFFF
                have.append((int(keys[b, p]) & ~0xFFFFFFFF, image0 + b, [f // W, f % W]))
                have.sort(key=lambda e: (e[0], e[1]))
                for j, (key, image, cell) in enumerate(have[:table.k]):
                    table.key[p, j], table.image[p, j] = key, image
                    table.cell[p, j] = torch.tensor(cell, dtype=torch.int32)

    def planes(net, img, protos, device):
        return net.distance_2_similarity(_oracle_distances(net, net.conv_features(img.unsqueeze(0)))[:, protos]).float()

    def crops(act, labels, chan, flat, num_classes, q=0.95, add_margin=5):
        lab = labels[0].numpy()
        h, w = act.shape[2:]
        out = [[] for _ in range(6)]
        for c, f in zip(chan.tolist(), flat.tolist()):
            plane = act[0, c].numpy()
            rf = PB.rf_box(f, h, w, *lab.shape)
            L = NR.patch_majority(lab, rf)
            u32 = R.upsample(plane, lab.shape).astype(np.float32)
            T = np.float32(R.threshold(u32, q))
            all_px = NR.gt_boxes(plane, lab, L, f, q, add_margin, threshold=T, u32=u32)
            gt = NR.gt_boxes(plane, lab, L, f, q, add_margin, u32=u32)
            for o, v in zip(out, (rf, L - 1, T, gt["threshold"], all_px["box"], gt["box"])):
                o.append(v)
        return (torch.tensor(out[0]), torch.tensor(out[1], dtype=torch.int32), torch.tensor(np.array(out[2], np.float32)),
                torch.tensor(np.array(out[3], np.float32)), torch.tensor(out[4]), torch.tensor(out[5]))

    monkeypatch.setattr(mod, "nearest_run_minima", minima)
    monkeypatch.setattr(mod, "nearest_run_merge", merge)
    monkeypatch.setattr(mod, "winning_image_planes", planes)
    monkeypatch.setattr(mod, "gt_crops", crops)
    return crops


@pytest.mark.parametrize("n,rng", [(3, None), (9, None), (2, range(2, 6))], ids=["n3", "n_above_the_images", "shard"])
def test_driver_bookkeeping(cpu_steps, n, rng):
    import scaleprotoseg_amd as spx

    net, data = feature_problem(MIXED)                                      # 7 images of three latent sizes
    P = net.num_prototypes
    calls = []
    item = data.__class__.__getitem__
    data.__class__ = type("Counted", (data.__class__,), {"__getitem__": lambda self, i: (calls.append(i), item(self, i))[1]})
    got = spx.nearest_images_to_prototypes(data, net, n, batch_size=3, image_range=rng)
    ids = list(rng) if rng is not None else list(range(len(data)))
    dist = [_oracle_distances(net, net.conv_features(data.items[i][0].unsqueeze(0)))[0] for i in ids]
    minima = np.stack([d.flatten(1).min(1).values.numpy() for d in dist])   # [images, P]
    idx, val = NR.topk_images(minima, n)
    keep = idx >= 0
    want_image = np.where(keep, np.array(ids)[np.maximum(idx, 0)], -1)
    assert np.array_equal(got.image.numpy(), want_image)
    assert np.array_equal(got.distance.numpy()[keep], val[keep]) and (got.distance.numpy()[~keep] == -1).all()
    assert (n > len(ids)) == bool((~keep).any())
    for p in range(P):
        for j in range(n):
            if not keep[p, j]:
                assert int(got.flat[p, j]) == -1 and got.rf_box[p, j].tolist() == [-1] * 4 and int(got.patch_class[p, j]) == -1
                assert got.bound_box[p, j].tolist() == got.bound_box_gt[p, j].tolist() == [-1] * 4
                assert float(got.threshold[p, j]) == float(got.threshold_gt[p, j]) == -1.0
                continue
            d = dist[int(idx[p, j])]
            f = int(d[p].flatten().argmin())
            assert int(got.flat[p, j]) == f
            lab = data.items[int(want_image[p, j])][1]
            act = net.distance_2_similarity(d[p:p + 1].unsqueeze(0)).float()
            rf, cls, thr, thr_gt, box, box_gt = cpu_steps(act, torch.as_tensor(lab).unsqueeze(0), torch.tensor([0]), torch.tensor([f]),
                                                          net.num_classes)
            assert got.rf_box[p, j].tolist() == rf[0].tolist() and int(got.patch_class[p, j]) == int(cls[0])
            assert got.bound_box[p, j].tolist() == box[0].tolist() and got.bound_box_gt[p, j].tolist() == box_gt[0].tolist()
            assert float(got.threshold[p, j]) == float(thr[0]) and float(got.threshold_gt[p, j]) == float(thr_gt[0])
    # every image once in pass 1, every distinct winning image once more in pass 2
    winners = sorted(set(want_image[keep].tolist()))
    assert sorted(calls) == sorted(ids + winners)
    plain = spx.nearest_images_to_prototypes(data, net, n, batch_size=3, image_range=rng, crops=False)
    assert torch.equal(plain.image, got.image) and torch.equal(plain.flat, got.flat) and plain.rf_box is None
