"""push_bounding_boxes / push_prototypes_multiscale(boxes=True) on the GPU against the fixture recorded from the reference's own
update_prototypes_on_image (tests/golden/push_boxes.npz) and, for other shapes, against the NumPy restatement
(tests/push_boxes_restatement.py).

Bounds.  The outputs are integers of a serial walk, so a row is either equal or not.  The kernel evaluates a sample in fp32 and
selects its own threshold, each within m = 64 * 2^-23 * max|a| of the float64 restatement; a query whose answer could change
under that (a pixel within 2 m of the threshold and no hit that is clear of it) makes its row "non-robust"
(push_boxes_restatement).  Every robust row must equal the reference exactly; non-robust rows are skipped and must be at
most 1 row in 8 per case.  With identity resampling everything is exact and every row must be equal."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import push_boxes_restatement as PB  # noqa: E402
from map_cases import PUSH_BOX_CASES as CASES, classes_of, planes_of  # noqa: E402
from support import gpu_device, ListData, proto_net  # noqa: E402
from support import release_cached_blocks  # noqa: E402,F401  (a module-scoped autouse fixture, taken by importing its name)

pytestmark = pytest.mark.gpu


def _gpu(planes, labels, rows, dev, **kw):
    import scaleprotoseg_amd as spx

    rf, box = spx.push_bounding_boxes(torch.as_tensor(planes).to(dev), torch.as_tensor(labels).to(dev), torch.as_tensor(rows), **kw)
    assert rf.dtype == box.dtype == torch.int64 and rf.is_cuda and tuple(rf.shape) == tuple(box.shape) == (len(rows), 4)
    return rf.cpu().numpy(), box.cpu().numpy()


def _compare(tag, rf, box, want_rf, want_box, robust, exact=False):
    R = len(robust)
    bad = int((~np.asarray(robust)).sum())
    differ = [r for r in range(R) if list(box[r]) != list(want_box[r])]
    print(f"{tag}: {R} rows, {bad} non-robust, {len(differ)} crops differ from the reference (rows {differ[:8]})")
    assert bad <= (0 if exact else R // 8)
    assert np.array_equal(rf, want_rf)                                   # the patch box is integer arithmetic: every row
    for r in range(R):
        if robust[r] or exact:
            assert list(box[r]) == list(want_box[r]), (tag, r, list(box[r]), list(want_box[r]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_parity(name):
    dev = gpu_device()
    c = CASES[name]
    planes, cls = planes_of(c), classes_of(c)
    P = planes.shape[1]
    rows = np.stack([c["img"], np.arange(P), cls, c["flat"]], axis=1)
    rf, box = _gpu(planes, c["labels"], rows, dev)
    _compare(name, rf, box, c["ref_rf"][:, 1:5], c["ref_box"][:, 1:5], c["robust"], exact=name.startswith("exact"))


# ---- other shapes, against the restatement ----------------------------------------------------------------------------
ABSENT = 7                                  # a class no label holds


def _bf16(a):
    return torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def _case(seed, N, C, h, w, H, W, R, whole=False):
    """Bump planes (channel C - 1 negative: T <= 0), blocky labels of the classes 0..2 and void, R rows: patches at the
    plane's peak or anywhere, the class under the peak or any; ``whole`` appends the row of an absent class on the negative
    plane, whose crop grows to the whole image (every pixel is a hit): the longest walk."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = np.zeros((N, C, h, w))
    for n in range(N):
        for c in range(C):
            for _ in range(int(g.integers(1, 4))):
                cy, cx, s, a = g.uniform(0, h - 1), g.uniform(0, w - 1), g.uniform(0.08, 0.25), g.uniform(0.5, 1.0)
                planes[n, c] += a * np.exp(-0.5 * (((yy - cy) / (s * h)) ** 2 + ((xx - cx) / (s * w)) ** 2))
            planes[n, c] += 0.02 * g.random((h, w))
    planes[:, C - 1] -= 2.0
    planes = _bf16(planes)
    cells = g.integers(0, 4, (N, 3, 4))
    labels = np.stack([np.kron(cells[n], np.ones((-(-H // 3), -(-W // 4)), np.int64))[:H, :W] for n in range(N)])
    rows = []
    for r in range(R):
        n, c = r % N, int(g.integers(0, C))
        f = int(planes[n, c].argmax()) if g.random() < 0.7 else int(g.integers(0, h * w))
        rfb = PB.rf_box(f, h, w, H, W)
        k = int(labels[n, min(rfb[0], H - 1), min(rfb[2], W - 1)]) - 1 if g.random() < 0.8 else int(g.integers(0, 3))
        rows.append([n, c, max(k, 0), f])
    if whole:
        rows.append([0, C - 1, ABSENT, (h // 2) * w + w // 2])
    return planes, labels, np.array(rows, np.int64)


def _restated(planes, labels, rows):
    out = [PB.boxes(planes[n, c], labels[n], int(k), int(f)) for n, c, k, f in rows]
    return (np.array([o["rf"] for o in out]), np.array([o["box"] for o in out]), np.array([o["robust"] for o in out]))


_SHAPES = {
    "w513_longer_than_a_workgroup": (31, 1, 4, 33, 65, 257, 513, 7, True),
    "w50_shorter_than_a_wave": (32, 2, 3, 5, 7, 33, 50, 8, True),
    "non_integer_ratios_129x257_to_300x700": (73, 1, 3, 129, 257, 300, 700, 8, False),
    "one_row": (41, 1, 2, 9, 11, 70, 85, 1, False),
    "300_rows_3_images_repeated_channels": (35, 3, 5, 9, 11, 70, 85, 300, False),
}
_SHARED = {}


def _shape_case(name):
    """(planes, labels, rows, restated rf, box, robust), computed once and left unchanged."""
    if name not in _SHARED:
        seed, N, C, h, w, H, W, R, whole = _SHAPES[name]
        planes, labels, rows = _case(seed, N, C, h, w, H, W, R, whole)
        _SHARED[name] = (planes, labels, rows) + _restated(planes, labels, rows)
    return _SHARED[name]


@pytest.mark.parametrize("name", sorted(_SHAPES))
def test_against_the_restatement(name):
    dev = gpu_device()
    planes, labels, rows, want_rf, want_box, robust = _shape_case(name)
    H, W = labels.shape[1:]
    rf, box = _gpu(planes, labels, rows, dev)
    _compare(name, rf, box, want_rf, want_box, robust)
    if _SHAPES[name][8]:                                                 # the longest walk: the crop is the whole image
        assert list(want_box[-1]) == [0, H, 0, W] and robust[-1] and list(box[-1]) == [0, H, 0, W]
    if name.startswith("w513"):
        assert ((want_box[:, 3] - want_box[:, 2]) > 256 + 10).any()      # a row segment longer than the 256 threads
    if name.startswith("300"):
        assert len({(n, c) for n, c, _, _ in rows}) < len(rows) / 4      # planes are named many times


def test_strided_pixel_major_and_label_types_and_repeats():
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    planes, labels, rows, _, _, _ = _shape_case("300_rows_3_images_repeated_channels")
    N, C, h, w = planes.shape
    p, l, r = torch.from_numpy(planes).to(dev), torch.from_numpy(labels).to(dev), torch.from_numpy(rows)
    rf, box = spx.push_bounding_boxes(p, l, r)
    again = spx.push_bounding_boxes(p, l, r)
    assert torch.equal(again[0], rf) and torch.equal(again[1], box)                       # two calls: identical tensors
    pix = p.permute(0, 2, 3, 1).reshape(N * h * w, C).contiguous()                        # the forward's [M, P] layout
    got = spx.push_bounding_boxes(pix, l, r, grid=(h, w))
    assert torch.equal(got[0], rf) and torch.equal(got[1], box)
    padded = torch.zeros(N, C + 2, h, w + 3, device=dev)[:, 1:C + 1, :, 2:w + 2]
    padded.copy_(p)
    assert not padded.is_contiguous()
    got = spx.push_bounding_boxes(padded, l, r)
    assert torch.equal(got[0], rf) and torch.equal(got[1], box)
    for dt in (torch.uint8, torch.int32):
        got = spx.push_bounding_boxes(p, l.to(dt), r)
        assert torch.equal(got[0], rf) and torch.equal(got[1], box), dt
    # rows on the device (never read by the host) and thresholds given = thresholds selected
    thr = spx.high_activation_threshold(p, labels.shape[1:], 0.95)
    got = spx.push_bounding_boxes(p, l, r.to(dev), thresholds=thr)
    assert torch.equal(got[0], rf) and torch.equal(got[1], box)
    got = spx.push_bounding_boxes(p, l, r.to(dev))
    assert torch.equal(got[0], rf) and torch.equal(got[1], box)
    # a row out of range: refused from a host table, -1 from a device table (and its neighbours untouched)
    bad = r.clone()
    bad[1, 3] = h * w
    with pytest.raises(spx.SpxError, match="row 1"):
        spx.push_bounding_boxes(p, l, bad, thresholds=thr)
    got = spx.push_bounding_boxes(p, l, bad.to(dev), thresholds=thr)
    keep = torch.ones(len(rows), dtype=torch.bool)
    keep[1] = False
    assert got[0][1].tolist() == got[1][1].tolist() == [-1] * 4
    assert torch.equal(got[0][keep], rf[keep]) and torch.equal(got[1][keep], box[keep])
    # the margin is the caller's
    wide = spx.push_bounding_boxes(p, l, r, thresholds=thr, add_margin=0)
    H, W = labels.shape[1:]
    back = torch.stack([(wide[1][:, 0] - 5).clamp_min(0), (wide[1][:, 1] + 5).clamp_max(H), (wide[1][:, 2] - 5).clamp_min(0),
                        (wide[1][:, 3] + 5).clamp_max(W)], dim=1)
    assert torch.equal(back, box)


def test_inside_a_captured_step():
    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd import graphs

    dev = gpu_device()
    planes, labels, rows, _, _, _ = _shape_case("w50_shorter_than_a_wave")
    p, l, r = torch.from_numpy(planes).to(dev), torch.from_numpy(labels).to(dev), torch.from_numpy(rows).to(torch.int32).to(dev)
    thr = spx.high_activation_threshold(p, labels.shape[1:], 0.95)
    rf, box = spx.push_bounding_boxes(p, l, r, thresholds=thr)
    graph, out = graphs.capture_step(lambda: spx.push_bounding_boxes(p, l, r, thresholds=thr), warmup=1)
    out[0].zero_()
    out[1].zero_()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], rf) and torch.equal(out[1], box)


# ---- the module, end to end ---------------------------------------------------------------------------------------------


def test_push_prototypes_multiscale_with_boxes(tmp_path):
    from scaleprotoseg_amd.push import push_prototypes_multiscale

    dev = gpu_device()
    S, Cs, K, per = 2, 16, 3, 2
    P = S * K * per
    net = proto_net(P, K, S, Cs, seed=11, backbone="pool", add_on=nn.Sequential(nn.Sigmoid()), device=dev).eval()
    gen = torch.Generator().manual_seed(12)
    data = ListData()
    H, W = 40, 56
    for _ in range(3):
        t = torch.randint(0, K + 1, (5, 7), generator=gen).repeat_interleave(8, 0).repeat_interleave(8, 1)
        # smooth images: the activation planes get bumps a crop can grow along
        img = torch.nn.functional.interpolate(torch.randn(1, 3, 5, 7, generator=gen), size=(H, W), mode="bicubic")[0]
        data.append((img, t.numpy().astype(np.int64)))
    with torch.no_grad():
        acts = []
        for img, _ in data:
            conv, dist = net.push_forward(img.unsqueeze(0).to(dev))
            acts.append(net.distance_2_similarity(dist)[0].cpu().numpy())
    h, w = acts[0].shape[1:]
    assert (h, w) == (10, 14)
    cls = net.prototype_class_identity.argmax(1).tolist()

    with_boxes, plain = copy.deepcopy(net), copy.deepcopy(net)
    root_a, root_b = str(tmp_path / "a"), str(tmp_path / "b")
    best, tot_idx, dup, rf_table, box_table = push_prototypes_multiscale(
        data, with_boxes, root_dir_for_saving_prototypes=root_a, log=lambda *_: None, boxes=True, epoch_number=3,
        proto_bound_boxes_filename_prefix="bb")
    best_b, _, dup_b = push_prototypes_multiscale(data, plain, root_dir_for_saving_prototypes=root_b, log=lambda *_: None)

    # the push itself is untouched by the boxes
    assert torch.equal(best, best_b) and dup == dup_b
    assert torch.equal(with_boxes.prototype_vectors.detach(), plain.prototype_vectors.detach())
    assert json.load(open(os.path.join(root_a, "unique_prototypes.json"))) == json.load(open(os.path.join(root_b, "unique_prototypes.json")))
    assert not os.path.exists(os.path.join(root_b, "epoch-3"))

    # the tables: the restatement on the un-pushed model's planes, driven by the same winners
    assert rf_table.shape == box_table.shape == (P, 6) and rf_table.dtype == box_table.dtype == np.int64
    want_rf, want_box, robust = [], [], []
    for p in range(P):
        i = int(best[p])
        got = PB.boxes(acts[i][p], data[i][1], cls[p], int(tot_idx[i][0, p]))
        want_rf.append([i, *got["rf"], cls[p]])
        want_box.append([i, *got["box"], cls[p]])
        robust.append(got["robust"])
    want_rf, want_box = np.array(want_rf), np.array(want_box)
    assert np.array_equal(rf_table[:, [0, 5]], want_rf[:, [0, 5]]) and np.array_equal(box_table[:, [0, 5]], want_box[:, [0, 5]])
    _compare("module", rf_table[:, 1:5], box_table[:, 1:5], want_rf[:, 1:5], want_box[:, 1:5], np.array(robust))
    assert (rf_table >= 0).all() and (box_table >= 0).all()                 # -1-free rows
    assert len(set(best.tolist())) <= 3

    # the reference's two files
    saved_rf = np.load(os.path.join(root_a, "epoch-3", "bb-receptive_field3.npy"))
    saved_box = np.load(os.path.join(root_a, "epoch-3", "bb3.npy"))
    assert saved_rf.dtype == saved_box.dtype == np.int64 and saved_rf.shape == saved_box.shape == (P, 6)
    assert np.array_equal(saved_rf, rf_table) and np.array_equal(saved_box, box_table)
