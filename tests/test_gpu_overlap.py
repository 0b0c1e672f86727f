"""ActivationOverlap / high_activation_threshold on the GPU against the fixture recorded from the reference's own
prototype_overlap / group_overlap (tests/golden/activation_overlap.npz) and, for other shapes, against the float64
restatement (tests/overlap_restatement.py).

Bounds.  The kernels evaluate the cubic upsample in fp32, the fixture in float64 rounded to fp32: a pixel's value may differ by
the rounding of 16 products and sums, bounded by m = 64 * 2^-23 * max|a| (overlap_restatement.MARGIN).  So a threshold may move
by m, and only the pixels within m of the threshold ("ambiguous", counted per plane as A) may change side:
|area - ref| <= A_j, |inter_jj' - ref| <= A_j + A_j', summed over the images that count.  With identity resampling the
values are exact and every counter must be equal."""
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
from support import gpu_device, group_net, proto_net  # noqa: E402
from support import release_cached_blocks  # noqa: E402,F401  (a module-scoped autouse fixture, taken by importing its name)

pytestmark = pytest.mark.gpu


def _run(planes, labels, table, q, dev):
    import scaleprotoseg_amd as spx

    m = spx.ActivationOverlap(table.shape[0], torch.as_tensor(table), dev, quantile=q)
    m.update(torch.as_tensor(planes).to(dev), torch.as_tensor(labels).to(dev))
    return m


def _present(labels, K):
    return np.array([[bool((labels[n] == k + 1).any()) for k in range(K)] for n in range(labels.shape[0])])


def _check_counts(res, ref_inter, ref_area, amb, labels, table):
    """Counters within the ambiguity of the planes that were counted."""
    K, J = table.shape
    present = _present(labels, K)
    assert res.images.tolist() == present.sum(0).tolist()
    for k in range(K):
        A = [int(sum(amb[n, table[k, j]] for n in range(labels.shape[0]) if present[n, k])) if table[k, j] >= 0 else 0 for j in range(J)]
        for j in range(J):
            d = abs(int(res.area[k, j]) - int(ref_area[k, j]))
            print(f"class {k} slot {j}: area {int(res.area[k, j])} ref {int(ref_area[k, j])} A {A[j]}")
            assert d <= A[j], (k, j)
            for j2 in range(J):
                want = int(ref_inter[k, j, j2]) if j2 > j else 0
                assert abs(int(res.inter[k, j, j2]) - want) <= (A[j] + A[j2] if j2 > j else 0), (k, j, j2)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_thresholds_and_counts(name):
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    c = CASES[name]
    planes, q, labels, table = planes_of(c), float(c["q"]), c["labels"], c["table"]
    H, W = labels.shape[1:]
    thr = spx.high_activation_threshold(torch.as_tensor(planes).to(dev), (H, W), q).cpu().numpy()
    for n in range(planes.shape[0]):
        for ch in range(planes.shape[1]):
            d = abs(float(thr[n, ch]) - float(c["thresholds"][n, ch]))
            print(f"plane {n},{ch}: |T - ref| {d:.3e} m {R.margin(planes[n, ch]):.3e}")
            assert d <= R.margin(planes[n, ch]), (n, ch)
    res = _run(planes, labels, table, q, dev).compute()
    if name.startswith("exact"):
        assert np.array_equal(res.inter.numpy(), c["ref_inter"]) and np.array_equal(res.area.numpy(), c["area"])
        union = res.area[:, :, None] + res.area[:, None, :] - res.inter
        assert np.array_equal(union.numpy() * (c["ref_union"] > 0), c["ref_union"])
        assert int(res.area[1, 2]) == 0                                  # the constant plane: empty mask
        assert int(res.inter[2, 0, 1]) == int(res.area[2, 0]) == int(res.area[2, 1]) > 0      # the duplicated plane
        assert res.total == int(c["ref_total_inter"]) / int(c["ref_total_union"])
    else:
        _check_counts(res, c["ref_inter"], c["area"], c["ambiguous"], labels, table)
    if str(c["kind"]) == "proto":
        # prototypes 0 and 2 hold the same plane: whatever the rounding, intersection = union = area
        assert int(res.inter[0, 0, 2]) == int(res.area[0, 0]) == int(res.area[0, 2]) > 0
        assert int(res.area[3].sum()) == 0 and int(res.area[4].sum()) == 0 and int(res.images[4]) == 0


def _random_case(seed, N, C, h, w, H, W, K, present):
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(N, 1, h, w, generator=g) * 2
    planes = (base + 0.3 * torch.rand(N, C, h, w, generator=g)).to(torch.bfloat16).float()
    labels = torch.zeros(N, H, W, dtype=torch.int64)
    for n in range(N):
        for i, k in enumerate(present[n]):
            labels[n, i * 3:i * 3 + 2, 5:W - 3] = k + 1
    return planes, labels


_SHARED = {}


def _wide_case(dev):
    """12 slots per class (78 pairs and areas: more than one pair per lane), a slot table that repeats a channel, 9 x 11 ->
    70 x 85."""
    if "wide" not in _SHARED:
        planes, labels = _random_case(7, 2, 13, 9, 11, 70, 85, 2, [[0, 1], [1]])
        table = np.stack([np.arange(12), np.array([12, 3, 5, 3] + [-1] * 8)])
        ref = R.overlap_counts(planes.numpy(), labels.numpy(), table, 0.9)
        m = _run(planes.numpy(), labels.numpy(), table, 0.9, dev)
        _SHARED["wide"] = (planes, labels, table, ref, m._buf.clone(), m.compute())
    return _SHARED["wide"]


def test_twelve_slots_and_a_repeated_channel_against_the_restatement():
    dev = gpu_device()
    planes, labels, table, ref, _, res = _wide_case(dev)
    _check_counts(res, ref["inter"], ref["area"], ref["ambiguous"], labels.numpy(), table)
    assert int(res.inter[1, 1, 3]) == int(res.area[1, 1]) == int(res.area[1, 3]) > 0      # the same channel in two slots
    ci, total = R.finalize(res.inter.numpy(), res.area.numpy(), table)
    assert res.class_iou == ci and res.total == total


def test_partially_staged_tall_plane_against_the_restatement():
    """150 x 60 latent rows do not fit the LDS stage at once: every band stages its own rows plus the halo."""
    dev = gpu_device()
    planes, labels = _random_case(11, 1, 3, 150, 60, 310, 97, 1, [[0]])
    table = np.array([[0, 1, 2]])
    ref = R.overlap_counts(planes.numpy(), labels.numpy(), table, 0.95)
    res = _run(planes.numpy(), labels.numpy(), table, 0.95, dev).compute()
    _check_counts(res, ref["inter"], ref["area"], ref["ambiguous"], labels.numpy(), table)


def test_strided_pixel_major_view_equals_contiguous():
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    planes, labels, table, _, buf, _ = _wide_case(dev)
    N, C, h, w = planes.shape
    pix = planes.permute(0, 2, 3, 1).reshape(N * h * w, C).contiguous().to(dev)          # the forward's [M, P] layout
    m = spx.ActivationOverlap(2, torch.as_tensor(table), dev, quantile=0.9)
    m.update(pix, labels.to(dev), grid=(h, w))
    assert torch.equal(m._buf, buf)
    padded = torch.zeros(N, C + 2, h, w + 3, device=dev)[:, 1:C + 1, :, 2:w + 2]
    padded.copy_(planes)
    assert not padded.is_contiguous()
    m2 = spx.ActivationOverlap(2, torch.as_tensor(table), dev, quantile=0.9)
    m2.update(padded, labels.to(dev).to(torch.uint8))
    assert torch.equal(m2._buf, buf)
    thr = spx.high_activation_threshold(pix, (70, 85), 0.9, grid=(h, w))
    assert torch.equal(thr, spx.high_activation_threshold(planes.to(dev), (70, 85), 0.9))


def test_two_updates_equal_the_sum_and_repeats_are_identical():
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    planes, labels, table, _, buf, _ = _wide_case(dev)
    p, l = planes.to(dev), labels.to(dev)
    again = spx.ActivationOverlap(2, torch.as_tensor(table), dev, quantile=0.9)
    again.update(p, l)
    assert torch.equal(again._buf, buf)                                  # the same call twice: identical counters
    parts = spx.ActivationOverlap(2, torch.as_tensor(table), dev, quantile=0.9)
    parts.update(p[:1], l[:1])
    parts.update(p[1:], l[1:])
    assert torch.equal(parts._buf, buf)
    again.update(p, l)
    assert torch.equal(again._buf, 2 * buf)
    again.reset()
    assert int(again._buf.abs().sum()) == 0


def test_update_inside_a_captured_step():
    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd import graphs

    dev = gpu_device()
    planes, labels, table, _, buf, _ = _wide_case(dev)
    p, l = planes.to(dev), labels.to(dev)
    m = spx.ActivationOverlap(2, torch.as_tensor(table), dev, quantile=0.9)
    graph, _ = graphs.capture_step(lambda: m.update(p, l), warmup=1)
    m.reset()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(m._buf, 2 * buf)


def _module_labels(N, H, W, classes):
    labels = torch.zeros(N, H, W, dtype=torch.int64)
    for n in range(N):
        for i, k in enumerate(classes[n]):
            labels[n, 4 + 9 * i:10 + 9 * i, 3:W - 5] = k + 1
    return labels


def test_for_prototypes_with_distances_on_a_real_module():
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    torch.manual_seed(5)
    P, K, S, Cs = 40, 10, 4, 64
    net = proto_net(P, K, S, Cs, device=dev).eval()
    conv = torch.randn(2, S * Cs, 9, 11, generator=torch.Generator().manual_seed(9)).to(dev)
    with torch.no_grad():
        _, dist = net.forward_from_conv_features(conv)
        act = net.distance_2_similarity(dist)
    labels = _module_labels(2, 70, 85, [[0, 4], [4, 9]])
    m = spx.ActivationOverlap.for_prototypes(net)
    m.update(labels=labels.to(dev), distances=dist)
    res = m.compute()
    table = m.slot_table_host.numpy()
    ref = R.overlap_counts(act.cpu().numpy(), labels.numpy(), table, 0.95)
    _check_counts(res, ref["inter"], ref["area"], ref["ambiguous"], labels.numpy(), table)
    assert set(res.class_iou) == {0, 4, 9} and res.images.tolist() == [1, 0, 0, 0, 2, 0, 0, 0, 0, 1]
    with pytest.raises(spx.SpxError, match="for_prototypes"):
        spx.ActivationOverlap(K, torch.as_tensor(table), dev).update(labels=labels.to(dev), distances=dist)


def test_for_groups_on_a_real_module():
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    torch.manual_seed(5)
    P, K, S, Cs, G = 40, 10, 4, 64, 6
    net = group_net(P, K, S, Cs, G, device=dev).eval()
    conv = torch.randn(2, S * Cs, 9, 11, generator=torch.Generator().manual_seed(9)).to(dev)
    with torch.no_grad():
        _, act = net.forward_from_conv_features(conv, return_activations=True)
        groups = net.compute_group(act)
    labels = _module_labels(2, 70, 85, [[1, 2], [2]])
    m = spx.ActivationOverlap.for_groups(net)
    m.update(groups, labels.to(dev), grid=(9, 11))
    cat = torch.cat(groups, dim=1)
    m2 = spx.ActivationOverlap.for_groups(net)
    m2.update(cat, labels.to(dev), grid=(9, 11))
    assert torch.equal(m._buf, m2._buf)
    res = m.compute()
    table = m.slot_table_host.numpy()
    assert table.shape == (K, G) and table[3].tolist() == list(range(18, 24))
    planes = cat.view(2, 9, 11, K * G).permute(0, 3, 1, 2).cpu().numpy()
    ref = R.overlap_counts(planes, labels.numpy(), table, 0.95)
    _check_counts(res, ref["inter"], ref["area"], ref["ambiguous"], labels.numpy(), table)
    assert set(res.class_iou) == {1, 2}
