"""GPU part consistency / stability (scaleprotoseg_amd/parts.py, csrc/spx_parts.hip) against tests/consistency_restatement.py and
the rows recorded from the reference (tests/golden/part_consistency.npz).

Everything compared here is an integer, a byte or the bits of an fp32 order statistic and its fp32 lerp, so every comparison is
exact.  Shapes: 37 x 53 (one and a bit tiles of 32 x 32 per axis) and 70 x 131 (three by five tiles, ragged on both axes)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import consistency_restatement as CR  # noqa: E402
from support import gpu_device, group_net, proto_net  # noqa: E402
from support import release_cached_blocks  # noqa: E402,F401  (a module-scoped autouse fixture, taken by importing its name)

pytestmark = pytest.mark.gpu

K_PAT, M_PAT = 2, 3
CASES = ("nonzero", "image", "explicit", "filtered")


# ---- labelling ---------------------------------------------------------------------------------------------------------------
def _patterns(H, W):
    """(labels, parts) uint8 / int32 [7, H, W]: one pattern per image."""
    lab = np.zeros((7, H, W), np.uint8)
    par = np.zeros((7, H, W), np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    # 0: a one-pixel serpentine through every tile: the even rows, joined at alternating ends
    lab[0] = 1
    par[0][::2] = 1
    for y in range(1, H, 2):
        par[0][y, W - 1 if (y // 2) % 2 == 0 else 0] = 1
    # 1: a two-key checkerboard: each key hangs together by diagonals only
    lab[1] = 2
    par[1] = 1 + (yy + xx) % 2
    # 2: the main diagonal and the anti-diagonal
    lab[2] = 1
    d = min(H, W)
    par[2][np.arange(d), np.arange(d)] = 1
    par[2][np.arange(d), W - 1 - np.arange(d)] = 2
    # 3: a frame that touches all four borders, a ring around an island of another part, a second class
    lab[3] = 1
    par[3][[0, H - 1], :] = 3
    par[3][:, [0, W - 1]] = 3
    par[3][5:H - 5, 5:W - 5] = 1
    par[3][8:H - 8, 8:W - 8] = 0
    par[3][12:H - 12, 12:W - 12] = 2
    lab[3][H // 2:, W // 2:] = 2                                # the same parts under another class are other components
    # 4: isolated pixels, some of them 8-neighbours of a pixel with another key
    g = np.random.default_rng(11)
    lab[4] = g.integers(0, K_PAT + 2, (H, W))                   # void and a label above K among them
    par[4] = np.where(g.random((H, W)) < 0.12, g.integers(-1, M_PAT + 3, (H, W)), 0)       # ids below 1 and above M among them
    # 5: no parts at all
    lab[5] = 1 + (xx // 9) % 2
    # 6: blocks of 7 x 11 whose keys repeat, so equal keys meet across tile borders
    lab[6] = 1 + ((yy // 7) + (xx // 11)) % 2
    par[6] = 1 + ((yy // 7) * 3 + (xx // 11)) % 3
    return lab, par


@pytest.fixture(scope="module", params=[(37, 53), (70, 131)], ids=lambda s: f"{s[0]}x{s[1]}")
def labelled(request):
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    lab, par = _patterns(*request.param)
    tl, tp = torch.from_numpy(lab).to(dev), torch.from_numpy(par).to(dev)
    comp = spx.part_components(tl, tp, M_PAT, num_classes=K_PAT)
    return lab, par, tl, tp, comp


def test_components_equal_the_flood_fill(labelled):
    lab, par, tl, tp, comp = labelled
    want = CR.component_table(lab, par, K_PAT, M_PAT)
    got = comp.table(tl, tp)
    assert len(want) > 50 and got == want
    per_image = {n: sum(1 for r in want if r[0] == n) for n in range(7)}
    assert per_image[0] == 1 and per_image[1] == 2 and per_image[5] == 0, per_image
    # every keyed pixel points at the smallest pixel of its component; the others at nothing
    parent = comp.parent.cpu().numpy()
    keyed = (lab >= 1) & (lab <= K_PAT) & (par >= 1) & (par <= M_PAT)
    assert np.array_equal(parent >= 0, keyed)
    roots = comp.count.cpu().numpy() > 0
    flat = np.arange(lab.shape[1] * lab.shape[2]).reshape(lab.shape[1:])
    assert np.array_equal(roots, keyed & (parent == flat[None]))
    assert (parent[keyed] <= np.broadcast_to(flat, lab.shape)[keyed]).all()
    # the totals of every B_t
    tot = comp.totals.cpu().numpy()
    for n in range(7):
        for k in range(K_PAT):
            for t in range(1, M_PAT + 1):
                ys, xs = np.nonzero((lab[n] == k + 1) & (par[n] == t))
                assert tot[n, k, t - 1].tolist() == [len(xs), int(xs.sum()), int(ys.sum())]


def test_components_twice_bit_for_bit(labelled):
    import scaleprotoseg_amd as spx

    _, _, tl, tp, comp = labelled
    again = spx.part_components(tl, tp, M_PAT, num_classes=K_PAT)
    assert torch.equal(again.workspace, comp.workspace) and torch.equal(again.totals, comp.totals)
    # int64 maps give the same components
    wide = spx.part_components(tl.long(), tp.long(), M_PAT, num_classes=K_PAT)
    assert torch.equal(wide.workspace, comp.workspace)


# ---- thresholds --------------------------------------------------------------------------------------------------------------
def _threshold_inputs(h, w, H, W):
    g = np.random.default_rng(h * 100 + H)
    K, J, C = 3, 2, 7
    table = np.array([[0, 3], [1, 4], [2, -1]])
    act = g.choice(np.array([-1.0, -0.5, 0.0, 0.25, 0.25, 1.0, 2.0, 3.5], np.float32), (2, C, h, w))      # ties, negatives, zeros
    act[:, 5:] = g.standard_normal((2, 2, h, w)).astype(np.float32)
    act[:, 4] = g.standard_normal((2, h, w)).astype(np.float32)
    act[0, 1] = 0.0                                              # class 1 of image 0: no non-zero activation in slot 0
    lab = np.zeros((2, H, W), np.uint8)
    lab[0] = 1 + (np.arange(W)[None, :] * 3 // W + np.arange(H)[:, None] * 2 // H) % 3
    lab[1, :H // 3] = 1                                          # image 1: class 1 absent, class 2 a few pixels, a label above K
    lab[1, H - 2:, W - 3:] = 3
    lab[1, H // 2, :] = K + 1
    return act, lab, table


@pytest.mark.parametrize("h,w,H,W", [(5, 7, 37, 53), (7, 7, 56, 56)])
@pytest.mark.parametrize("mode", ["nonzero", "image"])
def test_thresholds_bit_equal(h, w, H, W, mode):
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    act, lab, table = _threshold_inputs(h, w, H, W)
    got = spx.part_thresholds(torch.from_numpy(act).to(dev), torch.from_numpy(lab).to(dev), table, 0.8, mode)
    again = spx.part_thresholds(torch.from_numpy(act).to(dev), torch.from_numpy(lab).to(dev), table, 0.8, mode)
    want = CR.thresholds(act, lab, table, 0.8, mode)
    got_h = got.cpu().numpy()
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got_h), nan) and nan[:, 2, 1].all() and not nan[:, :, 0].any()
    assert np.array_equal(got_h.view(np.int32)[~nan], want.view(np.int32)[~nan])
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    if mode == "nonzero":
        assert np.isposinf(got_h[0, 1, 0]) and np.isposinf(got_h[1, 1]).all()      # no non-zero value; the class absent
        assert np.isfinite(got_h[0, 0]).all()
    # pixel-major input and a skipped class / an excluded channel
    flat = torch.from_numpy(act).to(dev).permute(0, 2, 3, 1).reshape(-1, act.shape[1]).contiguous()
    got2 = spx.part_thresholds(flat, torch.from_numpy(lab).to(dev).long(), table, 0.8, mode, grid=(h, w), include=[0, 1, 2, 4],
                               skip_classes=(1,))
    want2 = CR.thresholds(act, lab, table, 0.8, mode, include=[0, 1, 2, 4], skip_classes=(1,))
    assert np.array_equal(got2.cpu().numpy().view(np.int32)[~np.isnan(want2)], want2.view(np.int32)[~np.isnan(want2)])
    assert np.array_equal(np.isnan(got2.cpu().numpy()), np.isnan(want2)) and np.isnan(want2[:, 0, 1]).all()


# ---- presence ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(HERE, "golden", "part_consistency.npz")))


def _case_args(fx, name):
    mode = "image" if name == "image" else "nonzero"
    explicit = fx["explicit"] if name == "explicit" else None
    include = fx["include"].tolist() if name == "filtered" else None
    skip = tuple(fx["skip"].tolist()) if name == "filtered" else ()
    return mode, explicit, include, skip


def _on(dev, fx):
    return (torch.from_numpy(fx["activations"]).to(dev), torch.from_numpy(fx["labels"]).to(dev),
            torch.from_numpy(fx["parts"].astype(np.int32)).to(dev))


@pytest.mark.parametrize("name", CASES)
def test_presence_equals_the_fixture_and_the_restatement(fx, name):
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    M, q, table = int(fx["max_parts"]), float(fx["q"]), fx["slot_table"]
    mode, explicit, include, skip = _case_args(fx, name)
    act, lab, par = _on(dev, fx)
    thr = None if explicit is None else torch.from_numpy(explicit).to(dev)
    tab, valid = spx.part_presence(act, lab, par, table, M, q, mode, thr, include=include, skip_classes=skip)
    assert tab.dtype == torch.uint8 and tab.shape == (4, 3, 2, M + 1) and valid.shape == (4, 3) and tab.is_cuda
    want_tab, want_valid = CR.presence(fx["activations"], fx["labels"], fx["parts"], table, M, q, mode, explicit, include, skip)
    assert np.array_equal(tab.cpu().numpy(), want_tab) and np.array_equal(valid.cpu().numpy(), want_valid)
    rows_tab, rows_valid = CR.rows_to_table(fx[f"rows__{name}"], table, 4, M)
    has_slot = CR.existing(table, 6, include).any(1)
    assert np.array_equal(tab.cpu().numpy(), rows_tab) and np.array_equal(valid.cpu().numpy() * has_slot[None], rows_valid)
    tab2, valid2 = spx.part_presence(act, lab, par, table, M, q, mode, thr, include=include, skip_classes=skip)
    assert torch.equal(tab, tab2) and torch.equal(valid, valid2)


def test_a_part_id_above_max_parts_is_ignored(fx):
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    M, q, table = int(fx["max_parts"]), float(fx["q"]), fx["slot_table"]
    act, lab, par = _on(dev, fx)
    base = spx.part_presence(act, lab, par, table, M, q)
    more = par.clone()
    more[par <= 0] = M + 3                                       # where there was no part: still no part
    got = spx.part_presence(act, lab, more.long(), table, M, q)
    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    # one part fewer: what was part M is no part any more
    less = spx.part_presence(act, lab, par, table, M - 1, q)
    want = CR.presence(fx["activations"], fx["labels"], fx["parts"], table, M - 1, q)
    assert np.array_equal(less[0].cpu().numpy(), want[0]) and np.array_equal(less[1].cpu().numpy(), want[1])
    assert (base[0][..., M] != 255).any()                        # part M did occur


def test_presence_with_negative_activations_and_a_larger_image():
    """0 > T outside the class when T is negative; 70 x 131 from 9 x 11."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    g = np.random.default_rng(3)
    lab, par = _patterns(70, 131)
    table = np.array([[0, 2], [1, -1]])
    act = (g.standard_normal((7, 3, 9, 11)) - 0.7).astype(np.float32)
    for mode in ("nonzero", "image"):
        tab, valid = spx.part_presence(torch.from_numpy(act).to(dev), torch.from_numpy(lab).to(dev), torch.from_numpy(par).to(dev),
                                       table, M_PAT, 0.3, mode)
        want = CR.presence(act, lab, par, table, M_PAT, 0.3, mode)
        assert np.array_equal(tab.cpu().numpy(), want[0]) and np.array_equal(valid.cpu().numpy(), want[1])
        assert (want[0] == 0).any() and (want[0] == 1).any()


# ---- the running metrics -----------------------------------------------------------------------------------------------------
def _same_aggregate(res, agg):
    assert np.array_equal(res.ones.numpy(), agg["ones"]) and np.array_equal(res.times_present.numpy(), agg["times"])
    assert np.array_equal(res.rows.numpy(), agg["rows"])
    assert np.array_equal(res.mean.numpy(), agg["mean"], equal_nan=True)
    assert np.array_equal(res.is_consistent.numpy(), agg["is_consistent"])
    assert res.score == agg["score"] or (np.isnan(res.score) and np.isnan(agg["score"]))


@pytest.mark.parametrize("name", ["nonzero", "filtered", "explicit"])
def test_consistency_over_two_updates(fx, name):
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    M, q, table = int(fx["max_parts"]), float(fx["q"]), fx["slot_table"]
    mode, explicit, include, skip = _case_args(fx, name)
    act, lab, par = _on(dev, fx)
    thr = None if explicit is None else torch.from_numpy(explicit).to(dev)
    m = spx.PartConsistency(3, table, M, dev, q=q, threshold=mode, thresholds=thr, include=include, skip_classes=skip)
    m.update(act[:2], lab[:2], par[:2])
    m.update(act[2:].permute(0, 2, 3, 1).reshape(-1, 6).contiguous(), lab[2:], par[2:], grid=(5, 7))
    res = m.compute()
    tab, valid = CR.presence(fx["activations"], fx["labels"], fx["parts"], table, M, q, mode, explicit, include, skip)
    _same_aggregate(res, CR.consistency([tab], [valid], CR.existing(table, 6, include)))
    assert res.score == float(fx[f"score__{name}"])
    mean, cons = fx[f"mean__{name}"], fx[f"cons__{name}"]
    for r in range(len(cons)):
        k, j = int(mean[r, 0]), list(table[int(mean[r, 0])]).index(int(mean[r, 1]))
        assert np.array_equal(res.mean[k, j].numpy(), mean[r, 2:], equal_nan=True) and int(res.is_consistent[k, j]) == cons[r]
    m2 = spx.PartConsistency(3, table, M, dev, q=q, threshold=mode, thresholds=thr, include=include, skip_classes=skip)
    m2.update(act[:2], lab[:2], par[:2])
    m2.update(act[2:], lab[2:], par[2:])
    assert torch.equal(m._buf, m2._buf)
    m.reset()
    assert int(m._buf.abs().sum()) == 0


def test_consistency_for_prototypes_with_distances(fx):
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    M = int(fx["max_parts"])
    net = proto_net(6, 3, 1, 16, seed=4, device=dev).eval()
    _, lab, par = _on(dev, fx)
    dist = torch.from_numpy(fx["distances"]).to(dev)
    m = spx.PartConsistency.for_prototypes(net, M, consistency_threshold=0.6)
    tab, valid = m.update(labels=lab, parts=par, distances=dist)
    with torch.no_grad():
        act = net.distance_2_similarity(dist).cpu().numpy()      # the activations the device itself produced
    table = m.slot_table_host.numpy()
    want = CR.presence(act, fx["labels"], fx["parts"], table, M, 0.8, "nonzero")
    assert np.array_equal(tab.cpu().numpy(), want[0]) and np.array_equal(valid.cpu().numpy(), want[1])
    _same_aggregate(m.compute(), CR.consistency([want[0]], [want[1]], CR.existing(table, 6), 0.6))
    with pytest.raises(spx.SpxError, match="for_prototypes"):
        spx.PartConsistency(3, table, M, dev).update(labels=lab, parts=par, distances=dist)
    with pytest.raises(spx.SpxError, match="parts are required"):
        m.update(labels=lab, distances=dist)


def test_consistency_for_groups(fx):
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    M = int(fx["max_parts"])
    P, K, S, Cs, G = 12, 3, 2, 16, 2
    net = group_net(P, K, S, Cs, G, seed=6, device=dev).eval()
    conv = torch.randn(4, S * Cs, 5, 7, generator=torch.Generator().manual_seed(9)).to(dev)
    with torch.no_grad():
        _, act = net.forward_from_conv_features(conv, return_activations=True)
        groups = net.compute_group(act)
    _, lab, par = _on(dev, fx)
    m = spx.PartConsistency.for_groups(net, M, threshold="image", q=0.5)
    tab, valid = m.update(groups, lab, par, grid=(5, 7))
    cat = torch.cat(groups, dim=1)
    planes = cat.view(4, 5, 7, K * G).permute(0, 3, 1, 2).cpu().numpy()
    table = m.slot_table_host.numpy()
    assert table.shape == (K, G)
    want = CR.presence(planes, fx["labels"], fx["parts"], table, M, 0.5, "image")
    assert np.array_equal(tab.cpu().numpy(), want[0]) and np.array_equal(valid.cpu().numpy(), want[1])
    _same_aggregate(m.compute(), CR.consistency([want[0]], [want[1]], CR.existing(table, K * G)))


def test_stability(fx):
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    M, q, table = int(fx["max_parts"]), float(fx["q"]), fx["slot_table"]
    act, lab, par = _on(dev, fx)
    m = spx.PartStability(3, table, M, dev, q=q)
    m.update(lab, par, act, act.clone())
    same = m.compute()
    assert same.score == 1.0 and same.valid_rows == len(fx["rows__nonzero"]) == same.stable_rows
    m.reset()
    noisy = fx["activations"].copy()
    noisy[:, :3] = noisy[:, :3][:, :, ::-1, ::-1]                # three prototypes' planes turned round: other pixels win
    noisy[0, 4] += np.random.default_rng(5).standard_normal((5, 7)).astype(np.float32)
    ta, tb, valid = m.update(lab[:2], par[:2], act[:2], torch.from_numpy(noisy[:2]).to(dev))
    m.update(lab[2:], par[2:], act[2:], torch.from_numpy(noisy[2:]).to(dev))
    clean = CR.presence(fx["activations"], fx["labels"], fx["parts"], table, M, q)
    pert = CR.presence(noisy, fx["labels"], fx["parts"], table, M, q)
    assert np.array_equal(tb.cpu().numpy(), pert[0][:2]) and np.array_equal(ta.cpu().numpy(), clean[0][:2])
    stable, rows = CR.stability(clean[0], pert[0], clean[1], CR.existing(table, 6))
    res = m.compute()
    assert (res.stable_rows, res.valid_rows) == (stable, rows) and 0 < stable < rows
    assert res.score == stable / rows


def test_wrong_device_inputs_raise_before_any_launch(fx):
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    act, lab, par = _on(dev, fx)
    with pytest.raises(spx.SpxError, match="no CPU fallback"):
        spx.part_presence(act, lab.cpu(), par, fx["slot_table"], 4)
    with pytest.raises(spx.SpxError, match="no CPU fallback"):
        spx.part_presence(act, lab, par.cpu(), fx["slot_table"], 4)
    with pytest.raises(spx.SpxError, match="thresholds must be"):
        spx.part_presence(act, lab, par, fx["slot_table"], 4, thresholds=torch.zeros(7, device=dev))
