"""activation_heat_maps / dominant_slot_maps / ExplanationMaps on the GPU against the fixture recorded from the reference's own
plot_activation_proto / plot_activation_group (tests/golden/explanation_maps.npz) and, for other shapes, against the NumPy
restatement (tests/explain_restatement.py).

Bounds.  The outputs are bytes.  The kernel's fp32 sample lies within m0 = 64 * 2^-23 * max|a| of the float64 restatement, so a
byte can differ from the reference's only where that moves it: the "ambiguous" pixels of explain_restatement (a heat value
within 255 * 3 * m0 / d of an integer; two slots within 2 m0 max|wgt| of each other), at most 4 + H*W / 50 per row by a check of
the inputs on the CPU.  Everywhere else the bytes are equal; at an ambiguous pixel the heat byte is within 1 and the dominant
slot is one of the two largest; ``ranges`` are within m0; off the class the dominant map is 255 exactly; rows with hi == lo
are all zeros."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import explain_restatement as E  # noqa: E402
import overlap_restatement as OR  # noqa: E402
from map_cases import BAND_EDGE_WIDE, EXPLAIN_CASES as CASES, band_edge_case, class_planes, planes_of, weights_of  # noqa: E402
from support import bits_equal, gpu_device, group_net  # noqa: E402
from support import release_cached_blocks  # noqa: E402,F401  (a module-scoped autouse fixture, taken by importing its name)

pytestmark = pytest.mark.gpu

LABEL_TYPES = [torch.uint8, torch.int32, torch.int64]


def _strided(planes, dev):
    """The planes as a view into a larger buffer: no stride is the dense one."""
    N, C, h, w = planes.shape
    view = torch.zeros(N, C + 2, h + 1, w + 3, device=dev)[:, 1:C + 1, :h, 2:w + 2]
    view.copy_(torch.from_numpy(planes))
    assert not view.is_contiguous()
    return view


def _check_heat(tag, heat, ranges, want, want_ranges, amb, m0, degenerate):
    """heat uint8 [R, H, W] and ranges [R, 2] from the device against the expected bytes under the ambiguity rule."""
    heat, ranges = heat.cpu().numpy(), ranges.cpu().numpy()
    assert heat.dtype == np.uint8 and heat.shape == want.shape and ranges.dtype == np.float32
    diff = np.abs(heat.astype(np.int64) - want.astype(np.int64))
    print(f"{tag}: {len(want)} heat rows, {int(amb.sum())} ambiguous pixels, {int((diff > 0).sum())} bytes differ (all by "
          f"{int(diff.max())}), ranges off by {np.abs(ranges - want_ranges).max():.3g} (m0 {max(m0):.3g})")
    assert (diff[~amb] == 0).all(), (tag, np.argwhere((diff > 0) & ~amb)[:5])
    assert (diff <= 1).all()
    for i in range(len(want)):
        assert np.abs(ranges[i] - want_ranges[i]).max() <= m0[i], (tag, i, ranges[i], want_ranges[i])
        if degenerate[i]:
            assert not heat[i].any() and ranges[i, 0] == ranges[i, 1]


def _check_dominant(tag, dom, want, amb, first, second, on):
    dom = dom.cpu().numpy()
    assert dom.dtype == np.uint8 and dom.shape == want.shape
    print(f"{tag}: {len(want)} dominant rows, {int(amb.sum())} ambiguous pixels, {int((dom != want).sum())} bytes differ")
    assert (dom[~on] == E.OFF).all()
    assert (dom[~amb] == want[~amb]).all(), (tag, np.argwhere((dom != want) & ~amb)[:5])
    assert ((dom == first) | (dom == second))[amb].all()


def _fixture_expectation(c):
    """What the fixture says, plus the rows of the class that is absent from one image (the reference never visits them; the
    definition gives zeros, resp. 255 everywhere)."""
    planes, lab, table, wgt = planes_of(c), c["labels"], c["table"], weights_of(c)
    N, K = lab.shape[0], table.shape[0]
    H, W = lab.shape[1:]
    absent = [(n, k) for n in range(N) for k in range(K) if not (lab[n] == k + 1).any()]
    extra = [(n, k, j) for n, k in absent for j in range(table.shape[1]) if table[k, j] >= 0]
    rows = np.concatenate([c["heat_rows"], np.array(extra, np.int64)])
    z = len(extra)
    out = dict(planes=planes, rows=rows, heat=np.concatenate([c["heat"], np.zeros((z, H, W), np.uint8)]),
               ranges=np.concatenate([c["ranges"], np.zeros((z, 2), np.float32)]),
               heat_amb=np.concatenate([c["heat_ambiguous"], np.zeros((z, H, W), bool)]),
               degenerate=np.concatenate([c["degenerate"], np.ones(z, bool)]),
               m0=[OR.margin(planes[n, table[k, j]]) for n, k, j in rows])
    rows2 = np.concatenate([c["dom_rows"], np.array(absent, np.int64)])
    on = np.stack([lab[n] == k + 1 for n, k in rows2])
    top = [E.dominant_top2(class_planes(c, n, k), wgt[k], lab[n], k) for n, k in rows2]
    ref = np.concatenate([c["ref_argmax"], np.full((len(absent), H, W), E.OFF, np.uint8)])
    out.update(rows2=rows2, on=on, dom=np.where(on, ref, E.OFF).astype(np.uint8), wgt=wgt,
               dom_amb=np.concatenate([c["dom_ambiguous"], np.zeros((len(absent), H, W), bool)]),
               first=np.stack([t[1] for t in top]), second=np.stack([t[2] for t in top]))
    return out


_EXPECT = {}


def _expect(name):
    if name not in _EXPECT:
        _EXPECT[name] = _fixture_expectation(CASES[name])
    return _EXPECT[name]


@pytest.mark.parametrize("dtype", LABEL_TYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_parity(name, dtype):
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    c, e = CASES[name], _expect(name)
    lab = torch.from_numpy(c["labels"]).to(dtype).to(dev)
    act = _strided(e["planes"], dev)
    table = torch.from_numpy(c["table"])
    heat, ranges = spx.activation_heat_maps(act, lab, torch.from_numpy(e["rows"]), table)
    _check_heat(name, heat, ranges, e["heat"], e["ranges"], e["heat_amb"], e["m0"], e["degenerate"])
    assert e["degenerate"].any()
    wgt = None if str(c["kind"]) == "proto" else torch.from_numpy(e["wgt"]).to(dev)
    dom = spx.dominant_slot_maps(act, lab, torch.from_numpy(e["rows2"]), table, weights=wgt)
    _check_dominant(name, dom, e["dom"], e["dom_amb"], e["first"], e["second"], e["on"])
    for i in np.flatnonzero(c["tied"]):                       # two copies of one plane have the same bits: the first maximum wins
        assert not (dom[i] == 2).any() and (dom[i] == 0).any()
    # the same planes, dense and pixel-major: the same bytes
    dense = torch.from_numpy(e["planes"]).to(dev)
    N, C, h, w = dense.shape
    pix = dense.permute(0, 2, 3, 1).reshape(N * h * w, C).contiguous()
    for a, grid in ((dense, None), (pix, (h, w))):
        again = spx.activation_heat_maps(a, lab, torch.from_numpy(e["rows"]), table, grid=grid)
        assert torch.equal(again[0], heat) and torch.equal(again[1], ranges)
        assert torch.equal(spx.dominant_slot_maps(a, lab, torch.from_numpy(e["rows2"]), table, weights=wgt, grid=grid), dom)


@pytest.mark.parametrize("name", ["proto_5x7_33x41", "group_3x3_17x19"])
def test_every_byte_is_written_and_none_besides(name):
    """The output carved out of a larger buffer of 0xA5 at every alignment: the guard bytes stay, and the bytes between them are
    what the definition says (a surviving 0xA5 would have to be one)."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    c, e = CASES[name], _expect(name)
    lab = torch.from_numpy(c["labels"]).to(dev)
    act = torch.from_numpy(e["planes"]).to(dev)
    table = torch.from_numpy(c["table"])
    wgt = None if str(c["kind"]) == "proto" else torch.from_numpy(e["wgt"]).to(dev)
    H, W = c["labels"].shape[1:]
    assert W % 4 != 0 and (H * W) % 4 != 0
    base_heat, base_ranges = spx.activation_heat_maps(act, lab, torch.from_numpy(e["rows"]), table)
    base_dom = spx.dominant_slot_maps(act, lab, torch.from_numpy(e["rows2"]), table, weights=wgt)
    for guard in (64, 61, 62, 63):
        for rows, run, base in ((e["rows"], lambda out: spx.activation_heat_maps(act, lab, torch.from_numpy(e["rows"]), table, out=out)[0], base_heat),
                                (e["rows2"], lambda out: spx.dominant_slot_maps(act, lab, torch.from_numpy(e["rows2"]), table, weights=wgt, out=out), base_dom)):
            size = len(rows) * H * W
            buf = torch.full((guard + size + 67,), 0xA5, dtype=torch.uint8, device=dev)
            out = buf[guard:guard + size].view(len(rows), H, W)
            assert out.data_ptr() % 4 == guard % 4
            got = run(out)
            assert got.data_ptr() == out.data_ptr()
            assert (buf[:guard] == 0xA5).all() and (buf[guard + size:] == 0xA5).all(), guard
            assert torch.equal(out, base), guard
    _check_heat(name, base_heat, base_ranges, e["heat"], e["ranges"], e["heat_amb"], e["m0"], e["degenerate"])
    _check_dominant(name, base_dom, e["dom"], e["dom_amb"], e["first"], e["second"], e["on"])
    with pytest.raises(spx.SpxError, match="out must be"):
        spx.dominant_slot_maps(act, lab, torch.from_numpy(e["rows2"]), table, weights=wgt, out=torch.empty(1, H, W, dtype=torch.uint8, device=dev))


# ---- 65 x 65 -> 513 x 513: several workgroups per image, against the restatement -----------------------------------------
_BIG = {}


def _big_case():
    """(planes, labels, table, weights, rows, rows2, expectation), computed once and left unchanged."""
    if not _BIG:
        g = np.random.default_rng(20240711)
        N, K, J, h, w, H, W = 1, 4, 3, 65, 65, 513, 513
        table = np.arange(K * J).reshape(K, J)
        table[2, 2] = -1
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        planes = np.zeros((N, K * J, h, w))
        for ch in range(K * J):
            for _ in range(4):
                cy, cx, s, a = g.uniform(0, h - 1), g.uniform(0, w - 1), g.uniform(0.1, 0.3), g.uniform(-0.4, 1.0)
                planes[0, ch] += a * np.exp(-0.5 * (((yy - cy) / (s * h)) ** 2 + ((xx - cx) / (s * w)) ** 2))
            planes[0, ch] += 0.05 * g.random((h, w))
        planes = torch.from_numpy(planes.astype(np.float32)).to(torch.bfloat16).float().numpy()
        cells = g.integers(0, K + 2, (N, 9, 7))                                       # K + 1: a label of no class
        labels = np.stack([np.kron(cells[n], np.ones((57, 74), np.int64))[:H, :W] for n in range(N)])
        wgt = g.uniform(0.5, 1.5, (K, J)).astype(np.float32)
        wgt[1, 0] = -1.0
        rows = np.array([(0, k, j) for k in range(K) for j in range(J) if table[k, j] >= 0], np.int64)
        rows2 = np.array([(0, k) for k in range(K)], np.int64)
        cls = lambda k: [planes[0, c] if c >= 0 else None for c in table[k]]
        maps = [E.heat_map(planes[0, table[k, j]], labels[0], k) for _, k, j in rows]
        top = [E.dominant_top2(cls(k), wgt[k], labels[0], k) for _, k in rows2]
        e = dict(heat=np.stack([m[0] for m in maps]), ranges=np.array([(m[1], m[2]) for m in maps], np.float32),
                 heat_amb=np.stack([E.heat_ambiguous(planes[0, table[k, j]], labels[0], k) for _, k, j in rows]),
                 m0=[OR.margin(planes[0, table[k, j]]) for _, k, j in rows], degenerate=np.zeros(len(rows), bool),
                 dom=np.stack([E.dominant(cls(k), wgt[k], labels[0], k) for _, k in rows2]), on=np.stack([labels[0] == k + 1 for _, k in rows2]),
                 dom_amb=np.stack([t[0] for t in top]), first=np.stack([t[1] for t in top]), second=np.stack([t[2] for t in top]))
        cap = 4 + H * W / 50                                                          # the condition on the inputs, as in the tool
        assert (e["heat_amb"].reshape(len(rows), -1).sum(1) <= cap).all() and (e["dom_amb"].reshape(len(rows2), -1).sum(1) <= cap).all()
        assert all((labels[0] == k + 1).sum() > 10000 for k in range(K))
        _BIG.update(planes=planes, labels=labels, table=table, wgt=wgt, rows=rows, rows2=rows2, e=e)
    return _BIG


def test_513_against_the_restatement_and_itself():
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    b = _big_case()
    e = b["e"]
    act, lab = torch.from_numpy(b["planes"]).to(dev), torch.from_numpy(b["labels"]).to(dev)
    table, wgt = torch.from_numpy(b["table"]), torch.from_numpy(b["wgt"]).to(dev)
    rows, rows2 = torch.from_numpy(b["rows"]), torch.from_numpy(b["rows2"])
    heat, ranges = spx.activation_heat_maps(act, lab, rows, table)
    dom = spx.dominant_slot_maps(act, lab, rows2, table, weights=wgt)
    _check_heat("513", heat, ranges, e["heat"], e["ranges"], e["heat_amb"], e["m0"], e["degenerate"])
    _check_dominant("513", dom, e["dom"], e["dom_amb"], e["first"], e["second"], e["on"])
    assert (heat.amax((1, 2)) == 255).all() and (heat.amin((1, 2)) == 0).all()        # the extremes are exact: r = d and r = 0
    heat2, ranges2 = spx.activation_heat_maps(act, lab, rows, table)
    assert torch.equal(heat2, heat) and torch.equal(ranges2.view(torch.int32), ranges.view(torch.int32))
    assert torch.equal(spx.dominant_slot_maps(act, lab, rows2, table, weights=wgt), dom)


# ---- 129 x 65 -> 140 x 70: five bands over a plane that no band stages whole, tied to the masked select ----------------------
def test_ranges_of_a_partially_staged_plane_hold_the_selects_own_pixels():
    """A class of one pixel has the range (min(0, v), max(0, v)), and v is the class's masked threshold: the range pass and the
    select recompute that pixel from their own staged rows, and the bits are the same.  A class across the edge of a band
    against the restatement."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    c = band_edge_case("partially_staged_129x65")
    act, lab = torch.from_numpy(c["planes"]).to(dev), torch.from_numpy(c["labels"]).to(dev)
    table = torch.tensor([[0, 1]] * BAND_EDGE_WIDE)
    lone = [(L, j) for L in c["lone"] for j in range(2)]
    rows = torch.tensor([(0, L - 1, j) for L, j in lone] + [(0, BAND_EDGE_WIDE - 1, 0)])
    _, ranges = spx.activation_heat_maps(act, lab, rows, table)
    v = spx.high_activation_threshold_masked(act, lab, torch.tensor([(0, j, L) for L, j in lone]))
    assert torch.isfinite(v).all()
    zero = torch.zeros_like(v)
    assert bits_equal(ranges[:len(lone)], torch.stack([torch.minimum(v, zero), torch.maximum(v, zero)], dim=1))
    _, lo, hi = E.heat_map(c["planes"][0, 0], c["labels"][0], BAND_EDGE_WIDE - 1)
    assert lo < 0 < hi and np.abs(ranges[-1].cpu().numpy() - np.array([lo, hi])).max() <= OR.margin(c["planes"][0, 0])


# ---- the module ------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["group_5x7_33x41", "group_3x3_17x19"])
def test_for_groups_on_a_real_module(name):
    """The group path end to end: slots and weights from a PPNetMultiScaleGroup whose last_layer_group holds the fixture's head
    (a negative weight flips the argmax of class 0), the list compute_group returns as input."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    c, e = CASES[name], _expect(name)
    K, G, S, Cs = 3, 3, 2, 16
    torch.manual_seed(3)
    net = group_net(12, K, S, Cs, G, device=dev).eval()
    assert tuple(net.last_layer_group.weight.shape) == tuple(c["head"].shape)
    net.last_layer_group.weight.data.copy_(torch.from_numpy(c["head"]))
    ex = spx.ExplanationMaps.for_groups(net)
    assert np.array_equal(ex.slot_table.numpy(), c["table"])
    planes = torch.from_numpy(e["planes"]).to(dev)
    N, U, h, w = planes.shape
    groups = list(torch.split(planes.permute(0, 2, 3, 1).reshape(N * h * w, U), G, dim=1))       # what compute_group returns
    lab = torch.from_numpy(c["labels"]).to(dev)
    rows, rows2 = ex.rows_for(lab)
    assert np.array_equal(rows.numpy(), c["heat_rows"]) and np.array_equal(rows2.numpy(), c["dom_rows"])
    dom = ex.dominant_slots(torch.from_numpy(e["rows2"]), groups, lab, grid=(h, w))
    _check_dominant(name, dom, e["dom"], e["dom_amb"], e["first"], e["second"], e["on"])
    plain = spx.dominant_slot_maps(planes, lab, torch.from_numpy(e["rows2"]), ex.slot_table)
    on0 = torch.from_numpy(e["on"][0]).to(dev)
    assert (plain[0] != dom[0])[on0].float().mean() > 0.25                                       # the negative weight matters
    heat, ranges = ex.heat_maps(torch.from_numpy(e["rows"]), groups, lab, grid=(h, w))
    _check_heat(name, heat, ranges, e["heat"], e["ranges"], e["heat_amb"], e["m0"], e["degenerate"])
    # the weights are read at every call: an in-place edit is seen
    net.last_layer_group.weight.data.fill_(1.0)
    assert torch.equal(ex.dominant_slots(torch.from_numpy(e["rows2"]), groups, lab, grid=(h, w)), plain)


def test_for_prototypes_with_distances_and_no_synchronisation():
    """The module's two methods from ``distances=``, under torch's sync debug mode (the check the other modules' tests use):
    nothing in them waits for the device."""
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    c = CASES["proto_5x7_33x41"]

    class Net:
        num_classes = 3
        prototype_class_identity = torch.from_numpy(c["ident"])
        epsilon = 1e-4

        def distance_2_similarity(self, d):
            return torch.log((d + 1) / (d + self.epsilon))

    net = Net()
    ex = spx.ExplanationMaps.for_prototypes(net)
    dist = torch.from_numpy(c["distances"]).to(dev)
    lab = torch.from_numpy(c["labels"]).to(dev)
    rows, rows2 = ex.rows_for(lab)
    assert np.array_equal(rows.numpy(), c["heat_rows"]) and np.array_equal(rows2.numpy(), c["dom_rows"])
    act = net.distance_2_similarity(dist)
    want_heat, want_ranges = spx.activation_heat_maps(act, lab, rows, ex.slot_table)
    want_dom = spx.dominant_slot_maps(act, lab, rows2, ex.slot_table)
    ex.dominant_slots(rows2, labels=lab, distances=dist)                  # (the first call on a device uploads the slot table)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        heat, ranges = ex.heat_maps(rows, labels=lab, distances=dist)
        dom = ex.dominant_slots(rows2, labels=lab, distances=dist)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.equal(heat, want_heat) and torch.equal(ranges, want_ranges) and torch.equal(dom, want_dom)
    # the device's own log differs from NumPy's by an ulp here and there, so against the fixture every byte is within one
    assert (heat.cpu().numpy().astype(np.int64) - c["heat"]).__abs__().max() <= 1
