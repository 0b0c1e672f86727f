"""CPU checks of the packed training maps (no device):

* ``PackedLayout``: offsets, M, view strides, the strided views and the label packing, for ``odd`` (M = 376, a multiple of 8),
  ``one_up`` (M = 452, not a multiple of 8) and K = 1; its argument errors;
* the float64 restatement of the pack (tests/msc_pack_cases.py): every segment, read back through the layout's views, is the
  per-segment result of tests/msc_restatement.py;
* the gradient restatement: own term plus ``MR.gradients``, against torch autograd in float64 on the stock formula;
* the recorded training forward of the reference (tests/golden/msc_packed_forward.npz): list structure, shapes and order pinned,
  and ``oracle/ppnet_oracle.py`` reproduces every segment;
* ``msc_pack`` and ``fuse_feature_epilogue(packed=True)`` refuse what they must before any launch; the new entry points are in
  the library and refuse NULL arguments and a packed axis of 2^31 pixels."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import msc_cases as MC
import msc_pack_cases as PC
import msc_restatement as MR
import parity_cases as PAR
from oracle import ppnet_oracle as O
from support import group_net, proto_net

import scaleprotoseg_amd as spx
from scaleprotoseg_amd.msc import PackedLayout


def test_layout_offsets_and_strides():
    odd = PC.layout("odd")
    assert odd.grids == ((7, 9), (4, 5), (6, 7), (7, 9)) and odd.B == 2 and len(odd) == 4
    assert odd.sizes == (126, 40, 84, 126) and odd.offsets == (0, 126, 166, 250) and odd.M == 376 and odd.M % 8 == 0
    assert odd.segments == ((0, 2, 7, 9), (126, 2, 4, 5), (166, 2, 6, 7), (250, 2, 7, 9))
    assert [odd.view_strides(k) for k in range(4)] == [(63, 376, 9, 1), (20, 376, 5, 1), (42, 376, 7, 1), (63, 376, 9, 1)]
    assert odd.column(1, 1, 7) == 126 + 20 + 7 and odd.column(3, 1, 62) == 375
    up = PC.layout("one_up")
    assert up.sizes == (126, 2, 198, 126) and up.offsets == (0, 126, 128, 326) and up.M == 452 and up.M % 8 == 4
    assert up.view_strides(1) == (1, 452, 1, 1)
    ragged = PC.layout("one_up", with_max=False)
    assert ragged.M == 326 and len(ragged) == 3 and ragged.offsets == up.offsets[:3]
    one = PC.layout("odd", K=1)
    assert one.grids == ((7, 9), (7, 9)) and one.M == 252 and one.offsets == (0, 126)
    alone = PC.layout("odd", with_max=False, K=1)
    assert alone.M == 126 and alone.segments == ((0, 2, 7, 9),)
    for bad in (lambda: PackedLayout(0, [(2, 2)]), lambda: PackedLayout(1, []), lambda: PackedLayout(1, [(0, 3)]),
                lambda: PackedLayout(2, [(32768, 32768)])):
        with pytest.raises(spx.SpxError):
            bad()


@pytest.mark.parametrize("name", ["odd", "one_up"])
def test_layout_views_and_labels(name):
    lay = PC.layout(name)
    C_ = 3
    buf = torch.arange(C_ * lay.M, dtype=torch.float32).reshape(1, C_, 1, lay.M)
    for k, (off, B, h, w) in enumerate(lay.segments):
        v = lay.view(buf, k)
        assert tuple(v.shape) == (B, C_, h, w) and v.stride() == lay.view_strides(k) and v.data_ptr() == buf.data_ptr() + 4 * off
        for b, c, i in ((0, 0, 0), (B - 1, C_ - 1, h * w - 1), (B - 1, 1, (h * w) // 2)):
            assert float(v[b, c, i // w, i % w]) == c * lay.M + lay.column(k, b, i)
    # the split of a distance-shaped map gives the same views; row slices are the segments' rows
    parts = lay.split_columns(buf)
    assert all(torch.equal(p, lay.view(buf, k)) and p.stride() == lay.view_strides(k) for k, p in enumerate(parts))
    planes = lay.split_columns(buf.reshape(1, C_, lay.M))
    assert all(tuple(p.shape) == (lay.B, C_, h * w) and torch.equal(p, lay.view(buf, k).reshape(lay.B, C_, -1))
               for k, (p, (h, w)) in enumerate(zip(planes, lay.grids)))
    rows = torch.arange(lay.M * 2).reshape(lay.M, 2)
    assert [tuple(r.shape) for r in lay.split_rows(rows)] == [(n, 2) for n in lay.sizes]
    assert all(int(r[0, 0]) == 2 * o for r, o in zip(lay.split_rows(rows), lay.offsets))
    # labels: one map per segment, concatenated in the columns' order
    labels = [torch.full((lay.B, h, w), k + 1) + torch.arange(lay.B).view(-1, 1, 1) * 10 for k, (h, w) in enumerate(lay.grids)]
    row = lay.pack_labels(labels)
    assert tuple(row.shape) == (1, lay.M)
    for k, (h, w) in enumerate(lay.grids):
        for b in range(lay.B):
            assert (row[0, lay.column(k, b, 0):lay.column(k, b, 0) + h * w] == k + 1 + 10 * b).all()
    for bad in (labels[:3], labels[0], labels[:3] + [labels[3][:, :-1]], [labels[1]] + labels[1:]):
        with pytest.raises(spx.SpxError):
            lay.pack_labels(bad)


@pytest.mark.parametrize("name", PC.CASES)
def test_restatement_of_the_pack(name):
    maps = MC.case(name)["maps"]
    lay = PC.layout(name)
    z, zb, index = PC.restated(name)
    assert z.shape == (maps[0].shape[1], lay.M) and zb.shape == z.shape
    views = [lay.view(torch.from_numpy(z), k).numpy() for k in range(len(lay))]
    for k, m in enumerate(maps):
        assert np.array_equal(views[k], m.astype(np.float64), equal_nan=True)
        assert not lay.view(torch.from_numpy(zb), k).any()
    zmax, imax, bmax = MC.restated(name)[:3]
    assert np.array_equal(views[-1], zmax, equal_nan=True) and np.array_equal(index, imax)
    assert np.array_equal(lay.view(torch.from_numpy(zb), len(maps)).numpy(), bmax, equal_nan=True)
    # the ragged form holds the same plain segments and no maximum
    z0, zb0, none = PC.restated(name, with_max=False)
    assert none is None and np.array_equal(z0, z[:, :z0.shape[1]], equal_nan=True) and not zb0.any()


@pytest.mark.parametrize("sigmoid", [False, True])
@pytest.mark.parametrize("name", ["odd", "one_up", "pascal41"])
def test_gradient_restatement_against_autograd(name, sigmoid):
    """own + gather equals float64 autograd through the stock formula (F.interpolate, torch.max, torch.sigmoid) wherever the
    fixture's index is the float64 one; the bound is finite and positive where a gradient is."""
    c = MC.case(name)
    leaves = [torch.from_numpy(m).double().requires_grad_(True) for m in c["maps"]]
    B, C_, H, W = leaves[0].shape
    up = [leaves[0]] + [F.interpolate(l, size=(H, W), mode="bilinear", align_corners=False) for l in leaves[1:]]
    zmax, index = torch.max(torch.stack(up), dim=0)
    segs = leaves + [zmax]
    if sigmoid:
        segs = [torch.sigmoid(s) for s in segs]
    lay = PC.layout(name)
    gen = torch.Generator().manual_seed(5)
    g = torch.randn(C_, lay.M, generator=gen, dtype=torch.float64)
    y = PC.pack(lay, [s.detach().numpy() for s in segs])
    loss = sum((lay.view(g, k) * s).sum() for k, s in enumerate(segs))
    want = torch.autograd.grad(loss, leaves)
    grads, bounds = PC.gradients([m.shape[2:] for m in c["maps"]], B, index.numpy(), g.numpy(), y if sigmoid else None)
    for k, (got, w, b) in enumerate(zip(grads, want, bounds)):
        assert got.shape == tuple(w.shape) and np.abs(got - w.numpy()).max() <= 1e-12 * max(1.0, np.abs(got).max()), k
        assert np.isfinite(b).all() and (b[np.abs(got) > 0] > 0).all()
    own, ob = PC.gradients([m.shape[2:] for m in c["maps"]], B, None, g.numpy(), y if sigmoid else None, with_max=False)
    assert len(own) == len(leaves) and all(bool((b > 0).all()) == sigmoid for b in ob)      # no maximum: the own term alone


def test_recorded_training_forward():
    c = PC.recorded()
    B, S, Cs, P, K = (int(v) for v in c["shape"])
    grids = [tuple(int(v) for v in g) for g in c["grids"]]
    assert (B, S, Cs, P, K) == (2, 2, 16, 12, 3) and grids == [(7, 9), (4, 5), (6, 7), (7, 9)]
    assert c["tuple_lengths"].tolist() == [[2] * 4, [2] * 4, [3] * 4]          # forward passes its flags to every map (:336)
    bank, head = torch.from_numpy(c["bank"]), torch.from_numpy(c["head"])
    assert torch.equal(bank, O.bf16_representable(bank))
    assert torch.equal(torch.from_numpy(c["identity"]), O.default_class_identity(P, K, S)) and c["ranges"] == O.default_scale_ranges(P, S)
    for k, (h, w) in enumerate(grids):
        conv = torch.from_numpy(c["conv"][k])
        assert tuple(conv.shape) == (B, S * Cs, h, w) and torch.equal(conv, O.bf16_representable(conv))
        assert c["logits"][k].shape == (B, h, w, K) and c["distances"][k].shape == (B, P, h, w)
        assert c["activations"][k].shape == (B * h * w, P)
        logits, dist, act = O.forward_from_conv_features(conv, bank, c["ranges"], S, head)
        PAR.close_fwd(logits, c["logits"][k], "logits")
        PAR.close_fwd(dist, c["distances"][k], "distances")
        PAR.close_fwd(act, c["activations"][k], "activations")
    assert not np.array_equal(c["conv"][0], c["conv"][3])                      # the fourth map is its own, on the first grid


def test_refusals_without_a_device():
    maps = [torch.from_numpy(m) for m in MC.case("odd")["maps"]]
    with pytest.raises(spx.SpxError, match="GPU|gpu|device"):
        spx.msc_pack(maps)
    for bad, kw in (([], {}), (maps * 3, {}), ([maps[0], maps[1].double()], {}), ([maps[0], maps[1][:, :4]], {}),
                    ([maps[0], maps[1].transpose(2, 3)], {}), (maps, dict(activation="relu")), (maps, dict(dtype=torch.float16)),
                    ([maps[0][0]], {})):
        with pytest.raises(spx.SpxError):
            spx.msc_pack(bad, **kw)
    net = proto_net(40, 5, 4, 16, backbone="pool", stride=2)
    with pytest.raises(spx.SpxError, match="MSC"):
        net.fuse_feature_epilogue(torch.bfloat16, packed=True)
    net.features = spx.MSC(net.features)
    net.fuse_feature_epilogue(torch.bfloat16, packed=True)
    assert net._feature_packed and net._feature_epilogue is torch.bfloat16
    net.fuse_feature_epilogue(torch.bfloat16)
    assert not net._feature_packed
    net.fuse_feature_epilogue(torch.bfloat16, packed=True)
    net.fuse_feature_epilogue(None)
    assert not net._feature_packed and net._feature_epilogue is None
    for other in (proto_net(40, 5, 1, 16, cls=spx.PPNet, backbone="pool", stride=2), group_net(40, 5, 4, 16, 3)):
        other.features = spx.MSC(other.features)
        other.fuse_feature_epilogue(torch.bfloat16)                            # the unpacked form stays available
        with pytest.raises(spx.SpxError, match="PPNetMultiScale"):
            other.fuse_feature_epilogue(torch.bfloat16, packed=True)


def test_entry_points_refuse_bad_arguments():
    from scaleprotoseg_amd import _lib

    lib = _lib.load()
    for name in ("spx_msc_pack_fwd", "spx_msc_pack_bwd"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert getattr(lib, name)(None, 1, None) != 0 and b"NULL" in lib.spx_last_error()
    a = _lib.SpxMsc()
    a.K, a.B, a.C, a.in_dtype, a.out_dtype = 2, 3, 1, 1, 1
    for k in range(2):
        a.maps[k].data, a.maps[k].h, a.maps[k].w = 4096, 16384, 16384          # 3 segments of 3 * 2^28 pixels: M = 9 * 2^28 > 2^31
    a.out = 4096
    assert lib.spx_msc_pack_fwd(C.byref(a), 1, None) != 0 and b"M < 2^31" in lib.spx_last_error()
    a.g, a.g_dtype = 4096, 1
    assert lib.spx_msc_pack_bwd(C.byref(a), 1, None) != 0 and b"M < 2^31" in lib.spx_last_error()
    a.maps[0].h = a.maps[0].w = a.maps[1].h = a.maps[1].w = 4
    a.index = None
    assert lib.spx_msc_pack_bwd(C.byref(a), 1, None) != 0 and b"index" in lib.spx_last_error()
    a.K = 9
    assert lib.spx_msc_pack_fwd(C.byref(a), 1, None) != 0 and b"maps" in lib.spx_last_error()
