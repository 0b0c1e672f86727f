"""CPU checks of the multi-scale input fusion (no device):

* tests/msc_restatement.py reproduces what the reference's REAL ``MSC`` recorded (tests/golden/msc_features*.npz,
  tools/gen_msc_golden.py): ``logits_max`` within the per-element bound, the index wherever the float64 gap between the best and
  the second candidate exceeds the sum of their bounds, the gradients (with the reference's index) within the gradient bound;
  on the generated case of eight maps (tests/msc_cases.py) it reproduces the stock torch formula, the index on every pixel;
* ``spx.MSC`` on CPU tensors (the reference's stock formula) matches the fixture in eval and training mode; ``scales=[]``, a
  list-returning base, ``state_dict`` keys and ``str()``; ``PPNetMultiScale(spx.MSC(base), ...)`` constructs;
* ``msc_max`` refuses CPU tensors and every malformed input before any launch; ``fuse_feature_epilogue`` refuses a backbone that
  is not an ``spx.MSC`` and an add-on that is not the bare sigmoid."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import msc_cases as MC
import msc_restatement as MR
from support import proto_net

import scaleprotoseg_amd as spx


@pytest.mark.parametrize("name", MC.SHAPE_SETS + MC.SPECIAL)
def test_restatement_reproduces_the_reference_maximum(name):
    c = MC.case(name)
    z, idx, zb, u, b = MC.restated(name)
    ref = c["logits_max"].astype(np.float64)
    nan = np.isnan(ref)
    assert np.array_equal(nan, np.isnan(z))
    err = np.abs(z - ref)[~nan]
    ratio = err[zb[~nan] > 0] / zb[~nan][zb[~nan] > 0]
    print(f"{name}: reference error / bound at most {ratio.max() if ratio.size else 0.0:.3f}")
    assert (err <= zb[~nan]).all()
    sure = MR.decided(u, b) & ~nan
    assert np.array_equal(idx[sure], c["index"][sure])
    if name in MC.SHAPE_SETS:
        assert 1.0 - sure.mean() <= 1.2e-4        # what the restatement alone leaves undecided on these inputs
    if name == "tie":
        tied = c["maps"][0] == 0.5
        assert tied.sum() >= 100 and (idx[tied] == 0).all() and (c["index"][tied] == 0).all()       # the lowest k
    if name == "nan":
        assert nan.sum() >= 3 and np.array_equal(idx[nan], c["index"][nan])                          # the first NaN's index
        both = np.isnan(c["maps"][0]) & nan
        assert both.sum() == 2 and (idx[both] == 0).all()


@pytest.mark.parametrize("name", MC.SHAPE_SETS + ("tie",))
def test_restatement_reproduces_the_reference_gradients(name):
    c = MC.case(name)
    grads, bounds = MR.gradients([m.shape[2:] for m in c["maps"]], c["index"], c["g"])
    for k, (g, b) in enumerate(zip(grads, bounds)):
        err = np.abs(g - c[f"d{k}"])
        assert g.shape == c[f"d{k}"].shape and (err <= b).all(), (k, (err - b).max())
        assert k == 0 or np.abs(g).max() > 0 or name == "tie"


def test_restatement_reproduces_the_stock_formula_on_eight_maps():
    """The generated case with as many maps as the kernels take: float64 decides every pixel, every map wins its share, and the
    stock ``F.interpolate`` + ``torch.max`` formula is within the bound with an equal index."""
    maps = [torch.from_numpy(m) for m in MC.case("eight")["maps"]]
    z, idx, zb, u, b = MC.restated("eight")
    assert len(maps) == 8 and idx.size == 630 and MR.decided(u, b).all()
    assert np.bincount(idx.ravel(), minlength=8).min() >= 45
    H, W = maps[0].shape[2:]
    up = [maps[0]] + [F.interpolate(m, size=(H, W), mode="bilinear", align_corners=False) for m in maps[1:]]
    ref, ref_index = torch.max(torch.stack(up), dim=0)
    assert (np.abs(z - ref.numpy().astype(np.float64)) <= zb).all() and np.array_equal(idx, ref_index.numpy())
    grids = [m.shape[2:] for m in maps]
    assert spx.PackedLayout.of_maps(2, grids).M == 880 and spx.PackedLayout.of_maps(2, grids, with_max=False).M == 754


class _TableBase(nn.Module):
    """Hands out the recorded map for the input's size, as the stand-in of the golden tool did; two convolutions for the
    width dispatch of the model constructors."""

    def __init__(self, table):
        super().__init__()
        self.convs = nn.Sequential(nn.Conv2d(3, 5, 1), nn.Conv2d(5, 5, 1))
        self.table = table

    def forward(self, x):
        return self.table[tuple(x.shape[2:])]


def _recorded_module(c):
    x = torch.zeros(tuple(int(v) for v in c["x_shape"]))
    scales = [float(p) for p in c["scales"]]
    sizes = [tuple(x.shape[2:])] + [(int(np.floor(x.shape[2] * p)), int(np.floor(x.shape[3] * p))) for p in scales]
    maps = [torch.from_numpy(m) for m in c["maps"]]
    return spx.MSC(_TableBase(dict(zip(sizes, maps))), scales=scales), x, maps


@pytest.mark.parametrize("name", MC.SHAPE_SETS + MC.SPECIAL)
def test_module_on_cpu_matches_the_fixture(name):
    c = MC.case(name)
    msc, x, maps = _recorded_module(c)
    msc.eval()
    out = msc(x)
    ref = torch.from_numpy(c["logits_max"])
    assert out.shape == ref.shape and torch.equal(out.isnan(), ref.isnan()) and torch.equal(out.nan_to_num(0.0), ref.nan_to_num(0.0))
    msc.train()
    lst = msc(x)
    assert isinstance(lst, list) and len(lst) == len(maps) + 1
    assert [tuple(t.shape) for t in lst] == [tuple(int(v) for v in s) for s in c["train_shapes"]]
    assert all(a is b for a, b in zip(lst[:-1], maps))
    assert torch.equal(lst[-1].nan_to_num(0.0), ref.nan_to_num(0.0))


def test_module_surface():
    base = nn.Sequential(nn.Conv2d(3, 8, 1), nn.Conv2d(8, 8, 1))
    m = spx.MSC(base)
    assert m.base is base and m.scales == [0.5, 0.75]
    assert spx.MSC(base, scales=[0.25]).scales == [0.25]
    assert list(m.state_dict()) == ["base.0.weight", "base.0.bias", "base.1.weight", "base.1.bias"]
    assert str(m).startswith("MSC")
    x = torch.randn(1, 3, 8, 8)
    none = spx.MSC(base, scales=[])
    for mode in (True, False):
        none.train(mode)
        assert torch.equal(none(x), base(x))

    class Lists(nn.Module):
        def forward(self, x):
            return [x, x]

    out = spx.MSC(Lists(), scales=[])(x)
    assert isinstance(out, list) and out[0] is x
    with pytest.raises(NotImplementedError):
        spx.MSC(Lists())(x)


def test_model_constructs_around_the_module():
    """The add-on width the name dispatch takes from ``features.base``: what it is with the reference's class."""
    base = nn.Sequential(nn.Conv2d(3, 48, 1), nn.Conv2d(48, 32, 1), nn.Conv2d(32, 24, 1))
    for kind, first in (("deeplab_simple", None), ("bottleneck", 32)):
        net = spx.PPNetMultiScale(spx.MSC(base), 64, (20, 16, 1, 1), [], 5, add_on_layers_type=kind, patch_classification=True,
                                  num_scales=2)
        assert isinstance(net.features, spx.MSC)
        convs = [m for m in net.add_on_layers.modules() if isinstance(m, nn.Conv2d)]
        assert (convs[0].in_channels if convs else None) == first            # convs(base)[-2].out_channels = 32
    assert [k for k in net.state_dict() if k.startswith("features.")][0] == "features.base.0.weight"


def test_msc_max_refuses_bad_inputs_on_the_host():
    t = torch.zeros(2, 5, 7, 9)
    with pytest.raises(spx.SpxError, match="no CPU fallback"):
        spx.msc_max([t])
    with pytest.raises(spx.SpxError, match="activation"):
        spx.msc_max([t], activation="relu")
    with pytest.raises(spx.SpxError, match="0 maps"):
        spx.msc_max([])
    with pytest.raises(spx.SpxError, match="9 maps"):
        spx.msc_max([t] * 9)
    with pytest.raises(spx.SpxError, match="mixed dtypes"):
        spx.msc_max([t, t.bfloat16()])
    with pytest.raises(spx.SpxError, match="float32 or bfloat16"):
        spx.msc_max([t.half()])
    with pytest.raises(spx.SpxError, match="float32 or bfloat16"):
        spx.msc_max([t], dtype=torch.float16)
    for other in (torch.zeros(3, 5, 4, 5), torch.zeros(2, 4, 4, 5)):
        with pytest.raises(spx.SpxError, match=r"\(B, C\)"):
            spx.msc_max([t, other])
    with pytest.raises(spx.SpxError, match="not contiguous"):
        spx.msc_max([t, torch.zeros(2, 5, 4, 10)[..., ::2]])
    with pytest.raises(spx.SpxError, match="not contiguous"):
        spx.msc_max([t.permute(0, 1, 3, 2)])
    for bad in (torch.zeros(2, 5, 7, 8), torch.zeros(2, 5, 7, 9, dtype=torch.bfloat16), torch.zeros(2, 5, 9, 7).permute(0, 1, 3, 2)):
        with pytest.raises(spx.SpxError, match="out must be"):
            spx.msc_max([t], out=bad)
    with pytest.raises(spx.SpxError, match="no CPU fallback"):          # a well-formed call still needs the device
        spx.msc_max([t[:, 1:4], torch.zeros(2, 3, 1, 1)], activation="sigmoid", dtype=torch.bfloat16)
    # the C entry points refuse the same before any launch
    from scaleprotoseg_amd import _lib

    lib = _lib.load()
    a = _lib.SpxMsc()
    for fn in (lib.spx_msc_max_fwd, lib.spx_msc_max_bwd):
        assert fn(None, None) != 0 and b"NULL" in lib.spx_last_error()
        a.K = 9
        assert fn(C.byref(a), None) != 0 and b"9 maps" in lib.spx_last_error()
    a.K, a.B, a.C, a.in_dtype = 1, 1, 1, 2
    assert lib.spx_msc_max_fwd(C.byref(a), None) != 0 and b"dtype" in lib.spx_last_error()
    a.in_dtype, a.out_dtype, a.activation = 1, 1, 3
    assert lib.spx_msc_max_fwd(C.byref(a), None) != 0 and b"activation" in lib.spx_last_error()
    a.activation = 0
    assert lib.spx_msc_max_fwd(C.byref(a), None) != 0 and b"map 0 is NULL" in lib.spx_last_error()
    assert C.sizeof(_lib.SpxMscMap) == 32 and C.sizeof(_lib.SpxMsc) == 8 * 32 + 8 * 8 + 3 * 8 + 8 * 4


def test_fuse_feature_epilogue_refuses_what_it_cannot_fuse():
    net = proto_net(20, 5, 2, 16)                                  # the Backbone stand-in is not an spx.MSC
    with pytest.raises(spx.SpxError, match="not scaleprotoseg_amd.MSC"):
        net.fuse_feature_epilogue()
    base = nn.Sequential(nn.Conv2d(3, 32, 1), nn.Conv2d(32, 32, 1), nn.Conv2d(32, 32, 1))
    for cls, kw in ((spx.PPNetMultiScale, dict(num_scales=2)), (spx.PPNet, {}), (spx.PPNetMultiScaleGroup, dict(num_scales=2, num_groups=3))):
        neck = cls(spx.MSC(base), 64, (20, 16, 1, 1), [], 5, add_on_layers_type="bottleneck", patch_classification=True, **kw)
        with pytest.raises(spx.SpxError, match="nn.Sigmoid"):
            neck.fuse_feature_epilogue(torch.bfloat16)
        ok = cls(spx.MSC(base), 64, (20, 16, 1, 1), [], 5, add_on_layers_type="deeplab_simple", patch_classification=True, **kw)
        assert ok._feature_epilogue is None
        ok.fuse_feature_epilogue(torch.bfloat16)
        assert ok._feature_epilogue is torch.bfloat16
        with pytest.raises(spx.SpxError, match="dtype"):
            ok.fuse_feature_epilogue(torch.float16)
        ok.fuse_feature_epilogue(None)
        assert ok._feature_epilogue is None
        assert "_feature_epilogue" not in ok.state_dict()
