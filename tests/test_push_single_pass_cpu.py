"""The single-pass batched push without a GPU: the rule of spx_push_merge (tests/push_merge_restatement.py) against the CPU
oracle, the driver (push_single_pass / push_prototypes_multiscale(batch_size=...)) with its two device steps replaced by
oracle-based callables against today's two-pass push, argument errors and the ABI.  Everything is an equality of bits."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import push_merge_restatement as R  # noqa: E402
from oracle import ppnet_oracle as O  # noqa: E402
from scaleprotoseg_amd import PushTable, push_single_pass  # noqa: E402,F401  (the feature under test: no test here runs without it)
from test_dp_gloo import _patch_kernels_with_oracle, _run  # noqa: E402

QUIET = dict(log=lambda *_: None, device="cpu")


# ---- the rule against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 4])
def test_restatement_equals_the_oracle(S):
    N, per, Cs, H, W = 7, 3, 4, 3, 5
    P = S * per
    g = torch.Generator().manual_seed(40 + S)
    levels = torch.tensor([0.25, 0.5, 0.75, 2.0])
    vals = levels[torch.randint(0, 4, (N, P), generator=g)]                 # four levels: ties inside and across batches
    vals[:, 1] = 1e10                                                       # a prototype whose class never appears ...
    idx = torch.randint(0, H * W, (N, P), generator=g)
    idx[:, 1] = 0                                                           # ... has flat index 0 in every image
    convs = [torch.rand(1, S * Cs, H, W, generator=g) for _ in range(N)]
    best = O.min_across_images([vals[i:i + 1] for i in range(N)])
    bank = O.gather_push_patches(convs, best, [idx[i:i + 1] for i in range(N)], S, P).reshape(P, Cs)
    ar = torch.arange(P)
    scale = torch.tensor([p // (P // S) for p in range(P)])
    for batch in (1, 2, 3, N + 5):
        st = R.merge_all(P, Cs, idx, vals, torch.cat(convs), scale, batch)
        assert torch.equal(st["best_image"], best), batch
        assert torch.equal(st["best_flat"], idx[best, ar]) and torch.equal(st["best_value"], vals[best, ar])
        assert np.array_equal(st["best_patch"].numpy(), bank)
    assert int(best[1]) == 0 and float(vals[0, 1]) == 1e10


def test_restatement_nan_never_wins_and_an_equal_value_does_not_replace():
    st = R.new_state(2, 1)
    x = torch.arange(6, dtype=torch.float32).reshape(3, 2, 1, 1) + 1
    scale = torch.tensor([0, 1])
    R.merge(st, torch.zeros(3, 2, dtype=torch.int64), torch.tensor([[float("nan"), 3.0], [2.0, float("nan")], [2.0, 3.0]]), x, scale, 10)
    assert st["best_image"].tolist() == [11, 10] and st["best_value"].tolist() == [2.0, 3.0]
    assert st["best_patch"].flatten().tolist() == [3.0, 2.0]
    before = {k: v.clone() for k, v in st.items()}
    R.merge(st, torch.zeros(1, 2, dtype=torch.int64), torch.tensor([[2.0, float("nan")]]), x[:1], scale, 13)
    assert all(torch.equal(st[k], before[k]) for k in st)


# ---- the driver, device steps replaced ---------------------------------------------------------------------------------
class _Identity(torch.nn.Module):
    """Stand-in backbone: the data set's "images" ARE the features [S * Cs, h, w], so an image's features do not depend on its
    batch mates (a CPU convolution may round differently per batch shape).  ``str()`` starts with MSC and ``.base`` holds two
    Conv2d, which is all the model's constructor asks of a backbone."""

    def __init__(self, ch):
        super().__init__()
        self.base = torch.nn.Sequential(torch.nn.Conv2d(3, ch, 1), torch.nn.Conv2d(ch, ch, 1))

    def __repr__(self):
        return "MSC(standin)"

    def forward(self, x):
        return x


class _Data:
    """Feature "images" of the given latent (h, w) sizes in order; targets at four times that size, one label per latent
    pixel, class ``absent`` never appears."""

    convert_targets = None

    def __init__(self, sizes, K, absent, seed, channels=None):
        g = torch.Generator().manual_seed(seed)
        self.items = []
        for h, w in sizes:
            img = torch.rand(channels or S_ * CS_, h, w, generator=g)
            t = torch.randint(0, K + 1, (h, w), generator=g).repeat_interleave(4, 0).repeat_interleave(4, 1)
            t[t == absent + 1] = 0
            self.items.append((img, t.numpy()))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


S_, CS_, K_, PER_ = 2, 16, 3, 2
SAME = [(6, 8)] * 7
MIXED = [(6, 8)] * 2 + [(8, 10)] * 3 + [(6, 8)] + [(8, 6)]                # runs break at 2, 5 and 6


def _setup(sizes):
    import scaleprotoseg_amd as spx

    P = S_ * K_ * PER_
    torch.manual_seed(11)
    net = spx.PPNetMultiScale(_Identity(S_ * CS_), 64, (P, CS_, 1, 1), [], K_, add_on_layers_type="deeplab_simple",
                              patch_classification=True, num_scales=S_)
    net.add_on_layers = torch.nn.Identity()
    with torch.no_grad():
        net.prototype_vectors[1].copy_(net.prototype_vectors[0])          # forced duplicate
    return net, _Data(sizes, K_, absent=2, seed=12)


def _replace_device_steps():
    """push_run_minima / push_run_merge on the oracle and the restatement (tests only; the product path never does)."""
    from scaleprotoseg_amd import push as push_mod

    def minima(net, conv, labels, void_class, max_dist=1e10):
        ranges = {s: tuple(net.scale_num_prototypes[s]) for s in range(net.num_scales)}
        d = O.scale_l2_convolution(conv, net.prototype_vectors.detach(), ranges, net.num_scales)
        return O.push_masked_argmin(d, labels, net.prototype_class_identity, net.num_classes, max_dist, void_class)

    def merge(table, idx, val, conv, proto_scale, image0):
        B = table.check(idx, val, conv, proto_scale, image0)
        R.merge(dict(best_value=table.best_value, best_image=table.best_image, best_flat=table.best_flat,
                     best_patch=table.best_patch), idx, val, conv, proto_scale, image0)
        table.next_image = int(image0) + B

    push_mod.push_run_minima = minima
    push_mod.push_run_merge = merge


@pytest.fixture
def steps(monkeypatch):
    """Both paths on the CPU for one test: today's compute_distances / argmin_over_images as tests/test_dp_gloo.py replaces
    them, and the single pass's two device steps; everything is put back afterwards."""
    from scaleprotoseg_amd import push as push_mod

    for name in ("compute_distances", "argmin_over_images", "push_run_minima", "push_run_merge"):
        monkeypatch.setattr(push_mod, name, getattr(push_mod, name))        # registers the restore
    _patch_kernels_with_oracle(S_)
    _replace_device_steps()


def _state(net, root=None):
    out = dict(bank=net.prototype_vectors.detach().clone(), ranges={s: tuple(net.scale_num_prototypes[s]) for s in range(S_)},
               last=net.last_layer.weight.detach().clone(), ident=net.prototype_class_identity.clone())
    if root is not None:
        out["json"] = json.load(open(os.path.join(root, "unique_prototypes.json")))
    return out


def _same_state(a, b):
    assert torch.equal(a["bank"], b["bank"]) and torch.equal(a["last"], b["last"]) and torch.equal(a["ident"], b["ident"])
    assert a["ranges"] == b["ranges"] and a.get("json") == b.get("json")


def _spy(net):
    calls = []
    orig = net.conv_features

    def conv_features(x):
        calls.append(int(x.shape[0]))
        return orig(x)

    net.conv_features = conv_features
    return calls


@pytest.mark.parametrize("sizes", [SAME, MIXED], ids=["same", "mixed"])
@pytest.mark.parametrize("batch", [1, 3])
def test_driver_equals_the_two_pass_push(steps, tmp_path, sizes, batch):
    from scaleprotoseg_amd.push import push_prototypes_multiscale

    net0, data = _setup(sizes)
    calls0 = _spy(net0)
    best0, list_idx, dup0 = push_prototypes_multiscale(data, net0, str(tmp_path / "two"), **QUIET)
    assert isinstance(list_idx, list) and 1 in dup0 and len(dup0) >= 2
    flat0 = torch.cat(list_idx)[best0, torch.arange(len(best0))]

    net1, _ = _setup(sizes)
    calls1 = _spy(net1)
    best1, flat1, dup1 = push_prototypes_multiscale(data, net1, str(tmp_path / "one"), batch_size=batch, **QUIET)
    assert isinstance(flat1, torch.Tensor) and flat1.dtype == torch.int64
    assert torch.equal(best1, best0) and torch.equal(flat1, flat0) and list(dup1) == list(dup0)      # GLOBAL image indices
    _same_state(_state(net1, tmp_path / "one"), _state(net0, tmp_path / "two"))

    # one encoding per run of equally sized images, against N + one per distinct winner
    runs, last = [], None
    for h, w in sizes:
        if last == (h, w) and runs[-1] < batch:
            runs[-1] += 1
        else:
            runs.append(1)
        last = (h, w)
    assert calls1 == runs
    assert len(calls0) == len(sizes) + len(set(best0.tolist())) and set(calls0) == {1}


def _dp_case(rank, world):
    from scaleprotoseg_amd.push import push_prototypes_multiscale

    net, data = _setup(MIXED)
    _replace_device_steps()
    calls = _spy(net)
    best, flat, dup = push_prototypes_multiscale(data, net, batch_size=3, **QUIET)
    return _state(net), best.clone(), flat.clone(), list(dup), sum(calls)


def test_sharded_driver_equals_the_two_pass_push(steps, tmp_path):
    from scaleprotoseg_amd.push import push_prototypes_multiscale

    res = _run(_dp_case, tmp_path)
    net0, data = _setup(MIXED)
    best0, list_idx, dup0 = push_prototypes_multiscale(data, net0, **QUIET)
    flat0 = torch.cat(list_idx)[best0, torch.arange(len(best0))]
    for state, best, flat, dup, images in res:
        _same_state(state, _state(net0))
        assert torch.equal(best, best0) and torch.equal(flat, flat0) and dup == list(dup0)
    assert sum(r[4] for r in res) == len(MIXED)                              # every image encoded once, on one rank


def test_a_rank_with_an_empty_shard_never_wins(steps):
    from scaleprotoseg_amd.push import push_single_pass

    net, data = _setup(SAME)
    table = push_single_pass(data, net, batch_size=3, image_range=range(4, 4), device="cpu")
    assert torch.isinf(table.best_value).all() and (table.best_image == -1).all() and table.next_image == 0
    part = push_single_pass(data, net, batch_size=3, image_range=range(4, 7), device="cpu")
    assert ((part.best_image >= 4) & (part.best_image < 7)).all()


# ---- argument errors ---------------------------------------------------------------------------------------------------
def test_argument_errors(steps):
    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd.push import proto_scale_table, push_single_pass

    net, data = _setup(SAME)
    with pytest.raises(spx.SpxError, match="batch_size"):
        push_single_pass(data, net, batch_size=0, device="cpu")
    with pytest.raises(spx.SpxError, match="batch_size"):
        spx.push_prototypes_multiscale(data, net, batch_size=0, **QUIET)
    one = net.conv_features
    net.conv_features = lambda x: [one(x), one(x)]
    with pytest.raises(spx.SpxError, match="MSC"):
        push_single_pass(data, net, batch_size=2, device="cpu")

    P, Cs = 6, 4
    table = spx.PushTable(P, Cs, "cpu")
    idx, val = torch.zeros(2, P, dtype=torch.int64), torch.zeros(2, P)
    conv, scale = torch.zeros(2, 2 * Cs, 3, 3), torch.zeros(P, dtype=torch.int32)
    with pytest.raises(spx.SpxError, match="no CPU fallback"):
        table.merge(idx, val, conv, scale, 0)
    assert table.next_image == 0 and torch.isinf(table.best_value).all()
    with pytest.raises(spx.SpxError, match="table holds 6"):
        table.merge(idx[:, :5], val[:, :5], conv, scale, 0)
    with pytest.raises(spx.SpxError, match="int64"):
        table.merge(idx.int(), val, conv, scale, 0)
    with pytest.raises(spx.SpxError, match="contiguous"):
        table.merge(idx, val, conv.permute(0, 1, 3, 2), scale, 0)
    with pytest.raises(spx.SpxError, match="proto_scale"):
        table.merge(idx, val, conv, scale.long(), 0)
    table.next_image = 8
    with pytest.raises(spx.SpxError, match="increasing image order"):
        table.merge(idx, val, conv, scale, 7)

    assert proto_scale_table(6, 2) == [0, 0, 0, 1, 1, 1]
    with pytest.raises(spx.SpxError, match="channel block 2 of 2"):
        proto_scale_table(7, 2)


def test_a_scale_block_past_the_features_is_refused_before_any_image_is_encoded():
    import scaleprotoseg_amd as spx

    class Net:
        num_prototypes, num_scales = 7, 2
        prototype_vectors = torch.zeros(7, 4, 1, 1)
        prototype_shape = prototype_vectors.shape

        def eval(self):
            return self

        def conv_features(self, x):
            raise AssertionError("encoded an image")

    with pytest.raises(spx.SpxError, match="channel block"):
        spx.push_single_pass(_Data(SAME, 3, 2, 1), Net(), batch_size=2, device="cpu")


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_abi_entry():
    from scaleprotoseg_amd import _lib

    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "spx_hip.h")).read()
    assert "spx_push_merge" in _lib.SIGNATURES and hasattr(lib, "spx_push_merge") and "int spx_push_merge(" in text
    assert "#define SPX_ABI_VERSION 17" in text and _lib.ABI_VERSION == 17 and lib.spx_version() == 17
    err = lambda: lib.spx_last_error().decode()                            # noqa: E731
    assert lib.spx_push_merge(None, None, None, 0, 1, 1, 1, 1, 1, None, 0, None, None, None, None, None) != 0
    assert err().startswith("spx_push_merge") and "NULL" in err()
    a = [16] * 3                                                            # non-NULL stand-ins: refused before any is read
    for kw, msg in ((dict(x_dtype=2), "dtype code"), (dict(B=0), "empty"), (dict(Cs=9, C=8), "channels per scale"),
                    (dict(image0=-1), "image index")):
        v = dict(x_dtype=1, B=1, P=1, C=8, HW=4, Cs=4, image0=0)
        v.update(kw)
        assert lib.spx_push_merge(*a, v["x_dtype"], v["B"], v["P"], v["C"], v["HW"], v["Cs"], 16, v["image0"], 16, 16, 16, 16, None) != 0
        assert err().startswith("spx_push_merge") and msg in err(), (kw, err())
