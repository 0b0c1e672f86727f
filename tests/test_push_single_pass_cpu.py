"""The single-pass batched push without a GPU: the rule of spx_push_merge (tests/push_merge_restatement.py) against the CPU
oracle, the driver (push_single_pass / push_prototypes_multiscale(batch_size=...)) with its two device steps replaced by
oracle-based callables against today's two-pass push, argument errors and the ABI.  Everything is an equality of bits."""
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
from push_cases import MIXED, QUIET, SAME, FeatureData, feature_problem, push_state, replace_device_steps  # noqa: E402
from push_cases import same_push_state, steps  # noqa: E402,F401  (steps: a fixture, taken by importing its name)
from support import run_gloo  # noqa: E402


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

    net0, data = feature_problem(sizes)
    calls0 = _spy(net0)
    best0, list_idx, dup0 = push_prototypes_multiscale(data, net0, str(tmp_path / "two"), **QUIET)
    assert isinstance(list_idx, list) and 1 in dup0 and len(dup0) >= 2
    flat0 = torch.cat(list_idx)[best0, torch.arange(len(best0))]

    net1, _ = feature_problem(sizes)
    calls1 = _spy(net1)
    best1, flat1, dup1 = push_prototypes_multiscale(data, net1, str(tmp_path / "one"), batch_size=batch, **QUIET)
    assert isinstance(flat1, torch.Tensor) and flat1.dtype == torch.int64
    assert torch.equal(best1, best0) and torch.equal(flat1, flat0) and list(dup1) == list(dup0)      # GLOBAL image indices
    same_push_state(push_state(net1, tmp_path / "one"), push_state(net0, tmp_path / "two"))

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


# (what one rank runs in this file's sharded test; support.run_gloo spawns it)
def _dp_case(rank, world):
    from scaleprotoseg_amd.push import push_prototypes_multiscale

    net, data = feature_problem(MIXED)
    replace_device_steps()
    calls = _spy(net)
    best, flat, dup = push_prototypes_multiscale(data, net, batch_size=3, **QUIET)
    return push_state(net), best.clone(), flat.clone(), list(dup), sum(calls)


def test_sharded_driver_equals_the_two_pass_push(steps, tmp_path):
    from scaleprotoseg_amd.push import push_prototypes_multiscale

    res = run_gloo(_dp_case, tmp_path)
    net0, data = feature_problem(MIXED)
    best0, list_idx, dup0 = push_prototypes_multiscale(data, net0, **QUIET)
    flat0 = torch.cat(list_idx)[best0, torch.arange(len(best0))]
    for state, best, flat, dup, images in res:
        same_push_state(state, push_state(net0))
        assert torch.equal(best, best0) and torch.equal(flat, flat0) and dup == list(dup0)
    assert sum(r[4] for r in res) == len(MIXED)                              # every image encoded once, on one rank


def test_a_rank_with_an_empty_shard_never_wins(steps):
    from scaleprotoseg_amd.push import push_single_pass

    net, data = feature_problem(SAME)
    table = push_single_pass(data, net, batch_size=3, image_range=range(4, 4), device="cpu")
    assert torch.isinf(table.best_value).all() and (table.best_image == -1).all() and table.next_image == 0
    part = push_single_pass(data, net, batch_size=3, image_range=range(4, 7), device="cpu")
    assert ((part.best_image >= 4) & (part.best_image < 7)).all()


# ---- argument errors ---------------------------------------------------------------------------------------------------
def test_argument_errors(steps):
    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd.push import proto_scale_table, push_single_pass

    net, data = feature_problem(SAME)
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
        spx.push_single_pass(FeatureData(SAME, 3, 2, 1), Net(), batch_size=2, device="cpu")


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
