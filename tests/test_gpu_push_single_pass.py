"""The single-pass batched push on the GPU: spx_push_merge against its restatement (tests/push_merge_restatement.py), and the
pipeline push_prototypes_multiscale(batch_size=...) against the two-pass push (batch_size=None, the path this change leaves as
it was), in one process and sharded over two ranks.  Everything is an equality of bits."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import push_merge_restatement as R  # noqa: E402
from scaleprotoseg_amd import PushTable, push_single_pass  # noqa: E402,F401  (the feature under test: no test here runs without it)
from scaleprotoseg_amd import push as push_mod  # noqa: E402
from push_cases import bf16_bank_with_a_duplicate, push_problem, push_state, same_push_state  # noqa: E402
from support import RoundBf16, gpu_device, proto_net, run_gloo  # noqa: E402

pytestmark = pytest.mark.gpu

# the two-pass path's own device steps, as they are when this module is imported (a CPU rehearsal elsewhere in the suite
# replaces them in place)
_TWO_PASS_STEPS = dict(compute_distances=push_mod.compute_distances, argmin_over_images=push_mod.argmin_over_images)


@pytest.fixture(autouse=True)
def _product_steps(monkeypatch):
    for name, fn in _TWO_PASS_STEPS.items():
        monkeypatch.setattr(push_mod, name, fn)


# ---- the kernel against the restatement --------------------------------------------------------------------------------
#        B    P  S  Cs  H   W  dtype            first image0
CASES = {
    "smallest": (1, 8, 1, 16, 3, 5, torch.float32, 0),
    "bf16": (3, 40, 4, 16, 5, 7, torch.bfloat16, 5),
    "more_images_than_lanes": (70, 12, 2, 64, 2, 3, torch.float32, (1 << 31) + 11),
    "ragged": (5, 229, 4, 20, 9, 11, torch.bfloat16, 2),      # P % 4 != 0, Cs % 16 != 0, an arbitrary proto_scale table
}
LEVELS = torch.tensor([0.125, 0.25, 0.5, 1.0, 3.0])


def _batch(g, B, P, S, Cs, H, W, dtype):
    val = LEVELS[torch.randint(0, len(LEVELS), (B, P), generator=g)]       # few levels: ties in a batch and with the running best
    idx = torch.randint(0, H * W, (B, P), generator=g)
    val[:, 1] = 1e10                                                        # a class that never appears
    idx[:, 1] = 0
    val[:, 2] = float("nan")                                                # never wins
    if B > 1:
        val[B // 2, 3] = float("nan")                                       # a NaN among candidates
    x = torch.rand(B, S * Cs, H, W, generator=g).to(dtype)
    return idx, val, x


# (local: the bits of a float32 tensor, integer tensors as they are - not support.bits_equal, which takes two floats)
def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_table(table, state, tag):
    for name in ("best_value", "best_image", "best_flat", "best_patch"):
        got = getattr(table, name).cpu()
        assert got.dtype == state[name].dtype and torch.equal(_bits(got), _bits(state[name])), (tag, name)


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_equals_the_restatement(name):
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    B, P, S, Cs, H, W, dtype, image0 = CASES[name]
    g = torch.Generator().manual_seed(sorted(CASES).index(name))
    if name == "ragged":
        scale = torch.randint(0, S, (P,), generator=g).to(torch.int32)
    else:
        scale = torch.tensor([p // (P // S) for p in range(P)], dtype=torch.int32)
    table = spx.PushTable(P, Cs, dev)
    state = R.new_state(P, Cs)
    for step in range(3):                                                   # increasing image0, a gap before the last batch
        idx, val, x = _batch(g, B, P, S, Cs, H, W, dtype)
        R.merge(state, idx, val, x, scale, image0)
        table.merge(idx.to(dev), val.to(dev), x.to(dev), scale.to(dev), image0)
        _same_table(table, state, (name, step))
        image0 += B + step
    assert table.next_image == image0 - 2
    assert (state["best_image"][3] >= 0) and int(state["best_image"][2]) == -1 and int(state["best_image"][1]) == CASES[name][7]
    with pytest.raises(spx.SpxError, match="increasing image order"):
        table.merge(idx.to(dev), val.to(dev), x.to(dev), scale.to(dev), CASES[name][7])


def test_a_batch_that_improves_nothing_writes_nothing():
    import scaleprotoseg_amd as spx

    dev = gpu_device()
    B, P, S, Cs, H, W = 6, 37, 2, 24, 4, 5
    g = torch.Generator().manual_seed(9)
    table = spx.PushTable(P, Cs, dev)
    # a sentinel state no merge would produce: signalling-NaN payloads in the patches, negative flats, odd images
    value = torch.full((P,), 0.5)
    value[5] = float("-inf")
    image = torch.arange(P, dtype=torch.int64) * 7 - 3
    flat = -torch.arange(P, dtype=torch.int64) - 1
    patch = (0x7F800001 + torch.arange(P * Cs, dtype=torch.int32)).view(torch.float32).reshape(P, Cs)
    for name, t in (("best_value", value), ("best_image", image), ("best_flat", flat), ("best_patch", patch)):
        getattr(table, name).view(torch.int32).copy_(t.view(torch.int32).to(dev))
    val = torch.tensor([0.5, 0.75, float("nan"), float("inf"), 1e10])[torch.randint(0, 5, (B, P), generator=g)]   # none below 0.5
    idx = torch.randint(0, H * W, (B, P), generator=g)
    x = torch.rand(B, S * Cs, H, W, generator=g)
    scale = torch.tensor([p % S for p in range(P)], dtype=torch.int32)
    table.merge(idx.to(dev), val.to(dev), x.to(dev), scale.to(dev), 1000)
    _same_table(table, dict(best_value=value, best_image=image, best_flat=flat, best_patch=patch), "sentinel")


# ---- the pipeline against the two-pass push ----------------------------------------------------------------------------
S_, CS_, K_, PER_, ABSENT = 4, 16, 5, 2, 3
P_ = S_ * K_ * PER_
SAME = [(5, 7)] * 7
MIXED = [(5, 7)] * 2 + [(6, 9)] * 3 + [(5, 7)] + [(7, 5)]


class _FeatureData:
    """The data set's "images" are feature tensors [S * Cs, h, w] (identity backbone): an image's features do not depend on its
    batch mates.  Targets at 8 times the latent size, 0 = void, class ABSENT never appears."""

    convert_targets = None

    def __init__(self, sizes, seed):
        g = torch.Generator().manual_seed(seed)
        self.items = []
        for h, w in sizes:
            img = torch.randn(S_ * CS_, h, w, generator=g)
            t = torch.randint(0, K_ + 1, (h, w), generator=g).repeat_interleave(8, 0).repeat_interleave(8, 1)
            t[t == ABSENT + 1] = 0
            self.items.append((img, t.numpy().astype(np.int64)))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


# (local: a module and a data set, not the operator inputs of parity_cases.problem)
def _problem(dev, sizes, seed=3, fractional=False):
    """A net built like push_cases.push_problem (forced duplicate, absent class), identity backbone."""
    net = proto_net(P_, K_, S_, CS_, seed=seed, add_on=nn.Sequential(nn.Sigmoid(), RoundBf16()), init=bf16_bank_with_a_duplicate)
    if fractional:                                                          # not one-hot: the written map + push_masked_argmin
        ident = net.prototype_class_identity.clone()
        ident[4] = 0.0
        ident[4, 0] = ident[4, 1] = 0.5
        net.prototype_class_identity = ident
    return net.to(dev), _FeatureData(sizes, seed + 1)


_two_pass_cache = {}


def _two_pass(dev, key, tmp_root, **kw):
    """The two-pass push on a fresh model, once per problem: (state, best, flat, dup).  Kept unchanged."""
    if key not in _two_pass_cache:
        net, data = _problem(dev, **kw)
        root = os.path.join(tmp_root, "two_pass")
        best, list_idx, dup = push_mod.push_prototypes_multiscale(data, net, root, log=lambda *_: None)
        assert isinstance(list_idx, list)
        flat = torch.cat(list_idx)[best, torch.arange(P_, device=best.device)]
        _two_pass_cache[key] = (push_state(net, root), best.cpu(), flat.cpu(), list(dup))
    return _two_pass_cache[key]


@pytest.fixture(scope="module")
def shared_tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("push_single_pass"))


@pytest.mark.parametrize("batch", [1, 2, 3, 64])
def test_pipeline_equals_the_two_pass_push(shared_tmp, tmp_path, batch):
    dev = gpu_device()
    want, best0, flat0, dup0 = _two_pass(dev, "same", os.path.join(shared_tmp, "same"), sizes=SAME)
    assert 1 in dup0
    net, data = _problem(dev, sizes=SAME)
    absent = torch.nonzero(net.prototype_class_identity[:, ABSENT]).flatten().tolist()
    best, flat, dup = push_mod.push_prototypes_multiscale(data, net, str(tmp_path), log=lambda *_: None, batch_size=batch)
    assert isinstance(flat, torch.Tensor) and flat.dtype == torch.int64 and tuple(flat.shape) == (P_,)
    assert torch.equal(best.cpu(), best0) and torch.equal(flat.cpu(), flat0) and list(dup) == dup0
    same_push_state(push_state(net, str(tmp_path)), want)
    assert len(absent) == S_ * PER_
    for p in absent:                                                        # value 1e10 in every image: image 0, flat 0
        assert int(best[p]) == 0 and int(flat[p]) == 0


@pytest.mark.parametrize("batch", [2, 3])
def test_pipeline_with_mixed_image_sizes(shared_tmp, tmp_path, batch):
    dev = gpu_device()
    want, best0, flat0, dup0 = _two_pass(dev, "mixed", os.path.join(shared_tmp, "mixed"), sizes=MIXED)
    net, data = _problem(dev, sizes=MIXED)
    best, flat, dup = push_mod.push_prototypes_multiscale(data, net, str(tmp_path), log=lambda *_: None, batch_size=batch)
    assert torch.equal(best.cpu(), best0) and torch.equal(flat.cpu(), flat0) and list(dup) == dup0
    assert len(set(best0.tolist())) > 2 and int(best0.max()) >= 2           # winners beyond the first run: global indices
    same_push_state(push_state(net, str(tmp_path)), want)


def test_a_fractional_identity_row_takes_the_map_path(shared_tmp, tmp_path):
    from scaleprotoseg_amd.functional import identity_is_one_hot

    dev = gpu_device()
    want, best0, flat0, dup0 = _two_pass(dev, "fractional", os.path.join(shared_tmp, "fractional"), sizes=MIXED, fractional=True)
    net, data = _problem(dev, sizes=MIXED, fractional=True)
    assert not identity_is_one_hot(net.prototype_class_identity)
    fused = []
    orig = net.push_min_from_conv
    net.push_min_from_conv = lambda *a, **kw: fused.append(orig(*a, **kw)) or fused[-1]
    best, flat, dup = push_mod.push_prototypes_multiscale(data, net, str(tmp_path), log=lambda *_: None, batch_size=3)
    assert fused and all(f is None for f in fused)                          # every run went through the written map
    assert torch.equal(best.cpu(), best0) and torch.equal(flat.cpu(), flat0) and list(dup) == dup0
    same_push_state(push_state(net, str(tmp_path)), want)


def test_pool_backbone_at_batch_size_one(tmp_path):
    """The stand-in's 1x1 convolutions may round differently per batch shape, so only batch_size=1 is comparable."""
    dev = gpu_device()
    net0, data, P = push_problem(dev)
    best0, list_idx, dup0 = push_mod.push_prototypes_multiscale(data, net0, str(tmp_path / "two"), log=lambda *_: None)
    net1, _, _ = push_problem(dev)
    best1, flat1, dup1 = push_mod.push_prototypes_multiscale(data, net1, str(tmp_path / "one"), log=lambda *_: None, batch_size=1)
    assert torch.equal(best1, best0) and list(dup1) == list(dup0)
    assert torch.equal(flat1, torch.cat(list_idx)[best0, torch.arange(P, device=best0.device)])
    same_push_state(push_state(net1, str(tmp_path / "one")), push_state(net0, str(tmp_path / "two")))


def test_boxes_with_and_without_batching(tmp_path):
    dev = gpu_device()
    net0, data = _problem(dev, sizes=MIXED)
    out0 = push_mod.push_prototypes_multiscale(data, net0, str(tmp_path / "two"), log=lambda *_: None, boxes=True,
                                               epoch_number=3, proto_bound_boxes_filename_prefix="bb")
    net1, _ = _problem(dev, sizes=MIXED)
    out1 = push_mod.push_prototypes_multiscale(data, net1, str(tmp_path / "one"), log=lambda *_: None, boxes=True,
                                               epoch_number=3, proto_bound_boxes_filename_prefix="bb", batch_size=3)
    assert len(out0) == len(out1) == 5 and torch.equal(out1[0], out0[0]) and list(out1[2]) == list(out0[2])
    assert out1[3].dtype == np.int64 and np.array_equal(out1[3], out0[3]) and np.array_equal(out1[4], out0[4])
    assert (out1[3][:, 0] == out0[0].cpu().numpy()).all()
    same_push_state(push_state(net1, str(tmp_path / "one")), push_state(net0, str(tmp_path / "two")))
    for name in ("bb-receptive_field3.npy", "bb3.npy"):
        a, b = (np.load(os.path.join(str(tmp_path / d), "epoch-3", name)) for d in ("one", "two"))
        assert np.array_equal(a, b)


# ---- sharded: two ranks on one GPU -------------------------------------------------------------------------------------
# (what one rank runs in this file's sharded test; support.run_gloo spawns it)
def _dp_case(rank, world):
    net, data = _problem(torch.device("cuda:0"), sizes=MIXED)
    best, flat, dup = push_mod.push_prototypes_multiscale(data, net, log=lambda *_: None, batch_size=3)
    return push_state(net), best.cpu(), flat.cpu(), list(dup)


def test_sharded_single_pass_on_the_kernels(shared_tmp, tmp_path):
    dev = gpu_device()
    want, best0, flat0, dup0 = _two_pass(dev, "mixed", os.path.join(shared_tmp, "mixed"), sizes=MIXED)
    want = {k: v for k, v in want.items() if k != "json"}
    for state, best, flat, dup in run_gloo(_dp_case, tmp_path, gpu=True):
        same_push_state(state, want)
        assert torch.equal(best, best0) and torch.equal(flat, flat0) and dup == dup0
