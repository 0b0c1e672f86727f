"""The push's one driver and the data-set walk it shares with the pruning search (scaleprotoseg_amd/scan.py), without a GPU:
``global_min`` against the oracle's gather, the two-pass push with more ranks than images, what an empty data set raises, and
the run generator.  Stand-in backbone, data and device-step replacements of tests/push_cases.py; every comparison
is an equality of bits."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from oracle import ppnet_oracle as O  # noqa: E402
from push_cases import K_, MIXED, QUIET, S_, feature_problem, patch_kernels_with_oracle, push_state  # noqa: E402
from push_cases import same_push_state, steps  # noqa: E402,F401  (steps: a fixture, taken by importing its name)
from support import run_gloo  # noqa: E402


# (local: a NumPy array's float32 bytes; support.bits_equal compares tensors)
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).tobytes()


@pytest.mark.parametrize("rng", [range(0, 7), range(2, 6)], ids=["whole", "shard"])
def test_global_min_equals_the_oracle_gather(steps, rng):  # noqa: F811
    from scaleprotoseg_amd.push import global_min, min_across_dataset

    net, data = feature_problem(MIXED)
    P = net.num_prototypes
    convs = [net.conv_features(data[i][0].unsqueeze(0)) for i in rng]        # mixed sizes: 6x8, 8x10, 8x6 latent pixels
    assert len({tuple(c.shape[2:]) for c in convs}) >= 2
    best, list_idx = min_across_dataset(data, net, K_, void_class=0, device="cpu", image_range=rng)
    assert len(set(best.tolist())) > 1                                         # positions inside the range
    want = O.gather_push_patches(convs, best, list_idx, S_, P)
    got = global_min(best, list_idx, data, net, device="cpu", image_offset=rng.start)
    assert len(got) == P and got[0].shape == (net.prototype_shape[1], 1, 1)
    assert _bits(np.reshape(got, want.shape)) == _bits(want)


def _one_image_case(rank, world):
    from scaleprotoseg_amd.push import push_prototypes_multiscale

    net, data = feature_problem(MIXED[:1])
    patch_kernels_with_oracle(S_)
    best, list_idx, dup = push_prototypes_multiscale(data, net, **QUIET)
    return push_state(net), best.clone(), [t.clone() for t in list_idx], list(dup)


def test_two_pass_push_with_more_ranks_than_images(steps, tmp_path):  # noqa: F811
    from scaleprotoseg_amd.push import push_prototypes_multiscale

    res = run_gloo(_one_image_case, tmp_path)
    net0, data = feature_problem(MIXED[:1])
    best0, list_idx0, dup0 = push_prototypes_multiscale(data, net0, **QUIET)
    assert (best0 == 0).all() and len(list_idx0) == 1
    for state, best, _, dup in res:
        same_push_state(state, push_state(net0))
        assert torch.equal(best, best0) and dup == list(dup0)
    assert len(res[0][2]) == 1 and torch.equal(res[0][2][0], list_idx0[0]) and res[1][2] == []    # rank 1's shard is empty


def test_an_empty_data_set_raises_what_it_always_did(steps):  # noqa: F811
    """One rank, no image: the two-pass push fails in ``torch.cat`` of no per-image minima (ValueError), the single pass is
    refused by the driver (SpxError) - the types recorded before the three bodies became one."""
    import scaleprotoseg_amd as spx

    net, data = feature_problem(MIXED[:1])
    data.items = []
    with pytest.raises(ValueError, match="non-empty list"):
        spx.push_prototypes_multiscale(data, net, **QUIET)
    with pytest.raises(spx.SpxError, match="at least one image"):
        spx.push_prototypes_multiscale(data, net, batch_size=2, **QUIET)


def test_run_generator_boundaries_and_order():
    from scaleprotoseg_amd.scan import batches

    def item(h, w, lh, lw):
        return torch.empty(3, h, w), np.zeros((lh, lw), dtype=np.uint8)

    # images 0..2 alike | 3, 4: another image size | 5: the same image size, another label size | 6, 7: as 0..2 again
    data = [item(4, 6, 8, 12)] * 3 + [item(6, 6, 8, 12)] * 2 + [item(6, 6, 4, 6)] + [item(4, 6, 8, 12), item(4, 6, 8, 12)]
    ids = lambda rng, b: [[i for i, _, _ in run] for run in batches(data, rng, b)]  # noqa: E731
    assert ids(range(8), 8) == [[0, 1, 2], [3, 4], [5], [6, 7]]
    assert ids(range(8), 2) == [[0, 1], [2], [3, 4], [5], [6, 7]]                  # the batch size cuts a run, never joins two
    assert ids(range(8), 1) == [[i] for i in range(8)]
    assert ids(range(1, 7), 3) == [[1, 2], [3, 4], [5], [6]]                       # dataset indices, not positions
    assert ids(range(3, 3), 4) == [] and ids(range(0), 4) == []
    for run in batches(data, range(8), 3):
        for i, img, t in run:
            assert img is data[i][0] and isinstance(t, np.ndarray) and t.shape == data[i][1].shape
