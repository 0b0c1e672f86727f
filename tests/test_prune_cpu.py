"""CPU checks of the pruning's host side (scaleprotoseg_amd/prune.py): the table merge rule, the prune decision of
prune.py:33-42 restated with collections.Counter, the data-parallel merge at world size 2 over gloo, the ABI version.
No kernels run here."""
import os
from collections import Counter

import numpy as np
import pytest
import torch

from support import run_gloo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _key(d, void=False, flat=0):
    bits = int(np.float32(d).view(np.int32))
    return ((bits | (0x80000000 if void else 0)) << 32 | flat) - (1 << 64 if void else 0)   # uint64 bits as int64


def _table(rows, k):
    """rows: per prototype a list of (distance, void, image, label) -> packed [P, k, 9] (sorted as the kernel keeps it)."""
    P = len(rows)
    t = torch.zeros((P, k, 9), dtype=torch.int64)
    t[..., 0] = -1
    t[..., 1] = -1
    for j, r in enumerate(rows):
        r = sorted(r, key=lambda e: (e[1], e[0], e[2]))[:k]
        for s, (d, v, img, lab) in enumerate(r):
            t[j, s, 0] = _key(d, v, 3 * img)
            t[j, s, 1] = img
            t[j, s, 2] = lab
            t[j, s, 3:7] = torch.tensor([img, img + 1, 0, 2])
            t[j, s, 7:9] = torch.tensor([img, 1])
    return t


def _rule(entries, k):
    """The documented rule: the k smallest by (void, distance, image)."""
    return [e[2] for e in sorted(entries, key=lambda e: (e[1], e[0], e[2]))[:k]]


def _random_entries(gen, images, n_dist=4):
    return [(float(gen.integers(0, n_dist)) * 0.25, bool(gen.random() < 0.2), int(i), int(gen.integers(-1, 5))) for i in images]


def test_merge_tables_follows_rule_with_ties_and_voids():
    from scaleprotoseg_amd.prune import merge_nearest_tables

    gen = np.random.default_rng(0)
    k = 5
    for trial in range(20):
        a = [_random_entries(gen, range(0, 7)) for _ in range(6)]
        b = [_random_entries(gen, range(7, 10)) for _ in range(6)]
        c = [[] for _ in range(6)]                                     # a rank without images
        got = merge_nearest_tables([_table(a, k), _table(c, k), _table(b, k)], k)
        for j in range(6):
            exp = _rule(a[j] + b[j], k)
            assert got[j, :, 1].tolist() == exp + [-1] * (k - len(exp)), (trial, j)
            # the other fields travel with their entry
            for s, img in enumerate(exp):
                assert got[j, s, 3:7].tolist() == [img, img + 1, 0, 2]


def test_merge_tables_pads_short_rows():
    from scaleprotoseg_amd.prune import merge_nearest_tables

    t = _table([[(1.0, False, 0, 2)], [(0.5, True, 1, 3), (2.0, False, 0, 1)]], 2)
    got = merge_nearest_tables([t[:, :1]], 3)
    assert got.shape == (2, 3, 9)
    assert got[0, :, 1].tolist() == [0, -1, -1]
    assert got[1, :, 1].tolist() == [0, -1, -1]           # the non-void candidate ranks before the void one


def test_unpacked_fields_and_class_ids():
    from scaleprotoseg_amd.prune import _unpack

    t = _table([[(1.5, False, 0, 2), (0.25, True, 1, -1)], [(3.0, False, 2, 4), (0.0, False, 1, 4)]], 2)
    res = _unpack(t)
    assert res.distance.dtype == torch.float32
    assert res.distance.tolist() == [[1.5, 0.25], [0.0, 3.0]]
    assert res.all_void.tolist() == [[False, True], [False, False]]
    assert res.image.tolist() == [[0, 1], [1, 2]]
    ids = res.class_ids()
    assert isinstance(ids, np.ndarray) and ids.tolist() == [[2, -1], [4, 4]]
    short = _unpack(_table([[(1.0, False, 0, 2)], [(1.0, False, 0, 3), (2.0, False, 1, 3)]], 2))
    ids = short.class_ids()
    assert [r.tolist() for r in ids] == [[2], [3, 3]]


def test_prune_decision_equals_counter_restatement():
    from scaleprotoseg_amd.prune import _unpack, prune_decision

    gen = np.random.default_rng(1)
    P, k, K = 40, 6, 4
    rows = [_random_entries(gen, range(gen.integers(2, 9))) for _ in range(P)]
    res = _unpack(_table(rows, k))
    classes = torch.tensor(gen.integers(0, K, size=P))
    for thr in (0, 1, 2, 3, 7):
        exp = []
        for j in range(P):
            labels = [int(v) for v, i in zip(res.label[j], res.image[j]) if int(i) >= 0]
            if Counter(labels)[int(classes[j])] < thr:                # prune.py:39-42
                exp.append(j)
        assert prune_decision(res, classes, thr) == exp


def test_abi_version_is_17():
    from scaleprotoseg_amd import _lib

    assert _lib.ABI_VERSION == 17
    text = open(os.path.join(ROOT, "include", "spx_hip.h")).read()
    assert "#define SPX_ABI_VERSION 17" in text
    assert "#define SPX_PRUNE_MAX_K 64" in text
    for name in ("spx_prune_argmin", "spx_dist_prune_min", "spx_prune_footprint", "spx_prune_merge"):
        assert name in _lib.SIGNATURES


def test_nearest_table_rejects_k_outside_range():
    from scaleprotoseg_amd import SpxError
    from scaleprotoseg_amd.prune import NearestTable

    for k in (0, 65):
        with pytest.raises(SpxError, match="outside 1..64"):
            NearestTable(4, k, "cpu")


# ------------------------------------------------------------------------------------------------------------------
# data-parallel merge, world size 2 over gloo (support.run_gloo, as tests/test_dp_gloo.py)
# ------------------------------------------------------------------------------------------------------------------


def _dp_merge_case(rank, world):
    from scaleprotoseg_amd import dp

    gen = np.random.default_rng(7)
    rows = [_random_entries(gen, range(0, 11)) for _ in range(5)]
    shard = dp.shard_range(11, rank, world)
    local = _table([[e for e in r if e[2] in shard] for r in rows], 4)
    return dp.reduce_prune_tables(local, 4), _table(rows, 4)


def test_dp_merge_gloo_equals_single_rank(tmp_path):
    (g0, single), (g1, _) = run_gloo(_dp_merge_case, tmp_path)
    assert torch.equal(g0, g1)
    assert torch.equal(g0, single)
