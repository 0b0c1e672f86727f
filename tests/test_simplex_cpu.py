"""CPU side of the in-place simplex projection (spx_simplex_project, utils.projection_simplex_sort_): the NumPy restatement
the kernel is held to equals the stock formula bit for bit and reproduces the reference's recorded output; the C ABI carries
the symbol and refuses bad arguments before anything is launched; the two host helpers (threshold_group_projections_,
non_zero_proto) match the reference's formulas.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from simplex_restatement import case_rows, projection_simplex_rows
from support import group_net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 12, 63, 64, 65, 257, 1024)


# (local: a NumPy array's float32 bits as int32, compared with np.array_equal; support.bits_equal compares tensors)
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def test_restatement_reproduces_the_reference_fixture(golden):
    m = golden("misc")
    assert np.array_equal(_bits(projection_simplex_rows(m["simplex_in"])), _bits(m["simplex_out"]))


@pytest.mark.parametrize("z", [1.0, 0.5])
@pytest.mark.parametrize("n", SIZES)
def test_restatement_equals_the_stock_formula_bit_for_bit(n, z):
    from scaleprotoseg_amd.utils import projection_simplex_sort

    v = case_rows(n, 100 + n)
    ref = projection_simplex_sort(torch.from_numpy(v), z).numpy()
    assert np.array_equal(_bits(projection_simplex_rows(v, z)), _bits(ref))


def test_restatement_on_non_finite_rows():
    """rho = 0: a NaN anywhere makes the whole row NaN; a +inf leaves NaN in its place and 0 elsewhere; -inf is an ordinary
    (never selected) element."""
    from scaleprotoseg_amd.utils import projection_simplex_sort

    v = np.array([[1, np.nan, 0.5, 2], [1, np.inf, 0.5, 2], [1, -np.inf, 0.5, 2]], dtype=np.float32)
    got, ref = projection_simplex_rows(v), projection_simplex_sort(torch.from_numpy(v)).numpy()
    assert np.isnan(got[0]).all() and np.isnan(ref[0]).all()
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.nan_to_num(got), np.nan_to_num(ref))


@pytest.fixture(scope="module")
def lib():
    from scaleprotoseg_amd import _lib

    return _lib.load()


def test_symbol_is_declared_exported_and_bound(lib):
    from scaleprotoseg_amd import _lib

    text = open(os.path.join(ROOT, "include", "spx_hip.h")).read()
    assert re.search(r"\bint spx_simplex_project\(float\* const\* block_ptrs, const int32_t\* block_rows, const int32_t\* block_cols,"
                     r"\s*int32_t nblocks, float z,\s*void\* stream\);", text)
    assert int(re.search(r"#define SPX_ABI_VERSION (\d+)", text).group(1)) == 17 == _lib.ABI_VERSION == lib.spx_version()
    assert hasattr(lib, "spx_simplex_project")
    res, args = _lib.SIGNATURES["spx_simplex_project"]
    assert res is C.c_int and len(args) == 6 and args[4] is C.c_float


def _tables(ptrs, rows, cols):
    m = len(ptrs)
    return (C.c_void_p * m)(*ptrs), (C.c_int32 * m)(*rows), (C.c_int32 * m)(*cols)


def test_bad_arguments_are_refused_before_any_launch(lib):
    """Every call below names no real device memory: a launch would fault, a refusal returns with a message."""
    fake = 0x1000
    p, r, c = _tables([fake], [3], [12])
    for args in ((None, r, c), (p, None, c), (p, r, None)):
        assert lib.spx_simplex_project(*args, 1, 1.0, None) != 0
        assert b"NULL table" in lib.spx_last_error()
    assert lib.spx_simplex_project(p, r, c, 0, 1.0, None) != 0
    assert b"0 blocks" in lib.spx_last_error()
    p193, r193, c193 = _tables([fake] * 193, [3] * 193, [12] * 193)
    assert lib.spx_simplex_project(p193, r193, c193, 193, 1.0, None) != 0
    assert b"193 blocks" in lib.spx_last_error()
    for cols in (0, 1025):
        p2, r2, c2 = _tables([fake, fake], [3, 3], [12, cols])
        assert lib.spx_simplex_project(p2, r2, c2, 2, 1.0, None) != 0
        assert f"block 1 has {cols} columns".encode() in lib.spx_last_error()
    p2, r2, c2 = _tables([fake, fake], [3, 0], [12, 12])
    assert lib.spx_simplex_project(p2, r2, c2, 2, 1.0, None) != 0
    assert b"block 1 has 0 rows" in lib.spx_last_error()
    p2, r2, c2 = _tables([fake, None], [3, 3], [12, 12])
    assert lib.spx_simplex_project(p2, r2, c2, 2, 1.0, None) != 0
    assert b"block 1 is NULL" in lib.spx_last_error()


def test_in_place_projection_refuses_what_it_cannot_edit_in_place():
    import scaleprotoseg_amd as spx

    with pytest.raises(spx.SpxError, match="no CPU fallback"):
        spx.projection_simplex_sort_([torch.rand(3, 12)])
    with pytest.raises(spx.SpxError, match="no CPU fallback"):
        spx.projection_simplex_sort_([nn.Parameter(torch.rand(3, 12))])
    with pytest.raises(spx.SpxError):
        spx.projection_simplex_sort_([torch.rand(12, 3).t()])              # non-contiguous (and on the CPU)
    spx.projection_simplex_sort_([])                                       # nothing to do


def _group_net(seed=3):
    import scaleprotoseg_amd as spx

    g = torch.Generator().manual_seed(seed)

    def simplex_rows(net):
        for gp in net.group_projection:
            gp.weight.copy_(spx.projection_simplex_sort(torch.rand(gp.weight.shape, generator=g) * 3))

    return group_net(24, 3, 4, 8, 2, seed=seed, init=simplex_rows)


def _reference_non_zero_proto(model):
    """segmentation/utils.py:140-154, line by line."""
    out = []
    for cls_i in range(len(model.group_projection)):
        list_proto_idx = torch.nonzero(model.prototype_class_identity[:, cls_i]).flatten().tolist()
        for k in range(model.num_groups):
            group_weight = model.group_projection[cls_i].weight.data[k, :]
            out.extend(list_proto_idx[i] for i in torch.nonzero(group_weight).flatten().tolist())
    return np.unique(np.array(out)).tolist()


def test_threshold_and_non_zero_proto_match_the_reference_formulas():
    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd import functional as F

    net = _group_net()
    positive = torch.cat([gp.weight.detach().reshape(-1) for gp in net.group_projection])
    positive = positive[positive > 0].sort().values
    threshold = float(positive[len(positive) // 2])                        # a weight exactly AT the threshold survives (<)
    with torch.no_grad():
        net.group_projection[0].weight[1, 0] = threshold                   # ... and so does a second one
    before = [gp.weight.detach().clone() for gp in net.group_projection]
    ptrs = [gp.weight.data_ptr() for gp in net.group_projection]
    versions = [gp.weight._version for gp in net.group_projection]
    F._PACK_CACHE[("sentinel",)] = ()
    assert spx.non_zero_proto(net) == _reference_non_zero_proto(net)

    spx.threshold_group_projections_(net, threshold)
    assert not F._PACK_CACHE                                               # the pack cache was dropped
    n_zeroed = 0
    for gp, w0, ptr, ver in zip(net.group_projection, before, ptrs, versions):
        ref = w0.clone()
        ref[ref < threshold] = 0                                           # analysis/threshold_save.py:27-28
        assert torch.equal(gp.weight.detach(), ref)
        assert gp.weight.data_ptr() == ptr and gp.weight._version > ver
        n_zeroed += int((ref == 0).sum() - (w0 == 0).sum())
    assert n_zeroed > 0
    after = torch.cat([gp.weight.detach().reshape(-1) for gp in net.group_projection])
    assert float(net.group_projection[0].weight.detach()[1, 0]) == threshold and int((after == threshold).sum()) >= 2
    assert float(after[after > 0].min()) == threshold
    used = spx.non_zero_proto(net)
    assert used == _reference_non_zero_proto(net) == sorted(set(used))
    assert 0 < len(used) <= net.num_prototypes

    spx.threshold_group_projections_(net, 2.0)                             # everything below 2: no prototype is used
    assert spx.non_zero_proto(net) == []
