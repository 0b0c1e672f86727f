"""The distance backward held to float64 when the tiles of one launch differ in magnitude (tests/bwd_scale_cases.py has the
cases, the patterns, the references and the bounds; tests/test_bwd_scale_cases_cpu.py pins them).

Per case, one smallest shape per instance family of the parameter kernel, each workgroup walking three or more chunks:
  (a) dX of the run with per-tile scales equals 2^k(tile) times dX of the unscaled run bit for bit, and is 0 on zero tiles;
  (b) every row of dPrototypes and of dLastLayer against float64, each row to its OWN maximum (TOL_* of the case module), and
      the whole tensors at the suite's bounds;
  (c) uniform loss scales 2^16 and 2^-30: every gradient is the scaled gradient of the unscaled run bit for bit;
  (d) plain randn * 1e-3 gradients (equal exponents) against float64 at the suite's bounds: the walk and the multi-chunk sums;
  (e) two runs agree bit for bit.
Section 4: activations of uneven magnitude on the two-class-block head, dLastLayer per column."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import bwd_scale_cases as S
from parity_cases import assert_fwd
from support import BF16_DX_TOL, GRAD_TOL, gpu_device, grad_close, release_cached_blocks  # noqa: F401

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
INSTANCES = [(n, d) for n in sorted(S.CASES) for d in S.CASES[n][7]]
IDS = [f"{n}-{d}" for n, d in INSTANCES]


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_cases():
    yield
    for f in (_run, _ref, S.build, S.build_uneven_activations):
        f.cache_clear()


def _forward_backward(pb, gr, dtype, head=True, keep_forward=False):
    from scaleprotoseg_amd.functional import proto_head_forward

    dev = gpu_device()
    sh = pb.sh
    x = pb.conv.to(dev, DTYPES[dtype]).requires_grad_(True)
    pv = pb.bank.to(dev).requires_grad_(True)
    w = pb.Wl.to(dev).requires_grad_(True) if head else None
    logits, dist, act = proto_head_forward(x, pv, w, S.layout_of(pb.name, head), want_distances=True, want_activations=head)
    if head:
        torch.autograd.backward([logits, dist, act], [gr.g_logits.reshape(-1, sh.K).to(dev), gr.g_dist.to(dev), gr.g_act.to(dev)])
    else:
        torch.autograd.backward([dist], [gr.g_dist.to(dev)])
    torch.cuda.synchronize()
    out = dict(dx=x.grad.cpu(), dp=pv.grad.cpu(), dw=w.grad.cpu() if head else None)
    if keep_forward:
        out.update(logits=logits.detach().cpu(), dist=dist.detach().cpu(), act=act.detach().cpu())
    return out


@functools.lru_cache(maxsize=None)
def _run(name, dtype, variant, head=True, repeat=0):
    """One forward + backward on the device, results on the CPU; shared by the tests, never modified."""
    pb = S.build(name)
    return _forward_backward(pb, pb.grads[variant], dtype, head)


@functools.lru_cache(maxsize=None)
def _ref(name, variant, head=True):
    pb = S.build(name)
    return S.reference(pb, pb.grads[variant], head)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _check_dx_scaling(name, dtype, head):
    pb = S.build(name)
    sh = pb.sh
    base = _run(name, dtype, "masked", head)["dx"].view(sh.B, -1, sh.HW)
    got = _run(name, dtype, "tiles", head)["dx"].view(sh.B, -1, sh.HW)
    assert got.dtype == DTYPES[dtype] and torch.isfinite(got).all()
    s = pb.scale[:, None, :]                                                # [B, 1, HW]: 2^k of the pixel's tile, 0 on zero tiles
    want = (base.float() * s).to(got.dtype)                                 # exact: a power of two inside the normal range
    live = (s != 0).expand_as(got)
    assert (want[live].float().abs() < 2.0 ** 100).all()
    tiny = want[live].float().abs()
    assert (tiny[tiny > 0] > 2.0 ** -100).all()
    assert (got[~live] == 0).all(), "dX is not zero on a tile whose upstream gradients are all zero"
    bad = (_bits(got) != _bits(want)) & live
    if bad.any():
        b, c, px = [v[0].item() for v in torch.nonzero(bad, as_tuple=True)]
        pytest.fail(f"dX of the scaled run is not 2^k times the unscaled one: {int(bad.sum())} elements in "
                    f"{int(bad.any(dim=1).view(sh.B, -1).sum())} pixels, first at image {b} channel {c} pixel {px} (tile {px // S.TILE_PX}, "
                    f"class {pb.classes[b, px].item()}): {got[b, c, px].item():.9e} vs {want[b, c, px].item():.9e}")


def _check_rows(got, ref, what, tol, dim=0):
    r, nzero = S.row_ratios(got, ref, dim)
    worst = r.max().item()
    print(f"{what}: worst {'row' if dim == 0 else 'column'} against float64 {worst:.3e} of its own maximum (bound {tol:.2e}), "
          f"{nzero} all-zero")
    assert nzero == 0
    assert worst <= tol, f"{what}: {'row' if dim == 0 else 'column'} {int(r.argmax())} is off by {worst:.3e} of its maximum"


@pytest.mark.parametrize("name,dtype", INSTANCES, ids=IDS)
def test_dx_scales_with_its_tile_bit_for_bit(name, dtype):
    """(a)"""
    _check_dx_scaling(name, dtype, True)


@pytest.mark.parametrize("name,dtype", INSTANCES, ids=IDS)
def test_parameter_gradients_per_row_against_float64(name, dtype):
    """(b)"""
    got, ref = _run(name, dtype, "tiles"), _ref(name, "tiles")
    tag = f"tile scales {name}-{dtype}"
    _check_rows(got["dp"], ref.dp, f"{tag} dPrototypes", S.TOL_DP_ROW)
    _check_rows(got["dw"], ref.dw, f"{tag} dLastLayer", S.tol_dw_row(name))
    grad_close(got["dx"], ref.dx, "dX", tol=GRAD_TOL if dtype == "fp32" else BF16_DX_TOL, report=tag)
    grad_close(got["dp"], ref.dp, "dPrototypes", report=tag)
    grad_close(got["dw"], ref.dw, "dLastLayer", report=tag)


def test_without_a_head():
    """(a) and (b) on the k-split case with the distance gradient alone (no head, no logits)."""
    _check_dx_scaling("ksplit", "bf16", False)
    got, ref = _run("ksplit", "bf16", "tiles", False), _ref("ksplit", "tiles", False)
    assert got["dw"] is None
    _check_rows(got["dp"], ref.dp, "tile scales ksplit-bf16 without a head dPrototypes", S.TOL_DP_ROW)
    grad_close(got["dp"], ref.dp, "dPrototypes", report="tile scales ksplit-bf16 without a head")


@pytest.mark.parametrize("k", S.LOSS_SCALES)
@pytest.mark.parametrize("name", S.LOSS_SCALE_CASES)
def test_uniform_loss_scale_is_exact(name, k):
    """(c)"""
    for dtype in S.CASES[name][7]:
        base, got = _run(name, dtype, "plain"), _run(name, dtype, f"loss_scale_{k}")
        for key, what in (("dx", "dX"), ("dp", "dPrototypes"), ("dw", "dLastLayer")):
            want = (base[key].float() * 2.0 ** k).to(base[key].dtype)
            a = want.float().abs()
            assert (a < 2.0 ** 100).all() and (a[a > 0] > 2.0 ** -100).all()
            n = int((_bits(got[key]) != _bits(want)).sum())
            assert n == 0, f"{what} ({dtype}) under a loss scale of 2^{k}: {n} elements are not the scaled ones of the unscaled run"


@pytest.mark.parametrize("name,dtype", INSTANCES, ids=IDS)
def test_several_chunks_equal_exponents(name, dtype):
    """(d)"""
    got, ref = _run(name, dtype, "plain"), _ref(name, "plain")
    tag = f"plain gradients {name}-{dtype}"
    grad_close(got["dx"], ref.dx, "dX", tol=GRAD_TOL if dtype == "fp32" else BF16_DX_TOL, report=tag)
    grad_close(got["dp"], ref.dp, "dPrototypes", report=tag)
    grad_close(got["dw"], ref.dw, "dLastLayer", report=tag)


@pytest.mark.parametrize("name,dtype", INSTANCES, ids=IDS)
def test_two_runs_agree_bit_for_bit(name, dtype):
    """(e)"""
    for variant in ("tiles", "plain"):
        first, second = _run(name, dtype, variant), _run(name, dtype, variant, repeat=1)
        for key, what in (("dx", "dX"), ("dp", "dPrototypes"), ("dw", "dLastLayer")):
            assert first[key] is not second[key] and _same_bits(first[key], second[key]), f"{what} ({variant}) differs between two runs"


@pytest.mark.parametrize("name", S.STAIR_CASES)
def test_descending_staircase_beyond_the_skip_rule(name):
    """Every walk descends by 2^36, 2^36 and 2^48, 2^120 in all: the sums stay finite; the rows fed by tiles within 2^80
    of the largest hold the per-row bound; the rows fed by the last step alone - which the parameter kernel may drop - are
    finite and no larger than their reference.  dLastLayer of a one-class-block head comes from the pixel kernel's tile
    partials and holds its bound on every row."""
    pb = S.build(name)
    dtype = S.CASES[name][7][-1]
    gr, _ = S.build_staircase(name)
    ref = S.reference(pb, gr)
    got = _forward_backward(pb, gr, dtype)
    for key in ("dx", "dp", "dw"):
        assert torch.isfinite(got[key]).all(), f"{key} is not finite"
    tag = f"staircase {name}-{dtype}"
    near = pb.pm < len(S.STAIR_LEVELS) - 1
    last = pb.pm == len(S.STAIR_LEVELS) - 1
    _check_rows(got["dp"][near], ref.dp[near], f"{tag} dPrototypes, rows within 2^80", S.TOL_DP_ROW)
    _check_rows(got["dw"][pb.km < len(S.STAIR_LEVELS)], ref.dw[pb.km < len(S.STAIR_LEVELS)], f"{tag} dLastLayer", S.tol_dw_row(name))
    assert (got["dp"][pb.pm >= len(S.STAIR_LEVELS)] == 0).all() and (got["dw"][pb.km >= len(S.STAIR_LEVELS)] == 0).all()
    top, top_ref = got["dp"][last].double().abs().amax(dim=(1, 2, 3)), ref.dp[last].abs().amax(dim=(1, 2, 3))
    print(f"{tag} dPrototypes, rows of the last step: {int((top == 0).sum())} of {int(last.sum())} dropped")
    assert (top <= (1 + S.TOL_DP_ROW) * top_ref).all()
    grad_close(got["dx"], ref.dx, "dX", tol=BF16_DX_TOL, report=tag)
    grad_close(got["dp"], ref.dp, "dPrototypes", report=tag)
    grad_close(got["dw"], ref.dw, "dLastLayer", report=tag)


def test_uneven_activations():
    """Section 4: block exponents of the int16 activation blob that differ between blocks and tiles."""
    pb = S.build_uneven_activations()
    gr = pb.grads["plain"]
    ref = S.reference(pb, gr)
    got = _forward_backward(pb, gr, "bf16", keep_forward=True)
    assert_fwd(got["logits"], got["dist"], got["act"], ref.logits.float(), ref.dist.float(), ref.act.float())
    _check_rows(got["dw"], ref.dw, "uneven activations dLastLayer", S.TOL_DW_COL, dim=1)
    grad_close(got["dw"], ref.dw, "dLastLayer", report="uneven activations")
    grad_close(got["dp"], ref.dp, "dPrototypes", report="uneven activations")
    grad_close(got["dx"], ref.dx, "dX", tol=BF16_DX_TOL, report="uneven activations")
