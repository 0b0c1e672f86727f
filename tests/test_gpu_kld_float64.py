"""The KLD kernels (csrc/spx_kld.hip over csrc/spx_kld_walk.h) against float64 on planes whose loss is NOT zero: the cases of
tests/kld_cases.py (correlated slot planes, float64 loss 0.37 - 0.8; tests/test_kld_inputs_cpu.py checks that on the CPU and
holds the fp32 oracle to a quarter of every bound used here).  Reference: oracle.loss_oracle.kld_loss in float64 on the device.

  loss                       |l - l64| <= 1e-5 max(1, |l64|), with l64 >= 0.05
  gradient, globally         max|g - g64| <= 1e-4 max|g64|, no absolute floor
  gradient, per segment      over the pixels of an (image, class) segment: <= 1e-4 max(the segment's max|g64|, 4e-3 global max|g64|)
  pixels without a class     gradient exactly 0 (and those of a single-pixel segment)
  pair sums                  segment_pair_sums per element against float64 sum_px p_j (l_k - l_j), W given and W = 0:
                             <= 1e-5 (1 + |A64|) + 2 eps32 (|lse_j| (1 + |A64|) + |lse_k|), the fp32 storage of lse
  counts, lse                counts exact; |lse - lse64| <= 1e-5 max(1, |lse64|); lse 0 where the segment is empty
The bounds, and why the floor and the lse term are what they are, are stated in tests/kld_cases.py; the measured error / bound of
every case, and the arithmetic mutation these tests were tried on, in profiles/kld_float64_summary.md.  Each test prints its
error / bound before it asserts."""
import functools

import pytest
import torch

import kld_cases as KC
from support import gpu_device

pytestmark = pytest.mark.gpu

WALKS = ("grid", "linear")                                          # the reduction passes alone take both on every case
RUNS = [(n, w) for n in KC.CASE_NAMES for w in KC.case(n).walks]


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The float64 reference of a case on the device: computed once, shared by the tests, never modified."""
    return KC.reference(KC.case(name), torch.float64, gpu_device())


def _run(c, walk, dev):
    """(loss, gradient) of KLDLoss on the case's planes through the kernels."""
    from scaleprotoseg_amd.loss import ClassDistances, class_slot_table

    B, H, W = c.shape
    lab = c.labels.to(dev)
    v = c.planes.to(dev).clone().requires_grad_(True)
    loss = c.loss_module()(ClassDistances(v, lab.reshape(B, -1).int(), class_slot_table(c.ident).to(dev), c.grid(walk)), lab + 1)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), v.grad.detach()


@pytest.mark.parametrize("name,walk", RUNS)
def test_loss_and_gradient_against_float64(name, walk):
    """KLDLoss through the kernels: value, gradient globally and per segment, exact zeros; the tall cases twice, bit-identical."""
    dev = gpu_device()
    c = KC.case(name)
    ref = _reference(name)
    if c.tile_rows is not None:
        assert walk == "grid" and KC.segment_tile_rows(*c.shape) == c.tile_rows
    loss, grad = _run(c, walk, dev)
    if c.repeat:                                                       # integer atomics on the mixed rows: order-independent
        loss2, grad2 = _run(c, walk, dev)
        assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
    if c.zero:
        assert ref["loss"] == 0.0 and loss.item() == 0.0 and not grad.any()
        return
    assert ref["loss"] >= KC.MIN_LOSS                                   # the value assertion is live
    g_all, g_seg, void = KC.gradient_ratios(c, grad, ref["grad"])
    ratios = {"loss": KC.loss_ratio(loss.item(), ref), "grad": g_all, "grad/segment": g_seg}
    print(f"KLD64 {name} {walk}: loss {loss.item():.9g} float64 {ref['loss']:.9g}; error / bound: "
          + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    failed = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not failed, failed
    assert void == 0.0
    single = ref["counts"].reshape(-1) == 1                              # a segment of one pixel contributes nothing: gradient exactly 0
    if bool(single.any()):
        seg, _ = KC.segment_ids(c, dev)
        lone = torch.cat([single, single.new_zeros(1)])[seg]            # [B, HW]; the last entry: pixels without a class
        assert bool(lone.any()) and not grad.permute(0, 2, 1)[lone].any()


@pytest.mark.parametrize("name", [n for n in KC.CASE_NAMES if not KC.case(n).zero])
def test_pair_sums_against_float64(name):
    """The three reduction passes' A[b][c][j][k], element by element, under both walks."""
    from scaleprotoseg_amd.loss import segment_pair_sums

    dev = gpu_device()
    c = KC.case(name)
    ref = _reference(name)
    B, H, W = c.shape
    planes, lab = c.planes.to(dev), c.labels.reshape(B, -1).to(dev)
    ratios = {}
    for walk in WALKS:
        A = segment_pair_sums(planes, lab, c.K, W if walk == "grid" else 0)
        ratios[walk] = KC.pair_ratio(c, A, ref)
        assert not torch.diagonal(A, dim1=2, dim2=3).any()
        assert not A[ref["counts"] == 0].any()
    print(f"KLD64 {name}: pair sums, error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert ref["loss"] >= KC.MIN_LOSS
    failed = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not failed, failed


@pytest.mark.parametrize("name", KC.CASE_NAMES)
def test_counts_and_lse_against_float64(name):
    """Passes 0 and 1: pixel counts and log-sum-exp per (image, class, slot), under both walks."""
    from scaleprotoseg_amd import _lib
    from scaleprotoseg_amd.loss import _kld_segment_passes

    dev = gpu_device()
    c = KC.case(name)
    ref = _reference(name)
    B, H, W = c.shape
    planes, lab = c.planes.to(dev).contiguous(), c.labels.reshape(B, -1).to(dev).int().contiguous()
    ratios = {}
    for walk in WALKS:
        _, counts, lse, _ = _kld_segment_passes(_lib.load(), planes, lab, c.K, W if walk == "grid" else 0, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert torch.equal(counts.long(), ref["counts"])
        assert torch.equal(ref["counts"], torch.stack([torch.bincount(x[(x >= 0) & (x < c.K)], minlength=c.K) for x in lab.long()]))
        assert not lse[ref["counts"] == 0].any()
        ratios[walk] = KC.lse_ratio(lse, ref)
    print(f"KLD64 {name}: lse, error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    failed = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not failed, failed
