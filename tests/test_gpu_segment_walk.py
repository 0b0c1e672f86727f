"""GPU checks of the shared segment walk (csrc/spx_kld_walk.h) under both families that use it: the KLD loss against LO.kld_loss in
float64 and the activation losses against the float64 restatement of tests/activation_loss_cases.py, with the tolerances of
the existing tests of those kernels.  The planes are random [B, J, HW] tensors (no distance kernel; for the KLD loss both
independent slots, loss about 0, and tests/kld_cases.py's correlated ones, loss about 0.4); the label map (kld_cases.band_labels)
is built so that every branch of the walk runs whatever tile height the launcher picks (tiles start at multiples of 16 rows):
  rows  0 -  7  one class                         a uniform run
  rows  8 - 15  another class                     a class change inside one wave's walk: a publish mid-walk
  rows 16 - 19  void                              a step that is skipped
  rows 20 - 27  a random class per pixel, with    mixed steps: the per-lane path
                void, one value >= K, one < 0
  rows 28 - 36  a third class                     the ragged end
83 columns are two tile columns; the second has a 3-column strip and two waves without a step."""
import functools

import pytest
import torch

from oracle import loss_oracle as LO
from oracle import ppnet_oracle as O
from kld_cases import BAND_B, BAND_H, BAND_W, MIN_LOSS, band_classes, band_labels as _labels, correlated_planes
from activation_loss_cases import W3, check_against_reference64, identity, log_activation, reference64
from support import gpu_device

pytestmark = pytest.mark.gpu

B, H, W = BAND_B, BAND_H, BAND_W                           # 2 x 37 x 83
WIDTHS = (3, 7, 11, 16)                                   # one J per JT = 4, 8, 12, 16
WALKS = ("grid", "linear")


def _grid(walk):
    return (H, W) if walk == "grid" else (1, H * W)


@functools.lru_cache(maxsize=None)
def _kld_case(K, J, planes):
    """(target, labels0 int32, table, planes, loss module, float64 loss, float64 gradient), on the device; ``planes``: "independent"
    (rand * 30 per slot) or "correlated" (kld_cases.correlated_planes)."""
    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd.loss import ClassDistances, class_slot_table

    dev = gpu_device()
    P = K * J
    ident = O.default_class_identity(P, K, 1)
    lab = _labels(K, band_classes(K)).to(dev)
    t = lab + 1
    table = class_slot_table(ident).to(dev)
    assert tuple(table.shape) == (K, J)
    gen = torch.Generator(device=dev).manual_seed(1000 * K + J)
    base = torch.rand(B, J, H * W, device=dev, generator=gen) * 30 if planes == "independent" else correlated_planes(B, J, H * W, gen)
    loss_fn = spx.KLDLoss(ident, 1, {0: (0, P)})
    lab32 = lab.reshape(B, -1).int()
    v2 = base.double().clone().requires_grad_(True)
    l2 = LO.kld_loss(loss_fn, ClassDistances(v2, lab32, table, (H, W)), t)
    l2.backward()
    return t, lab32, table, base, loss_fn, l2.item(), v2.grad


def _check_kld(K, J, walk):
    from scaleprotoseg_amd.loss import ClassDistances

    for planes in ("independent", "correlated"):
        t, lab32, table, base, loss_fn, ref, ref_grad = _kld_case(K, J, planes)
        v1 = base.clone().requires_grad_(True)
        l1 = loss_fn(ClassDistances(v1, lab32, table, _grid(walk)), t)
        l1.backward()
        torch.cuda.synchronize()
        gmax = ref_grad.abs().max().item()
        gerr = (v1.grad.double() - ref_grad).abs().max().item()
        print(f"KLD K={K} J={J} {walk} {planes}: loss {l1.item():.9g} ref {ref:.9g}; gradient err {gerr:.3g} of max {gmax:.3g}")
        assert ref > 0 and gmax > 0
        if planes == "correlated":
            assert ref >= MIN_LOSS                                # the value assertion below is live
        assert abs(l1.item() - ref) <= 1e-5 * max(1.0, abs(ref))
        assert gerr <= 1e-4 * gmax


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("J", WIDTHS)
def test_kld_against_float64(J, walk):
    """Value within 1e-5 max(1, |l|), gradient within 1e-4 max|g| of LO.kld_loss in float64."""
    _check_kld(5, J, walk)


@pytest.mark.parametrize("walk", WALKS)
def test_kld_two_class_blocks(walk):
    """K = 31, J = 16: the pair pass's tables hold floor(61440 / (16*16*8 + 16*4)) = 29 classes, so classes 29 and 30 (both
    among the bands) are summed by a second class block; 31*16*12 + 31*4 + 8 bytes stay inside the reduction passes' tables."""
    assert 61440 // (16 * 16 * 8 + 16 * 4) == 29 and 31 * 16 * 12 + 31 * 4 + 8 <= 60 * 1024
    _check_kld(31, 16, walk)


ACT_COUNTS = {3: [[2, 2, 1, 2, 2], [1, 1, 1, 0, 1]],          # per scale, prototypes of each class: ragged, max J per class
              7: [[4, 4, 2, 4, 4], [3, 3, 3, 1, 3]],
              11: [[6, 6, 6, 3, 6], [5, 2, 5, 5, 5]],
              16: [[8, 8, 8, 8, 5], [8, 8, 1, 8, 8]]}


@functools.lru_cache(maxsize=None)
def _act_case(J, norm_type):
    """(identity, ranges, target, labels0, table, planes, float64 reference with the gradient as planes [B, J, HW]), on the CPU."""
    from scaleprotoseg_amd.loss import class_slot_table

    K = 5
    ident, rl = identity(ACT_COUNTS[J])
    P = ident.shape[0]
    table = class_slot_table(ident)
    assert tuple(table.shape) == (K, J)
    lab = _labels(K, ((0, 1, 2), (3, 4, 1))).reshape(B, -1)
    target = (lab + 1).reshape(B, H, W)
    gen = torch.Generator().manual_seed(2000 + J)
    planes = torch.rand(B, J, H * W, generator=gen) * 2.0
    # the P-wide map whose class-gathered entries are the planes (the restatement reads no other entry)
    ok = (lab >= 0) & (lab < K)
    idx = table[lab.clamp(0, K - 1)]                                          # [B, HW, J]
    valid = ok.unsqueeze(-1) & (idx >= 0)
    bi, pi, ji = torch.nonzero(valid, as_tuple=True)
    d = torch.rand(B, H * W, P, generator=gen) * 2.0
    d[bi, pi, idx[bi, pi, ji]] = planes[bi, ji, pi]
    vals, counts, total, grad = reference64(d.reshape(B * H * W, P), target, ident, rl, norm_type, W3, log_activation)
    gp = torch.zeros(B, J, H * W, dtype=torch.float64)
    gp[bi, ji, pi] = grad.reshape(B, H * W, P)[bi, pi, idx[bi, pi, ji]]
    return ident, rl, target, lab, table, planes, (vals, counts, total, gp)


@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("J", WIDTHS)
def test_activation_losses_against_float64(J, walk):
    """Terms and total within 1e-5 max(1, |v|), gradient within 1e-4 max|g| + 1e-12 of the float64 restatement, l1 and linf."""
    import scaleprotoseg_amd as spx
    from scaleprotoseg_amd.loss import ClassDistances

    dev = gpu_device()
    for nt in ("l1", "linf"):
        ident, rl, target, lab, table, planes, ref = _act_case(J, nt)
        x = planes.to(dev).requires_grad_(True)
        tgt = target.to(dev)
        cd = ClassDistances(values=x, labels=lab.to(dev).int(), table=table.to(dev), grid=_grid(walk), target=tgt,
                            target_version=tgt._version)
        ranges = {s: r for s, r in enumerate(rl)}
        tot, terms = spx.ActivationRegularizers(ident, len(rl), ranges, *W3, norm_type=nt)(cd, tgt)
        tot.backward()
        check_against_reference64(tot, terms, x.grad, ref, f"J={J} {walk} {nt}")
