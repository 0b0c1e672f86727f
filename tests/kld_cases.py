"""Inputs on which the KLD loss is NOT vanishing, shared by tests/test_kld_inputs_cpu.py (are the inputs and the bounds sound?)
and tests/test_gpu_kld_float64.py (do the kernels of csrc/spx_kld.hip keep the bounds?).  A plain module, no fixtures.

Independent ``rand * 30`` planes give every slot of a segment its own softmax peak: the symmetric KL of a pair is 15 - 40 and
exp(-kld), the loss, is 1e-6 or less, so a value assertion relative to max(1, |loss|) holds for a kernel that returns 0.  The
slots of a class are prototypes of that class; ``correlated_planes`` gives them one spatial profile plus noise and the loss is a
few tenths, as on the reference's own fixtures (0.17 - 0.23).

``reference`` restates the segment statistics (lse, the pair sums A, exp(-kld) per segment and pair) in a given precision;
the loss and its gradient come from oracle.loss_oracle.kld_loss."""
import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from oracle import loss_oracle as LO
from oracle import ppnet_oracle as O

# ---- the bounds of tests/test_gpu_kld_float64.py (tests/test_kld_inputs_cpu.py holds the fp32 ORACLE to a quarter of each)
LOSS_TOL = 1e-5          # |l - l64| <= LOSS_TOL * max(1, |l64|)
GRAD_TOL = 1e-4          # max|g - g64| <= GRAD_TOL * max|g64|, globally and per segment with the floor below
# A segment's gradient scale is max(its own max|g64|, SEG_FLOOR * the global max|g64|).  The floor only bears on a segment whose
# gradient cancels to (about) zero: the identical slots of the degenerate case.  There the fp32 ORACLE leaves 0.65e-7 of the global
# maximum (p_m sum_k Cf[m][k] l_k with zero row sums of Cf: rounding of terms that cancel), 0.65 of a bound with the floor at 1e-3;
# four times that needs 2.6e-3.  Every other contributing segment's own maximum is 0.17 of the global one or more (asserted at
# ten floors by tests/test_kld_inputs_cpu.py), so the floor loosens nothing that carries a gradient.
SEG_FLOOR = 4e-3
# |A - A64| <= PAIR_TOL * (1 + |A64|) + PAIR_LSE_ULPS * eps32 * (|lse_j| (1 + |A64|) + |lse_k|) per off-diagonal element of a
# segment with a pixel.  The second term: A[j][k] = sum_px p_j (l_k - l_j) with l = v - lse, p = exp(l), and lse is STORED in fp32
# (by the kernels and by the fp32 oracle alike).  A rounding d_j of lse_j, |d_j| <= eps32/2 |lse_j|, shifts l_k - l_j by d_j - d_k
# and scales p_j by 1 - d_j, so A[j][k] is off by up to eps32/2 (|lse_j| (1 + |A|) + |lse_k|): 0.24 to 0.29 of the first term
# alone at lse = 33 (span 30), 1.2 of it at lse = 230 (offset 200), 2.4 at lse = 260 (span 256) - measured on the fp32 oracle
# with float64 sums, i.e. with nothing else in it.  Four times the storage rounding is 2 eps32 (|lse_j| (1 + |A|) + |lse_k|).
# (The loss and the gradient see only A[j][k] + A[k][j] and l_k - A[m][k], where a shift of lse_k cancels; their bounds stay.)
PAIR_TOL = 1e-5
PAIR_LSE_ULPS = 2.0
EPS32 = 2.0 ** -23
LSE_TOL = 1e-5           # |lse - lse64| <= LSE_TOL * max(1, |lse64|)
MIN_LOSS = 0.05          # every value assertion is made against a float64 loss of at least this ...
MAX_LOSS = 0.95          # ... and the pairs are not all saturated at exp(-0) = 1 either
LIVE_TERM = 1e-3         # a (segment, pair) entry "bears on the value" when exp(-kld) >= LIVE_TERM
LIVE_SHARE = 0.9         # share of the valid entries that must do so (a case's stated degenerate pairs aside)


def correlated_planes(B, J, HW, gen, span=30.0, sigma=1.0, offset=0.0):
    """[B, J, HW] fp32 on the generator's device: one spatial profile ``rand * span`` shared by all slots, plus ``sigma * randn``
    per slot, plus ``offset``."""
    dev = gen.device
    common = torch.rand(B, 1, HW, generator=gen, device=dev) * span
    return (common + sigma * torch.randn(B, J, HW, generator=gen, device=dev) + offset).float()


# ---- label maps
BAND_B, BAND_H, BAND_W = 2, 37, 83


@functools.lru_cache(maxsize=None)
def band_labels(K, bands):
    """labels0 [B, H, W] (class 0..K-1, else none) of the segment walk's tests (tests/test_gpu_segment_walk.py has the table of
    its rows); ``bands[b]``: the three band classes of image b."""
    B, H, W = BAND_B, BAND_H, BAND_W
    gen = torch.Generator().manual_seed(37 * 83 + K)
    lab = torch.full((B, H, W), -1, dtype=torch.long)
    for b in range(B):
        c0, c1, c2 = bands[b]
        lab[b, 0:8], lab[b, 8:16], lab[b, 28:] = c0, c1, c2
        lab[b, 20:28] = torch.randint(-1, K, (8, W), generator=gen)
        lab[b, 21, 5], lab[b, 26, 70] = K + 1, -3
    for b in range(B):
        assert len(set(bands[b])) == 3
        assert (lab[b, 0:8] == bands[b][0]).all() and (lab[b, 8:16] == bands[b][1]).all()        # two classes, two 8-row bands
        assert (lab[b, 16:20] == -1).all() and (lab[b, 28:] == bands[b][2]).all()
        blocks = [lab[b, r:r + 4, c:c + 16] for r in (20, 24) for c in range(0, W, 16)]
        assert any(len(set(x[(x >= 0) & (x < K)].tolist())) >= 2 for x in blocks)                 # a mixed 16 x 4 step
        assert (lab[b] >= K).any() and (lab[b] < -1).any()
    return lab


def band_classes(K):
    return ((0, K - 1, 2), (K - 2, 1, K - 1)) if K > 5 else ((0, 1, 2), (3, 4, 1))


def tall_labels(B, H, W, K, gen):
    """Blocks of 64 x 8 pixels of one class (or void) each, and four rows of per-pixel random labels, void among them: long
    uniform runs down a 16-column strip, mixed steps inside them."""
    lab = torch.randint(-1, K, (B, (H + 63) // 64, (W + 7) // 8), generator=gen)
    lab = lab.repeat_interleave(64, 1).repeat_interleave(8, 2)[:, :H, :W].contiguous()
    lab[:, 5:9, :] = torch.randint(-1, K, (B, 4, W), generator=gen)
    return lab


def segment_tile_rows(B, H, W):
    """spx_segment_tile_rows (csrc/spx_kld_walk.h) restated: 64-row tiles if they make 512 workgroups, else 32, else 16."""
    t = 64
    while t > 16 and B * ((W + 63) // 64) * ((H + t - 1) // t) < 512:
        t //= 2
    return t


# ---- cases
@dataclass
class KldCase:
    name: str
    K: int
    J: int
    S: int
    ident: torch.Tensor                    # [P, K]
    ranges: dict                           # scale -> (lo, hi)
    labels: torch.Tensor                   # labels0 [B, H, W] long
    planes: torch.Tensor                   # [B, J, H*W] fp32
    walks: Tuple[str, ...] = ("grid", "linear")
    tile_rows: Optional[int] = None        # the tile height the launcher must pick for the grid walk (asserted), if the case is about it
    stated: Optional[torch.Tensor] = None  # [B, K, J, J] bool: the case's stated degenerate pairs (outside the LIVE_SHARE rule)
    zero: bool = False                     # no segment at all: the loss is exactly 0
    repeat: bool = False                   # run twice, bit-identical
    flat: Tuple[Tuple[int, int], ...] = () # (image, class) segments whose float64 gradient is 0 though they contribute: the floor's

    @property
    def shape(self):
        return tuple(self.labels.shape)

    def grid(self, walk):
        B, H, W = self.shape
        return (H, W) if walk == "grid" else (1, H * W)

    def loss_module(self):
        import scaleprotoseg_amd as spx

        return spx.KLDLoss(self.ident, self.S, self.ranges)


def _band_case(name, K, J, seed, S=1, labels=None, **planes_kw):
    P = K * J
    lab = band_labels(K, band_classes(K)) if labels is None else labels
    B, H, W = lab.shape
    gen = torch.Generator().manual_seed(seed)
    return KldCase(name, K, J, S, O.default_class_identity(P, K, S), O.default_scale_ranges(P, S), lab,
                   correlated_planes(B, J, H * W, gen, **planes_kw))


def _tall_case(name, B, H, W):
    K, J = 6, 10
    gen = torch.Generator().manual_seed(H)
    lab = tall_labels(B, H, W, K, gen)
    planes = correlated_planes(B, J, H * W, gen)
    rows = segment_tile_rows(B, H, W)
    mixed = lab[:, 4:12].reshape(B, 2, 4, W)                       # the two steps the four random rows fall into
    assert any(len(set(x[x >= 0].tolist())) >= 2 for x in mixed[:, :, :, :16].reshape(-1, 4, min(W, 16)))
    return KldCase(name, K, J, 1, O.default_class_identity(K * J, K, 1), O.default_scale_ranges(K * J, 1), lab, planes,
                   walks=("grid",), tile_rows=rows, repeat=True)


def _degenerate_case():
    """Ordinary segments beside degenerate ones (B = 3, K = 8, J = 7, the band map's size):
      class 0   ordinary, in images 0 and 1 (random rows)          class 4   ordinary; in image 1 slot 3 attains its maximum twice
      class 1   image 0 only: all slots are the SAME plane          class 5   ordinary
      class 2   image 0 only: a single pixel                        class 6   image 0 only: slot 2 is independent rand * 30
      class 3   image 0 only: exactly two pixels, 0.1 sigma apart   class 7   image 1 only
      image 2   all void"""
    K, J, B, H, W = 8, 7, 3, BAND_H, BAND_W
    gen = torch.Generator().manual_seed(8707)
    lab = torch.full((B, H, W), -1, dtype=torch.long)
    pool = torch.tensor([-1, 0, 4, 5])
    lab[0, 0:8], lab[0, 8:16], lab[0, 28:] = 0, 1, 6
    lab[1, 0:8], lab[1, 8:16], lab[1, 28:] = 5, 7, 4
    for b in (0, 1):
        lab[b, 20:28] = pool[torch.randint(0, 4, (8, W), generator=gen)]
    lab[0, 17, 40] = 2
    lab[0, 17, 3], lab[0, 19, 70] = 3, 3
    lab[1, 18, 7], lab[1, 16, 50] = K, -2                           # out of range on either side
    planes = correlated_planes(B, J, H * W, gen)
    flat = lab.reshape(B, -1)
    same = flat[0] == 1
    planes[0][:, same] = planes[0][0:1, same]                       # class 1: every slot is slot 0's plane
    odd = flat[0] == 6
    planes[0][2, odd] = torch.rand(int(odd.sum()), generator=gen) * 30
    pair = torch.nonzero(flat[0] == 3).flatten()                    # class 3: the second pixel lies 0.1 sigma from the first, so that
    planes[0][:, pair[1]] = planes[0][:, pair[0]] + 0.1 * torch.randn(J, generator=gen)      # neither softmax saturates
    twice = torch.nonzero(flat[1] == 4).flatten()
    top = planes[1][3, twice].max() + 0.5
    planes[1][3, twice[5]] = top
    planes[1][3, twice[-3]] = top
    assert int((flat[0] == 2).sum()) == 1 and int((flat[0] == 3).sum()) == 2 and (flat[2] == -1).all()
    assert not (flat[1] == 6).any() and not (flat[0] == 7).any() and (flat[1] == 7).any()
    assert int((planes[1][3, twice] == top).sum()) == 2
    stated = torch.zeros(B, K, J, J, dtype=torch.bool)
    stated[0, 6, 2, :] = True
    stated[0, 6, :, 2] = True                                       # the pairs of the independent slot: exp(-kld) about 0
    P = K * J
    return KldCase("degenerate", K, J, 1, O.default_class_identity(P, K, 1), O.default_scale_ranges(P, 1), lab, planes, stated=stated,
                   flat=((0, 1),))


BAND_WIDTHS = (3, 7, 11, 16)                                        # one J per compile-time width 4, 8, 12, 16
CASE_NAMES = tuple(f"band_J{J}" for J in BAND_WIDTHS) + ("band_K31_J16", "tall_32rows", "tall_64rows", "offset_plus200",
                                                         "offset_minus15", "span256", "degenerate", "all_void", "two_scales")


@functools.lru_cache(maxsize=None)
def case(name) -> KldCase:
    """The case on the CPU; built once, never modified by a test."""
    if name.startswith("band_J"):
        J = int(name[6:])
        return _band_case(name, 5, J, J)
    if name == "band_K31_J16":                                      # two class blocks in the pair pass (29 classes fit its tables)
        return _band_case(name, 31, 16, 3116)
    if name == "tall_32rows":
        c = _tall_case(name, 8, 2048, 16)
        assert c.tile_rows == 32
        return c
    if name == "tall_64rows":                                       # the second wave's strip is one column wide, waves 2 and 3 idle
        c = _tall_case(name, 8, 4096, 17)
        assert c.tile_rows == 64
        return c
    if name == "offset_plus200":
        return _band_case(name, 5, 7, 1, offset=200.0)
    if name == "offset_minus15":                                    # values on both sides of 0: float_key changes branch
        c = _band_case(name, 5, 7, 2, offset=-15.0)
        assert (c.planes < 0).any() and (c.planes > 0).any()
        return c
    if name == "span256":
        return _band_case(name, 5, 7, 3, span=256.0)
    if name == "degenerate":
        return _degenerate_case()
    if name == "all_void":
        c = _band_case(name, 5, 7, 4, labels=torch.full((BAND_B, BAND_H, BAND_W), -1, dtype=torch.long))
        c.labels[0, 3, 3], c.labels[1, 30, 80] = 5, -7               # out of range is void too
        c.zero = True
        return c
    if name == "two_scales":                                        # S = 2, default ranges: slots 0-5 and 6-11 of a class are not compared
        c = _band_case(name, 5, 12, 5, S=2)
        ok = c.loss_module()._pair_mask_build(_table(c))
        assert int(ok[0].sum()) == 2 * 15 and not ok[0, 0, 6] and ok[0, 0, 5] and ok[0, 6, 11]
        return c
    raise KeyError(name)


def _table(c):
    from scaleprotoseg_amd.loss import class_slot_table

    t = class_slot_table(c.ident)
    assert tuple(t.shape) == (c.K, c.J)
    return t


def segment_ids(c: KldCase, device=None):
    """(seg [B, HW] = b * K + class, or B * K for a pixel without a class; ok [B, HW])."""
    B = c.shape[0]
    lab = c.labels.reshape(B, -1).to(device)
    ok = (lab >= 0) & (lab < c.K)
    seg = torch.arange(B, device=lab.device).unsqueeze(1) * c.K + lab.clamp(0, c.K - 1)
    return torch.where(ok, seg, torch.full_like(seg, B * c.K)), ok


def reference(c: KldCase, dtype=torch.float64, device=None):
    """The loss of the case in ``dtype`` on ``device``: dict with
      loss (float), grad [B, J, HW] (float64)                      oracle.loss_oracle.kld_loss and autograd
      counts [B, K], lse [B, K, J] (0 where empty), A [B, K, J, J]   A[j][k] = sum_px p_j (l_k - l_j), restated here
      e [B, K, J, J] = exp(-kld), valid [B, K, J, J]                 kld = -(A[j][k] + A[k][j]) / 2; compared pairs of segments with >= 2 pixels"""
    from scaleprotoseg_amd.loss import ClassDistances

    B, H, W = c.shape
    K, J = c.K, c.J
    table = _table(c).to(device)
    fn = c.loss_module()
    lab = c.labels.to(device)
    v = c.planes.to(device=device, dtype=dtype).clone().requires_grad_(True)
    loss = LO.kld_loss(fn, ClassDistances(v, lab.reshape(B, -1).int(), table, (H, W)), lab + 1)
    if loss.requires_grad:
        loss.backward()
    grad = v.grad.double() if v.grad is not None else torch.zeros_like(v, dtype=torch.float64)
    seg, ok = segment_ids(c, device)
    nseg = B * K
    counts = torch.bincount(seg.reshape(-1), minlength=nseg + 1)[:nseg].reshape(B, K)
    lse = torch.zeros(nseg + 1, J, dtype=dtype, device=v.device)
    A = torch.zeros(nseg + 1, J, J, dtype=torch.float64, device=v.device)
    with torch.no_grad():
        for b in range(B):                                            # per image: [HW, J, J] temporaries, not [B * HW, J, J]
            d = v[b].t()                                              # [HW, J]
            idx = seg[b].unsqueeze(1).expand(-1, J)
            m = torch.full((nseg + 1, J), float("-inf"), dtype=dtype, device=v.device).scatter_reduce(0, idx, d, "amax")
            # per-pixel arithmetic in ``dtype``, every sum over pixels in float64 (as the oracle sums exp, and as the kernels'
            # integer fixed point does: what is measured in fp32 is the arithmetic, not a 50 000-term fp32 summation)
            s = torch.zeros(nseg + 1, J, dtype=torch.float64, device=v.device).index_add(0, seg[b], torch.exp(d - m[seg[b]]).double())
            here = s[:, 0] > 0
            lse[here] = (m.double() + torch.log(s)).to(dtype)[here]
            l = d - lse[seg[b]]
            A.index_add_(0, seg[b], (torch.exp(l).unsqueeze(2) * (l.unsqueeze(1) - l.unsqueeze(2))).double())
    A = A[:nseg].reshape(B, K, J, J)
    lse = lse[:nseg].reshape(B, K, J)
    pair_ok = fn._pair_mask_build(table.cpu()).to(v.device)
    valid = pair_ok.unsqueeze(0) & (counts >= 2).reshape(B, K, 1, 1)
    e = torch.exp(0.5 * (A + A.transpose(2, 3)).double())
    return {"loss": float(loss.detach()), "grad": grad, "counts": counts, "lse": lse.double(), "A": A.double(), "e": e, "valid": valid}


def segment_gradient_maxima(c: KldCase, ref_grad):
    """[B, K]: max |g64| over the pixels of each segment and all slots (0 where the segment is empty)."""
    B = c.shape[0]
    seg, _ = segment_ids(c, ref_grad.device)
    mag = ref_grad.abs().amax(dim=1).reshape(-1)
    out = torch.zeros(B * c.K + 1, dtype=torch.float64, device=mag.device).scatter_reduce(0, seg.reshape(-1), mag, "amax")
    return out[:B * c.K].reshape(B, c.K)


def gradient_ratios(c: KldCase, grad, ref_grad):
    """(global, per segment): the worst error / bound of a gradient [B, J, HW] against the float64 one, and the largest
    |gradient| at a pixel without a class (must be 0).  Per segment the bound is GRAD_TOL * max(the segment's own max|g64|,
    SEG_FLOOR * the global max|g64|), taken over the segment's pixels and all slots."""
    B = c.shape[0]
    seg, ok = segment_ids(c, ref_grad.device)
    nseg = B * c.K
    gmax = ref_grad.abs().max().item()
    err = (grad.double() - ref_grad).abs().amax(dim=1)                 # [B, HW]
    mag = ref_grad.abs().amax(dim=1)
    segmax = torch.zeros(nseg + 1, dtype=torch.float64, device=err.device).scatter_reduce(0, seg.reshape(-1), mag.reshape(-1), "amax")
    bound = GRAD_TOL * torch.maximum(segmax, torch.full_like(segmax, SEG_FLOOR * gmax))[seg]
    per_seg = (err[ok] / bound[ok]).max().item() if gmax > 0 else float("inf")
    void = grad.double().abs().amax(dim=1)[~ok].max().item() if bool((~ok).any()) else 0.0
    return err.max().item() / (GRAD_TOL * gmax) if gmax > 0 else float("inf"), per_seg, void


def pair_ratio(c: KldCase, A, ref):
    """Worst |A - A64| / bound (see PAIR_TOL) over the off-diagonal entries of the segments with a pixel."""
    off = ~torch.eye(c.J, dtype=torch.bool, device=A.device)
    sel = (ref["counts"] > 0).reshape(*ref["counts"].shape, 1, 1) & off
    mag = ref["lse"].abs()
    stored = PAIR_LSE_ULPS * EPS32 * (mag.unsqueeze(3) * (1.0 + ref["A"].abs()) + mag.unsqueeze(2))
    r = (A.double() - ref["A"]).abs() / (PAIR_TOL * (1.0 + ref["A"].abs()) + stored)
    return r[sel].max().item()


def lse_ratio(lse, ref):
    return ((lse.double() - ref["lse"]).abs() / (LSE_TOL * ref["lse"].abs().clamp_min(1.0))).max().item()


def loss_ratio(loss, ref):
    return abs(loss - ref["loss"]) / (LOSS_TOL * max(1.0, abs(ref["loss"])))
