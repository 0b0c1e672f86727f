"""Cases, per-tile magnitude patterns and float64 references of the distance backward's K1 -> K2 crossing;
tests/test_bwd_scale_cases_cpu.py pins this file, tests/test_gpu_bwd_tile_scales.py holds the kernels to it.  CPU tensors
only; nothing here touches a device.

G = dLoss/dDistances crosses from the pixel kernel (K1) to the parameter kernel (K2) as ONE fp16 plane with one power-of-two
exponent per (panel, 128-pixel tile); K2's workgroup w walks the chunks w, w + nslabs, ... and rescales its accumulators
whenever the exponent changes (chunk_scale in spx_bank.hip).  Every case here

  * walks at least three chunks per workgroup, with at least one walk crossing an image end - read off the library's own
    workspace size (``nslabs``), not off a restated cap;
  * multiplies the upstream gradients of tile (b, t) by s(b, t) = 2^k, k from LEVELS, or by zero, in a seeded pattern in which
    some walk sees every kind of transition (TRANSITIONS);
  * confines the gradients of a tile of class c to the prototypes p = c and the classes k = c (mod 6), and the head matrix
    to the entries with k = p (mod 6): every row of dPrototypes and every row of dLastLayer then sums terms of ONE magnitude,
    so a row-wise bound sees a small tile that a whole-tensor bound would not.

References are the oracle's own forward on ``.double()`` inputs under autograd (``reference``) and a float64 restatement of
what crosses (``restated``): G rounded to fp16 at the per-(panel, tile) scale, dLogits and a / ln 2 as bf16 hi + lo pairs,
activations of heads wider than 32 classes rounded to 15 bits of their (pixel, 32-prototype block) maximum.  TOL_* are four
times the restatement's own worst per-row ratio over all cases (profiles/tile_scales_summary.md)."""
import ctypes as C
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from oracle import ppnet_oracle as O

TILE_PX = 128
LEVELS = (20, 8, 0, -12, -24, -36)          # k of tile class 0..5
ZERO = 6                                    # tile class "zero": every upstream gradient of the tile is 0
TRANSITIONS = ("up", "down", "equal", "into_zero", "out_of_zero")

# name: (B, S, Cs, prototypes per scale, K, H, W, feature dtypes, pixels per K2 chunk)
CASES = {
    "ksplit": (3, 4, 64, 57, 19, 71, 71, ("fp32", "bf16"), 64),      # k-step split; ragged rows; 4 panels
    "nosplit": (3, 2, 96, 230, 19, 71, 71, ("fp32",), 64),           # 2 panels of 115 per scale; K1 accumulates dX
    "pipelined": (3, 4, 128, 190, 19, 71, 71, ("fp32",), 32),        # 6-block panels, one class block, Cs > 64
    "dma": (3, 2, 128, 300, 19, 64, 80, ("bf16",), 64),              # H*W % 64 == 0, bf16 features: the LDS-DMA kernel
    "two_class_blocks": (3, 4, 64, 57, 57, 71, 71, ("bf16",), 64),   # d_W inside K2, int16 activation blob
    "five_class_blocks": (2, 4, 64, 450, 150, 33, 65, ("fp32",), 64),  # ADE bank: 12 panels, separate d_bank / d_W launches
}
LOSS_SCALE_CASES = ("ksplit", "five_class_blocks")
LOSS_SCALES = (16, -30)
ACT_CASE = "two_class_blocks"
# a descending staircase beyond the 2^80 of K2's skip rule: the tiles a workgroup adds as its j-th chunk carry 2^STAIR_LEVELS[j]
# (and the pattern of class j), so EVERY walk descends by 2^36, 2^36 and 2^48, 2^120 in all.  The third chunk stays 2^72 below
# the first: clear of the skip rule's 2^80 whatever the tiles' own maxima; the fourth lies beyond it
STAIR_CASES = ("ksplit", "dma")
STAIR_LEVELS = (40, 4, -32, -80)

# four times the restatement's worst per-row ratio against exact float64, over all cases (test_bwd_scale_cases_cpu.py
# re-measures them; profiles/tile_scales_summary.md has the figures)
TOL_DP_ROW = 3.7e-3                        # 4 x 9.19e-4 (ksplit): G as one fp16 plane, 11 significant bits
TOL_DW_ROW_PAIRS = 2.3e-4                  # 4 x 5.69e-5 (nosplit): heads of <= 32 classes, a / ln 2 as a bf16 hi + lo pair
TOL_DW_ROW_INT16 = 6.3e-4                  # 4 x 1.56e-4 (five_class_blocks): wider heads, 15 bits of the block maximum
TOL_DW_COL = 1.25e-3                       # 4 x 3.11e-4: dLastLayer per column on ACT_CASE with uneven activations - a column
#                                            whose prototype is far from most pixels holds 15 bits of its BLOCK's maximum only


def tol_dw_row(name):
    return TOL_DW_ROW_PAIRS if CASES[name][4] <= 32 else TOL_DW_ROW_INT16


def shape_of(name):
    B, S, Cs, per, K, H, W, dtypes, cpx = CASES[name]
    return SimpleNamespace(B=B, S=S, Cs=Cs, per=per, P=per * S, K=K, H=H, W=W, HW=H * W, dtypes=dtypes, cpx=cpx,
                           tiles=-(-H * W // TILE_PX), ranges={s: (s * per, (s + 1) * per) for s in range(S)})


def layout_of(name, head=True):
    from scaleprotoseg_amd.functional import BankLayout

    sh = shape_of(name)
    return BankLayout(sh.P, sh.K if head else 1, sh.S, sh.Cs, tuple(sh.ranges[s] for s in range(sh.S)))


# ---------------------------------------------------------------------------------------------------------------------
# the walk, from the library
# ---------------------------------------------------------------------------------------------------------------------
def nslabs(name, B=None):
    """Workgroups per panel of K2's launch: spx_bank_bwd_workspace_bytes over the bytes of one slab (a one-tile image has two
    chunks, hence two slabs)."""
    from scaleprotoseg_amd import _lib

    sh = shape_of(name)
    lib, plan = _lib.load(), layout_of(name).plan()
    per_slab = lib.spx_bank_bwd_workspace_bytes(C.byref(plan), 1, 64) // 2
    return lib.spx_bank_bwd_workspace_bytes(C.byref(plan), sh.B if B is None else B, sh.HW) // per_slab


def walks(name):
    """Per workgroup the (image, tile) of each chunk it adds, in order: chunk c goes to workgroup c mod nslabs."""
    sh = shape_of(name)
    n = nslabs(name)
    per_img = sh.tiles * (TILE_PX // sh.cpx)
    out = [[] for _ in range(n)]
    for c in range(sh.B * per_img):
        out[c % n].append((c // per_img, (c % per_img) // (TILE_PX // sh.cpx)))
    return out


def transition(c0, c1):
    if c0 == ZERO or c1 == ZERO:
        return None if c0 == c1 else ("into_zero" if c1 == ZERO else "out_of_zero")
    return "equal" if c0 == c1 else ("up" if LEVELS[c1] > LEVELS[c0] else "down")


def transitions_per_walk(name):
    cls = tile_classes(name)
    return [{transition(cls[a], cls[b]) for a, b in zip(w, w[1:]) if a != b} - {None} for w in walks(name)]


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tile_classes(name):
    """[B, tiles] tile classes 0..6, seeded.  An image's (ragged) last tile gets a class whose k is not 0."""
    sh = shape_of(name)
    rng = np.random.default_rng(7100 + sorted(CASES).index(name))
    cls = rng.integers(0, 7, size=(sh.B, sh.tiles))
    cls[:, -1] = [(0, 5, 3, 1, 4)[b % 5] for b in range(sh.B)]
    cls.setflags(write=False)
    return cls


def stair_tile_levels(name):
    """[B, tiles]: the position (0..3) in its workgroup's walk of the first chunk of each tile (64-pixel chunks, an even slab
    count: both chunks of a tile have the same position)."""
    sh = shape_of(name)
    n = nslabs(name)
    assert sh.cpx == 64 and n % 2 == 0 and 2 * sh.B * sh.tiles <= len(STAIR_LEVELS) * n
    return (2 * np.arange(sh.B * sh.tiles).reshape(sh.B, sh.tiles)) // n


def build_staircase(name):
    """Upstream gradients of the staircase: as the "tiles" variant of ``build``, with level j in the place of tile class j.
    Returns (gradients, per-pixel level [B, HW])."""
    pb, sh = build(name), shape_of(name)
    lv = torch.from_numpy(np.repeat(stair_tile_levels(name), TILE_PX, axis=1)[:, :sh.HW].copy())
    s = torch.exp2(torch.tensor(STAIR_LEVELS, dtype=torch.float32))[lv]
    return pb.variant((lv[:, None, :] == pb.pm[None, :, None]).to(torch.float32),
                      (lv[:, :, None] == pb.km[None, None, :]).to(torch.float32), s), lv


def pixel_classes(name):
    sh = shape_of(name)
    return torch.from_numpy(np.repeat(tile_classes(name), TILE_PX, axis=1)[:, :sh.HW].copy())      # [B, HW]


def pixel_scale(name):
    """s per pixel, fp32 [B, HW]: 2^k of its tile, 0 on zero tiles."""
    c = pixel_classes(name)
    k = torch.tensor(LEVELS + (0,), dtype=torch.float32)[c]
    return torch.where(c == ZERO, torch.zeros(()), torch.exp2(k))


@functools.lru_cache(maxsize=None)
def build(name):
    """Inputs on the bf16 grid, the mod-6 head, base upstream gradients (randn * 1e-3) and the variants derived from them.
    Shared by the tests; never modified."""
    sh = shape_of(name)
    g = torch.Generator().manual_seed(20261021 + sorted(CASES).index(name))
    conv = O.bf16_representable(torch.sigmoid(torch.randn(sh.B, sh.S * sh.Cs, sh.H, sh.W, generator=g)))
    bank = O.bf16_representable(torch.rand(sh.P, sh.Cs, 1, 1, generator=g))
    km, pm = torch.arange(sh.K) % 6, torch.arange(sh.P) % 6
    Wl = (torch.randn(sh.K, sh.P, generator=g) * 0.3) * (km[:, None] == pm[None, :])
    g_logits = torch.randn(sh.B, sh.H, sh.W, sh.K, generator=g) * 1e-3
    g_dist = torch.randn(sh.B, sh.P, sh.H, sh.W, generator=g) * 1e-3
    g_act = torch.randn(sh.B * sh.HW, sh.P, generator=g) * 1e-3
    c = pixel_classes(name)                                              # zero tiles keep class 6: no prototype, no class
    s = pixel_scale(name)
    m_p = (c[:, None, :] == pm[None, :, None]).to(torch.float32)         # [B, P, HW]
    m_k = (c[:, :, None] == km[None, None, :]).to(torch.float32)         # [B, HW, K]
    # on zero tiles the "masked" run keeps class 0's pattern, so that run has no zero tile of its own
    c0 = torch.where(c == ZERO, torch.zeros_like(c), c)
    b_p = (c0[:, None, :] == pm[None, :, None]).to(torch.float32)
    b_k = (c0[:, :, None] == km[None, None, :]).to(torch.float32)

    def variant(mp, mk, sc):
        return SimpleNamespace(
            g_logits=(g_logits.view(sh.B, sh.HW, sh.K) * mk * sc[:, :, None]).view(sh.B, sh.H, sh.W, sh.K),
            g_dist=(g_dist.view(sh.B, sh.P, sh.HW) * mp * sc[:, None, :]).view(sh.B, sh.P, sh.H, sh.W),
            g_act=(g_act.view(sh.B, sh.HW, sh.P) * mp.transpose(1, 2) * sc[:, :, None]).reshape(sh.B * sh.HW, sh.P))

    one = torch.ones(sh.B, sh.HW)
    grads = {
        "plain": SimpleNamespace(g_logits=g_logits, g_dist=g_dist, g_act=g_act),     # 3(d): equal exponents
        "masked": variant(b_p, b_k, one),                                            # 3(a): the unscaled run
        "tiles": variant(m_p, m_k, s),                                               # 3(a), 3(b)
    }
    for k in LOSS_SCALES if name in LOSS_SCALE_CASES else ():
        f = 2.0 ** k
        grads[f"loss_scale_{k}"] = SimpleNamespace(g_logits=g_logits * f, g_dist=g_dist * f, g_act=g_act * f)
    return SimpleNamespace(name=name, sh=sh, conv=conv, bank=bank, Wl=Wl, grads=grads, scale=s, classes=c, variant=variant,
                           pm=pm, km=km)


@functools.lru_cache(maxsize=None)
def build_uneven_activations():
    """Section 4, on ACT_CASE: features overwritten so that the block exponents of the int16 activation blob differ between
    32-prototype blocks and between tiles.  Tiles t = 0 (mod 3): eight pixels sit exactly on prototypes 32..39 of their scale
    (whose values are multiples of 1/16; d = 0, activation ln(1 / 1e-4) = 9.21); tiles t = 1 (mod 3): every feature is 4.0 (distances in the hundreds, activations
    of a few 1e-3); the other tiles keep sigmoid(randn).  Upstream gradients: the plain ones."""
    pb = build(ACT_CASE)
    sh = pb.sh
    conv = pb.conv.clone().view(sh.B, sh.S, sh.Cs, sh.HW)
    bank = pb.bank.clone().view(sh.P, sh.Cs)
    for s in range(sh.S):
        # the prototypes pixels are put on hold multiples of 1/16: |x|^2, x.p and |p|^2 are then exact in fp32 in any order of
        # summation, so d is exactly 0 there on the device as in float64 (and the relu mask gives those pixels no gradient)
        lo = sh.ranges[s][0] + 32
        bank[lo:lo + 8] = torch.round(bank[lo:lo + 8] * 16.0) / 16.0
    on_proto = torch.zeros(sh.B, sh.HW, dtype=torch.bool)
    for b in range(sh.B):
        for t in range(sh.tiles):
            px0, px1 = t * TILE_PX, min((t + 1) * TILE_PX, sh.HW)
            if t % 3 == 1:
                conv[b, :, :, px0:px1] = 4.0
            elif t % 3 == 0:
                for j in range(8):
                    px = px0 + (5 + 13 * j) % (px1 - px0)
                    on_proto[b, px] = True
                    for s in range(sh.S):
                        conv[b, s, :, px] = bank[sh.ranges[s][0] + 32 + j]
    q = SimpleNamespace(**vars(pb))
    q.conv = conv.view(sh.B, sh.S * sh.Cs, sh.H, sh.W)
    q.bank = bank.view(sh.P, sh.Cs, 1, 1)
    q.on_proto = on_proto
    return q


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
def reference(pb, gr, head=True):
    """Exact float64: the oracle's forward on doubles under autograd.  dx [B, C, H, W], dp [P, Cs, 1, 1], dw [K, P] (None
    without a head), and what the restatement needs: G = dLoss/dDistances with the relu mask [B, P, HW], the activations
    [M, P]."""
    sh = pb.sh
    x = pb.conv.double().requires_grad_(True)
    p = pb.bank.double().requires_grad_(True)
    w = pb.Wl.double().requires_grad_(True)
    logits, d, act = O.forward_from_conv_features(x, p, sh.ranges, sh.S, w)
    d.retain_grad()
    loss = (d * gr.g_dist.double()).sum()
    if head:
        loss = loss + (logits * gr.g_logits.double()).sum() + (act * gr.g_act.double()).sum()
    loss.backward()
    G = (d.grad * (d.detach() > 0)).reshape(sh.B, sh.P, sh.HW)
    return SimpleNamespace(dx=x.grad, dp=p.grad, dw=w.grad if head else None, G=G, act=act.detach(),
                           logits=logits.detach(), dist=d.detach())


def _fp16(t):
    return t.to(torch.float32).to(torch.float16).to(torch.float64)


def _bf16_pair(t):
    """t (values of an fp32 tensor, as float64) as an exact-to-2^-17 bf16 hi + lo pair (split_bf16x2 in spx_common.h)."""
    t32 = t.to(torch.float32)
    hi = t32.to(torch.bfloat16).to(torch.float32)
    lo = (t32 - hi).to(torch.bfloat16).to(torch.float32)
    return hi.double(), lo.double()


def tile_exponents(pb, G, head=True):
    """e_t = 15 - frexp_exp(max |G| of the (panel, tile)), [npanels, B, tiles] (spx_bwd_impl.h; 15 for a zero tile)."""
    sh = pb.sh
    plan = layout_of(pb.name, head).plan()
    Gt = torch.nn.functional.pad(G, (0, sh.tiles * TILE_PX - sh.HW)).view(sh.B, sh.P, sh.tiles, TILE_PX)
    out = []
    for q in range(plan.npanels):
        p0, n = plan.panel_p0[q], plan.panel_np[q]
        mx = Gt[:, p0:p0 + n].abs().amax(dim=(1, 3))
        out.append(15 - torch.frexp(mx)[1].clamp(-100, 100))
    return torch.stack(out)


def restated(pb, gr, ref, head=True):
    """(dp, dw) float64 with the crossing's roundings and nothing else (exact sums, module docstring)."""
    sh = pb.sh
    plan = layout_of(pb.name, head).plan()
    e = tile_exponents(pb, ref.G, head)
    Gt = torch.nn.functional.pad(ref.G, (0, sh.tiles * TILE_PX - sh.HW)).view(sh.B, sh.P, sh.tiles, TILE_PX)
    G16 = torch.zeros_like(Gt)
    for q in range(plan.npanels):
        p0, n = plan.panel_p0[q], plan.panel_np[q]
        sc = torch.exp2(e[q].double())[:, None, :, None]
        G16[:, p0:p0 + n] = _fp16(Gt[:, p0:p0 + n] * sc) / sc
    G16 = G16.view(sh.B, sh.P, -1)[:, :, :sh.HW]
    x = pb.conv.double().view(sh.B, sh.S, sh.Cs, sh.HW)
    bank = pb.bank.double().view(sh.P, sh.Cs)
    dp = torch.zeros(sh.P, sh.Cs, dtype=torch.float64)
    for s in range(sh.S):
        lo, hi = sh.ranges[s]
        dp[lo:hi] = -2.0 * torch.einsum("bpm,bcm->pc", G16[:, lo:hi], x[:, s]) + 2.0 * bank[lo:hi] * G16[:, lo:hi].sum((0, 2))[:, None]
    if not head:
        return dp.view(sh.P, sh.Cs, 1, 1), None
    lh, ll = _bf16_pair(gr.g_logits.reshape(-1, sh.K))
    a2 = ref.act / math.log(2.0)
    if sh.K <= 32:
        ah, al = _bf16_pair(a2)
    else:
        # int16 codes round(a 2^-ea 32767), ea = frexp_exp of the largest |a| of the pixel's 32-prototype block of its panel;
        # K2 splits the code into an exact bf16 hi + lo pair
        ah, al = torch.zeros_like(a2), torch.zeros_like(a2)
        for q in range(plan.npanels):
            p0, n = plan.panel_p0[q], plan.panel_np[q]
            for j0 in range(p0, p0 + n, 32):
                j1 = min(j0 + 32, p0 + n)
                blk = a2[:, j0:j1].to(torch.float32).double()
                un = torch.exp2(torch.frexp(blk.abs().amax(dim=1, keepdim=True))[1].clamp(-100, 100).double()) / 32767.0
                code = torch.round(blk / un)
                ch = code.to(torch.bfloat16).double()
                ah[:, j0:j1], al[:, j0:j1] = ch * un, (code - ch) * un
    dw = math.log(2.0) * (lh.t() @ ah + lh.t() @ al + ll.t() @ ah)
    return dp.view(sh.P, sh.Cs, 1, 1), dw


# ---------------------------------------------------------------------------------------------------------------------
# measures
# ---------------------------------------------------------------------------------------------------------------------
def row_ratios(got, ref, dim):
    """Per slice along ``dim`` (0: rows of a [n, ...] tensor, 1: columns of a matrix): max|got - ref| / max|ref|; a slice
    whose reference is all zero must be all zero in ``got`` and reports 0.  Returns (ratios, number of all-zero slices)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape
    if dim == 1:
        got, ref = got.t(), ref.t()
    got, ref = got.reshape(got.shape[0], -1), ref.reshape(ref.shape[0], -1)
    scale = ref.abs().amax(dim=1)
    err = (got - ref).abs().amax(dim=1)
    zero = scale == 0
    assert (err[zero] == 0).all(), "a slice whose reference is exactly zero is not exactly zero"
    return torch.where(zero, torch.zeros_like(err), err / torch.where(zero, torch.ones_like(scale), scale)), int(zero.sum())
