"""Cases, the float64 reference, an fp32 restatement and the bounds of the pixel-wise cross entropy, shared by
tests/test_ce_inputs_cpu.py (are the inputs and the bounds sound?) and tests/test_gpu_ce_float64.py (do the four device
implementations keep them: csrc/spx_ce.hip, the epilogue of csrc/spx_fwd_impl.h, the prologue of csrc/spx_bwd_impl.h, the
grouping tail?).  A plain module, no fixtures; everything is seeded.

The reference is float64 cross entropy OF THE LOGITS GIVEN (on the GPU: the fp32 logits the kernel returned), so the head
product's error is not in it.  With l the logits, lse64 and p64 = exp(l - lse64) in float64:

  pred      exactly argmax of l, lowest index on ties, on every pixel (ignored ones too)
  lse       |lse - lse64| <= 8 eps32 max(1, |lse64|)
  count     exact
  loss      |loss - loss64| <= 4e-6 max(1, |loss64|); loss64 >= 0.05 asserted wherever a case has a loss at all
  d_logits  |d - d64| <= |coef| (4 eps32 (E p64 + onehot) + 2^-126) per element, E = 1 + sqrt(K) / 2 + |lse64| / 2 + 1.25 |l - lse64|;
            rows of ignored pixels exactly 0
  d W_g     max|dW - dW64| <= 1e-5 max|dW64| (the grouping tail's d_logits^T . gact)

The d_logits bound was first proposed as |coef| (4 eps32 (1 + |l| + |lse64|) p64 + 2^-126).  ``restatement`` - plain fp32, no
kernel - comes to 0.37 of that, and past it at the label's class, so both terms are re-derived from the roundings (figures in
profiles/ce_float64_summary.md):

  E        the relative error of p = exp2(fl(fl(l - lse) log2e)) is the absolute error of its natural-log argument: eps32 / 2 |lse|
           for lse STORED in fp32, eps32 / 2 |l - lse| for the subtraction, 0.67 eps32 |l - lse| for the product with the fp32
           constant (its rounding, and 0.17 eps32 of the constant's own), and what lse carries from its computation: the fp32 sum
           of K exponentials (a random walk of K roundings of eps32 / 2: sqrt(K) / 2 eps32; (K - 1) / 2 eps32 at worst), log2 and
           one addition (the 1).  The proposal's |l| + |lse| understates |l - lse| where the two differ in sign.
  onehot   at the label's class the kernels form fl(coef * fl(p - 1)).  fl(p - 1) is off by up to eps32 / 4 (a result in
           [-1, -1/2]) however small p is - p below eps32 / 4 is dropped altogether - and the product rounds by eps32 / 2 more:
           0.75 eps32 |coef|, against a term that vanishes with p.  Four times that, rounded up: 4 eps32 |coef|."""
import functools
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

EPS32 = 2.0 ** -23
LSE_ULPS = 8.0
LOSS_TOL = 4e-6
MIN_LOSS = 0.05
DL_ULPS = 4.0
DL_FLOOR = 2.0 ** -126
DW_TOL = 1e-5
QUARTER = 0.25           # the fp32 restatement stays within this share of every bound (tests/test_ce_inputs_cpu.py)
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
LOG2E = np.float32(1.44269504089)       # the kernels' constants (csrc/spx_common.h: ce_exp, ce_log)
LN2 = np.float32(0.69314718056)


@dataclass
class CeCase:
    name: str
    logits: torch.Tensor                 # [M, K] fp32
    labels: torch.Tensor                 # [M] int32: class 0..K-1, anything else is ignored
    no_loss: Optional[str] = None        # "zero": one class, the loss is exactly 0; "nan": no valid pixel, the loss is 0 / 0

    @property
    def M(self):
        return int(self.logits.shape[0])

    @property
    def K(self):
        return int(self.logits.shape[1])


def mixed_labels(M, K, gen):
    """[M] int32: valid classes; -1, -2, K, K + 7 and the int32 extremes scattered in; and, from 256 pixels up, two whole waves
    (pixels 64 .. 191) ignored with every one of those values."""
    lab = torch.randint(0, K, (M,), generator=gen, dtype=torch.int64)
    bad = torch.tensor([-1, -2, K, K + 7, INT32_MIN, INT32_MAX])
    hit = torch.rand(M, generator=gen) < 0.15
    lab[hit] = bad[torch.randint(0, 6, (int(hit.sum()),), generator=gen)]
    for i, v in enumerate(bad.tolist()):                       # every kind is present whatever the draw
        if M > 6 + i:
            lab[5 + i] = v
    lab[0] = K - 1
    if M >= 256:
        lab[64:192] = bad[torch.arange(128) % 6]
    return lab.to(torch.int32)


def _drawn(name, M, K, seed, scale=1.0, offset=0.0, labels=None, **kw):
    gen = torch.Generator().manual_seed(seed)
    logits = (torch.randn(M, K, generator=gen) * scale + offset).float()
    lab = mixed_labels(M, K, gen) if labels is None else labels
    return CeCase(name, logits, lab, **kw)


def _ties(name, M, K, seed):
    """Every third row has all classes equal, every other third an exact two-way tie at the top (the pair differs by row: one
    below class 8, one at or above it, so both orders of lane half and register meet in the fused layouts)."""
    c = _drawn(name, M, K, seed, scale=4.0)
    gen = torch.Generator().manual_seed(seed + 1)
    lg = c.logits
    rows = torch.arange(M)
    flat = rows % 3 == 0
    lg[flat] = torch.randn(int(flat.sum()), 1, generator=gen) * 4.0
    tie = rows % 3 == 1
    lo = torch.randint(0, min(8, K - 1), (M,), generator=gen)
    hi = torch.minimum(lo + 1 + torch.randint(0, K, (M,), generator=gen), torch.full((M,), K - 1))
    top = lg.max(dim=1).values + 1.5
    lg[rows[tie], lo[tie]] = top[tie]
    lg[rows[tie], hi[tie]] = top[tie]
    assert bool((lo < hi).all())
    return c


STANDALONE_SHAPES = ((37, 5), (833, 19), (300, 171), (130, 1), (33027, 19))
# (the K = 33 and K = 150 cases: the class counts of the fused epilogue's three- and five-block instances, for the CPU checks of
# the restatement and of the wrong variants; the stand-alone kernels run them too)
CASE_NAMES = ("m37_k5_scale1", "m833_k19_scale4", "m300_k171_scale30", "m130_k1", "m33027_k19", "m300_k33_scale4",
              "m300_k150_scale1", "offset_plus200", "span_3e4", "ties", "all_ignored", "last_pixel_only")


@functools.lru_cache(maxsize=None)
def case(name) -> CeCase:
    """The case on the CPU; built once, never modified by a test."""
    M, K = 833, 19                                       # 3 * 256 + 65: one full wave, a one-pixel wave, two empty waves at the end
    if name == "m37_k5_scale1":
        return _drawn(name, 37, 5, 375, scale=1.0)
    if name == "m833_k19_scale4":
        return _drawn(name, M, K, 83319, scale=4.0)
    if name == "m300_k171_scale30":
        return _drawn(name, 300, 171, 300171, scale=30.0)
    if name == "m130_k1":
        return _drawn(name, 130, 1, 1301, scale=4.0, no_loss="zero")
    if name == "m33027_k19":                             # 520 partial pairs: the finish kernel's strided loop
        return _drawn(name, 33027, 19, 33027, scale=4.0)
    if name == "m300_k33_scale4":
        return _drawn(name, 300, 33, 30033, scale=4.0)
    if name == "m300_k150_scale1":
        return _drawn(name, 300, 150, 300150, scale=1.0)
    if name == "offset_plus200":
        return _drawn(name, M, K, 200, scale=4.0, offset=200.0)
    if name == "span_3e4":
        return _drawn(name, M, K, 30000, scale=3e4)
    if name == "ties":
        return _ties(name, M, K, 7135)
    if name == "all_ignored":
        bad = torch.tensor([-1, -2, K, K + 7, INT32_MIN, INT32_MAX])
        return _drawn(name, M, K, 11, scale=4.0, labels=bad[torch.arange(M) % 6].to(torch.int32), no_loss="nan")
    if name == "last_pixel_only":
        lab = torch.full((M,), -1, dtype=torch.int32)
        lab[-1] = 7
        return _drawn(name, M, K, 12, scale=4.0, labels=lab)
    raise KeyError(name)


# ---- float64 reference
def reference(logits, labels, coef=None):
    """float64 cross entropy of ``logits`` [M, K] (any float type, any device) for int labels [M]: dict with lse, p [M, K], pred
    (lowest index on ties), valid [M], count (int), loss_sum, loss (nan without a valid pixel), and d [M, K] = coef * (p - onehot)
    on the valid rows, 0 elsewhere.  ``coef``: the factor the kernel used (default 1 / count in float64)."""
    l = logits.detach().double()
    M, K = l.shape
    lab = labels.reshape(-1).long().to(l.device)
    valid = (lab >= 0) & (lab < K)
    m = l.max(dim=1, keepdim=True).values
    lse = (m + torch.log(torch.exp(l - m).sum(dim=1, keepdim=True))).squeeze(1)
    p = torch.exp(l - lse.unsqueeze(1))
    ks = torch.arange(K, device=l.device)
    pred = torch.where(l == m, ks, torch.full_like(ks, K)).min(dim=1).values
    onehot = (ks.unsqueeze(0) == lab.unsqueeze(1)) & valid.unsqueeze(1)
    count = int(valid.sum())
    picked = l.gather(1, lab.clamp(0, K - 1).unsqueeze(1)).squeeze(1)
    loss_sum = float(((lse - picked) * valid).sum())
    loss = loss_sum / count if count else float("nan")
    c = (1.0 / count if count else 0.0) if coef is None else float(coef)
    d = c * (p - onehot.double()) * valid.unsqueeze(1)
    return {"lse": lse, "p": p, "pred": pred, "valid": valid, "onehot": onehot, "count": count, "loss_sum": loss_sum, "loss": loss,
            "d": d, "coef": c, "logits": l}


# ---- the kernels' formula in NumPy fp32
def class_dropped(K, variant):
    """[K] bool: the classes a wrong variant leaves out of the exp sum."""
    k = np.arange(K)
    if variant == "drop_block":
        return (k >= 32) & (k < 64)                      # one class block of the epilogue's accumulators
    if variant == "drop_half":
        return (k & 4) != 0                              # the rows (acc_row bit 2) the other lane half holds
    return np.zeros(K, dtype=bool)


VARIANTS = ("no_max", "drop_block", "drop_half", "mean_all", "tie_high", "onehot_plus1")


def restatement(logits, labels, variant=None, flush=False):
    """The kernels' arithmetic restated: per-pixel operations in fp32 (running maximum with the lowest index on ties,
    exp2((l - m) log2e), a sequential sum over the classes, m + log2(s) ln2, coef (exp2((l - lse) log2e) - onehot)), the sums
    over pixels in float64.  NumPy's exp2 / log2 are correctly rounded where v_exp_f32 / v_log_f32 are good to about an ulp: the
    factor of four between this and the bounds is their allowance.  ``variant``: one of VARIANTS, a deliberately wrong kernel.
    ``flush``: exponentials below 2^-126 become 0, as v_exp_f32 returns them (NumPy keeps the denormals) - the one error the
    2^-126 term of the d_logits bound is there for; it is strictly below that term, which is a limit and not an allowance."""
    l = logits.detach().cpu().numpy().astype(np.float32)
    lab = labels.reshape(-1).cpu().numpy().astype(np.int64)
    M, K = l.shape
    valid = (lab >= 0) & (lab < K)
    m = np.full(M, -3.0e38, dtype=np.float32)
    best = np.full(M, 0x7FFFFFFF, dtype=np.int64)
    for k in range(K):
        v = l[:, k]
        take = (v >= m) if variant == "tie_high" else (v > m)
        m = np.where(take, v, m)
        best = np.where(take, k, best)
    if variant == "no_max":
        m = np.zeros(M, dtype=np.float32)
    drop = class_dropped(K, variant)
    s = np.zeros(M, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for k in range(K):
            if not drop[k]:
                s = s + np.exp2((l[:, k] - m) * LOG2E)
        lse = m + np.log2(s) * LN2
        assert lse.dtype == np.float32 and s.dtype == np.float32
        picked = l[np.arange(M), np.clip(lab, 0, K - 1)]
        per_px = np.where(valid, lse - picked, np.float32(0.0)).astype(np.float32)
        count = int(valid.sum())
        loss_sum = np.float32(per_px.astype(np.float64).sum())
        denom = np.float32(M if variant == "mean_all" else count)
        loss = float(loss_sum / denom) if denom else float("nan")
        coef = np.float32(1.0) / np.float32(count) if count else np.float32(0.0)
        hot = lab + 1 if variant == "onehot_plus1" else lab
        onehot = ((np.arange(K)[None, :] == hot[:, None]) & valid[:, None]).astype(np.float32)
        p = np.exp2((l - lse[:, None]) * LOG2E)
        if flush:
            p = np.where(p < np.float32(DL_FLOOR), np.float32(0.0), p).astype(np.float32)
        d = np.where(valid[:, None], coef * (p - onehot), np.float32(0.0)).astype(np.float32)
    return {"lse": torch.from_numpy(lse), "pred": torch.from_numpy(best), "count": count, "loss": loss,
            "d": torch.from_numpy(d), "coef": float(coef)}


# ---- error / bound
def lse_ratio(lse, ref):
    """Worst |lse - lse64| / (8 eps32 max(1, |lse64|)); inf for a value that is not finite (an unwritten NaN among them)."""
    got = lse.detach().double().reshape(-1).to(ref["lse"].device)
    r = (got - ref["lse"]).abs() / (LSE_ULPS * EPS32 * ref["lse"].abs().clamp_min(1.0))
    return float(torch.nan_to_num(r, nan=float("inf")).max())


def loss_ratio(loss, ref):
    r = abs(float(loss) - ref["loss"]) / (LOSS_TOL * max(1.0, abs(ref["loss"])))
    return r if r == r else float("inf")


def dlogits_bound(ref):
    c = abs(ref["coef"])
    lse = ref["lse"].unsqueeze(1)
    mag = 1.0 + 0.5 * ref["logits"].shape[1] ** 0.5 + 0.5 * lse.abs() + 1.25 * (ref["logits"] - lse).abs()
    return c * (DL_ULPS * EPS32 * (mag * ref["p"] + ref["onehot"].double()) + DL_FLOOR)


def dlogits_ratio(d, ref):
    """(worst |d - d64| / bound over the valid rows, largest |d| on the ignored rows: must be 0).  ``ref`` was made with the
    coef the kernel used."""
    got = d.detach().double().reshape(ref["d"].shape).to(ref["d"].device)
    r = torch.nan_to_num((got - ref["d"]).abs() / dlogits_bound(ref), nan=float("inf"))
    v = ref["valid"]
    worst = float(r[v].max()) if bool(v.any()) else 0.0
    ignored = float(torch.nan_to_num(got[~v].abs(), nan=float("inf")).max()) if bool((~v).any()) else 0.0
    return worst, ignored


def pred_mismatches(pred, ref):
    return int((pred.reshape(-1).long().to(ref["pred"].device) != ref["pred"]).sum())


def dw_ratio(dw, d64, gact):
    """max|dW - d64^T . gact| / (1e-5 max|d64^T . gact|) for the grouping tail's d W_g [K2, U]."""
    ref = d64.t() @ gact.detach().double().to(d64.device)
    r = float((dw.detach().double().to(ref.device) - ref).abs().max()) / (DW_TOL * float(ref.abs().max()))
    return r if r == r else float("inf")


# ---- crafted inputs of the finish and label kernels
FINISH_SIZES = (1, 4, 255, 256, 257, 511, 512, 513, 1025, 4100)


def finish_pairs(n):
    """[n, 2] fp32 (sum, count) pairs: counts 0 .. 6 by a fixed pattern (exact in fp32 in any order, and no two neighbours alike,
    so a dropped or doubled pair shows in the total), sums random positive.  Returns (pairs, count, float64 sum)."""
    gen = torch.Generator().manual_seed(1000 + n)
    cnt = ((torch.arange(n) * 5 + 3) % 7).float()
    if n == 1:
        cnt[0] = 3.0
    s = torch.rand(n, generator=gen) * 40.0 + 0.5
    pairs = torch.stack([s, cnt], dim=1).contiguous()
    return pairs, int(cnt.sum()), float(s.double().sum())


def finish_restatement(pairs):
    """spx_ce_finish_kernel's order in NumPy fp32: thread t of 256 takes pairs t, t + 512, ... and t + 256, t + 768, ... in two
    accumulators, a wave's 64 values meet in an xor butterfly (32 .. 1), the four waves are added in order.  (sum, count, loss)."""
    a = pairs.detach().cpu().numpy().astype(np.float32)
    n = a.shape[0]
    acc = np.zeros((2, 256, 2), dtype=np.float32)
    for t in range(256):
        i = t
        while i + 256 < n:
            acc[0, t] += a[i]
            acc[1, t] += a[i + 256]
            i += 512
        if i < n:
            acc[0, t] += a[i]
    v = acc[0] + acc[1]
    lanes = np.arange(256)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[lanes ^ off]
    tot = ((v[0] + v[64]) + v[128]) + v[192]
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(tot[0]), float(tot[1]), float(tot[0] / tot[1])


SHIFT_SIZES = (1, 255, 256, 257, 1000)


def shift_values(n, K, dtype):
    """[n] labels (0 = void, c + 1 = class c) with the values at which a 32-bit shortcut goes wrong, cycled."""
    if dtype == torch.int64:
        vals = [0, 1, K, K + 1, 2 ** 31, 2 ** 31 + 1, -2 ** 31, 2 ** 32 + 3, 2 ** 40 + 3, -2 ** 40, INT32_MAX, INT32_MIN + 1, -1, 2]
    else:
        vals = [0, 1, K, K + 1, INT32_MAX, INT32_MIN, INT32_MIN + 1, -1, 2, 5]
    v = torch.tensor(vals, dtype=dtype)
    return v[(torch.arange(n) + (n % 3)) % len(vals)].contiguous()


def shift_expected(v):
    """(exact [n] bool, want [n] int64): where v - 1 lies in +-(2^31 - 1) the result is v - 1 (``exact``); elsewhere it only has
    to be negative (no class)."""
    w = v.long() - 1
    exact = (w >= -INT32_MAX) & (w <= INT32_MAX)
    return exact, w
