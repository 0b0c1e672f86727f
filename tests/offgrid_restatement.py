"""Float64 restatement of what the distance kernels compute for inputs OFF the bf16 grid ("operand sites"),
built on oracle/ppnet_oracle.py; CPU tensors only.

Write x~ = bf16_rne(x), p~ = bf16_rne(p).
  forward    every output is the oracle's at (x~, p~): X is rounded once in the staging (SpxXStager::write), |x|^2 comes from the
             staged values, the bank and |p|^2 from bf16(p) (spx_pack.hip).
  backward   G = dLoss/dDistances is the oracle's at (x~, p~), relu mask included; the outer linear factors take one operand per site
                 dX = 2 (sum_p G) x_a - 2 G^T p_b           a: the x the caller passed (fp32 or bf16), b: p~ (fp16(-2 p~), exact)
                 dP = -2 G^T x_c + 2 p_d sum(G)             c: fp16_rtz(x~) (= x~ inside fp16's normal range), d: the fp32 p
             head / grouping gradients do not meet these sites: float64 autograd at (x~, p~).
``site_operands`` is the one place that names them; ``sites=`` lets a test (or a reviewer) swap one and watch
tests/test_offgrid_cpu.py notice.  tests/test_offgrid_cpu.py pins this file; tests/test_gpu_offgrid.py holds the kernels to it."""
from types import SimpleNamespace

import torch

from oracle import ppnet_oracle as O

GRAD_TOL = 1e-3            # tests/support.py
DIST_TOL = 1e-4            # |d - d_ref| <= DIST_TOL (1 + d_ref), tests/parity_cases.py::assert_fwd

# id -> (B, S, Cs, P, K, H, W)
CASES = {
    "F1": (1, 4, 64, 228, 19, 9, 13),       # odd grid, scalar-load staging, 4 scales
    "F2": (1, 1, 256, 190, 19, 16, 64),     # aligned rows, vector staging
    "F3": (1, 2, 16, 16, 3, 5, 7),          # Cs = 16, unassigned prototypes
    "F4": (1, 4, 64, 1800, 150, 5, 8),      # several panels per scale, 5 class blocks
    "F5": (2, 1, 96, 100, 7, 8, 24),        # bf16 features: the LDS-DMA parameter kernel
    "F6": (1, 4, 64, 228, 57, 9, 13),       # 2 class blocks: int16 activation blobs
}
FP32_CASES = ("F1", "F2", "F3", "F4", "F6")      # fp32 features, off the grid together with the bank
BF16_CASES = ("F1", "F4", "F5")                  # bf16 features, off-grid bank (autocast)

# planted value -> its bf16 round-to-nearest-even (ulp of bf16 in [0.5, 1) is 2^-8, of fp32 2^-24)
_U = 2.0 ** -24
PLANTED = (
    (0.5 + 2.0 ** -9, 0.5),                                   # tie, lower neighbour even: down
    (0.5 + 2.0 ** -9 + _U, 0.5 + 2.0 ** -8),
    (0.5 + 2.0 ** -9 - _U, 0.5),
    (0.5 + 2.0 ** -8 + 2.0 ** -9, 0.5 + 2.0 ** -7),           # tie, lower neighbour odd: up
    (0.5 + 2.0 ** -8 + 2.0 ** -9 + _U, 0.5 + 2.0 ** -7),
    (0.5 + 2.0 ** -8 + 2.0 ** -9 - _U, 0.5 + 2.0 ** -8),
    (1.0 - 2.0 ** -10, 1.0),                                  # carry into the next binade
)


# ---------------------------------------------------------------------------------------------------------------------
# number formats, on the bits of an fp32 CPU tensor
# ---------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.detach().to(torch.float32).contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def _from_bits(u):
    u = u & 0xFFFFFFFF
    u = torch.where(u >= 2 ** 31, u - 2 ** 32, u)
    return u.to(torch.int32).view(torch.float32)


def bf16_rne(t):
    """fp32 -> nearest bf16-representable fp32, ties to even (finite inputs): add 0x7fff + the kept lsb, clear 16 bits."""
    u = _bits(t)
    return _from_bits((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).reshape(t.shape)


def bf16_trunc(t):
    """fp32 -> bf16 by dropping the low 16 bits (what the kernels must NOT do; for the sharpness checks)."""
    return _from_bits(_bits(t) & 0xFFFF0000).reshape(t.shape)


def fp16_rtz(t):
    """fp32 -> fp16 round-toward-zero (v_cvt_pkrtz_f16_f32), returned as fp32: the nearest-even cast stepped back by one
    code where it landed above |t|.  Beyond 65504 that gives 65504, not infinity."""
    t = t.detach().to(torch.float32)
    h = t.to(torch.float16)
    over = h.to(torch.float32).abs() > t.abs()              # (inf > |t| too)
    code = h.view(torch.int16).to(torch.int32)
    code = torch.where(over, code - 1, code)                 # sign-magnitude: one code towards zero
    return code.to(torch.int16).view(torch.float16).to(torch.float32)


def site_operands(conv, bank):
    """The operand each outer linear factor of the backward reads (module docstring), fp32 tensors."""
    xt = bf16_rne(conv)
    return dict(a=conv.detach().float(), b=bf16_rne(bank), c=fp16_rtz(xt), d=bank.detach().float())


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def planted_positions(n, count, stride):
    return [(3 + stride * i) % n for i in range(count)]


def build(case, x_dtype=torch.float32, seed=0, signed=False, plant=None):
    """Features sigmoid(randn) and bank rand, both left unrounded (``signed``: 3 randn and randn); head and upstream gradients
    as in tests/test_gpu_parity.py.  fp32 features: a few feature and bank elements are overwritten with PLANTED; bf16 features:
    conv holds the bf16 values (as fp32) the kernel is handed."""
    B, S, Cs, P, K, H, W = CASES[case] if isinstance(case, str) else case
    g = torch.Generator().manual_seed(20261018 + seed)
    r = torch.randn(B, S * Cs, H, W, generator=g)
    conv = 3.0 * r if signed else torch.sigmoid(r)
    bank = (torch.randn(P, Cs, 1, 1, generator=g) if signed else torch.rand(P, Cs, 1, 1, generator=g))
    ident = O.default_class_identity(P, K, S)
    Wl = O.last_layer_init(ident) + 0.05 * torch.randn(K, P, generator=g)
    plant = (x_dtype == torch.float32 and not signed) if plant is None else plant
    planted = None
    if plant:
        vals = torch.tensor([v for v, _ in PLANTED], dtype=torch.float64).to(torch.float32)
        assert torch.equal(vals.double(), torch.tensor([v for v, _ in PLANTED], dtype=torch.float64))     # all exact in fp32
        xi = planted_positions(conv.numel(), 2 * len(PLANTED), 97)
        pi = planted_positions(bank.numel(), 2 * len(PLANTED), 61)
        conv.view(-1)[xi] = vals.repeat(2)
        bank.view(-1)[pi] = vals.repeat(2)
        planted = SimpleNamespace(x_index=xi, p_index=pi, values=vals.repeat(2),
                                  rounded=torch.tensor([w for _, w in PLANTED], dtype=torch.float32).repeat(2))
    if x_dtype == torch.bfloat16:
        conv = bf16_rne(conv)
    g_logits = torch.randn(B, H, W, K, generator=g) * 1e-3
    g_dist = torch.randn(B, P, H, W, generator=g) * 1e-3
    g_act = torch.randn(B * H * W, P, generator=g) * 1e-3
    return SimpleNamespace(shape=(B, S, Cs, P, K, H, W), conv=conv, bank=bank, Wl=Wl, ident=ident,
                           ranges=O.default_scale_ranges(P, S), g_logits=g_logits, g_dist=g_dist, g_act=g_act,
                           x_dtype=x_dtype, planted=planted)


def on_grid(pb):
    """The same problem snapped to the grid (every site operand then coincides)."""
    q = SimpleNamespace(**vars(pb))
    q.conv, q.bank = bf16_rne(pb.conv), bf16_rne(pb.bank)
    return q


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
def forward_reference(pb, rounding=bf16_rne):
    """fp32 oracle at (x~, p~): (logits, distances, activations), as the on-grid tests call it."""
    return O.forward_from_conv_features(rounding(pb.conv), rounding(pb.bank), pb.ranges, pb.shape[1], pb.Wl)


def _loss(pb, d, w):
    P = d.shape[1]
    act = O.distance_2_similarity(d.permute(0, 2, 3, 1).contiguous().reshape(-1, P))
    logits = torch.nn.functional.linear(act, w)
    return (logits * pb.g_logits.double().reshape(-1, w.shape[0])).sum() + (d * pb.g_dist.double()).sum() \
        + (act * pb.g_act.double()).sum()


def autograd_f64(pb, conv, bank):
    """(dX, dP, dW, distances) of the test loss by float64 autograd at (conv, bank)."""
    S = pb.shape[1]
    x = conv.detach().double().requires_grad_(True)
    p = bank.detach().double().requires_grad_(True)
    w = pb.Wl.double().requires_grad_(True)
    d = O.scale_l2_convolution(x, p, pb.ranges, S)
    _loss(pb, d, w).backward()
    return x.grad, p.grad, w.grad, d.detach()


def straight_through(pb, rounding=bf16_rne):
    """Float64 autograd at (x~, p~) with the rounding treated as the identity."""
    return autograd_f64(pb, rounding(pb.conv), rounding(pb.bank))


def restated_gradients(pb, sites=None, rounding=bf16_rne, check_grid=True, loss_fn=None):
    """(dX, dP, dW) float64: G from the oracle at (x~, p~), outer factors from the four site operands.
    Asserts that every site operand stays within 2^-8 |v| of the input it stands for and, when the inputs are on the grid,
    that the result equals float64 autograd to 1e-12 relative.
    ``loss_fn(d)``: another scalar loss of the float64 distance map [B, P, H, W] (class gather, grouping tail); its parameters
    are the caller's own leaves, dW is then None."""
    B, S, Cs, P, K, H, W = pb.shape
    xt, pt = rounding(pb.conv).double(), rounding(pb.bank).double()
    op = site_operands(pb.conv, pb.bank) if sites is None else sites
    for k, v in (("a", pb.conv), ("c", pb.conv), ("b", pb.bank), ("d", pb.bank)):
        v = v.detach().double()
        assert ((op[k].double() - v).abs() <= 2.0 ** -8 * v.abs()).all(), f"site {k} drifted from its input"
    d = O.scale_l2_convolution(xt, pt, pb.ranges, S).detach().requires_grad_(True)
    w = pb.Wl.double().requires_grad_(True)
    (_loss(pb, d, w) if loss_fn is None else loss_fn(d)).backward()
    G = d.grad * (d.detach() > 0)                                              # relu mask, as autograd's (0 at d = 0)
    xa, xc = (op[k].double().view(B, S, Cs, H * W) for k in ("a", "c"))
    pb_, pd = (op[k].double().view(P, Cs) for k in ("b", "d"))
    dX = torch.zeros(B, S, Cs, H * W, dtype=torch.float64)
    dP = torch.zeros(P, Cs, dtype=torch.float64)
    for s in range(S):
        lo, hi = pb.ranges[s]
        Gs = G[:, lo:hi].reshape(B, hi - lo, H * W)
        dX[:, s] = 2.0 * Gs.sum(1, keepdim=True) * xa[:, s] - 2.0 * torch.einsum("bpm,pc->bcm", Gs, pb_[lo:hi])
        dP[lo:hi] = -2.0 * torch.einsum("bpm,bcm->pc", Gs, xc[:, s]) + 2.0 * pd[lo:hi] * Gs.sum((0, 2))[:, None]
    dX, dP = dX.view(B, S * Cs, H, W), dP.view(P, Cs, 1, 1)
    if loss_fn is not None:
        return dX, dP, None
    if check_grid and torch.equal(xt.float(), pb.conv.float()) and torch.equal(pt.float(), pb.bank.float()):
        ax, ap, aw, _ = autograd_f64(pb, pb.conv, pb.bank)
        for got, ref in ((dX, ax), (dP, ap), (w.grad, aw)):
            assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
    return dX, dP, w.grad


def max_normalised(got, ref):
    """grad_close's measure (tests/support.py): max|got - ref| / max|ref|."""
    return ((got.double() - ref.double()).abs().max() / (ref.double().abs().max() + 1e-30)).item()


def distance_ratio(d, d_ref):
    """Worst |d - d_ref| / (DIST_TOL (1 + d_ref)) over the map."""
    return ((d.double() - d_ref.double()).abs() / (DIST_TOL * (1 + d_ref.double()))).max().item()
