"""Problems, bounds and checkers of the operator parity suite (tests/test_gpu_parity.py) that other suites and the fuzz scripts
use as well; the stated tolerances are in that file's docstring.  The two randomised bodies live here so that
tests/fuzz_extended.py and tools/probes/one_seed.py can run them over seeds the suite does not carry."""
import numpy as np
import torch

from oracle import ppnet_oracle as O
from support import BF16_DX_TOL, GRAD_TOL, gpu_device, grad_close


def problem(B, S, Cs, P, K, H, W, seed=0, x_dtype=torch.float32):
    g = torch.Generator().manual_seed(20220227 + seed)
    conv = O.bf16_representable(torch.sigmoid(torch.randn(B, S * Cs, H, W, generator=g)))
    bank = O.bf16_representable(torch.rand(P, Cs, 1, 1, generator=g))
    ident = O.default_class_identity(P, K, S)
    Wl = O.last_layer_init(ident) + 0.05 * torch.randn(K, P, generator=g)
    return conv, bank, Wl, ident, O.default_scale_ranges(P, S)


def bank_layout(P, K, S, Cs, ranges):
    from scaleprotoseg_amd.functional import BankLayout

    return BankLayout(P, K, S, Cs, tuple(ranges[s] for s in range(S)))


def assert_fwd(logits, dist, act, ref_logits, ref_dist, ref_act):
    if dist is not None:
        err = (dist.cpu() - ref_dist).abs()
        assert (err <= 1e-4 * (1 + ref_dist)).all(), f"distance err {err.max().item()}"
    if act is not None:
        err = (act.cpu() - ref_act).abs()
        assert (err <= 2e-4 * (1 + ref_act.abs())).all(), f"activation err {err.max().item()}"
    if logits is not None:
        rl = ref_logits.reshape(-1, ref_logits.shape[-1])
        d = (logits.cpu().reshape(rl.shape) - rl).abs()
        err = d.max().item()
        assert err <= 1e-4 * max(1.0, rl.abs().max().item()), f"logit err {err}"
        # ... and per element, relative with an absolute floor (a logit is a signed sum of P terms that passes through zero):
        # |err| <= 1.1e-4 (|l| + 0.2 max|l|).  What bounds it is the operand precision of the head product - activations and head
        # weights enter the MFMA as bf16 hi + lo pairs, 2^-17 of each TERM |a_p w_kp| (a <= 9.2) - so an element's error scales
        # with the sum of its terms' magnitudes, not with the element.  700 fuzzed configurations peak at 1.002e-4 of this
        # measure (seed 378 of test_random_gather_and_tail in tests/test_gpu_parity.py); 1e-4 with a 0.1 floor would take 24-bit
        # operands (a third bf16 plane of W and a: twice the head MFMAs) - DESIGN.md 4
        floor = 0.2 * max(1.0, rl.abs().max().item())
        assert (d <= 1.1e-4 * (rl.abs() + floor)).all(), f"per-element logit err {(d / (rl.abs() + floor)).max().item()}"


def dx_tolerance(x_dtype, ranges=None):
    """fp32 features: 1e-3.  bf16 features: dX is returned in bf16 - ONE output rounding, also for scales of more than 192
    prototypes (several panels: their shares are summed in an fp32 scratch, round 4; through the bf16 buffer it was one
    rounding per panel)."""
    return GRAD_TOL if x_dtype == torch.float32 else BF16_DX_TOL


PUSH_FUSED_SHAPES = [
    # B, S, Cs,  P,   K,  H,   W
    (2, 4, 64, 228, 19, 33, 65),      # the gin's bank, odd grid (ragged last tile, unaligned rows)
    (1, 1, 256, 190, 19, 64, 128),    # north-star bank, 64 full tiles
    (3, 2, 32, 44, 11, 9, 13),        # tiny: one partial tile per image
    (1, 4, 64, 1800, 150, 17, 19),    # ADE bank: several panels per scale
]


def gather_labels(B, H, W, K, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, K + 1, (B, H, W), generator=g)      # reference convention: 0 = void, 1..K
    t[t == K] = 0                                            # last class absent ...
    t[0, 0, 0] = K                                           # ... but for one pixel
    return t


def random_case(rng):
    S = int(rng.choice([1, 2, 3, 4]))
    Cs = int(rng.choice([16, 32, 48, 64, 80, 128]))
    K = int(rng.choice([2, 3, 5, 19, 21, 40, 64, 70]))
    per_scale = [int(rng.integers(1, 7)) * max(1, K // int(rng.choice([1, 2, 4]))) for _ in range(S)]
    per_scale = [min(p, 230) for p in per_scale]
    if rng.random() < 0.4:                       # unequal scales, as after the push's de-duplication
        per_scale = [max(1, p - int(rng.integers(0, 5))) for p in per_scale]
    B = int(rng.integers(1, 4))
    H, W = int(rng.integers(1, 24)), int(rng.integers(1, 40))
    if rng.random() < 0.3:
        W = 8 * int(rng.integers(1, 12))         # aligned rows: vector staging path
    if rng.random() < 0.2:                       # (drawn last: the other seeds keep their round-3 configurations)
        # H*W a multiple of 64 and scales wider than 64 channels: the LDS-DMA parameter kernel (bf16 features, K <= 32)
        H, W, Cs = 8 * int(rng.integers(1, 4)), 8 * int(rng.integers(1, 6)), int(rng.choice([80, 96, 128]))
    return B, S, Cs, per_scale, K, H, W


def close_fwd(got, ref, kind):
    got, ref = got.detach().float().cpu(), torch.as_tensor(ref)
    assert got.shape == ref.shape, f"{kind}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    err = (got - ref).abs()
    if kind == "distances":
        assert (err <= 1e-4 * (1 + ref)).all(), f"distance err {err.max().item()}"
    elif kind == "activations":
        assert (err <= 2e-4 * (1 + ref.abs())).all(), f"activation err {err.max().item()}"
    else:
        assert err.max().item() <= 1e-4 * max(1.0, ref.abs().max().item()), f"{kind} err {err.max().item()}"
        if kind == "logits":    # per element: 1e-4 relative with an absolute floor (a logit is a signed sum through zero)
            floor = 0.2 * max(1.0, ref.abs().max().item())
            assert (err <= 1e-4 * (ref.abs() + floor)).all(), f"per-element logit err {(err / (ref.abs() + floor)).max().item()}"


def check_random_configuration(seed, grad_close=grad_close):
    """Randomised shapes (scale counts, unequal per-scale banks, channel widths with 16-channel tails, 1/2/5-block
    heads, odd and aligned grids, partial tiles, both feature dtypes): forward outputs and all gradients against the
    oracle, with the stated tolerances."""
    from scaleprotoseg_amd.functional import BankLayout, proto_head_forward

    dev = gpu_device()
    rng = np.random.default_rng(1000 + seed)
    B, S, Cs, per_scale, K, H, W = random_case(rng)
    P = sum(per_scale)
    ranges, lo = {}, 0
    for s, n in enumerate(per_scale):
        ranges[s] = (lo, lo + n)
        lo += n
    g = torch.Generator().manual_seed(seed)
    conv = O.bf16_representable(torch.sigmoid(torch.randn(B, S * Cs, H, W, generator=g)))
    bank = O.bf16_representable(torch.rand(P, Cs, 1, 1, generator=g))
    Wl = torch.randn(K, P, generator=g) * 0.3
    x_dtype = torch.bfloat16 if seed % 2 else torch.float32
    g_logits = torch.randn(B, H, W, K, generator=g) * 1e-3
    g_dist = torch.randn(B, P, H, W, generator=g) * 1e-3
    g_act = torch.randn(B * H * W, P, generator=g) * 1e-3
    l_ref, d_ref, a_ref, dx_ref, dp_ref, dw_ref = O.fwd_bwd_reference(conv, bank, ranges, S, Wl, g_logits, g_dist, g_act)

    x = conv.to(dev, x_dtype).requires_grad_(True)
    pv = bank.to(dev).requires_grad_(True)
    w = Wl.to(dev).requires_grad_(True)
    lay = BankLayout(P, K, S, Cs, tuple(ranges[s] for s in range(S)))
    logits, dist, act = proto_head_forward(x, pv, w, lay, want_distances=True, want_activations=True)
    torch.cuda.synchronize()
    assert_fwd(logits, dist, act, l_ref, d_ref, a_ref)
    ((logits * g_logits.reshape(-1, K).to(dev)).sum() + (dist * g_dist.to(dev)).sum() + (act * g_act.to(dev)).sum()).backward()
    torch.cuda.synchronize()
    tag = f"B{B} S{S} Cs{Cs} P{per_scale} K{K} {H}x{W} {x_dtype}"
    grad_close(x.grad, dx_ref, "dX " + tag, tol=dx_tolerance(x_dtype, ranges))
    # G enters dX and dPrototypes as ONE fp16 plane scaled per tile by a power of two (11 significant bits per element)
    grad_close(pv.grad, dp_ref, "dPrototypes " + tag)
    # d_W = dLogits^T . a: the activations cross HBM as block-scaled int16 codes and enter the MFMA as an exact bf16 hi + lo
    # pair, dLogits as split bf16
    grad_close(w.grad, dw_ref, "dLastLayer " + tag)


def check_random_gather_and_tail(seed, grad_close=grad_close):
    """Randomised shapes for the two extended modes: class-gathered distances (even seeds) and the fused grouping
    tail (odd seeds), forward + all gradients against the oracle."""
    from scaleprotoseg_amd.functional import BankLayout, ClassGather, class_gather_table, proto_head_forward

    dev = gpu_device()
    rng = np.random.default_rng(5000 + seed)
    S = int(rng.choice([1, 2, 4]))
    Cs = int(rng.choice([16, 32, 64]))
    K = int(rng.choice([2, 3, 5, 7, 19]))
    r = int(rng.integers(1, 4))
    P = K * S * r
    B, H, W = int(rng.integers(1, 3)), int(rng.integers(2, 14)), int(rng.integers(2, 30))
    x_dtype = torch.bfloat16 if (seed // 2) % 2 else torch.float32
    conv, bank, Wl, ident, ranges = problem(B, S, Cs, P, K, H, W, seed=100 + seed)
    lay_k = BankLayout(P, K, S, Cs, tuple(ranges[s] for s in range(S)))
    g = torch.Generator().manual_seed(seed)
    g_logits = torch.randn(B, H, W, K, generator=g) * 1e-3
    x = conv.to(dev, x_dtype).requires_grad_(True)
    pv = bank.to(dev).requires_grad_(True)
    c0 = conv.clone().requires_grad_(True)
    p0 = bank.clone().requires_grad_(True)
    # tiny banks (P as small as 4): dX is a sum of a handful of signed terms G_p (x - p), each carrying G's bf16
    # rounding (2^-8); with cancellation between them the error relative to max|dX| can pass the 4e-3 of the
    # realistic shapes, so these toy cases get 6e-3
    dx_tol = dx_tolerance(x_dtype, ranges)
    if seed % 2 == 0:
        target = gather_labels(B, H, W, K, seed=seed)
        lab0 = target.reshape(B, -1) - 1
        keys, J, table = class_gather_table(lay_k, ident, dev)
        gather = ClassGather(labels=lab0.to(dev, torch.int32).contiguous(), keys=keys, width=J, table=table)
        g_cls = torch.randn(B, H * W, J, generator=g) * 1e-3
        w0 = Wl.clone().requires_grad_(True)
        l_ref, d_ref, _ = O.forward_from_conv_features(c0, p0, ranges, S, w0)
        cd_ref = O.gather_class_distances(d_ref, lab0, ident)
        ((l_ref * g_logits).sum() + (cd_ref * g_cls).sum()).backward()
        w = Wl.to(dev).requires_grad_(True)
        logits, cd, _ = proto_head_forward(x, pv, w, lay_k, class_gather=gather)
        got = cd.detach().cpu().permute(0, 2, 1)
        cd_err = (got - cd_ref.detach()).abs()
        assert (cd_err <= 1e-4 * (1 + cd_ref.detach())).all(), f"class distance err {cd_err.max().item()}"
        assert_fwd(logits, None, None, l_ref.detach(), None, None)
        ((logits * g_logits.reshape(-1, K).to(dev)).sum() + (cd * g_cls.permute(0, 2, 1).contiguous().to(dev)).sum()).backward()
        torch.cuda.synchronize()
        grad_close(w.grad, w0.grad, "dLastLayer")
    else:
        G = int(rng.integers(2, 4))
        idx = [i for i in O.class_prototype_index(ident) if len(i) > 0]
        gw = [O.projection_simplex_sort(torch.rand(G, len(i), generator=g)) for i in idx]
        U = G * len(idx)
        wg = torch.randn(K, U, generator=g) * 0.5
        gw0 = [t.clone().requires_grad_(True) for t in gw]
        wg0 = wg.clone().requires_grad_(True)
        d_ref = O.scale_l2_convolution(c0, p0, ranges, S)
        act_ref = O.distance_2_similarity(d_ref).permute(0, 2, 3, 1).reshape(-1, P)
        units = torch.cat(O.compute_group(act_ref, ident, gw0), dim=-1)
        l_ref = torch.nn.functional.linear(units, wg0)
        (l_ref * g_logits.reshape(-1, K)).sum().backward()
        wd = torch.zeros(U, P)
        for k, i in enumerate(idx):
            wd[k * G:(k + 1) * G, i] = gw[k]
        wdd = wd.to(dev).requires_grad_(True)
        wgd = wg.to(dev).requires_grad_(True)
        logits, _, _, gact = proto_head_forward(x, pv, wdd, BankLayout(P, U, S, Cs, tuple(ranges[s] for s in range(S))),
                                                want_distances=False, group_tail=wgd)
        rl = l_ref.detach()
        err = (logits.detach().cpu() - rl).abs().max().item()
        assert err <= 1e-4 * max(1.0, rl.abs().max().item()), f"group logits err {err}"
        (logits * g_logits.reshape(-1, K).to(dev)).sum().backward()
        torch.cuda.synchronize()
        grad_close(wgd.grad, wg0.grad, "dLastLayerGroup")
    grad_close(x.grad, c0.grad, "dX", tol=dx_tol)
    grad_close(pv.grad, p0.grad, "dPrototypes")
