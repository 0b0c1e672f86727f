"""Float64 restatement of the cross-scale aggregation (segmentation/model/scale_head.py, model_multiscale.py:299-317): the
weighted sum of ``WeightedAgg``, its three combines, and the chain of ``_scale_l2_convolution`` under a scale head, built on
oracle/ppnet_oracle.py; CPU tensors only, nothing touches a device on import.

    a   = similarity(dist[scale i + 1])            s = sum_p proto_{i+1}[p, c] a[b, p, h, w]
    x'  = (x_i + s) / 2  |  sqrt(x_i s)  |  sigmoid(Linear(cat(x_i, s)))           dist[scale i] = l2(x', proto_i)

``chain(..., rounding=bf16_rne)`` rounds every distance input (x' and the bank rows) the way the distance kernels do
(tests/offgrid_restatement.py); ``x_primes=`` substitutes given aggregated features (the device's) for the chain's own, which is
how tests/test_gpu_scale_head.py holds the kernels link by link.  ``chain_gradients`` composes the chain's gradient from the
distance link's site formula (offgrid_restatement.restated_gradients) and float64 autograd of the aggregation link."""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import offgrid_restatement as R
from oracle import ppnet_oracle as O

EPS = 1e-4
HEADS = ("sum", "mult", "concat")
PHASES = ("proto", "group")


# ---------------------------------------------------------------------------------------------------------------------
# the aggregation link
# ---------------------------------------------------------------------------------------------------------------------
def similarity(d, fn="log", eps=EPS):
    return O.distance_2_similarity(d, eps, fn) if isinstance(fn, str) else fn(d)


def weighted_sum(activations, prototypes):
    """WeightedAgg's sum over the prototypes: activations [B, Pn, H, W], prototypes [Pn, Cs(, 1, 1)] -> [B, Cs, H, W]."""
    return torch.einsum("bphw,pc->bchw", activations, prototypes.reshape(prototypes.shape[0], -1))


def combine(head, x, s, linear=None):
    """``head``: "none" (s itself), "sum", "mult", or "concat" with ``linear`` = (weight [Cs, 2 Cs], bias [Cs])."""
    if head == "none":
        return s
    if head == "sum":
        return (x + s) / 2
    if head == "mult":
        return torch.sqrt(x * s)
    if head == "concat":
        y = torch.sigmoid(F.linear(torch.cat((x, s), dim=1).permute(0, 2, 3, 1), linear[0], linear[1]))
        return y.permute(0, 3, 1, 2)
    raise NotImplementedError(head)


def aggregate(x, source, prototypes, head, *, source_kind="distances", activation="log", eps=EPS, linear=None):
    """The op ``scale_aggregate`` and the module around it, in the dtype of its arguments (float64 for a reference)."""
    a = similarity(source, activation, eps) if source_kind == "distances" else source
    return combine(head, x, weighted_sum(a, prototypes), linear)


# ---------------------------------------------------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------------------------------------------------
def _ranges(ranges, S):
    return [tuple(int(v) for v in ranges[s]) for s in range(S)]


def chain(conv, bank, ranges, S, head, *, linear=None, activation="log", eps=EPS, rounding=None, x_primes=None):
    """(distances [B, P, H, W], [x'_0 .. x'_{S-1}]) in float64.  ``rounding``: applied to both inputs of every distance
    (None: none).  ``x_primes``: {scale: tensor} taken in place of the chain's own aggregated features of that scale."""
    conv, bank = conv.double(), bank.double().reshape(bank.shape[0], -1)
    linear = None if linear is None else tuple(t.double() for t in linear)
    rnd =(lambda t: t) if rounding is None else (lambda t: rounding(t.float()).double())
    rg = _ranges(ranges, S)
    Cs = conv.shape[1] // S
    dist, xs = [None] * S, [None] * S
    for i in range(S - 1, -1, -1):
        x = conv[:, i * Cs:(i + 1) * Cs]
        if i < S - 1:
            x = aggregate(x, dist[i + 1], bank[rg[i + 1][0]:rg[i + 1][1]], head, activation=activation, eps=eps, linear=linear)
        if x_primes is not None and i in x_primes:
            x = x_primes[i].double()
        xs[i] = x
        lo, hi = rg[i]
        dist[i] = O.l2_convolution(rnd(x), rnd(bank[lo:hi])[:, :, None, None])
    return torch.cat(dist, dim=1), xs


def head_loss(fx, phase, dist, params, activation="log", eps=EPS):
    """The loss of oracle/gen_golden.py::case_proto_phase on a float64 distance map: (loss, logits, activations).  ``params``:
    the head's float64 leaves - {"last_layer.weight"} or {"last_layer_group.weight", "group_projection.<j>.weight", "ident"}."""
    B, P, H, W = dist.shape
    act = similarity(dist.permute(0, 2, 3, 1).reshape(-1, P), activation, eps)
    if phase == "proto":
        logits = F.linear(act, params["last_layer.weight"])
    else:
        n = sum(1 for k in params if k.startswith("group_projection."))
        groups = O.compute_group(act, params["ident"], [params[f"group_projection.{j}.weight"] for j in range(n)])
        logits = F.linear(torch.cat(groups, dim=-1), params["last_layer_group.weight"])
    logits = logits.reshape(B, H, W, -1)
    loss = (logits * fx["g_logits"].double()).sum() + (dist * fx["g_dist"].double()).sum() + (act * fx["g_act"].double()).sum()
    return loss, logits, act


def chain_gradients(conv, bank, ranges, S, head, loss_of_dist, *, linear=None, activation="log", eps=EPS, x_primes=None,
                    rounding=R.bf16_rne):
    """Gradients of ``loss_of_dist(dist)`` through the chain as the kernels form them, float64:

      distance link    d_i = l2(rounding(x'_i), rounding(p_i)); its gradient by the site formula of
                       offgrid_restatement.restated_gradients with x'_i in the place of the features (``x_primes`` = the device's)
      aggregation link x'_i = aggregate(x_i, d_{i+1}, p_{i+1}): float64 autograd at (x_i, the restated d_{i+1}, the fp32 p_{i+1})

    Returns SimpleNamespace(conv, bank, linear = (dW, db) | None, dist = the restated map).  Parameters inside ``loss_of_dist``
    are the caller's own leaves."""
    conv, bank2 = conv.float(), bank.float().reshape(bank.shape[0], -1)
    rg = _ranges(ranges, S)
    B, C, H, W = conv.shape
    Cs = C // S
    dist, xs = chain(conv, bank2, rg, S, head, linear=None if linear is None else tuple(t.double() for t in linear),
                     activation=activation, eps=eps, rounding=rounding, x_primes=x_primes)
    d = dist.detach().requires_grad_(True)
    loss_of_dist(d).backward()
    G = [d.grad[:, lo:hi].clone() for lo, hi in rg]
    d_conv = torch.zeros(B, C, H, W, dtype=torch.float64)
    d_bank = torch.zeros_like(bank2, dtype=torch.float64)
    d_lin = None if linear is None else [torch.zeros_like(t, dtype=torch.float64) for t in linear]
    for i in range(S):
        lo, hi = rg[i]
        xp = xs[i].float()
        op = R.site_operands(xp, bank2[lo:hi])
        Gi = (G[i] * (dist[:, lo:hi] > 0)).reshape(B, hi - lo, H * W)
        xa, xc = (op[k].double().reshape(B, Cs, H * W) for k in ("a", "c"))
        pb, pd = (op[k].double().reshape(hi - lo, Cs) for k in ("b", "d"))
        d_xp = (2.0 * Gi.sum(1, keepdim=True) * xa - 2.0 * torch.einsum("bpm,pc->bcm", Gi, pb)).reshape(B, Cs, H, W)
        d_bank[lo:hi] += -2.0 * torch.einsum("bpm,bcm->pc", Gi, xc) + 2.0 * pd * Gi.sum((0, 2))[:, None]
        if i == S - 1:
            d_conv[:, i * Cs:(i + 1) * Cs] = d_xp
            continue
        lo1, hi1 = rg[i + 1]
        x = conv[:, i * Cs:(i + 1) * Cs].double().requires_grad_(True)
        src = dist[:, lo1:hi1].detach().clone().requires_grad_(True)
        p1 = bank2[lo1:hi1].double().requires_grad_(True)
        lin = None if linear is None else tuple(t.double().requires_grad_(True) for t in linear)
        out = aggregate(x, src, p1, head, activation=activation, eps=eps, linear=lin)
        out.backward(d_xp)
        d_conv[:, i * Cs:(i + 1) * Cs] = x.grad
        G[i + 1] += src.grad
        d_bank[lo1:hi1] += p1.grad
        if lin is not None:
            for acc, t in zip(d_lin, lin):
                acc += t.grad
    return SimpleNamespace(conv=d_conv, bank=d_bank.reshape(bank.shape), linear=d_lin, dist=dist)


# ---------------------------------------------------------------------------------------------------------------------
# the op's error bound (tests/test_gpu_scale_head.py)
# ---------------------------------------------------------------------------------------------------------------------
def s_error_bound(activations, prototypes):
    """E_s = sum_p |p_pc| 2^-21 (1 + |a_p|) + (Pn + 2) 2^-24 sum_p |p_pc a_p|  [B, Cs, H, W], float64: act_log's one-ulp
    reciprocal and logarithm with a factor 2 of headroom, and the fp32 accumulation chain."""
    a, p = activations.double().abs(), prototypes.double().abs().reshape(prototypes.shape[0], -1)
    Pn = p.shape[0]
    return 2.0 ** -21 * weighted_sum(1.0 + a, p) + (Pn + 2) * 2.0 ** -24 * weighted_sum(a, p)


def out_error_bound(mode, x, s, out64, E_s):
    """|out - out64| <= |d out / d s| E_s + 2^-22 |out64|."""
    if mode == "none":
        ds = torch.ones_like(s)
    elif mode == "sum":
        ds = torch.full_like(s, 0.5)
    else:
        ds = x.double() / (2.0 * out64)
    return ds.abs() * E_s + 2.0 ** -22 * out64.abs()


# ---------------------------------------------------------------------------------------------------------------------
# the fixture (tools/gen_scale_head_golden.py)
# ---------------------------------------------------------------------------------------------------------------------
def _load(path):
    z = np.load(path)
    cases = {}
    for key in z.files:
        name, field = key.split("__")
        cases.setdefault(name, {})[field] = z[key]
    return cases


_FIXTURES = {}


def fixture(gid, head, phase, golden_dir):
    """One recorded case as a dict of torch tensors / lists: the shared inputs of shape ``gid``, the head's distances and
    activations, and the phase's logits, gradients (``d.<name>``) and state dict (``sd.<key>``, ``state_keys``)."""
    import os

    name = "scale_head.npz" if gid == "G1" else f"scale_head_{gid.lower()}_{head}.npz"
    if name not in _FIXTURES:
        _FIXTURES[name] = _load(os.path.join(golden_dir, name))
    cases = _FIXTURES[name]
    out = {}
    for part in (gid, f"{gid}_{head}", f"{gid}_{head}_{phase}"):
        for k, v in cases[part].items():
            out[k] = [str(s) for s in v] if k == "state_keys" else torch.from_numpy(np.asarray(v))
    B, S, Cs, P, K, H, W, G = (int(v) for v in out["shape"])
    out["dims"] = SimpleNamespace(B=B, S=S, Cs=Cs, P=P, K=K, H=H, W=W, G=G)
    out["ranges"] = {s: tuple(int(v) for v in out["scale_ranges"][s]) for s in range(S)}
    out["linear"] = ((out["sd.scale_head.output_layer.linear_block.0.weight"], out["sd.scale_head.output_layer.linear_block.0.bias"])
                     if head == "concat" else None)
    return out


def head_params(fx, phase):
    """The float64 leaves ``head_loss`` takes, from a fixture's state dict."""
    if phase == "proto":
        return {"last_layer.weight": fx["sd.last_layer.weight"].double().requires_grad_(True)}
    d = fx["dims"]
    out = {"ident": O.default_class_identity(d.P, d.K, d.S),
           "last_layer_group.weight": fx["sd.last_layer_group.weight"].double().requires_grad_(True)}
    j = 0
    while f"sd.group_projection.{j}.weight" in fx:
        out[f"group_projection.{j}.weight"] = fx[f"sd.group_projection.{j}.weight"].double().requires_grad_(True)
        j += 1
    return out
