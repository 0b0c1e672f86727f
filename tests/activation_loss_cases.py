"""The activation losses' cases and checkers, shared by tests/test_activation_losses_cpu.py and the GPU suites: the fixture
recorded from the reference (tests/golden/activation_losses.npz, tools/gen_activation_loss_golden.py), a torch restatement of the
three terms from their definitions - what the GPU tests hold the kernels against - and the float64 comparison with its bounds."""
import math
import os

import numpy as np
import torch

from support import EPS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "activation_losses.npz")
CASES = ("even", "ragged", "ties")
TERMS = ("spat", "sampl", "l1", "linf")
W3 = (0.7, 1.3, 0.5)     # weights of the three terms in the GPU suites' weighted totals


def load_case(name):
    z = np.load(GOLDEN)
    c = {k[len(name) + 2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(name + "__")}
    c["ranges"] = [tuple(int(x) for x in r) for r in c["scales"].tolist()]
    return c


def log_activation(d, eps=EPS):
    return torch.log((d + 1) / (d + eps))


def restate(act, target, ident, ranges, norm_type="l1"):
    """The three terms from their definitions, in ``act``'s dtype, differentiable to ``act`` [B * HW, P] (or [B, HW, P]).
    Returns ({"spat", "sampl", "norm"}: 0-d tensors, {the same}: number of segments / items of each term).
      segment = (image, class with >= 1 prototype) with n pixels, Jc = the class's prototypes
      spat   segments with n >= 2: mean_j H_j / ln n, H_j = entropy of softmax over the segment's pixels of column j
      sampl  items (segment, scale) with n >= 1 and ns >= 2 prototypes of the class in the scale: mean_px H_px / ln ns, H_px =
             entropy of the softmax over the ns columns (an item with ns < 2 is skipped)
      norm   segments with n >= 1: mean_j sum_px |a| / n (l1) or mean_j max_px |a| (linf: amax splits the gradient evenly among ties)
    each the mean over its segments / items, 0 without any."""
    Bn = target.shape[0]
    P, K = ident.shape
    lab = target.reshape(Bn, -1).long() - 1
    a = act.reshape(Bn, -1, P)
    spat, sampl, norm = [], [], []
    for b in range(Bn):
        for c in range(K):
            protos = torch.nonzero(ident[:, c]).flatten().tolist()
            mask = lab[b] == c
            n = int(mask.sum())
            if not protos or n == 0:
                continue
            seg = a[b][mask][:, protos]                       # [n, Jc]
            if n >= 2:
                logp = torch.log_softmax(seg, dim=0)
                spat.append((-(logp.exp() * logp).sum(0)).mean() / math.log(n))
            for lo, hi in ranges:
                cols = [i for i, p in enumerate(protos) if lo <= p < hi]
                if len(cols) < 2:
                    continue
                logp = torch.log_softmax(seg[:, cols], dim=1)
                sampl.append((-(logp.exp() * logp).sum(1) / math.log(len(cols))).mean())
            if norm_type == "l1":
                norm.append((seg.abs().sum(0) / n).mean())
            elif norm_type == "linf":
                norm.append(seg.abs().amax(dim=0).mean())
            else:
                raise ValueError(norm_type)
    zero = (a * 0).sum()
    mean = lambda xs: torch.stack(xs).mean() if xs else zero
    return ({"spat": mean(spat), "sampl": mean(sampl), "norm": mean(norm)},
            {"spat": len(spat), "sampl": len(sampl), "norm": len(norm)})


def restate_term(term, act, target, ident, ranges):
    """One fixture term (spat / sampl / l1 / linf) of the restatement."""
    vals, counts = restate(act, target, ident, ranges, norm_type=term if term in ("l1", "linf") else "l1")
    key = "norm" if term in ("l1", "linf") else term
    return vals[key], counts[key]


def identity(scale_counts):
    """scale_counts[s][k]: prototypes of class k in scale s, laid out scale-major / class-minor."""
    rows, ranges = [], []
    for counts in scale_counts:
        lo = len(rows)
        for k, n in enumerate(counts):
            rows += [k] * n
        ranges.append((lo, len(rows)))
    ident = torch.zeros(len(rows), len(scale_counts[0]))
    for i, k in enumerate(rows):
        ident[i, k] = 1
    return ident, ranges


def reference64(d, target, ident, ranges, norm_type, weights, transform):
    """float64 restatement on ``d`` [B*HW, P] with a = transform(d): (terms dict, counts, gradient of the weighted total to d)."""
    dd = d.double().clone().requires_grad_(True)
    vals, counts = restate(transform(dd), target, ident, ranges, norm_type=norm_type)
    total = weights[0] * vals["spat"] + weights[1] * vals["sampl"] + weights[2] * vals["norm"]
    total.backward()
    return {k: v.item() for k, v in vals.items()}, counts, total.item(), dd.grad


def check_against_reference64(got_total, got_terms, got_grad, ref, what):
    vals, counts, total, grad = ref
    for i, k in enumerate(("spat", "sampl", "norm")):
        err = abs(got_terms[i].item() - vals[k])
        print(f"{what}: {k} got {got_terms[i].item():.9g} ref {vals[k]:.9g} err {err:.3g} items {counts[k]}")
        assert counts[k] > 0, (what, k, "no segment or item")
        assert err <= 1e-5 * max(1.0, abs(vals[k])), (what, k)
    assert abs(got_total.item() - total) <= 1e-5 * max(1.0, abs(total)), what
    gmax = grad.abs().max().item()
    gerr = (got_grad.double().cpu() - grad).abs().max().item()
    print(f"{what}: gradient err {gerr:.3g} of max {gmax:.3g}")
    assert gerr <= 1e-4 * gmax + 1e-12, what
