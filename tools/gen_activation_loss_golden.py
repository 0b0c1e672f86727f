"""Write tests/golden/activation_losses.npz from the reference's own loss classes (CPU only).

    SPX_REFERENCE=/path/to/ScaleProtoSeg python tools/gen_activation_loss_golden.py

Imports ``segmentation/model/loss.py`` of the reference checkout (it needs nothing but torch) and records, per case, the seeded
inputs (class identity, scale ranges, target, distances d, activations act = log((d+1)/(d+1e-4))), the values of
EntropySpatLoss / EntropySamplLoss / NormLoss("l1") / NormLoss("linf") and their gradients with respect to ``act`` and, by
autograd through the activation formula, with respect to ``d``.  Data only: nothing of the reference is written.
Keys: ``<case>__<field>``.  No (class, scale) of a case has fewer than two prototypes unless the class has none at all: the
reference's sample entropy is NaN for one (0 / ln 1) and raises for none, and neither is recorded."""
from __future__ import annotations

import importlib.util
import os
import sys
import warnings

sys.dont_write_bytecode = True

import numpy as np
import torch

REF = os.environ.get("SPX_REFERENCE")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "activation_losses.npz")
B, H, W = 2, 7, 9
EPS = 1e-4


def _identity(scale_counts):
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


def _target(K, g):
    """Labels 0 (void) .. K, one out-of-range label K + 1, and class 1 with exactly one pixel in image 1."""
    t = torch.randint(0, K + 1, (B, H, W), generator=g)
    t[0, 0, :2] = 0
    t[0, 3, 4] = K + 1
    t[1][t[1] == 1] = 2
    t[1, 5, 2] = 1
    assert (t == 0).any() and (t == K + 1).any() and int((t[1] == 1).sum()) == 1
    return t


def _case(name, scale_counts, g, L, ties=False):
    ident, ranges = _identity(scale_counts)
    P, K = ident.shape
    target = _target(K, g)
    d = (torch.rand(B * H * W, P, generator=g) * 2.0 + 0.01).float()
    if ties:
        # five pixels of segment (image 0, class 2) at distance exactly 0 to that class's first prototype: they share the
        # maximum activation ln(1 / eps)
        p = int(torch.nonzero(ident[:, 1]).flatten()[0])
        px = torch.nonzero(target[0].reshape(-1) == 2).flatten()
        assert len(px) >= 7
        d[px[:5], p] = 0.0
        assert (d[d != 0] >= 0.01).all()
    out = {"ident": ident.numpy(), "scales": np.array(ranges, dtype=np.int64), "target": target.numpy(), "d": d.numpy()}
    S = len(ranges)
    scale_table = {s: r for s, r in enumerate(ranges)}
    mods = (("spat", L.EntropySpatLoss(ident)), ("sampl", L.EntropySamplLoss(ident, S, scale_table)),
            ("l1", L.NormLoss(ident, "l1")), ("linf", L.NormLoss(ident, "linf")))
    for key, mod in mods:
        dd = d.clone().requires_grad_(True)
        act = torch.log((dd + 1) / (dd + EPS))
        act.retain_grad()
        v = mod(act, target)
        v.backward()
        assert torch.isfinite(v) and torch.isfinite(act.grad).all() and torch.isfinite(dd.grad).all(), (name, key)
        out["act"] = act.detach().numpy()
        out[key] = np.array(v.item(), np.float32)
        out["d_" + key + "_act"] = act.grad.numpy()
        out["d_" + key + "_d"] = dd.grad.numpy()
    return {f"{name}__{k}": v for k, v in out.items()}


def main():
    if not REF:
        sys.exit("set SPX_REFERENCE to the reference checkout")
    spec = importlib.util.spec_from_file_location("ref_loss", os.path.join(REF, "segmentation", "model", "loss.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)
    warnings.filterwarnings("ignore", message="Implicit dimension choice")
    g = torch.Generator().manual_seed(20220227)
    cases = {}
    cases.update(_case("even", [[2, 2, 2], [2, 2, 2]], g, L))
    # a class without prototypes, unequal counts per class and scale
    cases.update(_case("ragged", [[3, 2, 0, 2], [2, 3, 0, 4]], g, L))
    cases.update(_case("ties", [[2, 2, 2], [2, 2, 2]], g, L, ties=True))
    np.savez_compressed(OUT, **cases)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
