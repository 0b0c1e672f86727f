"""Write tests/golden/group_regularizers.npz from the reference's own loss classes (CPU only).

    SPX_REFERENCE=/path/to/ScaleProtoSeg python tools/gen_regularizer_golden.py

Imports ``segmentation/model/loss.py`` of the reference checkout (it needs nothing but torch) and records, per case, the
seeded inputs, EntropyGroup / CrossEntropyGroup / ScaleMax with their gradients to the group projection weights, and the
masked L1 of the group head (module_multiscale_group_train.py:283-285) and of the prototype head (module_multiscale.py:260-261)
with theirs.  Data only: nothing of the reference is written.  Keys: ``<case>__<field>``; weights and their gradients are
flat in block order (class blocks of the classes that own prototypes, each [G, n_j] row-major)."""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

REF = os.environ.get("SPX_REFERENCE")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "group_regularizers.npz")


def _simplex(v: torch.Tensor) -> torch.Tensor:
    """Euclidean projection of every row onto the probability simplex (sort form: leaves exact zeros)."""
    n = v.shape[1]
    u, _ = torch.sort(v, descending=True, dim=1)
    css = torch.cumsum(u, 1) - 1.0
    k = torch.arange(1, n + 1, dtype=v.dtype)
    cond = u - css / k > 0
    rho = cond.cumsum(1).argmax(1)
    theta = css.gather(1, rho[:, None]) / (rho[:, None] + 1).to(v.dtype)
    return torch.clamp(v - theta, min=0)


def _identity(P, K, scale_counts):
    """scale_counts[s][k]: prototypes of class k in scale s, laid out scale-major / class-minor."""
    rows, ranges, p = [], [], 0
    for counts in scale_counts:
        lo = p
        for k, n in enumerate(counts):
            for _ in range(n):
                rows.append(k)
                p += 1
        ranges.append((lo, p))
    assert p == P, (p, P)
    ident = torch.zeros(P, K)
    for i, k in enumerate(rows):
        ident[i, k] = 1
    return ident, ranges


def _case(name, ident, ranges, G, eps, weight_fn, g, L):
    P, K = ident.shape
    present = [k for k in range(K) if ident[:, k].sum() > 0]
    proj = nn.ModuleList([nn.Linear(int(ident[:, k].sum()), G, bias=False) for k in present])
    for j, lin in enumerate(proj):
        lin.weight.data = weight_fn(lin.weight.shape, g).float()
    U = G * len(present)
    gci = torch.zeros(U, K)
    for j, k in enumerate(present):
        gci[j * G:(j + 1) * G, k] = 1
    head_g = (torch.randn(K, U, generator=g) * 0.5).float()
    head_p = (torch.randn(K, P, generator=g) * 0.5).float()
    head_g[torch.rand(K, U, generator=g) < 0.1] = 0.0          # exact zeros: sgn(0) = 0
    head_p[torch.rand(K, P, generator=g) < 0.1] = 0.0
    net = types.SimpleNamespace(num_classes=K, prototype_class_identity=ident, group_class_identity=gci, num_groups=G,
                                group_projection=proj, num_scales=len(ranges),
                                scale_num_prototypes={s: r for s, r in enumerate(ranges)})
    ws = [lin.weight for lin in proj]
    out = {"ident": ident.numpy(), "scales": np.array(ranges, dtype=np.int64), "G": np.array(G), "eps": np.array(eps, np.float64),
           "w": torch.cat([w.detach().reshape(-1) for w in ws]).numpy(), "head_group": head_g.numpy(), "head_proto": head_p.numpy()}
    for key, mod in (("ent", L.EntropyGroup(net, epsilon=eps)), ("ceg", L.CrossEntropyGroup(net, epsilon=eps)), ("sm", L.ScaleMax(net))):
        v = mod()
        grads = torch.autograd.grad(v, ws)
        out[key] = np.array(v.item(), np.float32)
        out["d_" + key] = torch.cat([d.reshape(-1) for d in grads]).numpy()
    for key, W, I in (("l1_group", head_g, gci), ("l1_proto", head_p, ident)):
        Wp = W.clone().requires_grad_(True)
        v = (Wp * (1 - torch.t(I))).norm(p=1)
        (d,) = torch.autograd.grad(v, [Wp])
        out[key] = np.array(v.item(), np.float32)
        out["d_" + key] = d.numpy()
    return {f"{name}__{k}": v for k, v in out.items()}


def main():
    if not REF:
        sys.exit("set SPX_REFERENCE to the reference checkout")
    spec = importlib.util.spec_from_file_location("ref_loss", os.path.join(REF, "segmentation", "model", "loss.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)
    g = torch.Generator().manual_seed(20220227)
    simplex = lambda shape, g: _simplex(torch.randn(shape, generator=g))

    def raw(shape, g):        # non-simplex weights with entries in (0, eps), exactly eps and in (-eps, 0)
        w = torch.rand(shape, generator=g)
        m = torch.rand(shape, generator=g)
        w[m < 0.15] = 3e-6
        w[(m >= 0.15) & (m < 0.25)] = float(np.float32(1e-5))
        w[(m >= 0.25) & (m < 0.3)] = -4e-6
        return w

    cases = {}
    # group_scaleproto_cityscapes.gin: 228 prototypes, 19 classes, 4 scales, 3 groups
    ident, ranges = _identity(228, 19, [[3] * 19] * 4)
    cases.update(_case("city", ident, ranges, 3, 1e-5, simplex, g, L))
    # after pruning: uneven per-scale counts, class 3 absent, class 5 without prototypes in scale 1, class-less prototypes
    ident, ranges = _identity_ragged([[2, 3, 1, 0, 2, 1, 4, -1], [1, 2, 3, 0, 1, 0, 2, -1], [3, 1, 2, 0, 2, 2, 1]], 7)
    cases.update(_case("ragged", ident, ranges, 3, 1e-5, simplex, g, L))
    # raw (non-simplex) weights, a different epsilon
    ident, ranges = _identity(48, 4, [[3] * 4] * 4)
    cases.update(_case("raw", ident, ranges, 3, 1e-5, raw, g, L))
    cases.update(_case("raw_eps", ident, ranges, 2, 1e-3, raw, g, L))
    # a class with one prototype (log(1) = 0) and a weight below -eps: the non-finite cases
    ident, ranges = _identity(13, 3, [[1, 6, 6]])

    def nonfinite(shape, g):
        w = _simplex(torch.randn(shape, generator=g))
        if shape[1] == 6:
            w[0, 2] = -0.01
        return w

    cases.update(_case("single", ident, ranges, 3, 1e-5, nonfinite, g, L))
    np.savez_compressed(OUT, **cases)
    print(OUT, os.path.getsize(OUT), "bytes")


def _identity_ragged(scale_rows, K):
    """scale_rows[s] = per-class counts of scale s; an entry -1 is one class-less prototype."""
    labels, ranges, p = [], [], 0
    for row in scale_rows:
        lo = p
        for k, n in enumerate(row):
            if n == -1:
                labels.append(-1)
                p += 1
                continue
            labels += [k] * n
            p += n
        ranges.append((lo, p))
    ident = torch.zeros(p, K)
    for i, k in enumerate(labels):
        if k >= 0:
            ident[i, k] = 1
    return ident, ranges


if __name__ == "__main__":
    main()
