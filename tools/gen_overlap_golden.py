"""Write tests/golden/activation_overlap.npz by driving the reference's own ``prototype_overlap`` and ``group_overlap``
(segmentation/analysis/prototype_overlap.py:28-92, group_overlap.py:28-87; CPU only).

    SPX_REFERENCE=/path/to/ScaleProtoSeg python tools/gen_overlap_golden.py [output.npz]

The two functions are loaded from the reference checkout and called once per image with stand-ins for everything around them
(those of tools/reference_stubs.py, and):

* a fake ``ppnet`` that returns prepared tensors (``conv_features``, ``forward_from_conv_features``, ``compute_group``,
  ``prototype_class_identity``, ``epsilon``, ``num_groups``); ``.cuda()`` is a no-op;
* ``to_normalized_tensor`` and ``transforms.ToTensor`` stubs that only carry the image size;
* ``np.quantile(x, 0.95)`` inside the two functions answered at the case's ``q`` (the reference hard-codes 0.95; the fixture
  also records 0.8), by the real ``np.quantile`` on the same float32 array;
* the reference cannot take a label outside 0..K (it indexes the class identity with it), so the one out-of-range pixel of the
  recorded labels is handed to it as void: both belong to no class.

Data only is recorded, keys ``<case>__<field>``: the latent distances or activations (bf16-representable), labels, identity or
group sizes, q, numpy's thresholds of every plane, the reference's intersection and union per class / slot pair and in total,
the areas of the masks at numpy's thresholds, and per plane the count of "ambiguous" pixels with |u64 - T| <= m,
m = 64 * 2^-23 * max|a|.  The tool asserts ambiguous <= 4 + |mask| / 1000 for every plane (the seeds below satisfy it) except in the
exact case, whose quantised planes tie with their thresholds on purpose."""
from __future__ import annotations

import os
from collections import defaultdict

import numpy as np
import torch

import reference_stubs as S
import overlap_restatement as R

EPS = 1e-4
BLOCKS = (6, 7)
Q = {"value": 0.95}


class _NumpyAtQ:
    """numpy, with ``quantile(x, 0.95)`` answered at the case's q."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def quantile(a, q):
        assert q == 0.95
        return np.quantile(a, Q["value"])


class _ProtoNet:
    def __init__(self, ident):
        self.prototype_class_identity = ident
        self.epsilon = EPS
        self.num_classes = ident.shape[1]

    def conv_features(self, x):
        return x

    def forward_from_conv_features(self, conv):
        return None, self.distances


class _GroupNet:
    def __init__(self, K, G):
        self.num_classes, self.num_groups = K, G

    def conv_features(self, x):
        return torch.empty(1, 1, *self.grid)

    def forward_from_conv_features(self, conv, return_activations=False):
        assert return_activations
        return None, None

    def compute_group(self, activations):
        return self.groups


def _collect(class_val, tot_val, slots_of, N_present):
    """The reference's lists -> per (class, slot pair) sums.  It appends one entry per (image, pair j < j') in that order."""
    K = len(slots_of)
    J = max(1, max(len(s) for s in slots_of))
    inter = np.zeros((K, J, J), np.int64)
    union = np.zeros((K, J, J), np.int64)
    for k in range(K):
        pairs = [(a, b) for a in range(len(slots_of[k])) for b in range(a + 1, len(slots_of[k]))]
        li, lu = class_val[k]["intersection"], class_val[k]["union"]
        assert len(li) == len(lu) == len(pairs) * N_present[k], (k, len(li), len(pairs), N_present[k])
        for i, (vi, vu) in enumerate(zip(li, lu)):
            a, b = pairs[i % len(pairs)]
            inter[k, a, b] += int(vi)
            union[k, a, b] += int(vu)
    return dict(ref_inter=inter, ref_union=union, ref_total_inter=np.int64(np.sum(tot_val["intersection"])),
                ref_total_union=np.int64(np.sum(tot_val["union"])))


def _numpy_side(planes, lab, table, q, check=True):
    """numpy's thresholds of every plane and, from them, mask areas and ambiguous counts (the reference reports neither)."""
    N, C = planes.shape[:2]
    H, W = lab.shape[1:]
    thr = np.zeros((N, C), np.float32)
    amb = np.zeros((N, C), np.int64)
    cnt = np.zeros((N, C), np.int64)
    for n in range(N):
        for c in range(C):
            u = R.upsample(planes[n, c], (H, W))
            u32 = u.astype(np.float32)
            thr[n, c] = np.quantile(u32, q)
            cnt[n, c] = int((u32 > thr[n, c]).sum())
            amb[n, c] = int((np.abs(u - np.float64(thr[n, c])) <= R.margin(planes[n, c])).sum())
            assert not check or amb[n, c] <= 4 + cnt[n, c] / 1000, (n, c, amb[n, c], cnt[n, c])
    K, J = table.shape
    area = np.zeros((K, J), np.int64)
    for n in range(N):
        for k in range(K):
            if (lab[n] == k + 1).any():
                for j in range(J):
                    if table[k, j] >= 0:
                        area[k, j] += cnt[n, table[k, j]]
    return dict(thresholds=thr, ambiguous=amb, area=area)


def _proto_case(name, PO, seed, h, w, H, W, q):
    g = torch.Generator().manual_seed(seed)
    # classes: 0 three prototypes (the third a copy of the first), 1 two, 2 one, 3 none, 4 three but absent from every image
    cls = [0, 0, 0, 1, 1, 2, 4, 4, 4]
    K, P, N = 5, len(cls), 2
    ident = torch.zeros(P, K)
    ident[torch.arange(P), torch.tensor(cls)] = 1
    present = [[0, 1, 2, 3], [0, 2]]
    base = torch.rand(N, K, h, w, generator=g) * 1.5 + 0.05
    d = S.bf16(base[:, cls] + 0.3 * torch.rand(N, P, h, w, generator=g))
    d[:, 2] = d[:, 0]
    lab = S.labels(g, N, H, W, K, present, BLOCKS)
    Q["value"] = q
    net = _ProtoNet(ident)
    class_val = {k: defaultdict(list) for k in range(K)}
    tot_val = defaultdict(list)
    for n in range(N):
        net.distances = d[n:n + 1]
        PO.prototype_overlap(S.Sized(H, W), S.for_reference(lab[n], K), net, class_val, tot_val)
    slots_of = [[p for p in range(P) if cls[p] == k] for k in range(K)]
    table = np.full((K, 3), -1, np.int64)
    for k in range(K):
        table[k, :len(slots_of[k])] = slots_of[k]
    dn = d.numpy()
    act = np.log((dn + 1) / (dn + EPS))                       # prototype_overlap.py:60, float32 as there
    out = dict(kind=np.array("proto"), distances=dn, ident=ident.numpy(), labels=lab, q=np.float64(q), table=table)
    out.update(_collect(class_val, tot_val, slots_of, [sum(k in p for p in present) for k in range(K)]))
    out.update(_numpy_side(act, lab, table, q))
    return {f"{name}__{k}": v for k, v in out.items()}


def _group_case(name, GO, seed, h, w, H, W, q, exact=False):
    g = torch.Generator().manual_seed(seed)
    K, G, N = 3, 3, 2
    present = [[0, 1], [1, 2]] if exact else [[0, 1], [0]]
    base = torch.rand(N, K, 1, h, w, generator=g) * 2.0
    a = base + 0.3 * torch.rand(N, K, G, h, w, generator=g)
    if exact:
        a = torch.round(a * 4.0) / 4.0                        # multiples of 0.25: many ties across the threshold
        a[:, 1, 2] = 0.75                                     # a constant plane: empty mask
        a[:, 2, 1] = a[:, 2, 0]                               # a duplicated plane: intersection = union = area
    a = S.bf16(a).reshape(N, K * G, h, w)
    lab = S.labels(g, N, H, W, K, present, BLOCKS)
    Q["value"] = q
    net = _GroupNet(K, G)
    net.grid = (h, w)
    class_val = {k: defaultdict(list) for k in range(K)}
    tot_val = defaultdict(list)
    for n in range(N):
        pix = a[n].permute(1, 2, 0).reshape(h * w, K * G)     # the [M, U] layout compute_group's list is split from
        net.groups = list(torch.split(pix, G, dim=1))
        GO.group_overlap(S.Sized(H, W), S.for_reference(lab[n], K), net, class_val, tot_val)
    table = np.arange(K * G, dtype=np.int64).reshape(K, G)
    out = dict(kind=np.array("group"), activations=a.numpy(), labels=lab, q=np.float64(q), table=table)
    out.update(_collect(class_val, tot_val, [list(r) for r in table], [sum(k in p for p in present) for k in range(K)]))
    out.update(_numpy_side(a.numpy(), lab, table, q, check=not exact))      # the exact case is all ties
    return {f"{name}__{k}": v for k, v in out.items()}


def main():
    S.stub_modules()
    PO = S.load(os.path.join("segmentation", "analysis", "prototype_overlap.py"), numpy_proxy=_NumpyAtQ())
    GO = S.load(os.path.join("segmentation", "analysis", "group_overlap.py"), numpy_proxy=_NumpyAtQ())
    cases = {}
    shapes = (("s5x7", 5, 7, 33, 50), ("s9x11", 9, 11, 70, 85), ("s17x17", 17, 17, 129, 129), ("s33x65", 33, 65, 257, 513))
    seed = 20240611
    for tag, h, w, H, W in shapes:
        for q in (0.95, 0.8):
            seed += 1
            cases.update(_proto_case(f"proto_{tag}_q{int(q * 100)}", PO, seed, h, w, H, W, q))
    for tag, h, w, H, W in shapes[:2]:
        for q in (0.95, 0.8):
            seed += 1
            cases.update(_group_case(f"group_{tag}_q{int(q * 100)}", GO, seed, h, w, H, W, q))
    cases.update(_group_case("exact_70x85_q95", GO, seed + 1, 70, 85, 70, 85, 0.95, exact=True))
    out = S.out_path("activation_overlap.npz")
    np.savez_compressed(out, **cases)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
