"""NumPy restatement of the failure cases (scaleprotoseg_amd/failures.py); no device code is imported.

    predict       the first argmax over the classes of oracle.ppnet_oracle.upsample_bilinear_restated (pinned to F.interpolate
                  bit for bit by tests/test_oracle_golden.py), through the id map: uint8 [N, H, W]
    confusion     int64 [N, K+1, K]: conf[n, r, pred] += 1 per pixel with label != 0, r = label - 1 for 1 <= label <= K, else K
    failure_table iou = I / U in float64 (Python's / NumPy's correctly rounded division), fail = iou < threshold (strict),
                  miss = the lowest j != k with the largest conf[n, k, j] > 0, else -1; a class that is not present: NaN, -1, 0
    paired_heat   u = overlap_restatement.upsample (float64) rounded to float32, m = u * [label == a + 1]; lo_q, hi_q over all
                  rows of slot q; np.uint8-style trunc(255 * ((m - lo_q) / hi_q)) in float32, 255 where 255 x >= 256, all zeros
                  where hi_q <= 0.  ``flagged`` marks the pixels (255 x >= 256) and rows (hi_q <= 0) where the reference's own
                  conversion is undefined.

Ambiguity (a condition on the inputs, not a tolerance of the kernel).  With m0 = overlap_restatement.margin(plane) the kernel's
fp32 sample lies within m0 of the float64 value, so each of m, lo, hi moves by at most m0 and x = (m - lo) / hi by about
(2 + x) m0 / hi: a pixel is ambiguous when the float64 value 255 x lies within 255 (2 + x) m0 / hi of an integer (m0 the largest
of the slot's planes).  As in explain_restatement one kind of pixel is taken out, because nothing about it is rounded: outside
the class m is 0 exactly, and when lo_q is an exact 0 and every class sample of every row of the slot is above m0, the kernel's
lo is the same 0, r = 0 and the byte is 0 in any arithmetic."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import overlap_restatement as OR  # noqa: E402
from oracle import ppnet_oracle as O  # noqa: E402


def argmax_map(logits, size):
    """int64 [N, H, W]: the first argmax over the classes of the upsampled logits [N, h, w, K] (fp32)."""
    up = O.upsample_bilinear_restated(torch.from_numpy(np.ascontiguousarray(np.asarray(logits, np.float32).transpose(0, 3, 1, 2))), size)
    return np.argmax(up.numpy(), axis=1)


def predict(logits, size, id_map=None):
    k = argmax_map(logits, size)
    return (k if id_map is None else np.asarray(id_map)[k]).astype(np.uint8)


def confusion(k_star, labels, K):
    """int64 [N, K+1, K] from the class map ``k_star`` [N, H, W] (before any id map) and the labels."""
    lab = np.asarray(labels).astype(np.int64)
    N = lab.shape[0]
    conf = np.zeros((N, K + 1, K), np.int64)
    for n in range(N):
        on = lab[n] != 0
        r = np.where((lab[n] >= 1) & (lab[n] <= K), lab[n] - 1, K)
        np.add.at(conf[n], (r[on], k_star[n][on]), 1)
    return conf


def aggregate(k_star, labels, K):
    """int64 [K+1, K]: the rule of SegmentationMetrics over the whole batch at once."""
    lab = np.asarray(labels).astype(np.int64).ravel()
    on = lab != 0
    r = np.where((lab >= 1) & (lab <= K), lab - 1, K)
    return np.bincount(r[on] * K + np.asarray(k_star).ravel()[on], minlength=(K + 1) * K).reshape(K + 1, K)


def failure_table(conf, threshold):
    """(iou float64 [N, K], miss int32 [N, K], fail uint8 [N, K])."""
    conf = np.asarray(conf, np.int64)
    N, _, K = conf.shape
    iou = np.full((N, K), np.nan, np.float64)
    miss = np.full((N, K), -1, np.int32)
    fail = np.zeros((N, K), np.uint8)
    for n in range(N):
        for k in range(K):
            row = int(conf[n, k].sum())
            if row == 0:
                continue
            I = int(conf[n, k, k])
            U = row + int(conf[n, :, k].sum()) - I
            iou[n, k] = I / U
            fail[n, k] = iou[n, k] < float(threshold)
            others = conf[n, k].copy()
            others[k] = 0
            if others.max() > 0:
                miss[n, k] = int(np.argmax(others))                     # the first maximum: the lowest class
    return iou, miss, fail


def cases_and_rows(fail, miss, table, shared, ignore_miss=None):
    """(cases [F, 3] = (n, a, miss), rows [R, 4] = (n, c, a, q)) in the reference's order of visits: images, then classes
    ascending; per case the slots of a, then the slots of miss.  ``shared``: one range per (case, slot index) (groups:
    group_max[i]); otherwise one per (case, plane) (prototypes: proto_max[p])."""
    cases, rows, slots = [], [], {}
    N, K = fail.shape
    for n in range(N):
        for a in range(K):
            m = int(miss[n, a])
            if not fail[n, a] or m < 0 or (ignore_miss is not None and m == ignore_miss):
                continue
            i = len(cases)
            cases.append((n, a, m))
            for k in (a, m):
                for j, c in enumerate(np.asarray(table)[k]):
                    if c >= 0:
                        q = slots.setdefault((i, j) if shared else (i, int(c)), len(slots))
                        rows.append((n, int(c), a, q))
    return np.array(cases, np.int64).reshape(-1, 3), np.array(rows, np.int64).reshape(-1, 4)


def _masked(planes, labels, row, f64):
    n, c, a, _ = (int(v) for v in row)
    u = OR.upsample(planes[n, c], labels.shape[1:])
    return (u if f64 else u.astype(np.float32)) * (labels[n] == a + 1)


def paired_heat(planes, labels, rows, Q):
    """(heat uint8 [R, H, W], ranges float32 [Q, 2], flagged bool [R, H, W]) in float32, the reference's arithmetic."""
    planes, labels, rows = np.asarray(planes, np.float32), np.asarray(labels), np.asarray(rows)
    m = [_masked(planes, labels, r, False) for r in rows]
    lo = np.full(Q, np.inf, np.float32)
    hi = np.full(Q, -np.inf, np.float32)
    for r, mr in zip(rows, m):
        lo[r[3]] = min(lo[r[3]], mr.min())
        hi[r[3]] = max(hi[r[3]], mr.max())
    heat = np.zeros((len(rows),) + labels.shape[1:], np.uint8)
    flagged = np.zeros(heat.shape, bool)
    for i, (r, mr) in enumerate(zip(rows, m)):
        q = r[3]
        if not hi[q] > 0:
            flagged[i] = True
            continue
        v = np.float32(255.0) * ((mr - lo[q]).astype(np.float32) / hi[q]).astype(np.float32)
        flagged[i] = v >= 256
        heat[i] = np.where(flagged[i], 255, np.minimum(v, 255).astype(np.int64)).astype(np.uint8)
    return heat, np.stack([lo, hi], axis=1), flagged


def slot_margin(planes, rows, Q):
    """float [Q]: the largest m0 among the planes of each slot."""
    m0 = np.zeros(Q)
    for n, c, _, q in np.asarray(rows):
        m0[q] = max(m0[q], OR.margin(np.asarray(planes)[n, c]))
    return m0


def paired_ambiguous(planes, labels, rows, Q):
    """bool [R, H, W]: pixels whose byte may differ by one under an error of m0 per sample."""
    planes, labels, rows = np.asarray(planes, np.float32), np.asarray(labels), np.asarray(rows)
    m = [_masked(planes, labels, r, True) for r in rows]
    m0 = slot_margin(planes, rows, Q)
    lo, hi = np.full(Q, np.inf), np.full(Q, -np.inf)
    clear = np.ones(Q, bool)                                             # every class sample of every row of the slot is above m0
    for r, mr in zip(rows, m):
        q, on = r[3], labels[r[0]] == r[2] + 1
        lo[q], hi[q] = min(lo[q], mr.min()), max(hi[q], mr.max())
        clear[q] &= bool(on.any()) and bool(mr[on].min() > m0[q])
    amb = np.zeros((len(rows),) + labels.shape[1:], bool)
    for i, (r, mr) in enumerate(zip(rows, m)):
        q = r[3]
        if not hi[q] > 0:
            continue
        x = (mr - lo[q]) / hi[q]
        v = 255.0 * x
        amb[i] = np.abs(v - np.round(v)) <= 255.0 * (2.0 + x) * m0[q] / hi[q]
        if lo[q] == 0 and clear[q]:
            amb[i] &= labels[r[0]] == r[2] + 1
    return amb
