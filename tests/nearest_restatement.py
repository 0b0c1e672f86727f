"""NumPy restatement of the nearest-image / nearest-prototype analysis (scaleprotoseg_amd/nearest.py; the reference's
segmentation/analysis/nearest_img.py:33-63, :258-300 and nearest_proto.py:54-66), on the float64 upsample of
tests/overlap_restatement.py and the walk of tests/push_boxes_restatement.py.

    masked_threshold   np.percentile(u32[mask], 100 q) in the definition's form (overlap_restatement.threshold); +inf on an
                       empty mask, the reference's np.inf
    patch_majority     np.bincount(labels[rf[0]:rf[1], rf[2]:rf[3]].ravel()).argmax(): the slice clips the box, argmax takes
                       the smallest label on a tie
    gt_boxes           the crop on the plane masked to label L from the threshold over that label's pixels, with the robustness
                       flag of push_boxes_restatement.boxes for that threshold; T = +inf hits nowhere and nothing is ambiguous
    topk_images        per prototype (column) the n rows of smallest value, ascending by (value, row)
    nearest_protos     the n smallest entries of a column ascending by (value, index) among the included ones; with ``window`` the
                       reference's rule: the ``window`` smallest of all, of which the included are kept, n at the most"""
import numpy as np

import overlap_restatement as R
import push_boxes_restatement as PB


def masked_threshold(u32, mask, q=0.95):
    mask = np.asarray(mask, bool)
    if not mask.any():
        return np.float32(np.inf)
    return R.threshold(np.asarray(u32, np.float32)[mask], q)


def patch_majority(labels, rf):
    labels = np.asarray(labels)
    return int(np.bincount(labels[rf[0]:rf[1], rf[2]:rf[3]].ravel().astype(np.int64)).argmax())


def gt_boxes(plane, labels, L, f, q=0.95, add_margin=5, threshold=None, u32=None):
    """One row: dict(rf, box, threshold, robust) of the crop on ``plane`` masked to ``labels == L``; ``threshold`` None = the
    masked threshold of that label (else the given one, e.g. the all-pixel threshold)."""
    plane = np.asarray(plane)
    labels = np.asarray(labels)
    h, w = plane.shape
    H, W = labels.shape
    if u32 is None:
        u32 = R.upsample(plane, (H, W)).astype(np.float32)
    T = masked_threshold(u32, labels == L, q) if threshold is None else np.float32(threshold)
    if np.isinf(T):
        rf = PB.rf_box(int(f), h, w, H, W)
        box, _ = PB.walk(np.zeros((H, W), bool), rf, add_margin)
        return dict(rf=rf, box=list(box), threshold=T, robust=True)
    return PB.boxes(plane, labels, L - 1, f, q=q, add_margin=add_margin, threshold=T, u32=u32)


def topk_images(values, n):
    """(rows int64 [P, n], values [P, n]) of values [N_img, P]; -1 / inf where a column has fewer than n rows."""
    values = np.asarray(values)
    N, P = values.shape
    idx = np.full((P, n), -1, np.int64)
    val = np.full((P, n), np.inf, values.dtype)
    for p in range(P):
        order = sorted(range(N), key=lambda i: (values[i, p], i))[:n]
        idx[p, :len(order)] = order
        val[p, :len(order)] = values[order, p]
    return idx, val


def nearest_protos(column, n, include=None, window=None):
    """The list of prototypes for one pixel's column of distances [P]."""
    column = np.asarray(column)
    order = sorted(range(column.shape[0]), key=lambda p: (column[p], p))
    keep = set(range(column.shape[0])) if include is None else set(int(p) for p in include)
    if window is not None:
        order = order[:window]
    return [p for p in order if p in keep][:n]
