"""The reference-recorded cases of the full-resolution map operators, shared by the CPU and GPU tests of each: explanation
maps (tools/gen_explain_golden.py), activation overlap (tools/gen_overlap_golden.py) and push boxes
(tools/gen_push_boxes_golden.py), with what the tests read off a case."""
import functools

import numpy as np
import torch

from support import load_cases, planes_of

EXPLAIN_CASES = load_cases("explanation_maps")
OVERLAP_CASES = load_cases("activation_overlap")
PUSH_BOX_CASES = load_cases("push_boxes")


def weights_of(case):
    """float32 [K, J]: 1 for prototypes, last_layer_group.weight[k, channel of (k, j)] for groups."""
    table = case["table"]
    if str(case["kind"]) == "proto":
        return np.ones(table.shape, np.float32)
    K = table.shape[0]
    return np.stack([case["head"][k, np.maximum(table[k], 0)] for k in range(K)]).astype(np.float32)


def class_planes(case, n, k):
    planes, table = planes_of(case), case["table"]
    return [planes[n, c] if c >= 0 else None for c in table[k]]


def classes_of(case):
    return case["ident"].argmax(1)


# ---- classes at the edges of the bands of output rows ----------------------------------------------------------------------
# (h, w, H, W), the output rows [first, last] of label 1, the pixels that are a class of their own (labels 2, 3, ...) and the
# rows of label `wide` (0 = none).  257 x 50 from 5 x 7: the selects walk the bands [0, 256) and [256, 257).  140 x 70 from
# 129 x 65 (8385 floats, more than a band stages): the selects walk [0, 132) and [132, 140), the explain range pass bands of 32
# rows; the lone pixels sit in the last band and on the first and the last row of a band of either.
BAND_EDGES = {"two_bands_257x50": ((5, 7, 257, 50), (250, 256), [(256, 49), (0, 17), (255, 3)], None),
              "partially_staged_129x65": ((129, 65, 140, 70), (60, 100), [(139, 69), (132, 0), (131, 33), (128, 5), (127, 64)], (30, 40))}
BAND_EDGE_WIDE = 9                # the label of the `wide` rows


@functools.lru_cache(maxsize=None)
def band_edge_case(name):
    """dict: planes fp32 [1, 2, h, w] on the bf16 grid, labels uint8 [1, H, W], lone = the labels of the one-pixel classes.
    Computed once and left unchanged."""
    (h, w, H, W), (y0, y1), spots, wide = BAND_EDGES[name]
    g = np.random.default_rng(H * W)
    planes = torch.from_numpy(g.normal(size=(1, 2, h, w)).astype(np.float32)).to(torch.bfloat16).float().numpy()
    labels = np.zeros((1, H, W), np.uint8)
    labels[0, y0:y1 + 1] = 1
    if wide:
        labels[0, wide[0]:wide[1] + 1] = BAND_EDGE_WIDE
    for i, (y, x) in enumerate(spots):
        labels[0, y, x] = 2 + i
    return dict(planes=planes, labels=labels, lone=list(range(2, 2 + len(spots))))
