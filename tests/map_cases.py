"""The reference-recorded cases of the full-resolution map operators, shared by the CPU and GPU tests of each: explanation
maps (tools/gen_explain_golden.py), activation overlap (tools/gen_overlap_golden.py) and push boxes
(tools/gen_push_boxes_golden.py), with what the tests read off a case."""
import numpy as np

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
