"""Restatement of spx_push_merge (include/spx_hip.h) in plain torch on the CPU: a helper of the single-pass push tests, not
collected by pytest.

Per prototype p, (v, b) = the lexicographic minimum of (values[b, p], b) under fp32 `<` (a NaN is below nothing, so it never
wins); if v < best_value[p], strictly, the row takes v, image0 + b, f = indices[b, p] and the Cs features
x[b, proto_scale[p] * Cs + c, f]; otherwise nothing of the row changes."""
import torch


def new_state(P, Cs):
    return dict(best_value=torch.full((P,), float("inf"), dtype=torch.float32), best_image=torch.full((P,), -1, dtype=torch.int64),
                best_flat=torch.zeros((P,), dtype=torch.int64), best_patch=torch.zeros((P, Cs), dtype=torch.float32))


def merge(state, indices, values, x, proto_scale, image0):
    """Update ``state`` (new_state, or any four tensors of those shapes) in place with one batch.  indices int64 [B, P], values
    fp32 [B, P], x [B, C, H, W] or [B, C, HW] (bf16 or fp32), proto_scale int [P]."""
    B, P = values.shape
    Cs = state["best_patch"].shape[1]
    xs = x.reshape(B, x.shape[1], -1)
    for p in range(P):
        v, bb = float("inf"), -1
        col = values[:, p].tolist()
        for b in range(B):
            if col[b] < v:                       # strict and in image order: the lowest b on ties; False for a NaN
                v, bb = col[b], b
        if bb < 0 or not (v < float(state["best_value"][p])):
            continue
        f = int(indices[bb, p])
        s = int(proto_scale[p])
        state["best_value"][p] = values[bb, p]
        state["best_image"][p] = int(image0) + bb
        state["best_flat"][p] = f
        state["best_patch"][p] = xs[bb, s * Cs:(s + 1) * Cs, f].to(torch.float32)


def merge_all(P, Cs, indices, values, x, proto_scale, batch, image0=0):
    """State after merging images 0 .. N - 1 (indices / values [N, P], x [N, C, H, W]) ``batch`` at a time."""
    state = new_state(P, Cs)
    N = values.shape[0]
    for i in range(0, N, batch):
        merge(state, indices[i:i + batch], values[i:i + batch], x[i:i + batch], proto_scale, image0 + i)
    return state
