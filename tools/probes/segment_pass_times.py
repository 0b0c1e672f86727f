"""Per-pass times of the segment passes (csrc/spx_kld.hip, csrc/spx_actloss.hip) through the C ABI, on the shapes of
kld_loss_time.py / act_loss_time.py: KLD max, sum-exp, pair sums, gradient; activation losses pass A, pass B, backward.
Every pass is launched alone between two events, `iters` times after a warm-up; the line gives the median and the extremes in us.
Select the library with SPX_LIB_OVERRIDE to compare two builds (alternate the processes: A/B/A/B/A/B).
python tools/probes/segment_pass_times.py [tag]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

import scaleprotoseg_amd as spx
from kld_loss_time import _identity
from scaleprotoseg_amd import _lib
from scaleprotoseg_amd import loss as L


def timed(fn, iters=30, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def run(tag, name, B, P, K, S, H, W, patch):
    dev = torch.device("cuda:0")
    lib = _lib.load()
    ident = _identity(P, K, S)
    per = P // S
    lay = spx.BankLayout(P, K, S, 64, tuple((s * per, (s + 1) * per) for s in range(S)))
    _, J, table = spx.class_gather_table(lay, ident, dev)
    g = torch.Generator(device=dev).manual_seed(H * W + patch)
    patches = torch.randint(0, K + 1, (B, -(-H // patch), -(-W // patch)), device=dev, generator=g)
    target = patches.repeat_interleave(patch, 1).repeat_interleave(patch, 2)[:, :H, :W].contiguous()
    v = torch.rand(B, J, H * W, device=dev, generator=g) * 6
    lab = (target.reshape(B, -1) - 1).int().contiguous()
    HW, s, p = H * W, _lib.stream_ptr(), _lib.ptr
    out = {}

    # KLD: one valid sequence for the tables, then every pass alone on the same buffers (the integer tables only grow)
    a_fx, counts, lse, scale = L._kld_segment_passes(lib, v, lab, K, W, s)
    keys = torch.zeros(B * K * J, dtype=torch.int32, device=dev)
    cnt, rng = torch.zeros(B * K, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    ssum = torch.zeros(B * K * J, dtype=torch.int64, device=dev)
    out["kld max"] = timed(lambda: _lib.check(lib.spx_kld_segment_max(p(v), p(lab), B, J, HW, W, K, p(keys), p(cnt), p(rng), s)))
    out["kld sum-exp"] = timed(lambda: _lib.check(lib.spx_kld_segment_sumexp(p(v), p(lab), B, J, HW, W, K, p(keys), p(ssum), s)))
    out["kld pair sums"] = timed(lambda: _lib.check(lib.spx_kld_pair_sums(p(v), p(lab), B, J, HW, W, K, p(lse), p(scale), p(a_fx), s)))
    A, cf = torch.rand(B * K * J * J, device=dev), torch.rand(B * K * J * J, device=dev)
    grad = torch.empty_like(v)
    out["kld gradient"] = timed(lambda: _lib.check(lib.spx_kld_backward(p(v), p(lab), B, J, HW, K, p(lse), p(A), p(cf), None, p(grad), s)))

    # activation losses: the three terms, l1, log activation
    ranges = {q: lay.scale_ranges[q] for q in range(S)}
    sid = L.slot_scale_table(table, S, ranges).to(dev)
    cfg = {"K": K, "W": W, "mode": 1, "terms": 7, "norm_type": 0, "epsilon": 1e-4, "weights": (1.0, 1.0, 1.0)}
    d = L._act_desc(v, lab, sid, cfg)
    ws = torch.zeros((lib.spx_actloss_workspace_bytes(C.byref(d)) // 8,), dtype=torch.int64, device=dev)
    coef = torch.empty((B * K, 6, J), dtype=torch.float32, device=dev)
    res = torch.empty((7,), dtype=torch.float32, device=dev)
    _lib.check(lib.spx_actloss_segment_max(C.byref(d), p(ws), s))
    _lib.check(lib.spx_actloss_segment_sums(C.byref(d), p(ws), s))
    _lib.check(lib.spx_actloss_finish(C.byref(d), p(ws), p(coef), p(res), s))
    gt = torch.ones(1, device=dev)
    out["act pass A"] = timed(lambda: _lib.check(lib.spx_actloss_segment_max(C.byref(d), p(ws), s)))
    out["act pass B"] = timed(lambda: _lib.check(lib.spx_actloss_segment_sums(C.byref(d), p(ws), s)))
    out["act backward"] = timed(lambda: _lib.check(lib.spx_actloss_backward(C.byref(d), p(coef), p(gt), None, p(grad), s)))
    for k, (med, lo, hi) in out.items():
        print(f"{tag} | {name} [{B},{J},{HW}] | {k}: median {med:.1f} us (min {lo:.1f}, max {hi:.1f})", flush=True)


if __name__ == "__main__":
    tag = sys.argv[1] if len(sys.argv) > 1 else (os.environ.get("SPX_LIB_OVERRIDE") or "default")
    run(tag, "2 Mpx 1024x2048 P=190", 1, 190, 19, 1, 1024, 2048, 64)
    run(tag, "crops 10x65x65 P=228", 10, 228, 19, 4, 65, 65, 16)
