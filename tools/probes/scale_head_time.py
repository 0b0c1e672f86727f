"""Forward + backward time of the cross-scale aggregation op (csrc/spx_scale_agg.hip), alone.

    python tools/probes/scale_head_time.py [--reps 100] [--out profiles/scale_head_times.json]

Two variants on the same inputs, alternated call by call in one process:
  kernel  ``spx.scale_aggregate`` (similarity on load, s on the fp32 matrix pipe, combine in the epilogue; backward recomputes s)
  einsum  the similarity as torch code, ``torch.einsum("bphw,pc->bchw")`` and the elementwise combine, with torch autograd
(The reference's literal [B, Pn, Cs, H, W] broadcast does not fit in memory at these shapes.)
Shapes: cityscapes B=1, Cs=64, Pn=48, 129 x 257; ade B=1, Cs=64, Pn=375, 64 x 64.  Modes "sum" and "mult", distances under the log
similarity, fp32 x.  Each call (forward + backward of all three gradients) is timed by device events around it, ended by an event
synchronise, after a warm-up; the figure is the median over --reps calls, the spread the range of the medians of five consecutive
fifths.  Peak memory of one call is reported beside it.  One JSON line per (shape, mode); a run without a GPU fails."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

import scaleprotoseg_amd as spx  # noqa: E402

SHAPES = {"cityscapes": (1, 64, 48, 129, 257), "ade": (1, 64, 375, 64, 64)}
EPS = 1e-4


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def summary(ts):
    fifth = max(1, len(ts) // 5)
    parts = [median(ts[i:i + fifth]) for i in range(0, fifth * 5, fifth) if ts[i:i + fifth]]
    return {"median_ms": round(median(ts), 4), "spread_ms": round(max(parts) - min(parts), 4)}


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    spx.load_library()
    results = []
    for name, (B, Cs, Pn, H, W) in SHAPES.items():
        g = torch.Generator().manual_seed(0)
        x = torch.sigmoid(torch.randn(B, Cs, H, W, generator=g)).to(dev).requires_grad_(True)
        d = (torch.rand(B, Pn, H, W, generator=g) * 4).to(dev).requires_grad_(True)
        p = torch.rand(Pn, Cs, generator=g).to(dev).requires_grad_(True)
        go = torch.randn(B, Cs, H, W, generator=g).to(dev)
        for mode in ("sum", "mult"):
            def kernel():
                out = spx.scale_aggregate(x, d, p, mode=mode, epsilon=EPS)
                return torch.autograd.grad(out, (x, d, p), go)

            def einsum():
                a = torch.log((d + 1) / (d + EPS))
                s = torch.einsum("bphw,pc->bchw", a, p)
                out = (x + s) / 2 if mode == "sum" else torch.sqrt(x * s)
                return torch.autograd.grad(out, (x, d, p), go)

            for _ in range(args.warmup):
                kernel()
                einsum()
            torch.cuda.synchronize()
            tk, te = [], []
            for _ in range(args.reps):
                tk.append(timed(kernel))
                te.append(timed(einsum))
            gk, ge = kernel(), einsum()
            res = {"shape": name, "B": B, "Cs": Cs, "Pn": Pn, "H": H, "W": W, "mode": mode, "kernel": summary(tk), "einsum": summary(te),
                   "kernel_peak_bytes": peak(kernel), "einsum_peak_bytes": peak(einsum), "broadcast_bytes": B * Pn * Cs * H * W * 4,
                   "max_rel_difference": max(((a - b).abs().max() / b.abs().max()).item() for a, b in zip(gk, ge))}
            print(json.dumps(res), flush=True)
            results.append(res)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
