"""Cost of the simplex re-projection that ends every optimizer step of the group phase, alone.

    python tools/probes/simplex_time.py [--reps 300]

Two variants on the same weights, alternated call by call in one process:
  loop   the per-class formula with the result bound as a new storage (DataParallelStep's default:
         ``w.data = projection_simplex_sort(w.data)`` for every class)
  fused  ``projection_simplex_sort_(weights)``: one launch per 192 tensors, in place (csrc/spx_simplex.hip)
Shapes: cityscapes 19 x [3, 12], ade 150 x [3, 12], ragged 19 x [3, n_j] with n_j in 3..12 (a bank after pruning).
Each call is timed by device events around it (enqueue + execution, ended by an event synchronise) after a warm-up; the figure
is the median over --reps calls, the spread the range of the medians of five consecutive fifths of the calls.  The launches
of one call are counted under torch.profiler.  Prints one JSON line per shape."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

import scaleprotoseg_amd as spx  # noqa: E402

SHAPES = {
    "cityscapes": [(3, 12)] * 19,
    "ade": [(3, 12)] * 150,
    "ragged": [(3, 3 + (7 * j) % 10) for j in range(19)],
}


def launches(fn):
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_time_total > 0 and e.device_type.name != "CPU")


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
    return {"median_ms": round(median(ts), 4), "spread_ms": round(max(parts) - min(parts), 4),
            "fifths_ms": [round(p, 4) for p in parts]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    spx.load_library()
    for name, shapes in SHAPES.items():
        g = torch.Generator().manual_seed(0)
        init = [torch.rand(s, generator=g) for s in shapes]
        loop_ws = [torch.nn.Parameter(w.to(dev)) for w in init]
        fused_ws = [torch.nn.Parameter(w.to(dev)) for w in init]

        def loop():
            for w in loop_ws:
                w.data = spx.projection_simplex_sort(w.data)

        def fused():
            spx.projection_simplex_sort_(fused_ws)

        res = {"shape": name, "tensors": len(shapes), "loop_launches": launches(loop), "fused_launches": launches(fused)}
        for _ in range(args.warmup):
            loop()
            fused()
        torch.cuda.synchronize()
        t_loop, t_fused = [], []
        for _ in range(args.reps):
            t_loop.append(timed(loop))
            t_fused.append(timed(fused))
        res["loop"], res["fused"] = summary(t_loop), summary(t_fused)
        res["max_abs_difference"] = max((a.detach() - b.detach()).abs().max().item() for a, b in zip(loop_ws, fused_ws))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
