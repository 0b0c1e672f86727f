"""Time of the multi-scale input fusion (csrc/spx_msc.hip) against the stock sequence it replaces.

    python tools/probes/msc_time.py [--seconds 1.0] [--out profiles/msc_times.json]

Two variants on the same inputs, alternated call by call in one process after a warm-up, each call between device events, until
every variant has at least --seconds of measured time:
  stock   ``F.interpolate`` x2 -> ``torch.stack`` -> ``torch.max(dim=0)`` -> ``torch.sigmoid`` (-> ``.to(bfloat16)``): what the
          reference's MSC plus ``add_on_layers`` (and the distance kernel's input cast) run
  fused   ``spx.msc_max(maps, "sigmoid", torch.bfloat16)``: one launch
Shapes: pascal_eval B=2, C=256, 65x65 <- {33x33, 49x49} (forward; the number of device kernels of each variant is counted with
torch.profiler); pascal_train B=8, C=256, 41x41 <- {21x21, 31x31} (forward + backward to all three maps); cityscapes_k1 B=8,
C=256, 129x257, one map (sigmoid -> bf16; the share of the 8 TB/s HBM peak is reported).  Algorithmic bytes are counted from the
shapes: every map read once, the output written once, one byte per element more where the index is written (and, in the
backward, g, index and y read once and every gradient written once).  The figure is the median, the spread the range of the
medians of five consecutive fifths.  One JSON line per shape; a run without a GPU fails."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import scaleprotoseg_amd as spx  # noqa: E402

SHAPES = {
    # name: B, C, sizes of the maps, backward
    "pascal_eval": (2, 256, [(65, 65), (33, 33), (49, 49)], False),
    "pascal_train": (8, 256, [(41, 41), (21, 21), (31, 31)], True),
    "cityscapes_k1": (8, 256, [(129, 257)], False),
}
HBM_PEAK = 8.0e12


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
    return {"median_ms": round(median(ts), 4), "spread_ms": round(max(parts) - min(parts), 4), "calls": len(ts)}


def kernels_of(fn):
    """Device kernels one call launches (torch.profiler)."""
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
               and "memset" not in e.name.lower())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    spx.load_library()
    results = []
    for name, (B, C, sizes, backward) in SHAPES.items():
        g = torch.Generator().manual_seed(0)
        maps = [torch.randn(B, C, h, w, generator=g).to(dev).requires_grad_(backward) for h, w in sizes]
        H, W = sizes[0]
        go = torch.randn(B, C, H, W, generator=g).to(dev).to(torch.bfloat16)

        def stock():
            up = [maps[0]] + [F.interpolate(m, size=(H, W), mode="bilinear", align_corners=False) for m in maps[1:]]
            z = torch.max(torch.stack(up), dim=0)[0] if len(up) > 1 else up[0]
            y = torch.sigmoid(z).to(torch.bfloat16)
            return torch.autograd.grad(y, maps, go) if backward else y

        def fused():
            y = spx.msc_max(maps, activation="sigmoid", dtype=torch.bfloat16)
            return torch.autograd.grad(y, maps, go) if backward else y

        for _ in range(args.warmup):
            stock()
            fused()
        torch.cuda.synchronize()
        ts, tf, total_s, total_f = [], [], 0.0, 0.0
        while total_s < 1e3 * args.seconds or total_f < 1e3 * args.seconds:
            ts.append(timed(stock))
            tf.append(timed(fused))
            total_s, total_f = total_s + ts[-1], total_f + tf[-1]
        n_out, n_in = B * C * H * W, sum(B * C * h * w for h, w in sizes)
        esz = 4
        nbytes = n_in * esz + n_out * 2 + (n_out if backward and len(sizes) > 1 else 0)
        if backward:
            nbytes += n_out * (2 + 1 + 2) + n_in * esz
        res = {"shape": name, "B": B, "C": C, "maps": sizes, "backward": backward, "stock": summary(ts), "fused": summary(tf),
               "algorithmic_bytes": nbytes, "stock_kernels": kernels_of(stock), "fused_kernels": kernels_of(fused)}
        res["fused_share_of_hbm_peak"] = round(nbytes / (res["fused"]["median_ms"] * 1e-3) / HBM_PEAK, 4)
        if not backward:
            res["max_difference"] = (stock().float() - fused().float()).abs().max().item()
        print(json.dumps(res), flush=True)
        results.append(res)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
