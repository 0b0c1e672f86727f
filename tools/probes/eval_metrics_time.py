"""Time SegmentationMetrics.update (fused accumulate + top-k launches) against what a user composes today: the two
spx_upsample_argext maps (predicted class, nearest prototype) and torch bincount counting on them.  All sides run in
the same process on the same inputs; each time is the median of --reps event-timed calls after two warm-up calls.

    python tools/probes/eval_metrics_time.py [--shape city|pascal|ade|all] [--reps 20]

Prints one JSON line per (shape, variant) with the median ms, plus the peak extra device memory of one update."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

import scaleprotoseg_amd as spx  # noqa: E402

SHAPES = {  # name: (N, K, P, h, w, H, W, samples per image)
    "city": (1, 19, 228, 129, 257, 1024, 2048, 100),     # scaleproto_cityscapes
    "pascal": (2, 21, 210, 65, 65, 513, 513, 100),       # baseline_pascal
    "ade": (1, 150, 1800, 64, 64, 512, 512, 100),        # scaleproto_ade
}


def median_ms(f, reps):
    for _ in range(2):
        f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def run(name, reps):
    N, K, P, h, w, H, W, S = SHAPES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(N, h, w, K, generator=g) * 3).to(dev)          # [N, h, w, K] as the forward returns it
    dist = (torch.rand(N, P, h, w, generator=g) * 10).to(dev)
    cls = torch.arange(P) % K
    ident = torch.nn.functional.one_hot(cls, K).float()
    pred, _ = spx.upsample_argext(logits.permute(0, 3, 1, 2), (H, W), largest=True)
    ann = torch.randint(0, K + 1, (N, H, W), generator=g).to(dev)
    ann = torch.where(torch.rand(N, H, W, generator=g).to(dev) < 0.8, pred + 1, ann)   # a mostly-right model
    samples = torch.stack([torch.randint(0, H, (N, S), generator=g), torch.randint(0, W, (N, S), generator=g)], 2)
    samples = samples.to(torch.int32).to(dev)
    cls_d = cls.to(dev)
    m = spx.SegmentationMetrics(K, ident, dev)

    def maps():
        p, _ = spx.upsample_argext(logits.permute(0, 3, 1, 2), (H, W), largest=True)
        q, _ = spx.upsample_argext(dist, (H, W), largest=False)
        return p, q

    def composed():
        p, q = maps()
        a = ann.long()
        row = torch.where((a >= 1) & (a <= K), a - 1, torch.full_like(a, K))
        conf = torch.bincount((row * K + p)[a != 0], minlength=(K + 1) * K)
        ok = cls_d[q] == p
        hits = torch.bincount(q[ok], minlength=P)
        return conf, hits

    rows = []
    rows.append(("update (accumulate + top-k)", median_ms(lambda: m.update(logits, ann, dist, samples), reps)))
    rows.append(("update, accumulate only", median_ms(lambda: m.update(logits, ann, dist), reps)))
    rows.append(("update, logits only", median_ms(lambda: m.update(logits, ann), reps)))
    rows.append(("two upsample_argext maps", median_ms(maps, reps)))
    rows.append(("upsample_argext, distances only", median_ms(lambda: spx.upsample_argext(dist, (H, W)), reps)))
    rows.append(("maps + torch bincount counting", median_ms(composed, reps)))
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    m.update(logits, ann, dist, samples)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    for v, ms in rows:
        print(json.dumps({"shape": name, "N": N, "K": K, "P": P, "latent": [h, w], "out": [H, W], "samples": S,
                          "variant": v, "median_ms": round(ms, 4), "reps": reps}), flush=True)
    print(json.dumps({"shape": name, "update_extra_device_bytes": int(extra)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=["all", *SHAPES])
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    for name in (SHAPES if a.shape == "all" else [a.shape]):
        run(name, a.reps)


if __name__ == "__main__":
    main()
