"""Time one batch of the pruning's k-nearest search at the Cityscapes full-image shape (129 x 257 latent, 1024 x 2048
labels, P = 228, S = 4, K = 19, C = 256 fp32 features) against the push's pair as a yardstick.  All variants run in the
same process on the same inputs; each time is the median of --reps event-timed calls after two warm-up calls, divided
by B (ms per image).

    python tools/probes/prune_time.py [--batches 1,8] [--reps 20] [--search N]

Variants per B:
  fused               prune_nearest_from_features (spx_dist_prune_min: the map is never written)
  map                 distance map (proto_head_forward) + prune_nearest_from_map (spx_prune_argmin)
  map + push argmin   distance map + push_masked_argmin (the push's class-masked pair, the yardstick)
  footprint + merge   prune_footprint on the 1024 x 2048 labels + NearestTable.merge (k = 6)
  fused step          fused + footprint + merge: what find_k_nearest_patches_to_prototypes runs per batch
Prints one JSON line per (B, variant).

--search N times the whole search instead, uploads included: find_k_nearest_patches_to_prototypes (k = 6) over N synthetic host
images at that shape with the stand-in backbone of push_single_pass_time.py, per batch size: a host clock around the call,
ending in a device synchronise, one warm-up, then the median (min .. max) of three, and a checksum of the result."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

import scaleprotoseg_amd as spx  # noqa: E402
from scaleprotoseg_amd.prune import NearestTable  # noqa: E402

C, P, S, K, H, W, HF, WF = 256, 228, 4, 19, 129, 257, 1024, 2048


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


def run(B, reps):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    Cs, per = C // S, P // S
    layout = spx.BankLayout(P, 1, S, Cs, tuple((s * per, (s + 1) * per) for s in range(S)))
    x = torch.sigmoid(torch.randn(B, C, H, W, generator=g)).to(dev)
    bank = torch.rand(P, Cs, 1, 1, generator=g).to(dev)
    ident = torch.nn.functional.one_hot(torch.arange(P) % K, K).float().to(dev)
    full = torch.randint(0, K + 1, (B, HF // 32, WF // 32), generator=g)
    full = full.repeat_interleave(32, 1).repeat_interleave(32, 2)                    # blocky labels, 0 = void
    latent = torch.stack([spx.resize_label(full[b].numpy(), (W, H)) for b in range(B)]).to(dev)
    full_m1 = (full - 1).to(torch.int32).to(dev)
    tc = (torch.arange(P) % K).to(torch.int32).to(dev)
    table = NearestTable(P, 6, dev)

    def dmap():
        return spx.proto_head_forward(x, bank, None, layout, want_distances=True, activation="linear")[1]

    def fused():
        return spx.prune_nearest_from_features(x, bank, layout, latent, void_label=0)

    def footprint_merge(keys):
        lab, box = spx.prune_footprint(full_m1, keys, (H, W), tc)
        table.merge(keys, lab, box, W, 0)

    keys = fused()
    rows = [
        ("fused", median_ms(fused, reps)),
        ("map", median_ms(lambda: spx.prune_nearest_from_map(dmap(), latent, void_label=0), reps)),
        ("map + push argmin", median_ms(lambda: spx.push_masked_argmin(dmap(), latent, ident), reps)),
        ("distance map only", median_ms(dmap, reps)),
        ("footprint + merge", median_ms(lambda: footprint_merge(keys), reps)),
        ("fused step", median_ms(lambda: footprint_merge(fused()), reps)),
    ]
    for v, ms in rows:
        print(json.dumps({"B": B, "P": P, "S": S, "K": K, "latent": [H, W], "labels": [HF, WF], "variant": v,
                          "median_ms": round(ms, 4), "ms_per_image": round(ms / B, 4), "reps": reps}), flush=True)


def search(n_images, batches):
    from push_single_pass_time import _Images, _net

    dev = torch.device("cuda:0")
    net = _net(P, K, S, C // S, dev)
    data = _Images(n_images, H * 8, W * 8, K)
    for B in batches:
        ts = []
        for r in range(4):                                                   # call 0 is the warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = spx.find_k_nearest_patches_to_prototypes(data, net, 6, batch_size=B, log=lambda *_: None)
            torch.cuda.synchronize()
            if r:
                ts.append(time.perf_counter() - t0)
        ts.sort()
        print(json.dumps({"variant": "search", "images": n_images, "B": B, "median_s": round(ts[1], 4), "min_s": round(ts[0], 4),
                          "max_s": round(ts[2], 4), "checksum": [int(res.image.sum()), int(res.latent.sum()), int(res.label.sum())]}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--search", type=int, default=0, metavar="N")
    args = ap.parse_args()
    if args.search:
        return search(args.search, [int(b) for b in args.batches.split(",")])
    for B in (int(b) for b in args.batches.split(",")):
        run(B, args.reps)


if __name__ == "__main__":
    main()
