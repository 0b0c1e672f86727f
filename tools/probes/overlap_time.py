"""Time ActivationOverlap.update against the same metric written with torch ops on the GPU: per present class, chunks of its
planes through F.interpolate(mode="bicubic"), torch.quantile, boolean sums.  Both sides run in the same process on the same
inputs, alternating; each time is the median of --reps event-timed calls after two warm-up calls; peak extra device memory of
one call of each is recorded, and the two sets of counters are compared.

    python tools/probes/overlap_time.py [--shape city|ade|all] [--reps 10] [--out profiles/overlap_probe.jsonl]

Prints (and with --out also writes) one JSON line per shape."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import scaleprotoseg_amd as spx  # noqa: E402

SHAPES = {  # name: (K, slots per class, h, w, H, W, classes present, channels per torch chunk)
    "city": (19, 12, 129, 257, 1024, 2048, 14, 4),      # scaleproto_cityscapes: P = 228, one validation image
    "ade": (150, 12, 65, 65, 512, 512, 10, 12),         # scaleproto_ade: P = 1800, one crop
}


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def peak_extra(f):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    f()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def torch_overlap(planes, labels, table, q, chunk, inter, area, images):
    """The definition with torch ops; reads the present classes back to the host, as a user's loop would."""
    N = planes.shape[0]
    H, W = labels.shape[1:]
    K, J = table.shape
    for n in range(N):
        present = torch.unique(labels[n]).tolist()
        for k in range(K):
            if k + 1 not in present:
                continue
            images[k] += 1
            ch = table[k][table[k] >= 0]
            masks = []
            for c0 in range(0, len(ch), chunk):
                u = F.interpolate(planes[n:n + 1, ch[c0:c0 + chunk]], size=(H, W), mode="bicubic", align_corners=False)[0]
                t = torch.quantile(u.flatten(1), q, dim=1)
                masks.append(u > t[:, None, None])
            m = torch.cat(masks).flatten(1).to(torch.float32)              # [J, H*W] of 0 / 1: exact sums below 2^24 per product
            both = (m @ m.t()).to(torch.int64)
            area[k, :len(ch)] += torch.diagonal(both)
            inter[k, :len(ch), :len(ch)] += torch.triu(both, diagonal=1)


def run(name, reps):
    K, J, h, w, H, W, npresent, chunk = SHAPES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    P = K * J
    base = torch.rand(1, K, 1, h, w, generator=g) * 1.5 + 0.05
    d = (base + 0.3 * torch.rand(1, K, J, h, w, generator=g)).reshape(1, P, h, w)
    act = torch.log((d + 1) / (d + 1e-4)).to(dev)
    labels = (torch.randint(0, npresent + 1, (1, H // 64, W // 64), generator=g).repeat_interleave(64, 1).repeat_interleave(64, 2)).to(dev)
    table = torch.arange(P).view(K, J)
    m = spx.ActivationOverlap(K, table, dev)
    t_inter = torch.zeros(K, J, J, dtype=torch.int64, device=dev)
    t_area = torch.zeros(K, J, dtype=torch.int64, device=dev)
    t_images = torch.zeros(K, dtype=torch.int64, device=dev)
    table_d = table.to(dev)
    ours = lambda: m.update(act, labels)
    theirs = lambda: torch_overlap(act, labels, table_d, 0.95, chunk, t_inter, t_area, t_images)
    thr = lambda: spx.high_activation_threshold(act, (H, W))
    for _ in range(2):
        ours(), theirs(), thr()
    torch.cuda.synchronize()
    peak_ours, peak_theirs = peak_extra(ours), peak_extra(theirs)      # after the warm-up, before the counters that are compared
    m.reset()
    t_inter.zero_(), t_area.zero_(), t_images.zero_()
    a, b, c = [], [], []
    for _ in range(reps):
        a.append(timed(ours))
        b.append(timed(theirs))
        c.append(timed(thr))
    med = lambda v: sorted(v)[len(v) // 2]
    res = m.compute()
    d_inter = int((res.inter - t_inter.cpu()).abs().max())
    d_area = int((res.area - t_area.cpu()).abs().max())
    images_equal = bool(torch.equal(res.images, t_images.cpu()))
    line = {"shape": name, "K": K, "slots": J, "P": P, "latent": [h, w], "out": [H, W], "classes_present": int((res.images > 0).sum()),
            "reps": reps, "update_ms": round(med(a), 3), "update_ms_min_max": [round(min(a), 3), round(max(a), 3)],
            "thresholds_only_ms": round(med(c), 3), "torch_ms": round(med(b), 3), "torch_ms_min_max": [round(min(b), 3), round(max(b), 3)],
            "update_peak_extra_bytes": peak_ours, "torch_peak_extra_bytes": peak_theirs,
            "full_CHW_bytes": P * H * W * 4, "total_iou": res.total, "images_equal": images_equal,
            "max_abs_counter_difference_over_reps": {"inter": d_inter, "area": d_area},
            "mean_area_per_update": float(res.area.double().mean() / reps)}
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=["all", *SHAPES])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("overlap_time.py needs an AMD GPU")
    lines = [run(name, a.reps) for name in (SHAPES if a.shape == "all" else [a.shape])]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
