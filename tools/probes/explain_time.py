"""Explanation maps of one 10-slot class at 129x257 -> 1024x2048: the three kernels (range + heat through
``activation_heat_maps``, dominant through ``dominant_slot_maps``) against the same maps composed from torch ops on the same
device (F.interpolate bicubic, mask, amin / amax, scale, .to(uint8), argmax), once with blocky labels and once with the class
on every pixel (the most work: every pixel is sampled).  One process; per measurement two warm-up calls, then the median of 10
calls, each between two device events; peak memory above what is allocated before the call; everything measured twice.
python tools/probes/explain_time.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import torch.nn.functional as F

import scaleprotoseg_amd as spx


def measure(name, fn, calls=10):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ts = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    print(f"{name}: median {ts[len(ts) // 2]:.3f} ms (min {ts[0]:.3f}, max {ts[-1]:.3f}) over {calls} calls, peak +{peak:.1f} MiB", flush=True)


def run(tag, act, labels, table, k, J, H, W):
    share = float((labels == k + 1).float().mean())
    rows = torch.tensor([(0, k, j) for j in range(J)])
    rows2 = torch.tensor([(0, k)])
    print(f"{tag}: class {k} covers {100 * share:.1f} % of the image, {J} slots; bytes written: heat {J * H * W}, dominant {H * W}",
          flush=True)

    def torch_heat():
        u = F.interpolate(act[:, table[k]], size=(H, W), mode="bicubic", align_corners=False)[0]      # [J, H, W] fp32
        m = u * (labels[0] == k + 1)
        r = m - m.amin((1, 2), keepdim=True)
        return u, (255 * (r / r.amax((1, 2), keepdim=True))).to(torch.uint8)

    def torch_maps():
        u, heat = torch_heat()
        return heat, torch.where(labels[0] == k + 1, u.argmax(0), 255).to(torch.uint8)

    heat, _ = spx.activation_heat_maps(act, labels, rows, table)
    dom = spx.dominant_slot_maps(act, labels, rows2, table)
    th, td = torch_maps()
    torch.cuda.synchronize()
    print(f"{tag}: against torch: heat bytes differing {int((heat != th).sum())} of {heat.numel()} (largest "
          f"{int((heat.int() - th.int()).abs().max())}), dominant bytes differing {int((dom[0] != td).sum())} of {td.numel()}", flush=True)
    for rep in range(2):
        measure(f"{tag} run {rep}: spx range + heat ({J} rows)", lambda: spx.activation_heat_maps(act, labels, rows, table))
        measure(f"{tag} run {rep}: spx dominant (1 row, {J} slots)", lambda: spx.dominant_slot_maps(act, labels, rows2, table))
        measure(f"{tag} run {rep}: torch heat", torch_heat)
        measure(f"{tag} run {rep}: torch heat + dominant", torch_maps)


def main():
    dev = torch.device("cuda:0")
    h, w, H, W, J, K = 129, 257, 1024, 2048, 10, 19
    g = torch.Generator().manual_seed(1)
    act = (torch.rand(1, K * J, h, w, generator=g) * 4).to(dev)
    cells = torch.randint(0, K + 1, (1, 16, 32), generator=g)
    labels = cells.repeat_interleave(64, 1).repeat_interleave(64, 2).to(torch.uint8).to(dev)
    table = torch.arange(K * J).reshape(K, J)
    k = int(cells.flatten().bincount(minlength=K + 1)[1:].argmax())                  # the class with the most pixels
    run("blocky labels", act, labels, table, k, J, H, W)
    run("one class everywhere", act, torch.full_like(labels, k + 1), table, k, J, H, W)   # every pixel is sampled: the most work


if __name__ == "__main__":
    main()
