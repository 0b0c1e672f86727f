"""Failure cases at the evaluation shapes: ``predict_label_maps`` with ``conf`` (one launch) against what the library offered
before it - ``upsample_argext`` + a torch look-up + a torch per-image bincount - on the same inputs, alternated in one run after
warm-up; ``failure_table``; and the paired heat maps of one case (12 prototype planes per class, 24 rows).
Shapes: Cityscapes (N = 2, 129x257 -> 1024x2048, K = 19) and ADE (N = 2, 65x65 -> 512x512, K = 150).
One process; per measurement two warm-up calls, then the median of 10 calls, each between two device events; peak memory above
what is allocated before the call; bytes written counted from the shapes; everything measured twice.
python tools/probes/failure_time.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

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


def run(tag, N, h, w, H, W, K, J, dev):
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(N, h, w, K, generator=g).to(dev)
    cells = torch.randint(0, K + 1, (N, H // 64, W // 64), generator=g)
    labels = cells.repeat_interleave(64, 1).repeat_interleave(64, 2).to(torch.uint8).to(dev)
    id_map = torch.randperm(256, generator=g)[:K].to(torch.uint8).to(dev)
    conf = torch.zeros(N, K + 1, K, dtype=torch.int64, device=dev)
    out = torch.empty(N, H, W, dtype=torch.uint8, device=dev)
    chan = logits.permute(0, 3, 1, 2)

    def fused():
        return spx.predict_label_maps(logits, labels=labels, id_map=id_map, out=out, conf=conf)

    def composed():
        idx, _ = spx.upsample_argext(chan, (H, W), largest=True)                        # int64 index + fp32 value per pixel
        pred = id_map[idx]
        lab = labels.to(torch.int64).reshape(N, -1)
        row = torch.where((lab >= 1) & (lab <= K), lab - 1, torch.full_like(lab, K)) * K + idx.reshape(N, -1)
        row = row + torch.arange(N, device=dev)[:, None] * ((K + 1) * K)
        return pred, torch.bincount(row[lab != 0], minlength=N * (K + 1) * K).view(N, K + 1, K)   # (boolean indexing synchronises)

    conf.zero_()
    p0, c0 = fused()
    p1, c1 = composed()
    torch.cuda.synchronize()
    assert torch.equal(p0, p1) and torch.equal(c0, c1), f"{tag}: the fused pass and the composition disagree"
    print(f"{tag}: fused against composed: pred equal {bool(torch.equal(p0, p1))}, conf equal {bool(torch.equal(c0, c1))}; bytes written: "
          f"fused {N * H * W} (pred) + counters, composed {N * H * W * 12} (index + value) + {N * H * W} (pred) + "
          f"{N * H * W * 8 * 2} (row keys, selected keys)", flush=True)
    fc = torch.zeros(N, K + 1, K, dtype=torch.int64, device=dev) + c0
    # one failure case: the J planes of two classes over the pixels of the first, a range per plane (prototypes)
    act = (torch.rand(N, 2 * J, h, w, generator=g) * 4).to(dev)
    a = int(cells[0].flatten().bincount(minlength=K + 1)[1:].argmax())
    rows = torch.tensor([(0, c, a, c) for c in range(2 * J)])
    print(f"{tag}: class {a} covers {100 * float((labels[0] == a + 1).float().mean()):.1f} % of image 0; heat bytes written {2 * J * H * W}", flush=True)
    for rep in range(2):
        measure(f"{tag} run {rep}: predict_label_maps with conf (fused)", fused)
        measure(f"{tag} run {rep}: upsample_argext + look-up + bincount (composed)", composed)
        measure(f"{tag} run {rep}: predict_label_maps, bytes only", lambda: spx.predict_label_maps(logits, (H, W), id_map=id_map, out=out))
        measure(f"{tag} run {rep}: failure_table", lambda: spx.failure_table(fc, 0.5))
        measure(f"{tag} run {rep}: paired_heat_maps ({2 * J} rows)", lambda: spx.paired_heat_maps(act, labels, rows, 2 * J))


def main():
    dev = torch.device("cuda:0")
    run("cityscapes", 2, 129, 257, 1024, 2048, 19, 12, dev)
    run("ade", 2, 65, 65, 512, 512, 150, 12, dev)


if __name__ == "__main__":
    main()
