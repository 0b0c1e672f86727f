"""Part consistency / stability at the Cityscapes shape: one image of 1024 x 2048, latent 129 x 257, 190 prototypes of 19 classes
(10 slots each), M = 5, synthetic blocky labels and parts.  Per image: the time of each kernel group (components, thresholds in
both modes, presence with the labelling and thresholds given, the counters) and of ``PartConsistency.update``; and the thresholds
beside the same definition in stock torch ops on the same GPU (nearest ``F.interpolate``, mask, ``torch.quantile`` per plane).  The
labelling has no stock torch counterpart on the GPU and is measured alone.
One process; per measurement two warm-up calls, then the median of 10 calls, each between two device events; peak memory above
what is allocated before the call, beside the declared workspaces.  Writes the table as Markdown.
python tools/probes/parts_time.py [output.md]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import torch.nn.functional as F

import scaleprotoseg_amd as spx
from scaleprotoseg_amd import _lib, parts as PT

LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


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
    say(f"| {name} | {ts[len(ts) // 2]:.3f} | {ts[0]:.3f} | {ts[-1]:.3f} | {peak:.1f} |")
    return ts[len(ts) // 2]


def main():
    dev = torch.device("cuda:0")
    N, h, w, H, W, K, J, M, q = 1, 129, 257, 1024, 2048, 19, 10, 5, 0.8
    P = K * J
    g = torch.Generator().manual_seed(1)
    cells = torch.randint(0, K + 1, (N, H // 128, W // 128), generator=g)
    labels = cells.repeat_interleave(128, 1).repeat_interleave(128, 2).to(torch.uint8).to(dev)
    pcells = torch.randint(0, M + 1, (N, H // 32, W // 32), generator=g)
    parts = pcells.repeat_interleave(32, 1).repeat_interleave(32, 2).to(torch.int32).to(dev)
    d = (4 * torch.rand(N, P, h, w, generator=g)).to(dev)
    act = torch.log((d + 1) / (d + 1e-4))
    table = torch.arange(P).view(K, J)
    lib = _lib.load()

    comp = spx.part_components(labels, parts, M, num_classes=K)
    ncomp = int((comp.count > 0).sum())
    say("# Part consistency / stability: times at the Cityscapes shape")
    say()
    say(f"One image {H} x {W}, latent {h} x {w}, {P} prototypes of {K} classes ({J} slots each), M = {M}, q = {q}; labels in blocks of "
        f"128 x 128, parts in blocks of 32 x 32: {ncomp} components, {int(labels.unique().numel())} label values.  Device events, two "
        "warm-up calls, median of 10 calls; peak = the allocator's peak above what was allocated before the call.")
    say()
    say(f"Declared workspaces: components {lib.spx_part_components_workspace_bytes(N, H, W) / 2 ** 20:.1f} MiB (24 bytes per pixel, also "
        f"the result), thresholds {lib.spx_part_thresholds_workspace_bytes(N, K, h, w) / 2 ** 20:.1f} MiB; outputs: totals "
        f"{N * K * M * 3 * 8} bytes, thresholds {N * K * J * 4} bytes, table {N * K * J * (M + 1)} bytes.")
    say()
    say("| measurement | median ms | min ms | max ms | peak MiB |")
    say("|---|---|---|---|---|")

    m = spx.PartConsistency(K, table, M, dev, q=q)
    x = PT._Inputs(act, labels, parts, m.slot_table_host, dev, "counters")
    thr = PT._thresholds(lib, x, m.slot_table, None, q, 1)
    tab, valid = PT._presence(lib, x, m.slot_table, None, M, comp, thr)

    def fold():
        _lib.check(lib.spx_part_fold_consistency(_lib.ptr(tab), _lib.ptr(valid), _lib.ptr(m.slot_table), N, P, K, J, M, _lib.ptr(m._buf),
                                                 _lib.stream_ptr()))

    def stock(mode):
        up = F.interpolate(act, size=(H, W), mode="nearest")
        out = torch.empty(K, J, device=dev)
        for k in range(K):
            mask = labels[0] == k + 1
            u = up[0, k * J:(k + 1) * J] * mask
            for j in range(J):
                if mode == "image":
                    out[k, j] = torch.quantile(u[j].flatten(), q)
                else:
                    nz = u[j][u[j] != 0]                         # (boolean indexing synchronises)
                    out[k, j] = torch.quantile(nz, q) if nz.numel() else float("inf")
        return out

    for rep in range(2):
        measure(f"run {rep}: spx_part_components (memset, tile, merge, flatten)", lambda: spx.part_components(labels, parts, M, num_classes=K))
        measure(f"run {rep}: spx_part_thresholds, nonzero ({K * J} planes)", lambda: PT._thresholds(lib, x, m.slot_table, None, q, 1))
        measure(f"run {rep}: spx_part_thresholds, image", lambda: PT._thresholds(lib, x, m.slot_table, None, q, 0))
        measure(f"run {rep}: spx_part_presence (labelling and thresholds given)", lambda: PT._presence(lib, x, m.slot_table, None, M, comp, thr))
        measure(f"run {rep}: spx_part_fold_consistency", fold)
        measure(f"run {rep}: PartConsistency.update (all of the above)", lambda: m.update(act, labels, parts))
        measure(f"run {rep}: stock torch thresholds, image (interpolate, mask, quantile per class)", lambda: stock("image"), calls=5)
        measure(f"run {rep}: stock torch thresholds, nonzero (boolean indexing, quantile per plane)", lambda: stock("nonzero"), calls=5)
    same = stock("image")
    mine = PT._thresholds(lib, x, m.slot_table, None, q, 0)[0]
    present = torch.tensor([bool((labels[0] == k + 1).any()) for k in range(K)], device=dev)
    diff = (same - mine)[present].abs().max().item()
    say()
    say(f"Largest difference between the stock image-mode thresholds and the kernel's over the classes present: {diff:.3g} (torch's "
        "nearest index and its quantile arithmetic are its own; the bit-exact check is against tests/consistency_restatement.py).")
    say()
    say("Not measured: multi-image batches, the stability path (two threshold and presence passes over one labelling), hardware "
        "counters, and the host-side reference itself (cv2 is not available).")
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "profiles", "parts_summary.md")
    with open(out, "w") as fp:
        fp.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
