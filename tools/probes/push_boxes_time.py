"""Time of the push bounding boxes at the two full-size pushes: 228 rows at 129 x 257 -> 1024 x 2048 (scaleproto_cityscapes.gin)
and 1800 rows at 65 x 65 -> 512 x 512 (scaleproto_ade.gin), thresholds (spx_overlap_thresholds on the rows' planes) and crop
(spx_push_boxes with those thresholds) separately; per shape the typical rows (bump-shaped planes, the patch at the peak, the
class under it) and ONE worst-case row whose crop grows to the whole image (an absent class on a negative plane: every pixel
is a hit, H + W growth steps).  Device events around one call, median of 10 after 2 warm-ups.
python tools/probes/push_boxes_time.py [case ...]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

import scaleprotoseg_amd as spx


def _timed(fn, warmup=2, reps=10):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts = sorted(ts)
    return out, ts[len(ts) // 2], ts[0], ts[-1]


def _planes(R, h, w, K, gen, dev):
    """[1, R, h, w] bump planes in about [0, 1.5] and per plane the flat index of its peak."""
    yy = torch.arange(h, device=dev, dtype=torch.float32).view(1, h, 1)
    xx = torch.arange(w, device=dev, dtype=torch.float32).view(1, 1, w)
    a = torch.zeros(R, h, w, device=dev)
    for _ in range(3):
        cy = torch.rand(R, 1, 1, generator=gen, device=dev) * (h - 1)
        cx = torch.rand(R, 1, 1, generator=gen, device=dev) * (w - 1)
        s = 0.05 + 0.15 * torch.rand(R, 1, 1, generator=gen, device=dev)
        amp = 0.5 + 0.5 * torch.rand(R, 1, 1, generator=gen, device=dev)
        a += amp * torch.exp(-0.5 * (((yy - cy) / (s * h)) ** 2 + ((xx - cx) / (s * w)) ** 2))
    a += 0.02 * torch.rand(R, h, w, generator=gen, device=dev)
    return a.unsqueeze(0).contiguous(), a.reshape(R, -1).argmax(1)


def run(name, R, h, w, H, W, K, patch):
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(20241018)
    planes, peak = _planes(R, h, w, K, gen, dev)
    cells = torch.randint(0, K + 1, (1, -(-H // patch), -(-W // patch)), generator=gen, device=dev)
    labels = cells.repeat_interleave(patch, 1).repeat_interleave(patch, 2)[:, :H, :W].to(torch.uint8).contiguous()
    py = ((peak // w).double() * (H / h)).long().clamp_max(H - 1)
    px = ((peak % w).double() * (W / w)).long().clamp_max(W - 1)
    cls = (labels[0, py, px].long() - 1).clamp_min(0)
    rows = torch.stack([torch.zeros_like(peak), torch.arange(R, device=dev), cls, peak], dim=1).to(torch.int32).contiguous()
    thr, t_med, t_min, t_max = _timed(lambda: spx.high_activation_threshold(planes, (H, W), 0.95))
    print(f"{name}: thresholds of {R} planes {h}x{w} -> {H}x{W}: median {t_med:.3f} ms (min {t_min:.3f}, max {t_max:.3f})", flush=True)
    (rf, box), t_med, t_min, t_max = _timed(lambda: spx.push_bounding_boxes(planes, labels, rows, thresholds=thr))
    grow = ((box[:, 1] - box[:, 0]) - (rf[:, 1] - rf[:, 0]) + (box[:, 3] - box[:, 2]) - (rf[:, 3] - rf[:, 2]) - 20).clamp_min(0).float()
    print(f"{name}: crop of {R} typical rows: median {t_med:.3f} ms (min {t_min:.3f}, max {t_max:.3f}); growth steps per row "
          f"mean {grow.mean().item():.0f}, max {grow.max().item():.0f}", flush=True)
    # the worst case: one row, a negative plane (T <= 0), a class that is in no label
    neg = (planes[:, :1] - 2.0).contiguous()
    thr1 = spx.high_activation_threshold(neg, (H, W), 0.95)
    row1 = torch.tensor([[0, 0, K + 5, (h // 2) * w + w // 2]], dtype=torch.int32, device=dev)
    (rf1, box1), t_med, t_min, t_max = _timed(lambda: spx.push_bounding_boxes(neg, labels, row1, thresholds=thr1))
    assert box1[0].tolist() == [0, H, 0, W], box1
    print(f"{name}: crop of 1 worst-case row (grows to {H}x{W}): median {t_med:.3f} ms (min {t_min:.3f}, max {t_max:.3f})", flush=True)


if __name__ == "__main__":
    cases = [("cityscapes 228 rows", 228, 129, 257, 1024, 2048, 19, 128),
             ("ade 1800 rows", 1800, 65, 65, 512, 512, 150, 64)]
    sel = [int(a) for a in sys.argv[1:]] or range(len(cases))
    if not torch.cuda.is_available():
        sys.exit("push_boxes_time.py needs an MI355X")
    for i in sel:
        run(*cases[i])
