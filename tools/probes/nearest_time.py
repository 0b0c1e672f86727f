"""Time of the class-restricted select and of pass 2 of ``nearest_images_to_prototypes`` at the Cityscapes shape (latent 129 x 257 ->
1024 x 2048, P = 228, n = 3): the masked select per 64 rows against the unmasked select of the same 64 planes, the crop chain
(``nearest.gt_crops``: majority, both selects, both crops) of 684 rows spread over 57 winning images of 12 rows each, and the
host formula (the restatement's upsample, percentile over the class and walk, tests/nearest_restatement.py) on a few of the same
rows on this machine's CPU.  Planes and labels as tools/probes/push_boxes_time.py makes them.  Device events around one call,
median of 10 after 2 warm-ups.
python tools/probes/nearest_time.py [host rows, default 3]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

import scaleprotoseg_amd as spx
from push_boxes_time import _planes, _timed
from scaleprotoseg_amd import nearest


def main(host_rows):
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(20250303)
    h, w, H, W, K, patch = 129, 257, 1024, 2048, 19, 128
    R = 64
    planes, peak = _planes(R, h, w, K, gen, dev)
    cells = torch.randint(0, K + 1, (1, -(-H // patch), -(-W // patch)), generator=gen, device=dev)
    labels = cells.repeat_interleave(patch, 1).repeat_interleave(patch, 2)[:, :H, :W].to(torch.uint8).contiguous()
    zero = torch.zeros(R, dtype=torch.int32, device=dev)
    chan = torch.arange(R, dtype=torch.int32, device=dev)
    flat = peak.to(torch.int32)
    major = spx.patch_majority(labels, torch.stack([zero, flat], dim=1), (h, w), K)
    rows = torch.stack([zero, chan, major], dim=1).contiguous()
    share = [(labels[0] == int(m)).float().mean().item() for m in major.tolist()]
    print(f"class share of the image over the {R} rows: mean {sum(share) / R:.3f}, min {min(share):.3f}, max {max(share):.3f}")
    _, t_un, lo, hi = _timed(lambda: spx.high_activation_threshold(planes, (H, W), 0.95))
    print(f"unmasked select, {R} planes: median {t_un:.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
    _, t_m, lo, hi = _timed(lambda: spx.high_activation_threshold_masked(planes, labels, rows, 0.95))
    print(f"masked select, {R} rows (patch majority class): median {t_m:.3f} ms (min {lo:.3f}, max {hi:.3f}); ratio {t_m / t_un:.2f}", flush=True)
    whole = torch.full_like(labels, 3)
    all_rows = torch.stack([zero, chan, torch.full_like(zero, 3)], dim=1).contiguous()
    _, t_w, lo, hi = _timed(lambda: spx.high_activation_threshold_masked(planes, whole, all_rows, 0.95))
    print(f"masked select, {R} rows, every pixel in the class: median {t_w:.3f} ms (min {lo:.3f}, max {hi:.3f}); ratio {t_w / t_un:.2f}", flush=True)
    # pass 2 without the backbone: 57 images x 12 rows
    per, images = 12, 57
    act = planes[:, :per].contiguous()
    c12, f12 = chan[:per].contiguous(), flat[:per].contiguous()

    def pass2():
        out = None
        for _ in range(images):
            out = nearest.gt_crops(act, labels, c12, f12, K)
        return out

    out, t_p, lo, hi = _timed(pass2, warmup=1, reps=5)
    print(f"crop chain, {images} images x {per} rows = {images * per} rows: median {t_p:.1f} ms (min {lo:.1f}, max {hi:.1f}), "
          f"{t_p / images:.3f} ms per image", flush=True)
    one, t_1, lo, hi = _timed(lambda: nearest.gt_crops(act, labels, c12, f12, K))
    print(f"crop chain, one image of {per} rows: median {t_1:.3f} ms (min {lo:.3f}, max {hi:.3f})", flush=True)
    # the host formula on the same rows
    import nearest_restatement as NR
    import overlap_restatement as RS
    import push_boxes_restatement as PB

    lab = labels[0].cpu().numpy()
    pl = planes[0].cpu().numpy()
    rf, cls, thr, thr_gt, box, box_gt = (t.cpu().numpy() for t in one)
    took = []
    for r in range(host_rows):
        t0 = time.perf_counter()
        u32 = RS.upsample(pl[r], (H, W)).astype("float32")
        t1 = time.perf_counter()
        L = NR.patch_majority(lab, PB.rf_box(int(f12[r]), h, w, H, W))
        T = NR.masked_threshold(u32, lab == L)
        t2 = time.perf_counter()
        got = NR.gt_boxes(pl[r], lab, L, int(f12[r]), threshold=T, u32=u32)
        t3 = time.perf_counter()
        took.append((t1 - t0, t2 - t1, t3 - t2))
        same = got["box"] == box_gt[r].tolist()
        print(f"host row {r}: upsample {t1 - t0:.2f} s, majority + masked percentile {t2 - t1:.3f} s, walk (with the robustness "
              f"bookkeeping) {t3 - t2:.2f} s; T_gt host {float(T):.7g} device {float(thr_gt[r]):.7g}; crop equal: {same}", flush=True)
    if took:
        print("host mean per row: " + ", ".join(f"{sum(t[i] for t in took) / len(took):.3f} s" for i in range(3)))


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("nearest_time.py needs an MI355X")
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 3)
