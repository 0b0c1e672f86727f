"""Training-batch preparation at the Cityscapes training shape: B = 8 sources of 1024 x 2048 (uint8 HWC images, uint8 labels), window
513 x 513, scales (0.5, 1.5) drawn by ``draw_augmentation(random.Random(0), ...)``, one 65 x 65 latent grid, fp32 output.

* the launch alone: the arguments of one ``prepare_batch`` call are kept and ``spx_batch_prepare`` is enqueued 200 times back to
  back between two device events (the table is on the device, nothing else runs); median of 7 such windows, two warm-up windows;
* ``prepare_batch`` as a caller sees it (host validation, packing, the table's upload, launch), one call between two events, median
  of 20, new crop origins per call: with a temporary table per call and with the caller's ``BatchTable``;
* the bytes the launch has to read and write, computed from the shapes and the drawn parameters, over the launch's time, as a
  fraction of the HBM peak (8.0 TB/s spec; 6.3 TB/s is what a copy reaches).  The 64 MiB of sources fit the 256 MiB Infinity Cache, so
  repeated launches read from it: the figure is a rate of the kernel, not evidence of HBM traffic;
* the host-to-device bytes per batch of the uint8 route and of the reference's float64 route, computed from the shapes;
* ``resize_labels`` of [8, 513, 513] int64 device labels to 65 x 65 against the host loop it replaces (device -> host copy, PIL-rule
  ``resize_label`` per sample, stack, upload), host clock around a device synchronise, median of 10.
Writes the table as Markdown between two marker lines of the output file; what the file holds outside them is kept.
python tools/probes/batch_time.py [output.md]"""
import ctypes as C
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

import scaleprotoseg_amd as spx
from scaleprotoseg_amd import _lib, batch as BT
from scaleprotoseg_amd.utils import resize_label

LINES = []
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
HBM_SPEC, HBM_COPY = 8.0e12, 6.3e12
BEGIN = "<!-- tools/probes/batch_time.py writes from here -->"
END = "<!-- to here -->"


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def events(fn, calls, warm=2, per=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / per)
    return median(ts)


def wall(fn, calls, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return median(ts)


class Spy:
    """The library with the argument block of every spx_batch_prepare call kept."""

    def __init__(self, lib):
        self.lib, self.kept = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if name != "spx_batch_prepare":
            return fn

        def call(args, stream):
            self.kept.append(_lib.SpxBatch.from_buffer_copy(args._obj))
            return fn(args, stream)
        return call


def needed_bytes(params, h, w, Hc, Wc, grid):
    """Bytes one launch must move: the source rectangle under each window (3 image bytes and 1 label byte per source pixel), and
    the outputs (12 bytes of fp32 image and 8 of int64 label per window pixel, 8 + 4 per latent pixel)."""
    read = 0
    for (hs, ws), (y0, x0), _ in params:
        rows = min(Hc, hs - y0) * h / hs
        cols = min(Wc, ws - x0) * w / ws
        read += rows * cols * 4
    write = len(params) * (Hc * Wc * (12 + 8) + grid[0] * grid[1] * 12)
    return read, write


def main():
    dev = torch.device("cuda:0")
    B, h, w, Hc, Wc, grid, scales = 8, 1024, 2048, 513, 513, (65, 65), (0.5, 1.5)
    g = torch.Generator().manual_seed(1)
    images = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).to(dev) for _ in range(B)]
    labels = [torch.randint(0, 20, (h // 64, w // 64), generator=g).repeat_interleave(64, 0).repeat_interleave(64, 1).to(torch.uint8).to(dev)
              for _ in range(B)]
    rng = random.Random(0)
    params = [spx.draw_augmentation(rng, (h, w), (Hc, Wc), scales) for _ in range(B)]
    kw = dict(window=(Hc, Wc), mean=MEAN, std=STD, grids=[grid])

    say("# Training-batch preparation: times at the Cityscapes training shape")
    say()
    say(f"B = {B} sources of {h} x {w} (uint8 HWC images, uint8 labels), window {Hc} x {Wc}, scales {scales}, one {grid[0]} x {grid[1]} "
        f"grid, fp32 image, int64 window labels, int64 and shifted int32 latent labels.  Drawn scaled sizes: "
        f"{', '.join(f'{p.scaled[0]} x {p.scaled[1]}' for p in params)}.  Measured on {torch.cuda.get_device_name(0)}.")
    say()
    say("| measurement | median ms | min ms | max ms |")
    say("|---|---|---|---|")

    spy = Spy(_lib.load())
    real_load = _lib.load
    _lib.load = lambda: spy
    batch = spx.prepare_batch(images, labels, params, **kw)
    _lib.load = real_load
    args = spy.kept[0]
    lib, stream = real_load(), _lib.stream_ptr()

    def launches():
        for _ in range(200):
            lib.spx_batch_prepare(C.byref(args), stream)

    t_launch = events(launches, 7, per=200)
    say("| spx_batch_prepare, the launch alone (200 back to back, per launch) | %.4f | %.4f | %.4f |" % t_launch)
    fresh = iter(range(10 ** 6))

    def new_crop(**more):
        n = next(fresh)
        p = [spx.AugmentParams(q.scaled, (q.origin[0], (q.origin[1] + n) % (max(q.scaled[1], Wc) - Wc + 1)), q.flip) for q in params]
        spx.prepare_batch(images, labels, p, **kw, **more)

    t_call = events(new_crop, 20)
    say("| prepare_batch, a temporary table per call | %.3f | %.3f | %.3f |" % t_call)
    own = spx.BatchTable(dev, B, args.n_index + 4096)
    t_own = events(lambda: new_crop(table=own), 20)
    say("| prepare_batch, the caller's BatchTable (table=) | %.3f | %.3f | %.3f |" % t_own)
    u8 = events(lambda: new_crop(dtype=torch.uint8), 20)
    say("| prepare_batch, uint8 image output | %.3f | %.3f | %.3f |" % u8)

    dev_labels = batch.labels
    t_dev = events(lambda: spx.resize_labels(dev_labels, grids=[grid]), 20)
    say(f"| resize_labels [{B}, {Hc}, {Wc}] int64 -> {grid[0]} x {grid[1]} (events) | %.3f | %.3f | %.3f |" % t_dev)
    t_dev_wall = wall(lambda: spx.resize_labels(dev_labels, grids=[grid]), 10)
    say("| the same, host clock around a synchronise | %.3f | %.3f | %.3f |" % t_dev_wall)

    def host_loop():
        return torch.stack([resize_label(t.cpu().numpy(), (grid[1], grid[0])) for t in dev_labels]).to(dev)

    t_host = wall(host_loop, 10)
    say("| the host loop it replaces (copy back, resize_label per sample, stack, upload), host clock | %.3f | %.3f | %.3f |" % t_host)
    assert torch.equal(host_loop(), spx.resize_labels(dev_labels, grids=[grid])[0]) and torch.equal(batch.latent[0], host_loop())

    read, write = needed_bytes(params, h, w, Hc, Wc, grid)
    rate = (read + write) / (t_launch[0] * 1e-3)
    say()
    say(f"Bytes one launch has to move, from the shapes and the drawn parameters: {read / 2 ** 20:.1f} MiB read (the source rectangle under "
        f"each window, 3 image bytes and 1 label byte per source pixel), {write / 2 ** 20:.1f} MiB written (12 + 8 bytes per window pixel, 12 "
        f"per latent pixel).  Over the launch's median time: {rate / 1e12:.2f} TB/s = {100 * rate / HBM_SPEC:.0f} % of the 8.0 TB/s HBM "
        f"spec ({100 * rate / HBM_COPY:.0f} % of the 6.3 TB/s a copy reaches).  The sources ({B * h * w * 4 / 2 ** 20:.0f} MiB) fit the "
        "256 MiB Infinity Cache and the same launch is repeated, so the reads are served from it; the writes are not.")
    say()
    up_u8 = B * h * w * (3 + 1) + B * 80 + 4 * args.n_index
    up_f64 = B * (3 * Hc * Wc * 8 + Hc * Wc * 8)
    say(f"Host-to-device bytes per batch, computed from the shapes (not measured): uint8 route {up_u8 / 2 ** 20:.1f} MiB (whole sources, "
        f"3 + 1 bytes per pixel, and the {B * 80 + 4 * args.n_index} bytes of descriptors and tables); the reference's route "
        f"{up_f64 / 2 ** 20:.1f} MiB (float64 window image, 24 bytes per pixel, and int64 window labels), after which the step casts the "
        "image to fp32 on the device and copies the labels back for the latent resize.")
    say()
    say("Not measured: the reference's host path itself (cv2 is not available), hardware counters, other window sizes, and a data "
        "loader feeding the device.")
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "profiles", "batch_summary.md")
    old = open(out).read() if os.path.exists(out) else ""
    body = BEGIN + "\n" + "\n".join(LINES) + "\n" + END + "\n"
    if BEGIN in old and END in old:                                  # the hand-written sections around the markers stay
        body = old[:old.index(BEGIN)] + body + old[old.index(END) + len(END) + 1:]
    with open(out, "w") as fp:
        fp.write(body)


if __name__ == "__main__":
    main()
