"""Times of the single-pass batched push (profiles/push_single_pass_summary.md), one process, device events.

merge: spx_push_merge alone at the two full-size pushes - Cityscapes (P = 228, S = 4, Cs = 64, 129 x 257, B in 1 / 8 / 32) and ADE
       (P = 1800, 65 x 65, B in 8 / 32) - once when every row improves (a fresh table) and once when none does (the same batch
       merged again at a later image index), beside the fused minimum of the same batch (spx_dist_push_min).  Two warm-ups,
       then the median of 10 calls.
push:  the whole push_prototypes_multiscale over 64 synthetic images at the Cityscapes shape with a stand-in backbone (average
       pool by 8 and two 1x1 convolutions), batch_size None (the two-pass path) and 1 / 8 / 32: wall time around a device
       synchronise (one warm-up, median of 3) and the number of conv_features calls.
stages: the single pass's loop with a synchronise and a host clock after every stage, summed over the runs: where the wall time
       goes (upload, device stack, conv_features, labels, minima, merge), and for batch_size 8 also the variant that stacks the
       run on the host and uploads it in one copy, which the driver does not use.
python tools/probes/push_single_pass_time.py [merge] [push] [stages] [--images N]"""
import copy
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
import torch.nn as nn

import scaleprotoseg_amd as spx
from scaleprotoseg_amd import push as push_mod


class _Standin(nn.Module):
    def __init__(self, ch, stride=8):
        super().__init__()
        self.base = nn.Sequential(nn.Conv2d(3, ch, 1), nn.Conv2d(ch, ch, 1))
        self.pool = nn.AvgPool2d(stride)

    def __repr__(self):
        return "MSC(standin)"

    def forward(self, x):
        return self.base(self.pool(x))


def _net(P, K, S, Cs, dev):
    torch.manual_seed(0)
    net = spx.PPNetMultiScale(_Standin(S * Cs), 64, (P, Cs, 1, 1), [], K, add_on_layers_type="deeplab_simple",
                              patch_classification=True, num_scales=S)
    net.add_on_layers = nn.Sigmoid()
    return net.to(dev).eval()


def _timed(fn, warmup=2, reps=10):
    """fn(i) for call i; device events around each timed call."""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ts = []
    for i in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(warmup + i)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def merge_cost(name, P, K, S, Cs, H, W, batches, dev):
    net = _net(P, K, S, Cs, dev)
    gen = torch.Generator(device=dev).manual_seed(20241019)
    scale = torch.tensor(push_mod.proto_scale_table(P, S), dtype=torch.int32, device=dev)
    for B in batches:
        conv = torch.rand(B, S * Cs, H, W, generator=gen, device=dev)
        labels = torch.randint(0, K + 1, (B, H, W), generator=gen, device=dev)
        out = []
        t_min = _timed(lambda i: out.append(push_mod.push_run_minima(net, conv, labels, 0)))
        idx, val = out[-1]
        fresh = [spx.PushTable(P, Cs, dev) for _ in range(12)]
        t_all = _timed(lambda i: fresh[i].merge(idx, val, conv, scale, 0))
        assert bool((fresh[0].best_image >= 0).all())
        full = fresh[0]
        t_none = _timed(lambda i: full.merge(idx, val, conv, scale, B * (i + 1)))
        assert torch.equal(full.best_image, fresh[1].best_image) and torch.equal(full.best_patch, fresh[1].best_patch)
        fmt = lambda t: f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"                      # noqa: E731
        print(f"merge | {name} | P={P} {H}x{W} B={B} | fused minimum {fmt(t_min)} ms | merge, every row improves {fmt(t_all)} ms | "
              f"merge, none improves {fmt(t_none)} ms", flush=True)
        del conv, labels, fresh, full, out


class _Images:
    convert_targets = None

    def __init__(self, n, h, w, K, seed=1):
        g = torch.Generator().manual_seed(seed)
        self.items = []
        for _ in range(n):
            img = torch.randn(3, h, w, generator=g)
            t = torch.randint(0, K + 1, (-(-h // 64), -(-w // 64)), generator=g).repeat_interleave(64, 0).repeat_interleave(64, 1)
            self.items.append((img, t[:h, :w].numpy().astype(np.uint8)))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def whole_push(n_images, dev, reps=3):
    P, K, S, Cs = 228, 19, 4, 64
    net0 = _net(P, K, S, Cs, dev)
    data = _Images(n_images, 129 * 8, 257 * 8, K)
    results = {}
    for bs in (None, 1, 8, 32):
        ts, calls, state = [], 0, None
        for r in range(reps + 1):
            net = copy.deepcopy(net0)
            n_calls = []
            orig = net.conv_features
            net.conv_features = lambda x, orig=orig, n_calls=n_calls: n_calls.append(1) or orig(x)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = push_mod.push_prototypes_multiscale(data, net, log=lambda *_: None, batch_size=bs)
            torch.cuda.synchronize()
            if r:                                                            # call 0 is the warm-up
                ts.append(time.perf_counter() - t0)
            calls, state = len(n_calls), (out[0].cpu(), net.prototype_vectors.detach().cpu())
        ts = sorted(ts)
        results[bs] = state
        print(f"push | {n_images} images 129x257 P={P} | batch_size={bs} | wall {ts[len(ts) // 2]:.3f} s ({ts[0]:.3f} .. {ts[-1]:.3f}) | "
              f"conv_features calls {calls}", flush=True)
    same = {bs: bool(torch.equal(results[bs][0], results[None][0])) for bs in (1, 8, 32)}
    print(f"push | winners equal to the two-pass path's: {same} (the stand-in's convolutions may round differently per batch shape)",
          flush=True)


def stage_times(n_images, dev):
    """Where a single pass spends its wall time: the loop of push_single_pass restated with a device synchronise and a host
    clock after every stage (so the stages cannot overlap, and the sum exceeds the push's own time), summed over all runs."""
    from scaleprotoseg_amd.scan import batches
    from scaleprotoseg_amd.utils import resize_label

    P, K, S, Cs = 228, 19, 4, 64
    net = _net(P, K, S, Cs, dev)
    data = _Images(n_images, 129 * 8, 257 * 8, K)
    scale = torch.tensor(push_mod.proto_scale_table(P, S), dtype=torch.int32, device=dev)
    names = ("host stack", "upload", "device stack", "conv_features", "labels (resize + stack)", "minima", "merge")
    for bs, host_stack in ((1, False), (8, False), (32, False), (8, True)):
        for rep in range(2):                                                 # pass 0 is the warm-up
            acc = dict.fromkeys(names, 0.0)
            table = spx.PushTable(P, Cs, dev)

            def lap(name, t0):
                torch.cuda.synchronize()
                acc[name] += time.perf_counter() - t0
                return time.perf_counter()

            with torch.no_grad():
                for run in batches(data, range(len(data)), bs):
                    t = time.perf_counter()
                    if host_stack:                                           # the variant the driver does NOT use
                        x = torch.stack([img for _, img, _ in run])
                        t = lap("host stack", t)
                        x = x.to(dev)
                        t = lap("upload", t)
                    else:                                                    # push_single_pass: image by image, stacked on the device
                        parts = [img.to(dev) for _, img, _ in run]
                        t = lap("upload", t)
                        x = torch.stack(parts)
                        t = lap("device stack", t)
                    conv = net.conv_features(x).detach().contiguous()
                    t = lap("conv_features", t)
                    labels = torch.stack([resize_label(np.asarray(tg), (conv.shape[3], conv.shape[2])) for _, _, tg in run])
                    t = lap("labels (resize + stack)", t)
                    idx, val = push_mod.push_run_minima(net, conv, labels, 0)
                    t = lap("minima", t)
                    push_mod.push_run_merge(table, idx, val, conv, scale, run[0][0])
                    t = lap("merge", t)
        print(f"stages | {n_images} images batch_size={bs}{' (run stacked on the host, then one upload)' if host_stack else ''} | " + " | ".join(f"{k} {1e3 * v:.1f} ms" for k, v in acc.items())
              + f" | sum {1e3 * sum(acc.values()):.1f} ms", flush=True)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("push_single_pass_time.py needs an MI355X")
    args = sys.argv[1:]
    n_images = int(args[args.index("--images") + 1]) if "--images" in args else 64
    parts = [a for a in args if a in ("merge", "push", "stages")] or ["merge", "push", "stages"]
    dev = torch.device("cuda:0")
    if "merge" in parts:
        merge_cost("cityscapes", 228, 19, 4, 64, 129, 257, (1, 8, 32), dev)
        merge_cost("ade", 1800, 150, 4, 64, 65, 65, (8, 32), dev)
    if "push" in parts:
        whole_push(n_images, dev)
    if "stages" in parts:
        stage_times(n_images, dev)
