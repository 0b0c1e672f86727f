"""Time of the group model's packed training route (``forward_packed``: ``msc_pack`` + ONE distance launch + the grouping tail
over MSC's four training outputs, ``SegmentedCrossEntropy``: three launches) against the list route of the same commit (four
feature launches, a forward and two backward launches per map, ``PixelWiseCrossEntropyLoss`` per segment).

    python tools/probes/group_packed_time.py [--seconds 1.0] [--out profiles/group_packed_times.json]

Pairs of variants on the same inputs, alternated call by call in one process after a warm-up, each call between device events,
until every variant has at least --seconds of measured time (tools/probes/msc_packed_time.py's method).  The model is
``PPNetMultiScaleGroup`` on ``spx.MSC`` around a stand-in base that hands out prepared fp32 maps (leaves that take a gradient) by
the size of its input, in training mode, after ``fuse_feature_epilogue(torch.bfloat16)``.
  step      features + forward(return_activations, return_distances) + cross entropy + backward of the mean cross entropy and of
            prepared upstream gradients on the four distance maps, down to the maps, the bank, the group projections and the tail:
            list = ``net(x, ...)`` and ``PixelWiseCrossEntropyLoss(ignore_index=-1, return_correct=True)`` per segment (the
            trainers' setting: a ``nonzero()`` host read each) / packed = ``net.forward_packed(x, ...)`` and ``SegmentedCrossEntropy``
  step_nosync   the same with ``return_correct=False`` on the list route (no host read: the launches alone)
  ce        the cross entropy alone, forward + backward, on prepared logits: the twelve launches of four ``PixelWiseCrossEntropyLoss``
            calls (``return_correct=False``) / the three segmented launches (on the packed logits, nothing concatenated)
Shape: B = 8, C = 256, 41x41 <- {21x21, 31x31}, the group bank of group_scaleproto_pascal.gin (P = 252 in four scales of 64
channels, K = 21, three groups per class: 63 units).  Device kernels per call and their names (torch.profiler) are reported for
the step and the cross entropy.  The figure is the median, the spread the range of the medians of five consecutive fifths.  One
JSON line per shape; a run without a GPU fails."""
import argparse
import collections
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import scaleprotoseg_amd as spx  # noqa: E402

SHAPES = {
    # name: B, S, Cs, P, K, G, grids of the three base outputs
    "pascal_group_p252_s4": (8, 4, 64, 252, 21, 3, [(41, 41), (21, 21), (31, 31)]),
}
FLAGS = dict(return_activations=True, return_distances=True)


class TableBase(nn.Module):
    """Hands out the prepared map whose key is the input's spatial size; ``base`` holds the two convolutions the model's
    constructor reads the width from."""

    def __init__(self, table, channels):
        super().__init__()
        self.base = nn.Sequential(nn.Conv2d(3, channels, 1), nn.Conv2d(channels, channels, 1))
        self.table = table

    def __repr__(self):
        return "DEEPLAB(standin)"

    def forward(self, x):
        return self.table[tuple(x.shape[2:])]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def summary(ts):
    fifth = max(1, len(ts) // 5)
    parts = [median(ts[i:i + fifth]) for i in range(0, fifth * 5, fifth) if ts[i:i + fifth]]
    return {"median_ms": round(median(ts), 4), "spread_ms": round(max(parts) - min(parts), 4), "calls": len(ts)}


def kernels_of(fn):
    """Names of the device kernels one call launches, with their counts (torch.profiler; copies and memsets apart)."""
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    names = collections.Counter()
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            names[e.name[:120]] += 1
    return dict(names)


def alternate(a, b, seconds, warmup):
    for _ in range(warmup):
        a()
        b()
    torch.cuda.synchronize()
    ta, tb, sa, sb = [], [], 0.0, 0.0
    while sa < 1e3 * seconds or sb < 1e3 * seconds:
        ta.append(timed(a))
        tb.append(timed(b))
        sa, sb = sa + ta[-1], sb + tb[-1]
    return summary(ta), summary(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    spx.load_library()
    results = []
    for name, (B, S, Cs, P, K, G, grids) in SHAPES.items():
        gen = torch.Generator().manual_seed(0)
        C = S * Cs
        maps = [torch.randn(B, C, h, w, generator=gen).to(dev).requires_grad_(True) for h, w in grids]
        sizes = [(8, 8), (4, 4), (6, 6)]                                     # x, and x at the scales 0.5 and 0.75
        feats = spx.MSC(TableBase(dict(zip(sizes, maps)), C), scales=[0.5, 0.75])
        torch.manual_seed(1)
        net = spx.PPNetMultiScaleGroup(feats, 64, (P, Cs, 1, 1), [], K, add_on_layers_type="deeplab_simple", patch_classification=True,
                                       num_scales=S, num_groups=G).to(dev).train()
        net.fuse_feature_epilogue(torch.bfloat16)
        x = torch.zeros(B, 3, 8, 8, device=dev)
        seg = grids + [grids[0]]
        g_dist = [(torch.randn(B, P, h, w, generator=gen) * 1e-3).to(dev) for h, w in seg]
        targets = [torch.randint(0, K + 1, (B, h, w), generator=gen).to(dev) for h, w in seg]
        leaves = maps + [net.prototype_vectors, net.last_layer_group.weight] + [gp.weight for gp in net.group_projection]
        one = torch.ones((), device=dev)
        pw_correct = spx.PixelWiseCrossEntropyLoss(ignore_index=-1, return_correct=True)
        pw_plain = spx.PixelWiseCrossEntropyLoss(ignore_index=-1)
        seg_ce = spx.SegmentedCrossEntropy(ignore_index=-1)

        def clear():
            for t in leaves:
                t.grad = None

        def step(route):
            def run():
                clear()
                if route == "packed":
                    out = net.forward_packed(x, **FLAGS)
                    ce = seg_ce([o[0] for o in out], targets).mean
                else:
                    out = net(x, **FLAGS)
                    ce = 0.0
                    for o, t in zip(out, targets):
                        ce = ce + (pw_correct(o[0], t)[0] if route == "list" else pw_plain(o[0], t)) / len(out)
                torch.autograd.backward([ce] + [o[1] for o in out], [one] + g_dist)
            return run

        with torch.no_grad():
            packed_out = net.forward_packed(x)
        base = packed_out[0][0].spx_packed[0].detach().clone().requires_grad_(True)
        lay = packed_out[0][0].spx_packed[1]
        offsets = tuple(lay.offsets) + (lay.M,)
        seg_logits = [t.detach().clone().reshape(B, h, w, K).requires_grad_(True) for t, (h, w) in zip(lay.split_rows(base), seg)]
        labels0 = spx.functional.shifted_labels_i32(lay.pack_labels(targets).reshape(-1), dev)

        def ce(route):
            def run():
                if route == "segmented":
                    base.grad = None
                    spx.segmented_cross_entropy(base, labels0, offsets).mean.backward()
                else:
                    total = 0.0
                    for l, t in zip(seg_logits, targets):
                        l.grad = None
                        total = total + pw_plain(l, t) / len(seg_logits)
                    total.backward()
            return run

        res = {"shape": name, "B": B, "C": C, "S": S, "P": P, "K": K, "G": G, "grids": seg, "M": lay.M}
        res["step_list"], res["step_packed"] = alternate(step("list"), step("packed"), args.seconds, args.warmup)
        res["step_nosync_list"], res["step_nosync_packed"] = alternate(step("list_nosync"), step("packed"), args.seconds, args.warmup)
        res["ce_list"], res["ce_segmented"] = alternate(ce("list"), ce("segmented"), args.seconds, args.warmup)
        for what, fn in (("step_list", step("list")), ("step_packed", step("packed")), ("ce_list", ce("list")),
                         ("ce_segmented", ce("segmented"))):
            names = kernels_of(fn)
            res[what + "_kernels"] = sum(names.values())
            res[what + "_kernel_names"] = names
        print(json.dumps(res), flush=True)
        results.append(res)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
