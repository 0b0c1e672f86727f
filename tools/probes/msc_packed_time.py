"""Time of the packed training maps (``msc_pack`` + ONE distance launch over MSC's four training outputs) against the list path (four
feature launches, one distance forward and two backward launches per map).

    python tools/probes/msc_packed_time.py [--seconds 1.0] [--out profiles/msc_packed_times.json]

Pairs of variants on the same inputs, alternated call by call in one process after a warm-up, each call between device events,
until every variant has at least --seconds of measured time.  The model is ``PPNetMultiScale`` on ``spx.MSC`` around a stand-in
base that hands out prepared fp32 maps (leaves that take a gradient) by the size of its input, in training mode, with
``fuse_feature_epilogue(torch.bfloat16)``; the input is 8 x 8, so the input pyramid both paths share is two tiny launches.
  step        ``net(x)`` -> [(logits, distances)] x 4, ``torch.autograd.backward`` with prepared upstream gradients on all eight
              outputs, down to the three maps, the bank and the head:  list (``packed=False``, the parent's code) / packed
  gathered    the same with class-gathered distances: list = ``net(x)`` then ``from_distance_map`` per segment (the P-wide map is
              written and gathered again) / packed = ``net(x, target_labels=[t_0 .. t_3])`` (``ClassDistances`` per segment)
  features    the features alone, forward + backward: ``feats.fused`` (four launches each way) / ``feats.fused_packed`` (one)
Shapes: B = 8, C = 256, 41x41 <- {21x21, 31x31}, K = 21 with P = 210 (one scale of 256 channels) and with the bank of
scaleproto_pascal.gin, P = 252 (four scales of 64 channels).  Device kernels per call and their names (torch.profiler) are
reported for the step: a per-segment full-size zero fill in the packed backward would show there.  The figure is the median,
the spread the range of the medians of five consecutive fifths.  One JSON line per shape; a run without a GPU fails."""
import argparse
import collections
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import scaleprotoseg_amd as spx  # noqa: E402
from scaleprotoseg_amd import _gathered  # noqa: E402

SHAPES = {
    # name: B, S, Cs, P, K, grids of the three base outputs
    "pascal_p210": (8, 1, 256, 210, 21, [(41, 41), (21, 21), (31, 31)]),
    "pascal_p252_s4": (8, 4, 64, 252, 21, [(41, 41), (21, 21), (31, 31)]),
}


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
    for name, (B, S, Cs, P, K, grids) in SHAPES.items():
        gen = torch.Generator().manual_seed(0)
        C = S * Cs
        maps = [torch.randn(B, C, h, w, generator=gen).to(dev).requires_grad_(True) for h, w in grids]
        sizes = [(8, 8), (4, 4), (6, 6)]                                     # x, and x at the scales 0.5 and 0.75
        feats = spx.MSC(TableBase(dict(zip(sizes, maps)), C), scales=[0.5, 0.75])
        torch.manual_seed(1)
        net = spx.PPNetMultiScale(feats, 64, (P, Cs, 1, 1), [], K, add_on_layers_type="deeplab_simple", patch_classification=True,
                                  num_scales=S).to(dev).train()
        x = torch.zeros(B, 3, 8, 8, device=dev)
        seg = grids + [grids[0]]
        g_logits = [(torch.randn(B, h, w, K, generator=gen) * 1e-3).to(dev) for h, w in seg]
        g_dist = [(torch.randn(B, P, h, w, generator=gen) * 1e-3).to(dev) for h, w in seg]
        targets = [torch.randint(0, K + 1, (B, h, w), generator=gen).to(dev) for h, w in seg]
        leaves = maps + [net.prototype_vectors, net.last_layer.weight]
        table = _gathered.class_slot_table(net.prototype_class_identity).to(dev)
        J = int(table.shape[1])
        g_planes = [(torch.randn(B, J, h * w, generator=gen) * 1e-3).to(dev) for h, w in seg]

        def clear():
            for t in leaves:
                t.grad = None

        def step(packed):
            def run():
                clear()
                net.fuse_feature_epilogue(torch.bfloat16, packed=packed)
                out = net(x)
                torch.autograd.backward([o[0] for o in out] + [o[1] for o in out], g_logits + g_dist)
            return run

        def gathered(packed):
            def run():
                clear()
                net.fuse_feature_epilogue(torch.bfloat16, packed=packed)
                if packed:
                    out = net(x, target_labels=targets)
                    planes = [o[1].values for o in out]
                else:
                    out = net(x)
                    planes = [_gathered.from_distance_map(o[1], t, table).planes for o, t in zip(out, targets)]
                torch.autograd.backward([o[0] for o in out] + planes, g_logits + g_planes)
            return run

        M = sum(B * h * w for h, w in seg)
        g_feat = [torch.randn(B, C, h, w, generator=gen).to(dev).to(torch.bfloat16) for h, w in seg]
        g_packed = torch.cat([g.permute(1, 0, 2, 3).reshape(C, -1) for g in g_feat], dim=1).reshape(1, C, 1, M).contiguous()

        def features(packed):
            def run():
                clear()
                if packed:
                    torch.autograd.backward([feats.fused_packed(x, "sigmoid", torch.bfloat16).features], [g_packed])
                else:
                    torch.autograd.backward(feats.fused(x, "sigmoid", torch.bfloat16), g_feat)
            return run

        res = {"shape": name, "B": B, "C": C, "S": S, "P": P, "K": K, "grids": seg, "M": M, "J": J}
        for what, make in (("step", step), ("gathered", gathered), ("features", features)):
            res[what + "_list"], res[what + "_packed"] = alternate(make(False), make(True), args.seconds, args.warmup)
        for what, fn in (("step_list", step(False)), ("step_packed", step(True)), ("gathered_packed", gathered(True))):
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
