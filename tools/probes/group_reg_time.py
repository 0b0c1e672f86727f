"""Cost of the weight-side regularisers (GroupRegularizers, csrc/spx_reg.hip) inside a captured training step.

    python tools/probes/group_reg_time.py [--replays 60]

Workloads (drop-in modules, fused cross entropy, bf16 features, one process, one GPU):
  city_group   group phase, Cityscapes bank (228 prototypes, 19 classes, G = 3), crop step 10 x 65 x 65
  ade_group    group phase, ADE bank (1800 prototypes, 150 classes, G = 3), 2 x 65 x 65
  city_proto   prototype phase, Cityscapes bank, 10 x 65 x 65, with the masked L1 of last_layer
Each step (forward + loss + backward) is captured with graphs.capture_step, without and with the regularisers; the time is
the median of --replays event-timed replays.  The yardstick is the same terms computed the reference's way (per-class
loops with a host read per class, segmentation/model/loss.py:351-464 and the L1 of the training modules) in eager mode on
the same GPU, forward + backward, median of 10 calls.  The kernels each variant adds are listed from one eager step under
torch.profiler.  Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
from collections import Counter

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import scaleprotoseg_amd as spx  # noqa: E402
from scaleprotoseg_amd.graphs import capture_step  # noqa: E402
from scaleprotoseg_amd.model_multiscale_group import PPNetMultiScale as GroupNet  # noqa: E402

WEIGHTS = dict(group_ent=0.05, crs_ent_group=0.0, scale_max=0.0, l1=1e-3)      # group_scaleproto_cityscapes.gin


class BB(nn.Module):
    def __init__(self, ch):
        super().__init__()
        self.base = nn.Sequential(nn.Conv2d(3, ch, 1), nn.Conv2d(ch, ch, 1))

    def __repr__(self):
        return "MSC(standin)"


def make(kind, dev):
    torch.manual_seed(0)
    mk = dict(add_on_layers_type="deeplab_simple", patch_classification=True, num_scales=4)
    if kind == "city_group":
        B, K, net = 10, 19, GroupNet(BB(256), 64, (228, 64, 1, 1), [], 19, num_groups=3, **mk)
    elif kind == "ade_group":
        B, K, net = 2, 150, GroupNet(BB(256), 64, (1800, 64, 1, 1), [], 150, num_groups=3, **mk)
    else:
        B, K, net = 10, 19, spx.PPNetMultiScale(BB(256), 64, (228, 64, 1, 1), [], 19, **mk)
    net.add_on_layers = nn.Sequential()
    net = net.to(dev)
    x = torch.sigmoid(torch.randn(B, 256, 65, 65, device=dev)).bfloat16()
    tgt = torch.randint(0, K + 1, (B, 65, 65), device=dev)
    return net, x, tgt


def step_fn(net, x, tgt, reg):
    ce = spx.PixelWiseCrossEntropyLoss(ignore_index=-1)
    params = [p for p in net.parameters() if p.requires_grad]

    def step():
        for p in params:
            p.grad = None
        logits, _ = net.forward_from_conv_features(x, ce_target=tgt)
        loss = ce(logits, tgt)
        if reg is not None:
            loss = loss + reg(logits)[0]
        loss.backward()
        return loss.detach()

    return step


def replay_median(graph, n):
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def kernels_of(step):
    from torch.profiler import ProfilerActivity, profile

    step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    return Counter({e.key: e.count for e in prof.key_averages() if e.device_time_total > 0 and e.device_type.name != "CPU"})


def reference_style_terms(net, w, group):
    """The terms as the reference computes them: a class loop with host reads (ident sums, argmax().item(), nonzero)."""
    ident = net.prototype_class_identity
    if not group:
        return w["l1"] * (net.last_layer.weight * (1 - torch.t(ident))).norm(p=1)
    G, eps = net.num_groups, 1e-5
    ents, cegs, maxes = [], [], []
    for k in range(net.num_classes):
        if ident[:, k].sum() == 0:
            continue
        Wj = net.group_projection[net.group_class_identity[:, k].argmax().item() // G].weight
        for g in range(G):
            ents.append(-torch.sum(Wj[g] * torch.log(Wj[g] + eps)) / torch.log(torch.tensor(Wj.shape[1], device=Wj.device)))
        for i in range(G):
            for j in range(G):
                if i != j:
                    cegs.append(-torch.sum(Wj[i] * torch.log(torch.clamp(Wj[j], eps))))
        prev = 0
        for s in range(net.num_scales):
            lo, hi = net.scale_num_prototypes[s]
            n = len(torch.nonzero(ident[lo:hi, k]).flatten().cpu())
            if n == 0:
                continue
            maxes.append(torch.mean(torch.max(Wj[:, prev:prev + n], dim=1).values))
            prev += n
    l1 = (net.last_layer_group.weight * (1 - torch.t(net.group_class_identity))).norm(p=1)
    return (w["l1"] * l1 + w["crs_ent_group"] * -torch.stack(cegs).mean() + w["scale_max"] * -torch.stack(maxes).mean()
            + w["group_ent"] * torch.stack(ents).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=60)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    spx.load_library()
    for kind in ("city_group", "ade_group", "city_proto"):
        net, x, tgt = make(kind, dev)
        group = kind.endswith("group")
        w = WEIGHTS if group else dict(l1=1e-4)
        reg = spx.GroupRegularizers(net, **w)
        res = {"workload": kind}
        kern = {}
        for name, r in (("without", None), ("with", reg)):
            step = step_fn(net, x, tgt, r)
            kern[name] = kernels_of(step)
            graph, _ = capture_step(step, warmup=2)
            res[f"{name}_ms"] = round(replay_median(graph, args.replays), 4)
            del graph
        res["added_ms"] = round(res["with_ms"] - res["without_ms"], 4)
        added = kern["with"] - kern["without"]
        res["added_kernels"] = sum(added.values())
        res["added_kernel_names"] = {k[:90]: v for k, v in added.items()}
        # yardstick: the reference-style eager terms (forward + backward of the terms alone)
        if group:
            net.prototype_class_identity = net.prototype_class_identity.to(dev)
            net.group_class_identity = net.group_class_identity.to(dev)
        else:
            net.prototype_class_identity = net.prototype_class_identity.to(dev)
        ts = []
        for i in range(12):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            reference_style_terms(net, w, group).backward()
            e1.record()
            e1.synchronize()
            if i >= 2:
                ts.append(e0.elapsed_time(e1))
        ts.sort()
        res["reference_style_eager_terms_ms"] = round(ts[len(ts) // 2], 4)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
