"""Device kernels of one forward + backward of the class-gathered losses, per input form, counted with torch.profiler, and a
checksum of the gradient's bytes, on the Cityscapes crop shape (B = 10, 65 x 65, P = 228, K = 19, S = 4; 3 groups per class for the group form).  Public API only, so the
same file runs in a checkout of an earlier commit for a comparison.
python tools/probes/gathered_launch_counts.py"""
import hashlib
import os
import sys
from collections import Counter

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from torch.profiler import ProfilerActivity, profile

import scaleprotoseg_amd as spx
from kld_loss_time import _identity

dev = torch.device("cuda:0")
B, P, K, S, H, W, G = 10, 228, 19, 4, 65, 65, 3
ident = _identity(P, K, S)
per = P // S
lay = spx.BankLayout(P, K, S, 64, tuple((s * per, (s + 1) * per) for s in range(S)))
_, J, table = spx.class_gather_table(lay, ident, dev)
ranges = {s: lay.scale_ranges[s] for s in range(S)}
gen = torch.Generator(device=dev).manual_seed(3)
patches = torch.randint(0, K + 1, (B, 5, 5), device=dev, generator=gen)
target = patches.repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :H, :W].contiguous()
clone = target.clone()
vals = (torch.rand(B, J, H * W, device=dev, generator=gen) * 6).requires_grad_(True)
cd = spx.ClassDistances(vals, (target.reshape(B, -1) - 1).int(), table, (H, W), target=target, target_version=target._version)
dist = (torch.rand(B, P, H, W, device=dev, generator=gen) * 6).requires_grad_(True)
act = torch.rand(B * H * W, P, device=dev, generator=gen).requires_grad_(True)
gci = torch.eye(K).repeat_interleave(G, dim=0)
groups = [torch.randn(B * H * W, G, device=dev, generator=gen).requires_grad_(True) for _ in range(K)]
kld = spx.KLDLoss(ident, S, ranges)
kld_group = spx.KLDLossGroup(ident, gci, G)
reg = spx.ActivationRegularizers(ident, S, ranges, 1.0, 1.0, 1.0)

PATHS = {      # name: (call, leaves)
    "KLDLoss, ClassDistances, its own target": (lambda: kld(cd, target), [vals]),
    "KLDLoss, ClassDistances, cloned target": (lambda: kld(cd, clone), [vals]),
    "KLDLoss, full map": (lambda: kld(dist, target), [dist]),
    "KLDLossGroup, list": (lambda: kld_group(groups, target), groups),
    "ActivationRegularizers, ClassDistances": (lambda: reg(cd, target)[0], [vals]),
    "ActivationRegularizers, activation tensor": (lambda: reg(act, target)[0], [act]),
}

for name, (fn, leaves) in PATHS.items():
    for _ in range(2):
        fn().backward()
    torch.cuda.synchronize()
    for t in leaves:
        t.grad = None
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        loss = fn()
        loss.backward()
        torch.cuda.synchronize()
    kernels, copies = Counter(), 0
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            if "memcpy" in e.name.lower():
                copies += 1
            else:
                kernels[e.name] += 1
    mine = sum(n for k, n in kernels.items() if k.startswith("spx") or "spx_" in k)
    digest = hashlib.sha1(b"".join(t.grad.cpu().numpy().tobytes() for t in leaves)).hexdigest()[:12]
    print(f"{name}: {sum(kernels.values())} kernels ({mine} of the library), {copies} copies; loss {loss.item():.9g}, "
          f"gradient bytes {digest}", flush=True)
    if "-v" in sys.argv:
        for k, n in sorted(kernels.items()):
            print(f"    {n} x {k[:110]}")
