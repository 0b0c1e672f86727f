"""ActivationRegularizers (spatial entropy + sample entropy + l1 norm) forward + backward against KLDLoss forward + backward on the
SAME class-gathered planes, eager, alternating in one process; the whole measurement twice to show the spread.
python tools/probes/act_loss_time.py [case ...]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

import scaleprotoseg_amd as spx
from kld_loss_time import _identity


def run(name, B, P, K, S, H, W, patch, iters=20, rounds=5):
    dev = torch.device("cuda:0")
    ident = _identity(P, K, S)
    per = P // S
    lay = spx.BankLayout(P, K, S, 64, tuple((s * per, (s + 1) * per) for s in range(S)))
    _, J, table = spx.class_gather_table(lay, ident, dev)
    patches = torch.randint(0, K + 1, (B, -(-H // patch), -(-W // patch)), device=dev)
    target = patches.repeat_interleave(patch, 1).repeat_interleave(patch, 2)[:, :H, :W].contiguous()
    vals = (torch.rand(B, J, H * W, device=dev) * 6).requires_grad_(True)
    cd = spx.ClassDistances(vals, (target.reshape(B, -1) - 1).int(), table, (H, W), target=target, target_version=target._version)
    ranges = {s: lay.scale_ranges[s] for s in range(S)}
    act_fn = spx.ActivationRegularizers(ident, S, ranges, 1.0, 1.0, 1.0)
    kld_fn = spx.KLDLoss(ident, S, ranges)
    losses = {"ActivationRegularizers": lambda: act_fn(cd, target)[0], "KLDLoss": lambda: kld_fn(cd, target)}

    def step(fn):
        vals.grad = None
        loss = fn()
        loss.backward()
        return loss

    for fn in losses.values():
        for _ in range(3):
            step(fn)
    torch.cuda.synchronize()
    for rep in range(2):
        best = {k: [] for k in losses}
        for _ in range(rounds):                      # alternate the two losses, `iters` steps each
            for k, fn in losses.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    loss = step(fn)
                e1.record()
                torch.cuda.synchronize()
                best[k].append(e0.elapsed_time(e1) / iters)
        for k, ts in best.items():
            ts = sorted(ts)
            print(f"{name} [{B},{J},{H * W}] run {rep}: {k} fwd+bwd median {ts[len(ts) // 2]:.3f} ms (min {ts[0]:.3f}, max {ts[-1]:.3f}) "
                  f"over {rounds} x {iters} steps", flush=True)


if __name__ == "__main__":
    cases = [("north star 1024x2048 P=190 S=1", 1, 190, 19, 1, 1024, 2048, 64),
             ("cityscapes crops 10x65x65 P=228 S=4", 10, 228, 19, 4, 65, 65, 16),
             ("native 129x257 P=228 S=4", 1, 228, 19, 4, 129, 257, 16)]
    sel = [int(a) for a in sys.argv[1:]] or range(len(cases))
    for i in sel:
        run(*cases[i])
