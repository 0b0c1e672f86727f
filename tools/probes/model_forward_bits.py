"""Probe: every path of ``forward_from_conv_features`` of the two model classes (the case list of tests/test_model_forward_cpu.py)
on real tensors, forward and backward, printed as one line per output and per gradient - name, dtype, shape, sha1 of the bytes -
and one line per case with the C-ABI calls it made, in order.  Two revisions of the package compute the same thing where their
outputs are equal line for line:

    python tools/probes/model_forward_bits.py --root <tree holding scaleprotoseg_amd/> > a.txt      (one process per revision)
    python tools/probes/model_forward_bits.py --compare a.txt b.txt                                 (no GPU)

Both revisions should load the same built library (``SPX_LIB_OVERRIDE``)."""
import hashlib
import os
import sys


def compare(a, b):
    la, lb = (open(p).read().splitlines() for p in (a, b))
    differ = [(x, y) for x, y in zip(la, lb) if x != y]
    for x, y in differ[:20]:
        print(f"- {x}\n+ {y}")
    n = {kind: sum(l.startswith(kind) for l in la) for kind in ("tensor", "calls")}
    print(f"{len(la)} and {len(lb)} lines ({n['tensor']} tensors, {n['calls']} call logs), {len(differ) + abs(len(la) - len(lb))} differ")
    return 1 if differ or len(la) != len(lb) or not la else 0


if len(sys.argv) == 4 and sys.argv[1] == "--compare":
    raise SystemExit(compare(sys.argv[2], sys.argv[3]))
ROOT = os.path.abspath(sys.argv[2]) if len(sys.argv) == 3 and sys.argv[1] == "--root" else \
    os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import scaleprotoseg_amd as spx  # noqa: E402
import scaleprotoseg_amd._lib as L  # noqa: E402
import scaleprotoseg_amd.model_multiscale as MM  # noqa: E402
import scaleprotoseg_amd.model_multiscale_group as MG  # noqa: E402
from scaleprotoseg_amd.loss import ClassDistances  # noqa: E402
from scaleprotoseg_amd.msc import PackedLayout, PackedMaps  # noqa: E402

assert os.path.dirname(os.path.abspath(spx.__file__)) == os.path.join(ROOT, "scaleprotoseg_amd"), spx.__file__


class LoggingLib:
    """What ``_lib.load()`` returns from here on: the library, with the name of every entry point called kept in ``calls``."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.calls.append(name)
            return fn(*args)

        return call


LIB = L._lib = LoggingLib(L.load())

P, K, S, CS, G = 40, 5, 4, 16, 3
B, GRIDS = 2, ((3, 4), (2, 3))
MODES = (dict(), dict(return_activations=True), dict(return_activations=True, return_distances=True))
LIMITS = {"narrow": {}, "wide": {(MM, "MAX_FUSED_HEAD_ROWS"): K - 1}, "fused": {}, "wide_tail": {(MG, "MAX_FUSED_TAIL_CLASSES"): K - 1},
          "product": {(MG, "MAX_FUSED_HEAD_ROWS"): G * K - 1}}
CASES = [("proto", b) for b in ("narrow", "wide")] + [("group", b) for b in ("fused", "wide_tail", "product")]
dev = torch.device("cuda:0")


class Backbone(nn.Module):
    def __init__(self, ch):
        super().__init__()
        self.base = nn.Sequential(nn.Conv2d(3, ch, 1), nn.Conv2d(ch, ch, 1))

    def __repr__(self):
        return "MSC(standin)"

    def forward(self, x):
        return x


def make(kind, **kw):
    torch.manual_seed(0)
    kw = dict(add_on_layers_type="deeplab_simple", patch_classification=True, num_scales=S, **kw)
    if kind == "proto":
        return spx.PPNetMultiScale(Backbone(S * CS), 64, (P, CS, 1, 1), [], K, **kw).to(dev)
    net = spx.PPNetMultiScaleGroup(Backbone(S * CS), 64, (P, CS, 1, 1), [], K, num_groups=G, **kw)
    with torch.no_grad():
        for gp in net.group_projection:
            gp.weight.copy_(torch.softmax(torch.randn(gp.weight.shape), dim=1))
        net.last_layer_group.weight.add_(0.1 * torch.randn(net.last_layer_group.weight.shape))
    return net.to(dev)


def show(name, t):
    if t is None:
        print(f"tensor {name}: None")
        return
    raw = t.detach().contiguous().reshape(-1).cpu().view(torch.uint8).numpy().tobytes()
    print(f"tensor {name}: {str(t.dtype)[6:]} {tuple(t.shape)} {hashlib.sha1(raw).hexdigest()}")


def run(name, kind, branch, net, x, fwd):
    """One forward and backward: ``fwd()`` -> a tuple, or a list of one tuple per segment."""
    saved = {key: getattr(*key) for key in LIMITS[branch]}
    for key, v in LIMITS[branch].items():
        setattr(*key, v)
    try:
        LIB.calls.clear()
        out = fwd()
        outs, grads = [], []
        g = torch.Generator().manual_seed(1)
        for k, tup in enumerate(out if isinstance(out, list) else [out]):
            for j, t in enumerate(tup):
                what = f"{name}/seg{k}/out{j}"
                if isinstance(t, ClassDistances):
                    show(what + "/labels", t.labels)
                    t = t.values
                show(what, t)
                outs.append(t)
                grads.append((torch.randn(t.shape, generator=g) * 1e-2).to(dev, t.dtype))
                if j == 0 and hasattr(t, "spx_ce"):
                    show(what + "/ce_loss", t.spx_ce.loss)
                    show(what + "/ce_pred", t.spx_ce.pred)
                    outs.append(t.spx_ce.loss)
                    grads.append(torch.ones_like(t.spx_ce.loss))
                if kind == "group" and hasattr(t, "spx_group"):
                    groups = torch.cat(net.compute_group(t), dim=1)
                    show(what + "/groups", groups)
                    outs.append(groups)
                    grads.append((torch.randn(groups.shape, generator=g) * 1e-2).to(dev, groups.dtype))
        assert all(t.requires_grad for t in outs), name
        torch.autograd.backward(outs, grads)
        torch.cuda.synchronize()
        show(f"{name}/d_x", x.grad)
        show(f"{name}/d_prototype_vectors", net.prototype_vectors.grad)
        if kind == "proto":
            show(f"{name}/d_last_layer", net.last_layer.weight.grad)
        else:
            show(f"{name}/d_last_layer_group", net.last_layer_group.weight.grad)
            for i, gp in enumerate(net.group_projection):
                show(f"{name}/d_group_projection{i}", gp.weight.grad)
        print(f"calls {name}: {' '.join(LIB.calls)}", flush=True)
    finally:
        for key, v in saved.items():
            setattr(*key, v)


def features(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.sigmoid(torch.randn(shape, generator=g)).to(dev, torch.bfloat16).requires_grad_(True)


def labels(grid, seed):
    return torch.randint(0, K + 1, (B,) + tuple(grid), generator=torch.Generator().manual_seed(seed)).to(dev)


def case(name, kind, branch, packed, kwargs=None, **net_kw):
    lay = PackedLayout(B, GRIDS)
    x = features((1, S * CS, 1, lay.M) if packed else (B, S * CS) + GRIDS[0], 2 + packed)
    arg = PackedMaps(features=x, layout=lay, index=None) if packed else x
    net = make(kind, **net_kw)
    run(name, kind, branch, net, x, lambda: net.forward_from_conv_features(arg, **(kwargs or {})))


for kind, branch in CASES:
    for m, mode in enumerate(MODES):
        case(f"{kind}/{branch}/single/mode{m}", kind, branch, False, mode)
        case(f"{kind}/{branch}/packed/mode{m}", kind, branch, True, mode)
        case(f"{kind}/{branch}/single+ce/mode{m}", kind, branch, False, dict(mode, ce_target=labels(GRIDS[0], 5)))
        if kind == "proto":
            case(f"{kind}/{branch}/single+target/mode{m}", kind, branch, False, dict(mode, target_labels=labels(GRIDS[0], 6)))
            case(f"{kind}/{branch}/packed+target/mode{m}", kind, branch, True,
                 dict(mode, target_labels=[labels(g, 7 + k) for k, g in enumerate(GRIDS)]))
for kind in ("proto", "group"):
    for m, mode in enumerate(MODES):
        case(f"{kind}/callable/single/mode{m}", kind, "narrow", False, mode,
             prototype_activation_function=lambda d: torch.log((d + 1) / (d + 1e-3)))
