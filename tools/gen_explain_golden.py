"""Write tests/golden/explanation_maps.npz by driving the reference's own ``plot_activation_proto`` and ``plot_activation_group``
(segmentation/analysis/sample_activations_prototype.py:30-133, sample_activations_group.py:29-131; CPU only).

    SPX_REFERENCE=/path/to/ScaleProtoSeg python tools/gen_explain_golden.py [output.npz]

The two functions are loaded from the reference checkout and called once per image with stand-ins for everything around them
(those of tools/reference_stubs.py, and):

* a fake ``ppnet`` that returns prepared tensors (``conv_features``, ``forward_from_conv_features``, ``compute_group``,
  ``prototype_class_identity``, ``epsilon``, ``num_groups``, ``last_layer_group``); ``.cuda()`` is a no-op;
* ``to_normalized_tensor`` and ``transforms.ToTensor`` stubs that only carry the image size; ``plt`` does nothing, the files the
  functions would write are never written (their class folders are made in a temporary directory);
* ``cv2.applyColorMap`` records its uint8 argument: the heat map;  the ``ListedColormap`` object records the array it is called
  with: the argmax map;  ``np.amin`` inside the two functions also records the minimum and maximum of its argument, the masked
  map: ``ranges``;
* the reference cannot take a label outside 0..K (it looks the class name up with it), so the one out-of-range pixel of the
  recorded labels is handed to it as void: both belong to no class.

Data only is recorded, keys ``<case>__<field>``: the latent distances or activations (bf16-representable), labels, identity or
head weights, the slot table, the rows in the reference's order, per heat row the bytes, (lo, hi), whether hi == lo (the
reference then divides 0 by 0 and its bytes are undefined: zeros are recorded), and the mask of ambiguous pixels; per dominant
row the reference's argmax array, its ambiguous mask and whether the row holds a deliberate tie.  Ambiguity is defined in
tests/explain_restatement.py.  The tool asserts ambiguous <= 4 + H*W / 50 for every row (the seeds below satisfy it) except the
dominant rows of the deliberately tied class."""
from __future__ import annotations

import os
import tempfile
import types
import warnings

import numpy as np
import torch

import reference_stubs as S
import explain_restatement as E

EPS = 1e-4
BLOCKS = (5, 6)
REC = []                                                          # ("range", lo, hi) / ("heat", bytes) / ("argmax", array)


class _RecordingNumpy:
    """numpy, with ``amin`` also recording the range of its argument."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def amin(a):
        REC.append(("range", np.float32(np.amin(a)), np.float32(np.amax(a))))
        return np.amin(a)


def _apply_color_map(src, colormap):
    assert src.dtype == np.uint8 and src.ndim == 2 and colormap == "COLORMAP_JET"
    REC.append(("heat", src.copy()))
    return np.zeros(src.shape + (3,), np.uint8)


class _Colormap:
    def __init__(self, colors):
        self.n = len(colors)

    def __call__(self, index):
        assert index.ndim == 2 and index.max() < self.n
        REC.append(("argmax", np.asarray(index).copy()))
        return np.zeros(index.shape + (4,))


def _stub_modules():
    """The shared stand-ins, with a ``cv2`` that also has ``applyColorMap`` and a ``matplotlib`` with the recording colormap."""
    nothing = lambda *a, **kw: None
    S.stub_modules()
    S.mod("cv2", resize=S.resize, INTER_CUBIC="INTER_CUBIC", applyColorMap=_apply_color_map, COLORMAP_JET="COLORMAP_JET")
    cm = types.SimpleNamespace(viridis=lambda x: np.zeros(np.shape(x) + (4,)))
    plt = S.mod("matplotlib.pyplot", cm=cm, imsave=nothing, close=nothing)
    S.mod("matplotlib", pyplot=plt, colors=S.mod("matplotlib.colors", ListedColormap=_Colormap)).__path__ = []


class _ProtoNet:
    def __init__(self, ident):
        self.prototype_class_identity = ident
        self.epsilon = EPS

    def conv_features(self, x):
        return x

    def forward_from_conv_features(self, conv):
        return self.logits, self.distances


class _GroupNet:
    def __init__(self, K, G, head):
        self.num_classes, self.num_groups = K, G
        self.last_layer_group = types.SimpleNamespace(weight=types.SimpleNamespace(data=head))

    def conv_features(self, x):
        return torch.empty(1, 1, *self.grid)

    def forward_from_conv_features(self, conv, return_activations=False):
        assert return_activations
        return self.logits, None

    def compute_group(self, activations):
        return self.groups


def _drive(fn, net, lab, K, H, W, h, w, g):
    """Call the reference once per image; the recorded events in its order."""
    names = {k: f"class{k}" for k in range(K)}
    events = []
    with tempfile.TemporaryDirectory() as tmp, warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for n in range(lab.shape[0]):
            net.select(n)
            net.logits = torch.randn(1, h, w, K, generator=g)
            del REC[:]
            fn(S.Sized(H, W, channels=3, dtype=np.float32), n, S.for_reference(lab[n], K), net, names, tmp)
            events.append(list(REC))
    return events


def _collect(events, planes, weights, lab, table, present, tied_class=None):
    """The recorded events -> arrays, next to the ambiguity masks of the restatement; asserts the caps."""
    K, J = table.shape
    H, W = lab.shape[1:]
    cap = 4 + H * W / 50
    heat_rows, heat, ranges, degenerate, heat_amb = [], [], [], [], []
    dom_rows, argmax, dom_amb, tied = [], [], [], []
    for n, ev in enumerate(events):
        ev = list(ev)
        for k in sorted(present[n]):
            slots = [j for j in range(J) if table[k, j] >= 0]
            for j in slots:
                kind, lo, hi = ev.pop(0)
                assert kind == "range"
                kind, bytes_ = ev.pop(0)
                assert kind == "heat" and bytes_.shape == (H, W)
                flat = bool(hi == lo)
                amb = E.heat_ambiguous(planes[n, table[k, j]], lab[n], k)
                assert amb.sum() <= cap, ("heat", n, k, j, int(amb.sum()), cap)
                heat_rows.append((n, k, j))
                heat.append(np.zeros((H, W), np.uint8) if flat else bytes_)
                ranges.append((lo, hi))
                degenerate.append(flat)
                heat_amb.append(amb)
            kind, arg = ev.pop(0)
            assert kind == "argmax" and arg.shape == (H, W)
            cls_planes = [planes[n, table[k, j]] if table[k, j] >= 0 else None for j in range(J)]
            amb, _, _ = E.dominant_top2(cls_planes, weights[k], lab[n], k)
            assert k == tied_class or amb.sum() <= cap, ("dominant", n, k, int(amb.sum()), cap)
            dom_rows.append((n, k))
            argmax.append(np.asarray(slots)[arg].astype(np.uint8))       # the position among the class's slots -> the column
            dom_amb.append(amb)
            tied.append(k == tied_class)
        assert not ev
    return dict(heat_rows=np.array(heat_rows, np.int64), heat=np.stack(heat), ranges=np.array(ranges, np.float32),
                degenerate=np.array(degenerate), heat_ambiguous=np.stack(heat_amb), dom_rows=np.array(dom_rows, np.int64),
                ref_argmax=np.stack(argmax), dom_ambiguous=np.stack(dom_amb), tied=np.array(tied))


def _proto_case(name, PA, seed, h, w, H, W, tie):
    g = torch.Generator().manual_seed(seed)
    # classes: 0 three prototypes, 1 two (one empty slot), 2 three (with ``tie`` the third is a copy of the first)
    cls = [0, 0, 0, 1, 1, 2, 2, 2]
    K, P, N = 3, len(cls), 2
    ident = torch.zeros(P, K)
    ident[torch.arange(P), torch.tensor(cls)] = 1
    present = [[0, 1, 2], [0, 2]]                                 # class 1 is absent from image 1
    base = torch.rand(N, K, h, w, generator=g) * 1.5 + 0.05
    d = S.bf16(base[:, cls] * (0.5 + torch.rand(N, P, h, w, generator=g)))
    if tie:
        d[:, 7] = d[:, 5]
    lab = S.labels(g, N, H, W, K, present, BLOCKS)
    net = _ProtoNet(ident)
    net.select = lambda n: setattr(net, "distances", d[n:n + 1])
    events = _drive(PA.plot_activation_proto, net, lab, K, H, W, h, w, g)
    table = np.full((K, 3), -1, np.int64)
    for k in range(K):
        own = [p for p in range(P) if cls[p] == k]
        table[k, :len(own)] = own
    dn = d.numpy()
    act = np.log((dn + 1) / (dn + EPS))                       # sample_activations_prototype.py:85, float32 as there
    out = dict(kind=np.array("proto"), distances=dn, ident=ident.numpy(), labels=lab, table=table)
    out.update(_collect(events, act, np.ones((K, 3)), lab, table, present, tied_class=2 if tie else None))
    return {f"{name}__{k}": v for k, v in out.items()}


def _group_case(name, GA, seed, h, w, H, W):
    g = torch.Generator().manual_seed(seed)
    K, G, N = 3, 3, 2
    present = [[0, 1, 2], [0, 1]]                                 # class 2 is absent from image 1
    base = torch.rand(N, K, 1, h, w, generator=g) * 2.0
    a = base * (0.6 + 0.4 * torch.rand(N, K, G, h, w, generator=g)) - 0.3
    a[:, 0, 0] += 0.5                                             # the strongest group of class 0: its negative weight flips the argmax
    # a constant plane: hi == lo.  Zero is the only constant that stays one in every arithmetic (the taps' weights sum to 1
    # only nearly, so another constant comes back with its last bits varying and hi - lo a few ulps)
    a[:, 1, 2] = 0.0
    a = S.bf16(a).reshape(N, K * G, h, w)
    head = S.bf16(torch.rand(K, K * G, generator=g) * 1.5 + 0.25)
    head[0, 0] = -0.75
    lab = S.labels(g, N, H, W, K, present, BLOCKS)
    net = _GroupNet(K, G, head)
    net.grid = (h, w)

    def select(n):
        pix = a[n].permute(1, 2, 0).reshape(h * w, K * G)         # the [M, U] layout compute_group's list is split from
        net.groups = list(torch.split(pix, G, dim=1))

    net.select = select
    events = _drive(GA.plot_activation_group, net, lab, K, H, W, h, w, g)
    table = np.arange(K * G, dtype=np.int64).reshape(K, G)
    weights = np.stack([head.numpy()[k, k * G:(k + 1) * G] for k in range(K)])
    out = dict(kind=np.array("group"), activations=a.numpy(), head=head.numpy(), labels=lab, table=table)
    out.update(_collect(events, a.numpy(), weights, lab, table, present))
    # the negative weight changes the picture
    plain = E.dominant([a.numpy()[0, j] for j in range(G)], np.ones(G), lab[0], 0)
    assert (plain != out["ref_argmax"][0])[lab[0] == 1].mean() > 0.25
    return {f"{name}__{k}": v for k, v in out.items()}


def main():
    _stub_modules()
    PA = S.load(os.path.join("segmentation", "analysis", "sample_activations_prototype.py"), numpy_proxy=_RecordingNumpy())
    GA = S.load(os.path.join("segmentation", "analysis", "sample_activations_group.py"), numpy_proxy=_RecordingNumpy())
    cases = {}
    cases.update(_proto_case("proto_5x7_33x41", PA, 20240702, 5, 7, 33, 41, tie=False))
    cases.update(_proto_case("proto_3x3_17x19_tied", PA, 20240703, 3, 3, 17, 19, tie=True))
    cases.update(_group_case("group_5x7_33x41", GA, 20240704, 5, 7, 33, 41))
    cases.update(_group_case("group_3x3_17x19", GA, 20240705, 3, 3, 17, 19))
    out = S.out_path("explanation_maps.npz")
    np.savez_compressed(out, **cases)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
