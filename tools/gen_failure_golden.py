"""Write tests/golden/failure_cases.npz by driving the reference's own ``failure_cases`` with its ``plot_activation_proto`` /
``plot_activation_group`` (segmentation/analysis/failure_cases.py) and ``run_evaluation`` (segmentation/eval_test.py); CPU only.

    SPX_REFERENCE=/path/to/ScaleProtoSeg python tools/gen_failure_golden.py [output.npz]

``failure_cases()`` runs whole, as data type ``ade`` (no id conversion), over temporary ``.npy`` files (an image's first byte
carries its index), with the stand-ins of tools/reference_stubs.py and:

* ``torch.load`` inside the two files returns a fake ``ppnet`` that hands out prepared tensors (``forward``, ``compute_group``,
  ``prototype_class_identity``, ``num_groups``, ``last_layer_group``); ``.cuda()`` and ``.eval()`` do nothing;
* ``log`` records the logged IoU of every failure case (four decimals), and ``Counter`` is a subclass that remembers the
  image's ``CLS_I`` and ``CLS_U``, so the intersection and union the quotient was formed from are recorded as integers; the two
  plot functions are wrapped: the wrapper records the
  (image, class, miss) triple and then calls the reference's function of the case's kind (the other kind only records);
* inside the plot functions ``cv2.applyColorMap`` records its uint8 argument, the heat map, and ``np.max`` / ``np.min`` of a LIST
  (the reduction of ``proto_max[p]`` / ``group_max[i]``) record the shared ranges; ``plt`` does nothing, files go to a temporary
  directory;
* ``run_evaluation`` runs whole with the reference's own ``segmentation/constants.py``: ``np.vectorize`` records the look-up it is
  given (the Cityscapes table), ``Image.fromarray`` the id-mapped bytes.

Data only is recorded, keys ``<case>__<field>``.  Conditions, asserted here: inputs are bf16-representable and labels lie in
0..K; no case has tied misprediction counts or a failing class without mispredictions; every heat row has at most
4 + H*W / 50 ambiguous pixels (tests/failure_restatement.py defines them; the seeds below satisfy it).  Pixels where 255 x >= 256
and rows of a slot with hi <= 0 are recorded with a flag: the reference's ``np.uint8`` conversion is undefined there."""
from __future__ import annotations

import collections
import os
import tempfile
import types
import warnings

import numpy as np
import torch

import reference_stubs as S
import failure_restatement as FR

EPS = 1e-4
BLOCKS = (5, 6)
REC = []                          # ("hi", v) / ("lo", v) / ("heat", bytes) / ("lut", f) / ("pred", bytes)
LOGGED = []                       # (file name, IoU string)
TRIPLES = []                      # (n, class, miss) as the group wrapper sees them


class _RecordingNumpy:
    """numpy, with ``max`` / ``min`` of a list and ``vectorize`` also recording."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def max(a):
        if isinstance(a, list):
            REC.append(("hi", np.float32(np.max(a))))
        return np.max(a)

    @staticmethod
    def min(a):
        if isinstance(a, list):
            REC.append(("lo", np.float32(np.min(a))))
        return np.min(a)

    @staticmethod
    def vectorize(f):
        REC.append(("lut", f))
        return np.vectorize(f)


class _Counter(collections.Counter):
    """``Counter``, remembering the ones made empty: per image the reference makes CLS_I, then CLS_U."""

    made = []

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not args and not kw:
            _Counter.made.append(self)


class _Torch:
    """torch, with ``load`` returning the fake net and ``stack`` keeping the stand-in images."""

    def __init__(self, net):
        self.net = net

    def __getattr__(self, name):
        return getattr(torch, name)

    def load(self, path):
        return self.net

    @staticmethod
    def stack(items, dim=0):
        return _Batch(items)


class _Img:
    """What ``transform(img)`` returns: the image's index and size."""

    def __init__(self, img):
        self.n, self.H, self.W = int(img[0, 0, 0]), img.shape[0], img.shape[1]

    def _same(self, *_):
        return self

    unsqueeze = cuda = detach = cpu = _same

    def numpy(self):
        return np.zeros((3, self.H, self.W), np.float32)


class _Batch:
    def __init__(self, items):
        self.ns = [t.n for t in items]

    def cuda(self):
        return self


def _apply_color_map(src, colormap):
    assert src.dtype == np.uint8 and src.ndim == 2 and colormap == "COLORMAP_JET"
    REC.append(("heat", src.copy()))
    return np.zeros(src.shape + (3,), np.uint8)


class _Saved:
    def convert(self, mode):
        return self

    def save(self, path):
        pass


def _from_array(a):
    assert a.dtype == np.uint8 and a.ndim == 2
    REC.append(("pred", a.copy()))
    return _Saved()


def _stub_modules(tmp):
    nothing = lambda *a, **kw: None
    S.stub_modules()
    S.mod("cv2", resize=S.resize, INTER_CUBIC="INTER_CUBIC", applyColorMap=_apply_color_map, COLORMAP_JET="COLORMAP_JET")
    cm = types.SimpleNamespace(viridis=lambda x: np.zeros(np.shape(x) + (4,)))
    plt = S.mod("matplotlib.pyplot", cm=cm, imsave=nothing, close=nothing)
    S.mod("matplotlib", pyplot=plt).__path__ = []
    S.mod("PIL", Image=S.mod("PIL.Image", Image=object, fromarray=_from_array))
    tr = S.mod("torchvision.transforms", ToTensor=lambda: _Img, Normalize=lambda **kw: None, Compose=lambda fs: fs[0],
               Resize=lambda **kw: (lambda t: t), InterpolationMode=types.SimpleNamespace(BILINEAR="bilinear"))
    S.mod("torchvision", transforms=tr)
    S.mod("settings", log=lambda s: LOGGED.append(s), data_path={"ade": tmp, "cityscapes": tmp})


class _Net:
    """The fake ``ppnet``: ``logits`` [N, h, w, K], ``acts`` [N, h*w, P] or None, ``groups`` [N, h*w, K*G] or None."""

    def __init__(self, logits, acts=None, ident=None, groups=None, G=0, head=None):
        self.logits, self.acts, self.groups, self.num_groups = logits, acts, groups, G
        self.prototype_class_identity = ident
        self.last_layer_group = types.SimpleNamespace(weight=types.SimpleNamespace(data=head))

    def cuda(self):
        return self

    def eval(self):
        return self

    def forward(self, x, return_activations=False):
        if isinstance(x, _Batch):
            return self.logits[x.ns], None
        self.n = x.n
        return self.logits[x.n:x.n + 1], (self.acts[x.n] if self.acts is not None else torch.empty(0))

    def compute_group(self, activations):
        return list(torch.split(self.groups[self.n], self.num_groups, dim=1))


def _write_images(tmp, split, N, H, W, ann=None):
    img_dir = os.path.join(tmp, "img_with_margin_0", split)
    ann_dir = os.path.join(tmp, "annotations", split)
    os.makedirs(img_dir)
    os.makedirs(ann_dir)
    for n in range(N):
        img = np.zeros((H, W, 3), np.uint8)
        img[0, 0, 0] = n
        np.save(os.path.join(img_dir, f"img{n}.npy"), img)
        if ann is not None:
            np.save(os.path.join(ann_dir, f"img{n}.npy"), ann[n].astype(np.int64))      # the reference computes cls_i - 1 in the type


def _drive(FC, kind, net, lab, K, threshold, tmp):
    """One run of failure_cases(); per case (n, a, miss): the logged IoU, the ranges in the reference's key order, the heat rows."""
    N, H, W = lab.shape
    _write_images(tmp, "val", N, H, W, lab)
    FC.torch = _Torch(net)
    FC.data_path = {"ade": tmp}
    FC.ADE20k_ID_2_LABEL = {k: f"class{k}" for k in range(K)}
    FC.Counter = _Counter
    real = {"group": FC._real_group, "proto": FC._real_proto}
    found, counts = {}, {}

    def wrap(which):
        def call(img, img_id, ann, acts, logits, ppnet, names, cls, miss, out):
            key = (int(img[0, 0, 0]), int(cls) - 1, int(miss) - 1)
            if which == "group":
                TRIPLES.append(key)
                inter, union = _Counter.made[-2], _Counter.made[-1]          # CLS_I and CLS_U of the image being visited
                counts[key] = (int(inter[int(cls) - 1]), int(union[int(cls) - 1]))
            if which == kind:
                del REC[:]
                real[which](img, img_id, ann, acts, logits, ppnet, names, cls, miss, out)
                found[key] = list(REC)
        return call

    FC.plot_activation_group, FC.plot_activation_proto = wrap("group"), wrap("proto")
    del TRIPLES[:], LOGGED[:]
    os.environ["RESULTS_DIR"] = tmp
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        FC.failure_cases("model", "push", "ade", threshold)
    logged = [s for s in LOGGED if s.startswith("Failure case")]
    assert len(logged) == len(TRIPLES) == len(found) > 0
    iou = {t: s.rsplit(" ", 1)[1] for t, s in zip(TRIPLES, logged)}
    assert all(f"img{t[0]}.npy" in s for t, s in zip(TRIPLES, logged))
    assert all(f"{counts[t][0] / counts[t][1]:.4f}" == iou[t] for t in TRIPLES)      # the counters are those of the logged quotient
    return iou, counts, found


def _case(FC, name, kind, seed, h, w, H, W, threshold):
    g = torch.Generator().manual_seed(seed)
    K, G, N = 3, 3, 3
    cls = [0, 0, 0, 1, 1, 2, 2, 2]
    present = [[0, 1, 2], [0, 2], [1, 2]]
    lab = S.for_reference(S.labels(g, N, H, W, K, present, BLOCKS), K)
    assert lab.max() <= K
    # logits that follow the labels loosely: some classes pass, some fail
    onehot = torch.nn.functional.one_hot(torch.from_numpy(lab[:, ::H // h, ::W // w][:, :h, :w].astype(np.int64)), K + 1)[..., 1:].float()
    logits = S.bf16(1.6 * onehot + torch.randn(N, h, w, K, generator=g))
    out = dict(kind=np.array(kind), threshold=np.float64(threshold), logits=logits.numpy(), labels=lab)
    if kind == "proto":
        P = len(cls)
        ident = torch.zeros(P, K)
        ident[torch.arange(P), torch.tensor(cls)] = 1
        base = torch.rand(N, K, h, w, generator=g) * 1.5 + 0.05
        d = S.bf16(base[:, cls] * (0.5 + torch.rand(N, P, h, w, generator=g)))
        dn = d.numpy()
        planes = np.log((dn + 1) / (dn + EPS))                    # the model's log activation in float32, as tests/support.py
        net = _Net(logits, acts=torch.from_numpy(planes).permute(0, 2, 3, 1).reshape(N, h * w, P), ident=ident)
        table = np.full((K, 3), -1, np.int64)
        for k in range(K):
            own = [p for p in range(P) if cls[p] == k]
            table[k, :len(own)] = own
        out.update(distances=dn, ident=ident.numpy(), table=table)
    else:
        base = torch.rand(N, K, 1, h, w, generator=g) * 2.0
        a = S.bf16(base * (0.6 + 0.4 * torch.rand(N, K, G, h, w, generator=g)) - 0.3).reshape(N, K * G, h, w)
        head = S.bf16(torch.rand(K, K * G, generator=g) * 1.5 + 0.25)
        planes = a.numpy()
        net = _Net(logits, groups=a.permute(0, 2, 3, 1).reshape(N, h * w, K * G), G=G, head=head)
        table = np.arange(K * G, dtype=np.int64).reshape(K, G)
        out.update(activations=planes, head=head.numpy(), table=table)
    with tempfile.TemporaryDirectory() as tmp:
        iou, counts, found = _drive(FC, kind, net, lab, K, threshold, tmp)
    triples = sorted(found)
    # the conditions on the recorded cases
    k_star = FR.argmax_map(logits.numpy(), (H, W))
    conf = FR.confusion(k_star, lab, K)
    r_iou, r_miss, r_fail = FR.failure_table(conf, threshold)
    for n in range(N):
        for a in range(K):
            if r_fail[n, a]:
                others = np.delete(conf[n, a], a)
                assert others.max() > 0 and (others == others.max()).sum() == 1, ("tie or no misprediction", n, a)
    cases, rows = FR.cases_and_rows(r_fail, r_miss, table, kind == "group")
    assert [tuple(c) for c in cases.tolist()] == triples, (cases.tolist(), triples)
    assert 0 < len(cases) < sum(len(p) for p in present) and len(set(cases[:, 2].tolist())) > 1      # a present class passes
    Q = int(rows[:, 3].max()) + 1
    heat, ranges = [], []
    for t in triples:
        ev = found[t]
        his = [v for kd, v in ev if kd == "hi"]
        los = [v for kd, v in ev if kd == "lo"]
        assert len(his) == len(los)
        ranges += list(zip(los, his))
        heat += [v for kd, v in ev if kd == "heat"]
    heat, ranges = np.stack(heat), np.array(ranges, np.float32)
    assert heat.shape == (len(rows), H, W) and ranges.shape == (Q, 2)
    _, _, flagged = FR.paired_heat(planes, lab, rows, Q)
    amb = FR.paired_ambiguous(planes, lab, rows, Q)
    cap = 4 + H * W / 50
    assert (amb.reshape(len(rows), -1).sum(1) <= cap).all(), (name, amb.reshape(len(rows), -1).sum(1), cap)
    heat = np.where(flagged, 0, heat).astype(np.uint8)            # undefined in the reference: not recorded
    out.update({"cases": cases, "logged_iou": np.array([iou[t] for t in triples]),
                "counts": np.array([counts[t] for t in triples], np.int64), kind + "_rows": rows, kind + "_heat": heat,
                kind + "_ranges": ranges, kind + "_flagged": flagged})
    for key in ("logits", "distances", "activations", "head"):
        if key in out:
            t = torch.from_numpy(out[key])
            assert torch.equal(t.to(torch.bfloat16).float(), t), key
    print(name, "cases", cases.tolist(), "iou", [iou[t] for t in triples], "rows", len(rows), "slots", Q, "flagged", int(flagged.sum()),
          "ambiguous", int(amb.sum()))
    return {f"{name}__{k}": v for k, v in out.items()}


def _eval_test(seed, h, w, H, W):
    """run_evaluation over two test images with the Cityscapes mapping: the look-up table and the id-mapped bytes."""
    g = torch.Generator().manual_seed(seed)
    K, N = 19, 2
    logits = S.bf16(torch.randn(N, h, w, K, generator=g))
    S.load(os.path.join("segmentation", "constants.py"), name="segmentation.constants")
    ET = S.load(os.path.join("segmentation", "eval_test.py"), numpy_proxy=_RecordingNumpy())
    ET.torch = _Torch(_Net(logits))
    with tempfile.TemporaryDirectory() as tmp:
        ET.data_path = {"cityscapes": tmp}
        os.environ["RESULTS_DIR"] = tmp
        _write_images(tmp, "test", N, H, W)
        names = []
        real_split = np.array_split
        ET.np.array_split = lambda files, n: [names.extend(list(b)) or b for b in real_split(files, n)]
        del REC[:]
        ET.run_evaluation("model", "push", 2, "False")
    get = [v for kd, v in REC if kd == "lut"][0]
    lut = np.array([get(k + 1) for k in range(K)], np.int64)
    assert lut.min() >= 0 and lut.max() <= 255
    preds = [v for kd, v in REC if kd == "pred"]
    assert len(preds) == len(names) == N
    order = np.argsort([int(str(f)[3:-4]) for f in names])
    pred = np.stack([preds[i] for i in order])
    assert pred.shape == (N, H, W)
    return dict(proto__test_logits=logits.numpy(), proto__test_lut=lut.astype(np.uint8), proto__test_pred=pred)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        _stub_modules(tmp)
        FC = S.load(os.path.join("segmentation", "analysis", "failure_cases.py"), numpy_proxy=_RecordingNumpy())
    FC._real_group, FC._real_proto = FC.plot_activation_group, FC.plot_activation_proto
    cases = {}
    cases.update(_case(FC, "proto", "proto", 20241001, 5, 7, 33, 41, 0.5))
    cases.update(_case(FC, "group", "group", 20241002, 3, 3, 17, 19, 0.5))
    cases.update(_eval_test(20241003, 5, 7, 33, 41))
    out = S.out_path("failure_cases.npz")
    np.savez_compressed(out, **cases)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
