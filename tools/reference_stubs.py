"""What gen_overlap_golden.py, gen_push_boxes_golden.py and gen_explain_golden.py put around the reference's functions so that
they run on the CPU with prepared tensors: the stand-ins are shared, the fake nets and the cases are each tool's own.

* ``resize``: ``cv2.resize(..., INTER_CUBIC)`` as the float64 restatement of tests/overlap_restatement.py rounded to float32
  (``cv2`` is not needed and was never run against the restatement);
* ``Sized``: the PIL image and every tensor made from it, carrying the image size and index only;
* ``stub_modules``: the modules the reference imports (``cv2``, ``PIL``, ``torchvision``, ``matplotlib``, ``tqdm``, ``argh``, its own
  ``segmentation`` package, ...), empty but for the names it uses; a tool adds its own with ``mod``;
* ``load``: one file of the reference checkout as a module, optionally with a proxy in place of its ``np``;
* ``bf16``, the blocky ``labels`` and ``for_reference``, which hands the reference a label outside 0..K as void.

Importing this module puts tests/ on the path (the restatements live there)."""
from __future__ import annotations

import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import overlap_restatement as R  # noqa: E402


def reference_root() -> str:
    ref = os.environ.get("SPX_REFERENCE")
    if not ref:
        sys.exit("set SPX_REFERENCE to the reference checkout")
    return ref


def out_path(name: str) -> str:
    """Where a tool writes: its first argument, or tests/golden/``name`` (the committed fixture)."""
    return sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "..", "tests", "golden", name)


def resize(src, dsize, interpolation):
    assert interpolation == "INTER_CUBIC" and src.dtype == np.float32
    if src.ndim == 3 and src.shape[2] == 1:                   # a one-channel image comes back 2-D from cv2.resize
        src = src[:, :, 0]
    return R.upsample(src, (dsize[1], dsize[0])).astype(np.float32)


class Sized:
    """Stands for the PIL image and for every tensor made from it: carries (H, W) and the image's index only; ``numpy()`` is
    zeros of ``channels`` x H x W in ``dtype``."""

    def __init__(self, H, W, n=0, channels=1, dtype=np.uint8):
        self.height, self.width, self.n, self.channels, self.dtype = H, W, n, channels, dtype

    def crop(self, box):
        assert box == (0, 0, self.width, self.height)
        return self

    def _same(self, *_):
        return self

    convert = unsqueeze = to = cuda = detach = cpu = _same

    def numpy(self):
        return np.zeros((self.channels, self.height, self.width), self.dtype)


def _open(f):
    """The "image file" of the push tool's data set: a text file with the image's size and index."""
    H, W, n = (int(v) for v in f.read().split())
    return Sized(H, W, n)


def mod(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def stub_modules():
    mod("argh", dispatch_command=lambda *a, **kw: None)
    mod("cv2", resize=resize, INTER_CUBIC="INTER_CUBIC")
    mod("matplotlib", pyplot=mod("matplotlib.pyplot"))
    mod("PIL", Image=mod("PIL.Image", Image=Sized, open=_open))
    mod("torchvision", transforms=mod("torchvision.transforms", ToTensor=lambda: (lambda img: img)))
    mod("tqdm", tqdm=lambda it, **kw: it)
    mod("find_nearest", to_normalized_tensor=lambda img: img)
    mod("settings", log=print)
    mod("segmentation").__path__ = []
    names = ("CITYSCAPES_19_EVAL_CATEGORIES", "CITYSCAPES_CATEGORIES", "COCO_ID_2_LABEL", "EM_ID_2_LABEL", "PASCAL_CATEGORIES",
             "PASCAL_ID_MAPPING", "ADE20k_ID_2_LABEL")
    mod("segmentation.constants", **{n: {} for n in names})
    mod("segmentation.data").__path__ = []
    mod("segmentation.data.dataset", PatchClassificationDataset=object, resize_label=None)
    mod("segmentation.model").__path__ = []
    mod("segmentation.model.model", PPNet=object)
    mod("segmentation.model.model_multiscale", PPNetMultiScale=object)
    mod("segmentation.model.model_multiscale_group", PPNetMultiScale=object)


def load(rel, name=None, numpy_proxy=None):
    """The file ``rel`` of the reference checkout as the module ``name`` (importable by the files loaded after it)."""
    name = name or "ref_" + os.path.basename(rel)[:-3]
    spec = importlib.util.spec_from_file_location(name, os.path.join(reference_root(), rel))
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    if numpy_proxy is not None:
        m.np = numpy_proxy
    return m


def bf16(t):
    return t.to(torch.bfloat16).to(torch.float32)


def labels(g, N, H, W, K, present, blocks):
    """Blocky labels: image n holds the classes present[n] plus void, and one pixel with the label K + 2; about ``blocks`` =
    (rows, columns) of blocks per image."""
    lab = np.zeros((N, H, W), np.uint8)
    for n in range(N):
        vals = np.array([0] + [k + 1 for k in present[n]])
        by, bx = max(1, H // blocks[0]), max(1, W // blocks[1])
        grid = vals[torch.randint(0, len(vals), (H // by + 1, W // bx + 1), generator=g).numpy()]
        lab[n] = np.kron(grid, np.ones((by, bx), np.int64))[:H, :W]
        for i, v in enumerate(vals):                 # every listed value occurs
            lab[n, i, 0] = v
        lab[n, H - 1, W - 1] = K + 2
    return lab


def for_reference(lab, K):
    out = lab.copy()
    out[out > K] = 0
    return out
