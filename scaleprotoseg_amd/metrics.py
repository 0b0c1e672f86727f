"""Evaluation metrics of segmentation/eval_valid_multiscale.py:229-275 on the GPU: mIoU and per-class IoU, pixel accuracy,
how often each prototype is a pixel's nearest, and the top-k class purity of a pixel's nearest prototypes.

The reference upsamples the latent logits / distances of every image to the label size, copies the two full-resolution
maps to the host and counts with NumPy loops (one pass per class, one per (class, prototype)).  Here one HIP launch per
batch (``spx_eval_accumulate``) interpolates, reduces and counts, and only integer counters ever leave the chip; a
second small launch (``spx_eval_topk``) handles the sample pixels of the top-k purity.  ``update`` never waits for the
device, so it can sit in a captured step; ``compute`` makes the one device-to-host copy and finalises in float64.
"""
from __future__ import annotations

import ctypes as C
from collections import Counter
from dataclasses import dataclass
from typing import Dict, Optional

import torch

from . import _lib
from ._lib import SpxError
from ._maps import LABEL_BYTES, dev_ptr, label_map, on_device, strides


def prototype_classes(prototype_class_identity: torch.Tensor) -> torch.Tensor:
    """cls(p): the FIRST argmax of each identity row (eval_valid_multiscale.py:109-112, ``np.argmax``), int32 on the host."""
    ident = prototype_class_identity.detach().cpu()
    if ident.dim() != 2 or ident.shape[0] < 1 or ident.shape[1] < 1:
        raise SpxError("prototype_class_identity must be [P, K]")
    return torch.argmax(ident.to(torch.float64), dim=1).to(torch.int32).contiguous()


def _check_maps(logits: torch.Tensor, labels: torch.Tensor, distances: Optional[torch.Tensor]):
    """(H, W) of inputs whose shapes and types fit; nothing here needs the device."""
    if logits.dim() != 4 or logits.dtype != torch.float32:
        raise SpxError("logits must be fp32 [N, h, w, K]")
    N, h, w, _ = logits.shape
    H, W = label_map(labels, N, "logits")
    if distances is not None:
        if distances.dim() != 4 or distances.dtype != torch.float32:
            raise SpxError("distances must be fp32 [N, P, h, w]")
        if distances.shape[0] != N or tuple(distances.shape[2:]) != (h, w):
            raise SpxError(f"distances {tuple(distances.shape)} do not match logits {tuple(logits.shape)}")
    return H, W


def eval_accumulate(logits: torch.Tensor, labels: torch.Tensor, conf: torch.Tensor, distances: Optional[torch.Tensor] = None,
                    proto_class: Optional[torch.Tensor] = None, hits: Optional[torch.Tensor] = None) -> None:
    """Add one batch to the int64 counters ``conf`` [K+1, K] and ``hits`` [P] (``spx_eval_accumulate``).  ``logits`` fp32
    [N, h, w, K] and ``distances`` fp32 [N, P, h, w] are read through their strides; ``labels`` [N, H, W] set the output
    size.  ``proto_class`` is the device int32 table of :func:`prototype_classes`."""
    lib = _lib.load()
    H, W = _check_maps(logits, labels, distances)
    N, h, w, K = logits.shape
    if conf.dtype != torch.int64 or conf.numel() != (K + 1) * K:
        raise SpxError(f"conf must be int64 with {(K + 1) * K} elements")
    lab = labels.detach().contiguous()
    lg = logits.detach()
    P, dptr, dst, cptr, hptr = 0, None, None, None, None
    if distances is not None:
        d = distances.detach()
        P = int(d.shape[1])
        if proto_class is None or hits is None:
            raise SpxError("distances need proto_class and hits")
        if proto_class.dtype != torch.int32 or proto_class.numel() != P or hits.dtype != torch.int64 or hits.numel() != P:
            raise SpxError(f"proto_class must be int32 and hits int64, both with {P} elements")
        dptr, dst, cptr, hptr = dev_ptr(d, "distances"), strides(d), _lib.ptr(proto_class), _lib.ptr(hits)
    _lib.check(lib.spx_eval_accumulate(dev_ptr(lg, "logits"), strides(lg, (0, 3, 1, 2)), dptr, dst, cptr,
                                       dev_ptr(lab, "labels"), LABEL_BYTES[lab.dtype], N, K, P, h, w, H, W,
                                       _lib.ptr(conf), hptr, _lib.stream_ptr()))


def eval_topk(logits: torch.Tensor, distances: torch.Tensor, proto_class: torch.Tensor, samples: torch.Tensor, size,
              topk: torch.Tensor, seen: Optional[torch.Tensor] = None) -> None:
    """Add the top-k purity of the sample pixels ``samples`` int [N, S, 2] = (y, x) at output ``size`` = (H, W) to the
    int64 counters ``topk`` [P] and ``seen`` [1] (``spx_eval_topk``)."""
    lib = _lib.load()
    if logits.dim() != 4 or logits.dtype != torch.float32 or distances.dim() != 4 or distances.dtype != torch.float32:
        raise SpxError("logits must be fp32 [N, h, w, K] and distances fp32 [N, P, h, w]")
    N, h, w, K = logits.shape
    P = int(distances.shape[1])
    if distances.shape[0] != N or tuple(distances.shape[2:]) != (h, w):
        raise SpxError(f"distances {tuple(distances.shape)} do not match logits {tuple(logits.shape)}")
    if samples.dim() != 3 or samples.shape[0] != N or samples.shape[2] != 2 or samples.dtype not in (torch.int32, torch.int64):
        raise SpxError("samples must be int32 or int64 [N, S, 2] (y, x)")
    if topk.dtype != torch.int64 or topk.numel() != P or proto_class.dtype != torch.int32 or proto_class.numel() != P:
        raise SpxError(f"topk must be int64 and proto_class int32, both with {P} elements")
    if seen is not None and (seen.dtype != torch.int64 or seen.numel() != 1):
        raise SpxError("seen must be one int64")
    S = int(samples.shape[1])
    dev_ptr(samples, "samples")
    smp = samples.detach().contiguous()
    lg, d = logits.detach(), distances.detach()
    _lib.check(lib.spx_eval_topk(dev_ptr(lg, "logits"), strides(lg, (0, 3, 1, 2)), dev_ptr(d, "distances"),
                                 strides(d), _lib.ptr(proto_class), _lib.ptr(smp), smp.element_size(), N, S, K, P, h, w,
                                 int(size[0]), int(size[1]), _lib.ptr(topk), _lib.ptr(seen), _lib.stream_ptr()))


@dataclass
class SegmentationResult:
    """What eval_valid_multiscale.py:272-275 reports, from the exact integer counters."""

    pixel_accuracy: float                    # 100 * correct / total (non-void pixels)
    class_iou: Dict[int, float]              # {c: 100 * I_c / U_c} for the classes with U_c > 0
    mean_iou: float                          # mean of class_iou's values (nan when it is empty)
    confusion: torch.Tensor                  # int64 [K+1, K]; row K = non-void labels outside 1..K
    prototype_counts: Optional[torch.Tensor]  # int64 [P]: pixels whose nearest prototype p is of the predicted class
    mean_top_k: Optional[torch.Tensor]       # float64 [P], percent; None when no samples were seen
    samples_seen: int
    prototype_class: Optional[torch.Tensor] = None  # int32 [P]: cls(p)

    def class_prototype_counts(self) -> Dict[int, Counter]:
        """The reference's ``cls_prototype_counts`` form: {class: Counter({i: n})}, ``i`` the index of the prototype
        among its class's prototypes in bank order (``cls2protos``, :107-112, :245-253)."""
        K = self.confusion.shape[1]
        out = {c: Counter() for c in range(K)}
        if self.prototype_counts is None:
            return out
        seen_per_class = [0] * K
        for p, c in enumerate(self.prototype_class.tolist()):
            out[c][seen_per_class[c]] += int(self.prototype_counts[p])
            seen_per_class[c] += 1
        return out


def finalize(conf: torch.Tensor, hits: Optional[torch.Tensor] = None, topk: Optional[torch.Tensor] = None,
             samples_seen: int = 0, prototype_class: Optional[torch.Tensor] = None) -> SegmentationResult:
    """Host-side float64 finalisation (:272-275) of int64 counters.  mean_top_k divides by the samples actually seen
    (the reference divides by len(batches) * batch_size, which exceeds the image count for uneven batches)."""
    conf = conf.to(torch.int64).cpu()
    K = conf.shape[1]
    cd = conf.to(torch.float64)
    inter = torch.diagonal(cd[:K])
    union = cd[:K].sum(1) + cd.sum(0) - inter
    total = cd.sum().item()
    pixel_accuracy = 100.0 * inter.sum().item() / total if total > 0 else float("nan")
    class_iou = {c: 100.0 * inter[c].item() / union[c].item() for c in range(K) if union[c].item() > 0}
    mean_iou = sum(class_iou.values()) / len(class_iou) if class_iou else float("nan")
    mean_top_k = None
    if topk is not None and samples_seen > 0:
        k1 = torch.arange(1, topk.numel() + 1, dtype=torch.float64)
        mean_top_k = 100.0 * topk.cpu().to(torch.float64) / (k1 * samples_seen)
    return SegmentationResult(pixel_accuracy, class_iou, mean_iou, conf, None if hits is None else hits.cpu(), mean_top_k,
                              int(samples_seen), prototype_class)


class SegmentationMetrics:
    """Running evaluation counters on one GPU.

        m = SegmentationMetrics.for_model(ppnet)
        for img, ann in loader:
            logits, distances = ppnet(img)                  # [N, h, w, K], [N, P, h, w]
            m.update(logits, ann, distances, samples)       # ann [N, H, W]; samples int [N, S, 2] (y, x), optional
        res = m.compute()                                   # res.mean_iou, res.pixel_accuracy, ...

    All counters live in one int64 device buffer [conf (K+1)*K | hits P | topk P | samples_seen 1], so ``compute``
    is one copy and ``all_reduce`` one collective."""

    def __init__(self, num_classes: int, prototype_class_identity: Optional[torch.Tensor], device):
        self.device = torch.device(device)
        _lib.require_gpu(self.device, "SegmentationMetrics")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.num_classes = K = int(num_classes)
        if K < 1:
            raise SpxError("num_classes must be >= 1")
        if prototype_class_identity is not None:
            if prototype_class_identity.dim() != 2 or prototype_class_identity.shape[1] != K:
                raise SpxError(f"prototype_class_identity must be [P, {K}]")
            host = prototype_classes(prototype_class_identity)
            P = host.numel()
            _lib.check(_lib.load().spx_eval_check_classes(C.cast(host.data_ptr(), C.POINTER(C.c_int32)), P, K))
            self.prototype_class_host = host
            self.proto_class = host.to(self.device)
        else:
            P = 0
            self.prototype_class_host = None
            self.proto_class = None
        self.num_prototypes = P
        n = (K + 1) * K
        self._buf = torch.zeros(n + 2 * P + 1, dtype=torch.int64, device=self.device)
        self.conf = self._buf[:n].view(K + 1, K)
        self.hits = self._buf[n:n + P]
        self.topk = self._buf[n + P:n + 2 * P]
        self.samples_seen = self._buf[n + 2 * P:]

    @classmethod
    def for_model(cls, ppnet, device=None) -> "SegmentationMetrics":
        """For a PPNetMultiScale, PPNetMultiScaleGroup or PPNet: its classes and prototype_class_identity, on the device
        of its prototype bank unless ``device`` is given."""
        if device is None:
            device = ppnet.prototype_vectors.device
        return cls(ppnet.num_classes, ppnet.prototype_class_identity, device)

    def reset(self) -> None:
        self._buf.zero_()

    def update(self, logits: torch.Tensor, labels: torch.Tensor, distances: Optional[torch.Tensor] = None,
               samples: Optional[torch.Tensor] = None) -> None:
        """Count one batch: ``logits`` [N, h, w, K] and ``distances`` [N, P, h, w] as the forward returns them (any strides),
        ``labels`` [N, H, W] uint8 / int32 / int64 (0 = void, c + 1 = class c), ``samples`` int [N, S, 2] (y, x) for the
        top-k purity.  Enqueues work on the current stream only; never synchronises."""
        if logits.dim() != 4 or logits.shape[3] != self.num_classes:
            raise SpxError(f"logits must be [N, h, w, {self.num_classes}]")
        if distances is not None and (self.proto_class is None or distances.dim() != 4 or distances.shape[1] != self.num_prototypes):
            raise SpxError(f"distances must be [N, {self.num_prototypes}, h, w] (and the metrics built with a class identity)")
        if samples is not None and distances is None:
            raise SpxError("samples need distances")
        on_device(((logits, "logits"), (labels, "labels"), (distances, "distances"), (samples, "samples")), self.device, "metrics")
        eval_accumulate(logits, labels, self.conf, distances, self.proto_class, None if distances is None else self.hits)
        if samples is not None:
            eval_topk(logits, distances, self.proto_class, samples, labels.shape[1:], self.topk, self.samples_seen)

    def all_reduce(self, group=None) -> None:
        """Sum the counters of every rank (dp._all_reduce_sum): a validation set sharded over the ranks ends as one
        result, whose compute() is the same on every rank."""
        from .dp import _all_reduce_sum

        _all_reduce_sum(self._buf, group)

    def compute(self) -> SegmentationResult:
        host = self._buf.cpu()
        K, P = self.num_classes, self.num_prototypes
        n = (K + 1) * K
        seen = int(host[n + 2 * P])
        return finalize(host[:n].view(K + 1, K), host[n:n + P] if P else None, host[n + P:n + 2 * P] if P else None, seen,
                        self.prototype_class_host)
