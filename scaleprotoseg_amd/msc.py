"""Multi-scale input fusion: the reference's ``MSC`` wrapper (segmentation/utils.py:71-111) with its pixel-wise maximum, the add-on
sigmoid of the ``deeplab_simple`` configurations and the cast to the distance kernel's bf16 in ONE launch (csrc/spx_msc.hip).

The operator ``msc_max(maps, activation="none", dtype=None, out=None, return_index=False)``
---------------------------------------------------------------------------------------------
``maps``: a list of 1 to 8 device tensors [B, C, h_k, w_k], all fp32 or all bf16.  ``maps[0]`` fixes the output grid (H, W) =
(h_0, w_0); scaled maps may be smaller or larger.  Batch and channel strides are free (a channel slice is read in place), the
h x w plane itself must be contiguous.  The result is contiguous [B, C, H, W] in ``dtype`` or else the inputs' dtype; all
arithmetic is fp32.  The contract:

* ``u_0 = maps[0]``.  For k >= 1, ``u_k[Y, X]`` is bilinear with ``align_corners=False``:
  ``r = h_k / H``, ``s = max(0, r (Y + 0.5) - 0.5)``, ``i0 = min(floor(s), h_k - 1)``, ``i1 = min(i0 + 1, h_k - 1)``,
  ``ly = s - i0``; the columns follow the same rule;
  ``u = (1 - ly) ((1 - lx) v00 + lx v01) + ly ((1 - lx) v10 + lx v11)`` in fp32, in this operation order, nothing contracted
  into a fused multiply-add.  A 1 x 1 source is legal (``i0 = i1 = 0``).
* ``z = max_k u_k``; among equal values the lowest k wins; if any candidate is NaN the result is NaN and the index is the first
  NaN's.  Both rules are ``torch.max(dim=0)``'s.
* ``activation="sigmoid"``: ``y = 1 / (1 + exp(-z))`` with ``expf``, not the fast intrinsic; ``"none"``: ``y = z``.
* a bf16 result is the round-to-nearest-even of the fp32 ``y``.
* ``K = 1`` is legal: the launch is then the activation and the cast alone, the ``deeplab_simple`` add-on of the configurations
  with ``scales = []``.

With ``return_index=True`` the call returns ``(y, index)``, ``index`` uint8 [B, C, H, W]: the winning k.

Autograd: gradients go to every map that requires one.  The forward saves the uint8 index (written only when a gradient is
needed or ``return_index=True``) and the output ``y``.  The sigmoid's derivative is ``y (1 - y)`` from the SAVED output in its
own dtype: with a bf16 output the derivative carries that rounding (the gradient is that of the rounded ``y``, not of the fp32
one).  The upstream gradient may be fp32 or bf16; the gradients are in the maps' dtype.  The backward is a gather (one thread
per source element, contributions added in ascending (Y, X) order): no float atomics, no workspace, two runs agree bit for bit.
``out=`` is for calls without a gradient; with a map that requires one it raises.

Both launches go to the current stream and read nothing on the host: they are legal inside ``graphs.capture_step``.

The module ``MSC(base, scales=None)``
-------------------------------------
A drop-in for the reference's class: attributes ``base`` and ``scales`` (default ``[0.5, 0.75]``), ``state_dict`` keys
``base.*``, ``str()`` starting with ``MSC``; ``forward`` follows the reference line by line (empty ``scales`` returns the base
output, a list output of the base raises ``NotImplementedError``, training returns ``[full] + pyramid + [max]``, eval the max).
The input pyramid stays stock torch.  On device tensors the max is ``msc_max``; on CPU tensors the module runs the reference's
stock formula, so that its structure can be tested without a GPU.  ``fused(x, activation, dtype)`` returns what ``forward``
returns with activation and dtype applied by the same launch (in training the three unfused list elements go through the K = 1
launch); ``_PrototypeBankMixin.fuse_feature_epilogue`` makes a model's ``conv_features`` call it.

The packed training maps ``msc_pack(maps, activation="none", dtype=None, with_max=True, out=None)``
---------------------------------------------------------------------------------------------------
In training the reference's ``MSC`` returns four maps, ``[full] + pyramid + [max]``, and the model runs its prototype path on
each.  ``msc_pack`` writes them in ONE launch (``spx_msc_pack_fwd``) side by side on one pixel axis: a contiguous buffer
``[C, M]``, segment ``k < K`` = ``act(maps[k])`` at its own grid, segment ``K`` (``with_max``) = the ``msc_max`` of all maps, pixel
``(b, i)`` of segment ``k`` at column ``off_k + b h_k w_k + i``, ``off_k = sum_{j<k} B h_j w_j``, no padding (``PackedLayout``, pure
Python).  Every value, the index and the rounding are ``msc_max``'s, bit for bit.  The result is a ``PackedMaps``: ``features``
``[1, C, 1, M]`` is what the distance kernels take as a one-image batch of M pixels - distances, activations, logits and
gradients are per-pixel quantities, so one forward and one backward launch serve all four maps -, ``views()`` are the maps
``[B, C, h_k, w_k]`` as strided views, ``index`` the uint8 winner ``[B, C, H, W]`` (None without the maximum).  With
``with_max=False`` any maps of a common B and C form a ragged batch.  The backward (``spx_msc_pack_bwd``) is one launch for all
maps: per source element its own segment's term ``g y (1 - y)`` first, then the gather over the maximum's segment in
``msc_max``'s order, summed in fp32 and rounded once; no atomics, no workspace, capturable.  ``out=`` ([C, M], calls without a
gradient) may be any element-aligned contiguous buffer: the kernel stores vectors when M is a multiple of 4 and ``out`` is
aligned to 8 (bf16) / 16 (fp32) bytes, and element by element otherwise.  Limits: ``M < 2^31``, ``C M < 2^40``.
``MSC.fused_packed(x, activation, dtype)`` returns the ``PackedMaps`` in training and what ``fused`` returns otherwise.

Left out: the input-image pyramid (stock ``F.interpolate``), list outputs of the base (the reference raises on them too) and
add-ons other than the bare sigmoid.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import SpxError

MSC_ACTIVATIONS = {"none": 0, "sigmoid": 1}
_DTYPE_CODE = {torch.bfloat16: 0, torch.float32: 1}


def _describe(shapes, map_dtype, out_dtype, activation: int, maps: Sequence[torch.Tensor] = ()) -> "_lib.SpxMsc":
    """The descriptor of a call on maps of ``shapes``; the forward passes the ``maps`` too, the backward reads their sizes only."""
    a = _lib.SpxMsc()
    a.K, a.B, a.C = len(shapes), int(shapes[0][0]), int(shapes[0][1])
    a.in_dtype, a.out_dtype, a.activation = _DTYPE_CODE[map_dtype], _DTYPE_CODE[out_dtype], activation
    for k, s in enumerate(shapes):
        a.maps[k].h, a.maps[k].w = int(s[2]), int(s[3])
    for k, m in enumerate(maps):
        d = a.maps[k]
        d.data, d.batch_stride, d.channel_stride = m.data_ptr(), int(m.stride(0)), int(m.stride(1))
    return a


class _MscFn(torch.autograd.Function):
    """Both operators.  ``layout`` None: ``msc_max``, the output is [B, C, H, W].  A ``PackedLayout``: ``msc_pack``, the output is
    [C, M] and ``want_index`` says whether the layout ends with the maximum's segment (``with_max``)."""

    @staticmethod
    def forward(ctx, activation, out_dtype, out, want_index, layout, *maps):
        lib = _lib.load()
        B, Cc, H, W = maps[0].shape
        need = any(ctx.needs_input_grad[5:])
        if out is not None:
            ctx.mark_dirty(out)
        y = out if out is not None else torch.empty((B, Cc, H, W) if layout is None else (Cc, layout.M), dtype=out_dtype,
                                                    device=maps[0].device)
        # (msc_max with K = 1 has one candidate: the backward needs no index, a caller that asks for one gets the zeros it is)
        if want_index or (layout is None and need and len(maps) > 1):
            index = torch.empty((B, Cc, H, W), dtype=torch.uint8, device=y.device)
        else:
            index = None
        ctx.shapes, ctx.map_dtype = [tuple(m.shape) for m in maps], maps[0].dtype
        ctx.activation, ctx.out_dtype, ctx.layout, ctx.with_max = activation, out_dtype, layout, want_index
        a = _describe(ctx.shapes, ctx.map_dtype, out_dtype, activation, maps)
        a.out, a.index = y.data_ptr(), None if index is None else index.data_ptr()
        if layout is None:
            _lib.check(lib.spx_msc_max_fwd(C.byref(a), _lib.stream_ptr()))
        else:
            _lib.check(lib.spx_msc_pack_fwd(C.byref(a), int(want_index), _lib.stream_ptr()))
        if need:
            ctx.save_for_backward(y, index)
        if index is None:
            index = torch.empty(0, dtype=torch.uint8, device=y.device)
        ctx.mark_non_differentiable(index)
        return y, index

    @staticmethod
    def backward(ctx, g, _g_index):
        lib = _lib.load()
        y, index = ctx.saved_tensors
        if g.dtype not in _DTYPE_CODE:
            g = g.float()
        g = g.contiguous()
        grads: List[Optional[torch.Tensor]] = [
            torch.empty(s, dtype=ctx.map_dtype, device=g.device) if ctx.needs_input_grad[5 + k] else None
            for k, s in enumerate(ctx.shapes)]
        a = _describe(ctx.shapes, ctx.map_dtype, ctx.out_dtype, ctx.activation)
        a.g_dtype = _DTYPE_CODE[g.dtype]
        for k, t in enumerate(grads):
            a.grads[k] = None if t is None else t.data_ptr()
        a.out, a.g = y.data_ptr(), g.data_ptr()
        a.index = None if index is None else index.data_ptr()
        if ctx.layout is None:
            _lib.check(lib.spx_msc_max_bwd(C.byref(a), _lib.stream_ptr()))
        else:
            _lib.check(lib.spx_msc_pack_bwd(C.byref(a), int(ctx.with_max), _lib.stream_ptr()))
        return (None, None, None, None, None, *grads)


def msc_max(maps: Sequence[torch.Tensor], activation: str = "none", dtype: Optional[torch.dtype] = None,
            out: Optional[torch.Tensor] = None, return_index: bool = False):
    """Pixel-wise maximum over ``maps[0]`` and the bilinearly resampled ``maps[1:]``, then ``activation``, then the cast to
    ``dtype``: one launch.  The contract is the module docstring's.  Returns ``y`` or ``(y, index)``."""
    maps, out_dtype, _ = _check_call("msc_max", maps, activation, dtype, out)
    y, index = _MscFn.apply(MSC_ACTIVATIONS[activation], out_dtype, out, bool(return_index), None, *maps)
    return (y, index) if return_index else y


class PackedLayout:
    """The segment arithmetic of the packed pixel axis, on the host alone: ``grids`` = the (h, w) of every segment in order (for
    the training maps: the K maps, then the first grid again for the maximum), ``B`` the common batch."""

    def __init__(self, B: int, grids: Sequence[Tuple[int, int]]):
        self.B = int(B)
        self.grids = tuple((int(h), int(w)) for h, w in grids)
        if self.B < 1 or not self.grids or any(h < 1 or w < 1 for h, w in self.grids):
            raise SpxError(f"PackedLayout: batch {B} and grids {tuple(grids)} (all >= 1, at least one grid)")
        self.sizes = tuple(self.B * h * w for h, w in self.grids)          # columns per segment
        offs = [0]
        for n in self.sizes:
            offs.append(offs[-1] + n)
        self.offsets, self.M = tuple(offs[:-1]), offs[-1]
        if self.M >= 2 ** 31:
            raise SpxError(f"PackedLayout: {self.M} packed pixels (M < 2^31)")

    @classmethod
    def of_maps(cls, B: int, grids: Sequence[Tuple[int, int]], with_max: bool = True) -> "PackedLayout":
        grids = list(grids)
        return cls(B, grids + ([grids[0]] if with_max else []))

    def __len__(self) -> int:
        return len(self.grids)

    @property
    def segments(self) -> Tuple[Tuple[int, int, int, int], ...]:
        """((off, B, h, w), ...)"""
        return tuple((o, self.B, h, w) for o, (h, w) in zip(self.offsets, self.grids))

    def column(self, k: int, b: int, i: int) -> int:
        h, w = self.grids[k]
        return self.offsets[k] + b * h * w + i

    def view_strides(self, k: int) -> Tuple[int, int, int, int]:
        """Element strides of segment k taken as [B, C, h, w] out of the [C, M] buffer."""
        h, w = self.grids[k]
        return (h * w, self.M, w, 1)

    def view(self, buffer: torch.Tensor, k: int) -> torch.Tensor:
        """Segment k of ``buffer`` ([..., rows, M] contiguous, e.g. [C, M], [1, C, 1, M] or a distance map [1, P, 1, M]) as the
        strided view [B, rows, h, w]."""
        rows = buffer.numel() // self.M
        h, w = self.grids[k]
        return buffer.as_strided((self.B, rows, h, w), self.view_strides(k), buffer.storage_offset() + self.offsets[k])

    def check_labels(self, labels, what: str = "target_labels") -> None:
        if isinstance(labels, torch.Tensor) or len(labels) != len(self.grids):
            n = "a tensor" if isinstance(labels, torch.Tensor) else f"{len(labels)} maps"
            raise SpxError(f"{what}: a list with one label map per segment ({len(self.grids)}), got {n}")
        for k, (t, (h, w)) in enumerate(zip(labels, self.grids)):
            if tuple(t.shape) != (self.B, h, w):
                raise SpxError(f"{what}[{k}] must be [{self.B}, {h}, {w}] (the segment's grid), got {tuple(t.shape)}")

    def pack_labels(self, labels: Sequence[torch.Tensor]) -> torch.Tensor:
        """One [B, h_k, w_k] label map per segment -> the packed label row [1, M], in the maps' common dtype."""
        self.check_labels(labels)
        return torch.cat([t.reshape(-1) for t in labels]).reshape(1, self.M)

    def split_rows(self, t: torch.Tensor) -> Tuple[torch.Tensor, ...]:
        """[M, n] -> the segments' row slices [B h_k w_k, n] (one backward pass assembles their gradients)."""
        return torch.split_with_sizes(t, list(self.sizes), dim=0)

    def split_columns(self, t: torch.Tensor) -> Tuple[torch.Tensor, ...]:
        """[1, R, (1,) M] -> the segments as [B, R, h_k, w_k] views (4-d input) or [B, R, h_k w_k] (3-d input)."""
        R = t.shape[1]
        parts = torch.split_with_sizes(t.reshape(R, self.M), list(self.sizes), dim=1)
        if t.dim() == 4:
            return tuple(p.reshape(R, self.B, h, w).permute(1, 0, 2, 3) for p, (h, w) in zip(parts, self.grids))
        return tuple(p.reshape(R, self.B, h * w).permute(1, 0, 2) for p, (h, w) in zip(parts, self.grids))


@dataclass
class PackedMaps:
    """The result of ``msc_pack``: ``features`` [1, C, 1, M] (contiguous; what ``forward_from_conv_features`` takes), the
    ``layout`` and the uint8 ``index`` [B, C, H, W] of the maximum's segment (None without one)."""

    features: torch.Tensor
    layout: PackedLayout
    index: Optional[torch.Tensor] = None

    @property
    def segments(self):
        return self.layout.segments

    @property
    def M(self) -> int:
        return self.layout.M

    def views(self) -> List[torch.Tensor]:
        """The segments as [B, C, h_k, w_k] views, strides (h_k w_k, M, w_k, 1)."""
        return [self.layout.view(self.features, k) for k in range(len(self.layout))]


def _check_call(who: str, maps, activation: str, dtype, out, with_max: Optional[bool] = None):
    """The argument checks of ``msc_max`` (``with_max`` None) and ``msc_pack``, before any launch -> (maps as a list, the output's
    dtype, the ``PackedLayout`` or None)."""
    if activation not in MSC_ACTIVATIONS:
        raise SpxError(f"{who}: unknown activation {activation!r} (one of {sorted(MSC_ACTIVATIONS)})")
    if isinstance(maps, torch.Tensor):
        maps = [maps]
    maps = list(maps)
    if not 1 <= len(maps) <= _lib.SPX_MSC_MAX_MAPS:
        raise SpxError(f"{who}: {len(maps)} maps (1 to {_lib.SPX_MSC_MAX_MAPS})")
    for k, m in enumerate(maps):
        if m.dtype not in _DTYPE_CODE:
            raise SpxError(f"{who}: map {k} is {m.dtype}; float32 or bfloat16")
        if m.dtype != maps[0].dtype:
            raise SpxError(f"{who}: mixed dtypes ({maps[0].dtype} and {m.dtype})")
        if m.dim() != 4 or min(m.shape) < 1:
            raise SpxError(f"{who}: map {k} must be a non-empty [B, C, h, w], got {tuple(m.shape)}")
        if tuple(m.shape[:2]) != tuple(maps[0].shape[:2]):
            raise SpxError(f"{who}: map {k} has (B, C) = {tuple(m.shape[:2])}, map 0 {tuple(maps[0].shape[:2])}")
        h, w = int(m.shape[2]), int(m.shape[3])
        if (w > 1 and m.stride(3) != 1) or (h > 1 and m.stride(2) != w) or m.stride(0) < 0 or m.stride(1) < 0:
            raise SpxError(f"{who}: the {h} x {w} plane of map {k} is not contiguous (strides {tuple(m.stride())})")
    out_dtype = dtype if dtype is not None else maps[0].dtype
    if out_dtype not in _DTYPE_CODE:
        raise SpxError(f"{who}: dtype {out_dtype}; float32 or bfloat16")
    layout, shape = None, tuple(maps[0].shape)
    if with_max is not None:
        B, Cc = shape[:2]
        layout = PackedLayout.of_maps(B, [tuple(m.shape[2:]) for m in maps], with_max)
        if Cc * layout.M >= 2 ** 40:
            raise SpxError(f"{who}: C * M = {Cc} * {layout.M} (below 2^40)")
        shape = (Cc, layout.M)
    if out is not None:
        if tuple(out.shape) != shape or out.dtype != out_dtype or not out.is_contiguous():
            raise SpxError(f"{who}: out must be a contiguous {out_dtype} {shape}, got {out.dtype} "
                           f"{tuple(out.shape)} with strides {tuple(out.stride())}")
    for k, m in enumerate(maps + ([out] if out is not None else [])):
        _lib.require_gpu(m, f"{who}: out" if k == len(maps) else f"{who}: map {k}")
        if m.device != maps[0].device:
            raise SpxError(f"{who}: {m.device} and {maps[0].device} in one call")
    if out is not None and torch.is_grad_enabled() and any(m.requires_grad for m in maps):
        raise SpxError(f"{who}: out= is for calls without a gradient")
    return maps, out_dtype, layout


def msc_pack(maps: Sequence[torch.Tensor], activation: str = "none", dtype: Optional[torch.dtype] = None,
             with_max: bool = True, out: Optional[torch.Tensor] = None) -> PackedMaps:
    """``act(maps[k])`` at every map's own grid and (``with_max``) the ``msc_max`` of all of them, side by side on one pixel
    axis, cast to ``dtype``: one launch.  The contract is the module docstring's.  Returns a ``PackedMaps``."""
    maps, out_dtype, layout = _check_call("msc_pack", maps, activation, dtype, out, bool(with_max))
    y, index = _MscFn.apply(MSC_ACTIVATIONS[activation], out_dtype, out, bool(with_max), layout, *maps)
    return PackedMaps(features=y.view(1, maps[0].shape[1], 1, layout.M), layout=layout, index=index if with_max else None)


class MSC(nn.Module):
    """Multi-scale inputs (segmentation/utils.py:71-111) on ``msc_max``; see the module docstring."""

    def __init__(self, base: nn.Module, scales=None):
        super().__init__()
        self.base = base
        self.scales = scales if scales is not None else [0.5, 0.75]

    def _run(self, x, activation: Optional[str], dtype, packed: bool = False):
        logits = self.base(x)
        if len(self.scales) == 0:
            return logits if activation is None else self._finish(logits, activation, dtype)
        if isinstance(logits, list):
            raise NotImplementedError("MSC and multiscale outptus are not supported yet.")
        pyramid = []
        for p in self.scales:
            h = F.interpolate(x, scale_factor=p, mode="bilinear", align_corners=False)
            pyramid.append(self.base(h))
        if packed and self.training:
            return msc_pack([logits] + pyramid, activation, dtype, with_max=True)
        if logits.is_cuda:
            fused = msc_max([logits] + pyramid, activation or "none", dtype)
        else:
            if activation is not None:
                _lib.require_gpu(logits, "MSC.fused: the base output")
            _, _, H, W = logits.shape
            up = [F.interpolate(l, size=(H, W), mode="bilinear", align_corners=False) for l in pyramid]
            fused = torch.max(torch.stack([logits] + up), dim=0)[0]
        if not self.training:
            return fused
        singles = [logits] + pyramid
        if activation is not None:
            singles = [self._finish(t, activation, dtype) for t in singles]
        return singles + [fused]

    @staticmethod
    def _finish(t, activation: str, dtype):
        """The activation and the cast alone (the K = 1 launch); a list output of the base element by element."""
        if isinstance(t, list):
            return [msc_max([e], activation, dtype) for e in t]
        return msc_max([t], activation, dtype)

    def forward(self, x):
        return self._run(x, None, None)

    def fused(self, x, activation: str = "sigmoid", dtype: Optional[torch.dtype] = torch.bfloat16):
        """What ``forward`` returns, with ``activation`` and the cast to ``dtype`` applied by the same launch."""
        return self._run(x, activation, dtype)

    def fused_packed(self, x, activation: str = "sigmoid", dtype: Optional[torch.dtype] = torch.bfloat16):
        """In training (with scales): the four maps of ``fused`` as ONE ``PackedMaps`` (``msc_pack``: one launch instead of
        four).  In eval, or with empty ``scales``: what ``fused`` returns."""
        return self._run(x, activation, dtype, packed=True)
