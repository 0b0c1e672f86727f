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

Left out: the input-image pyramid (stock ``F.interpolate``), list outputs of the base (the reference raises on them too), add-ons
other than the bare sigmoid, and one ragged launch of the distance kernel over the four training outputs.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import SpxError

MSC_ACTIVATIONS = {"none": 0, "sigmoid": 1}
_DTYPE_CODE = {torch.bfloat16: 0, torch.float32: 1}


def _describe(maps: Sequence[torch.Tensor], out_dtype, activation: int) -> "_lib.SpxMsc":
    a = _lib.SpxMsc()
    a.K, a.B, a.C = len(maps), int(maps[0].shape[0]), int(maps[0].shape[1])
    a.in_dtype, a.out_dtype, a.activation = _DTYPE_CODE[maps[0].dtype], _DTYPE_CODE[out_dtype], activation
    for k, m in enumerate(maps):
        d = a.maps[k]
        d.data, d.batch_stride, d.channel_stride = m.data_ptr(), int(m.stride(0)), int(m.stride(1))
        d.h, d.w = int(m.shape[2]), int(m.shape[3])
    return a


class _MscMaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, activation, out_dtype, out, want_index, *maps):
        lib = _lib.load()
        B, Cc, H, W = maps[0].shape
        need = any(ctx.needs_input_grad[4:])
        if out is not None:
            ctx.mark_dirty(out)
        y = out if out is not None else torch.empty((B, Cc, H, W), dtype=out_dtype, device=maps[0].device)
        # (K = 1 has one candidate: the backward needs no index, a caller that asks for one gets the zeros it is)
        index = torch.empty((B, Cc, H, W), dtype=torch.uint8, device=y.device) if want_index or (need and len(maps) > 1) else None
        a = _describe(maps, out_dtype, activation)
        a.out, a.index = y.data_ptr(), None if index is None else index.data_ptr()
        _lib.check(lib.spx_msc_max_fwd(C.byref(a), _lib.stream_ptr()))
        ctx.activation, ctx.out_dtype = activation, out_dtype
        ctx.shapes = [tuple(m.shape) for m in maps]
        ctx.map_dtype = maps[0].dtype
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
            torch.empty(s, dtype=ctx.map_dtype, device=g.device) if ctx.needs_input_grad[4 + k] else None
            for k, s in enumerate(ctx.shapes)]
        a = _lib.SpxMsc()
        a.K, a.B, a.C = len(ctx.shapes), ctx.shapes[0][0], ctx.shapes[0][1]
        a.in_dtype, a.out_dtype, a.g_dtype = _DTYPE_CODE[ctx.map_dtype], _DTYPE_CODE[ctx.out_dtype], _DTYPE_CODE[g.dtype]
        a.activation = ctx.activation
        for k, s in enumerate(ctx.shapes):
            a.maps[k].h, a.maps[k].w = s[2], s[3]              # (the backward reads the maps' sizes only)
            a.grads[k] = None if grads[k] is None else grads[k].data_ptr()
        a.out, a.g = y.data_ptr(), g.data_ptr()
        a.index = None if index is None else index.data_ptr()
        _lib.check(lib.spx_msc_max_bwd(C.byref(a), _lib.stream_ptr()))
        return (None, None, None, None, *grads)


def msc_max(maps: Sequence[torch.Tensor], activation: str = "none", dtype: Optional[torch.dtype] = None,
            out: Optional[torch.Tensor] = None, return_index: bool = False):
    """Pixel-wise maximum over ``maps[0]`` and the bilinearly resampled ``maps[1:]``, then ``activation``, then the cast to
    ``dtype``: one launch.  The contract is the module docstring's.  Returns ``y`` or ``(y, index)``."""
    if activation not in MSC_ACTIVATIONS:
        raise SpxError(f"msc_max: unknown activation {activation!r} (one of {sorted(MSC_ACTIVATIONS)})")
    if isinstance(maps, torch.Tensor):
        maps = [maps]
    maps = list(maps)
    if not 1 <= len(maps) <= _lib.SPX_MSC_MAX_MAPS:
        raise SpxError(f"msc_max: {len(maps)} maps (1 to {_lib.SPX_MSC_MAX_MAPS})")
    for k, m in enumerate(maps):
        if m.dtype not in _DTYPE_CODE:
            raise SpxError(f"msc_max: map {k} is {m.dtype}; float32 or bfloat16")
        if m.dtype != maps[0].dtype:
            raise SpxError(f"msc_max: mixed dtypes ({maps[0].dtype} and {m.dtype})")
        if m.dim() != 4 or min(m.shape) < 1:
            raise SpxError(f"msc_max: map {k} must be a non-empty [B, C, h, w], got {tuple(m.shape)}")
        if tuple(m.shape[:2]) != tuple(maps[0].shape[:2]):
            raise SpxError(f"msc_max: map {k} has (B, C) = {tuple(m.shape[:2])}, map 0 {tuple(maps[0].shape[:2])}")
        h, w = int(m.shape[2]), int(m.shape[3])
        if (w > 1 and m.stride(3) != 1) or (h > 1 and m.stride(2) != w) or m.stride(0) < 0 or m.stride(1) < 0:
            raise SpxError(f"msc_max: the {h} x {w} plane of map {k} is not contiguous (strides {tuple(m.stride())})")
    out_dtype = dtype if dtype is not None else maps[0].dtype
    if out_dtype not in _DTYPE_CODE:
        raise SpxError(f"msc_max: dtype {out_dtype}; float32 or bfloat16")
    if out is not None:
        if tuple(out.shape) != tuple(maps[0].shape) or out.dtype != out_dtype or not out.is_contiguous():
            raise SpxError(f"msc_max: out must be a contiguous {out_dtype} {tuple(maps[0].shape)}, got {out.dtype} "
                           f"{tuple(out.shape)} with strides {tuple(out.stride())}")
    for k, m in enumerate(maps + ([out] if out is not None else [])):
        _lib.require_gpu(m, "msc_max: out" if k == len(maps) else f"msc_max: map {k}")
        if m.device != maps[0].device:
            raise SpxError(f"msc_max: {m.device} and {maps[0].device} in one call")
    if out is not None:
        if torch.is_grad_enabled() and any(m.requires_grad for m in maps):
            raise SpxError("msc_max: out= is for calls without a gradient")
    y, index = _MscMaxFn.apply(MSC_ACTIVATIONS[activation], out_dtype, out, bool(return_index), *maps)
    return (y, index) if return_index else y


class MSC(nn.Module):
    """Multi-scale inputs (segmentation/utils.py:71-111) on ``msc_max``; see the module docstring."""

    def __init__(self, base: nn.Module, scales=None):
        super().__init__()
        self.base = base
        self.scales = scales if scales is not None else [0.5, 0.75]

    def _run(self, x, activation: Optional[str], dtype):
        logits = self.base(x)
        if len(self.scales) == 0:
            return logits if activation is None else self._finish(logits, activation, dtype)
        if isinstance(logits, list):
            raise NotImplementedError("MSC and multiscale outptus are not supported yet.")
        pyramid = []
        for p in self.scales:
            h = F.interpolate(x, scale_factor=p, mode="bilinear", align_corners=False)
            pyramid.append(self.base(h))
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
