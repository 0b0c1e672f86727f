"""Cross-scale aggregation heads (segmentation/model/scale_head.py) on the aggregation kernel.

``WeightedAgg(output_type, channel_dim=...)`` feeds a scale's features the activations of the scale above it:
``s = sum_p prototypes[p] . activations[:, p]`` combined with ``x`` by ``OutSum`` ((x + s) / 2), ``OutMult`` (sqrt(x . s)) or
``OutConcat`` (sigmoid(Linear(cat(x, s)))).  Constructor arguments, attribute names and ``state_dict`` keys are the reference's
(``output_layer.linear_block.0.{weight,bias}`` for "concat", none for the others), so its checkpoints load as they are.
``s`` and the sum / mult combine are one HIP launch (``functional.scale_aggregate``); the [B, Pn, Cs, H, W] product the reference
sums over is never formed.  The concat head's Linear + Sigmoid is stock torch on the NHWC view of (x, s).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .functional import scale_aggregate


class OutSum(nn.Module):
    """(x + s) / 2, fused into the aggregation kernel's epilogue."""

    kernel_mode = "sum"

    def forward(self, x: torch.Tensor, scale_x: torch.Tensor) -> torch.Tensor:
        return (x + scale_x) / 2


class OutMult(nn.Module):
    """sqrt(x . s), fused into the aggregation kernel's epilogue."""

    kernel_mode = "mult"

    def forward(self, x: torch.Tensor, scale_x: torch.Tensor) -> torch.Tensor:
        return torch.sqrt(x * scale_x)


class OutConcat(nn.Module):
    """sigmoid(Linear_{2 Cs -> Cs}(cat(x, s))) per pixel; the kernel hands out ``s``, this layer runs on it as stock torch."""

    kernel_mode = "none"

    def __init__(self, channel_dim: int) -> None:
        super().__init__()
        self.linear_block = nn.Sequential(nn.Linear(2 * channel_dim, channel_dim), nn.Sigmoid())

    def forward(self, x: torch.Tensor, scale_x: torch.Tensor) -> torch.Tensor:
        nhwc = torch.cat((x.to(scale_x.dtype), scale_x), dim=1).permute(0, 2, 3, 1)
        return self.linear_block(nhwc).permute(0, 3, 1, 2)


def factory_output_layer(output_type: str, **kwargs) -> nn.Module:
    """The combine layer of ``WeightedAgg`` by name; the keyword arguments (``channel_dim``) reach "concat" only, as upstream."""
    if output_type == "sum":
        return OutSum()
    if output_type == "mult":
        return OutMult()
    if output_type == "concat":
        return OutConcat(**kwargs)
    raise NotImplementedError(f"Unknown output type: {output_type}")


class WeightedAgg(nn.Module):
    def __init__(self, output_type: str, **kwargs) -> None:
        super().__init__()
        self.output_layer = factory_output_layer(output_type, **kwargs)

    def _combine(self, x, source, prototypes, **source_args):
        mode = self.output_layer.kernel_mode
        out = scale_aggregate(x, source, prototypes, mode=mode, **source_args)
        return self.output_layer(x, out) if mode == "none" else out

    def forward(self, x: torch.Tensor, activations: torch.Tensor, prototypes: torch.Tensor) -> torch.Tensor:
        """x [B, Cs, H, W], activations [B, Pn, H, W], prototypes [Pn, Cs, 1, 1] (or [Pn, Cs]) -> fp32 [B, Cs, H, W]."""
        return self._combine(x, activations, prototypes, source_kind="activations")

    def from_distances(self, x: torch.Tensor, distances: torch.Tensor, prototypes: torch.Tensor, activation: str,
                       epsilon: float) -> torch.Tensor:
        """The same on the distance map of the scale above: the built-in similarity is applied inside the kernel."""
        return self._combine(x, distances, prototypes, source_kind="distances", activation=activation, epsilon=epsilon)
