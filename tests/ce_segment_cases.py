"""Cases of the segmented cross entropy (csrc/spx_ce.hip: spx_ce_seg_fwd / _finish / _bwd), shared by
tests/test_ce_segments_cpu.py (are the cases sound?) and tests/test_gpu_ce_segments.py (do the kernels keep the rule?).
A plain module: no fixtures, no device on import, everything seeded, nothing modified by a test.

The rule.  Segment k is the rows [off_k, off_{k+1}) of one [M, K] logits tensor.  For every segment the loss, the lse and pred
rows, the counts and d_logits (given the upstream gradient g_k) carry the BITS the stand-alone path
(``cross_entropy_from_logits``) gives on the contiguous slice: block j of segment k starts at row off_k + 256 j, so a pixel sits
in the lane the stand-alone launch gives it, the wave butterfly and the finish's order are the stand-alone kernels', and the
coefficient is one fp32 division g_k / count_k.  Beside that every segment keeps the float64 bounds of tests/ce_cases.py.

The segment sizes cover every boundary kind: a segment ending one row short of a wave (63), a one-row segment, one that starts a
second block by one row (257), exactly one wave (64), a block and a wave (320); exactly two blocks twice; sixteen segments
(the limit) of mixed small sizes; the Pascal training layout of tests/msc_pack_cases.py (M = 9 528); S = 1, where the segmented
path IS the stand-alone path on the whole tensor."""
import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

import ce_cases as CC
import msc_pack_cases as PC

from scaleprotoseg_amd.msc import PackedLayout

MAX_SEGMENTS = 16
SIXTEEN = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 3, 300, 17, 511, 513)
_P = PC.PASCAL
PASCAL_SIZES = PackedLayout.of_maps(_P["B"], _P["grids"], True).sizes


@dataclass
class SegCase:
    name: str
    logits: torch.Tensor                 # [M, K] fp32
    labels: torch.Tensor                 # [M] int32: class 0..K-1, anything else is ignored
    sizes: Tuple[int, ...]
    nan_segment: Optional[int] = None    # the segment without a valid pixel (loss 0 / 0)
    zero_loss: bool = False              # K = 1: every loss is exactly 0

    @property
    def K(self):
        return int(self.logits.shape[1])

    @property
    def S(self):
        return len(self.sizes)

    @property
    def offsets(self):
        offs = [0]
        for n in self.sizes:
            offs.append(offs[-1] + n)
        return tuple(offs)

    def slices(self):
        """(k, logits[off_k:off_{k+1}], labels[...]) - contiguous row slices (views)."""
        o = self.offsets
        return [(k, self.logits[o[k]:o[k + 1]], self.labels[o[k]:o[k + 1]]) for k in range(self.S)]


#            name              sizes                     K   seed  scale
_SPECS = (("mixed5_k21", (63, 1, 257, 64, 320), 21, 521, 4.0),
          ("one_row_k4", (1,), 4, 14, 1.0),
          ("whole_k33", (833,), 33, 83333, 4.0),                  # S = 1: the stand-alone path whole
          ("two_blocks_k1", (256, 256), 1, 2561, 4.0),
          ("sixteen_k33", SIXTEEN, 33, 1633, 4.0),
          ("sixteen_k4", SIXTEEN, 4, 164, 1.0),
          ("pascal_k21", PASCAL_SIZES, 21, 9528, 4.0),
          ("no_valid_k4", (63, 1, 257, 64, 320), 4, 404, 1.0))
CASE_NAMES = tuple(s[0] for s in _SPECS)


@functools.lru_cache(maxsize=None)
def case(name) -> SegCase:
    spec = {s[0]: s for s in _SPECS}[name]
    _, sizes, K, seed, scale = spec
    gen = torch.Generator().manual_seed(seed)
    M = sum(sizes)
    logits = (torch.randn(M, K, generator=gen) * scale).float()
    labels = torch.cat([CC.mixed_labels(n, K, gen) for n in sizes])      # per segment: row 0 of each is valid
    nan_segment = None
    if name == "no_valid_k4":
        nan_segment = 2                                               # the 257-row one: a whole block and a one-row block
        bad = torch.tensor([-1, -2, K, K + 7, CC.INT32_MIN, CC.INT32_MAX])
        o = sum(sizes[:2])
        labels[o:o + sizes[2]] = bad[torch.arange(sizes[2]) % 6].to(torch.int32)
    return SegCase(name, logits, labels, tuple(sizes), nan_segment, zero_loss=(K == 1))


@functools.lru_cache(maxsize=None)
def references(name):
    """The float64 reference of every slice (tests/ce_cases.py: ``reference``), built once."""
    return tuple(CC.reference(lg, lab) for _, lg, lab in case(name).slices())


def upstream(S, seed):
    """(g_losses [S], g_mean []) fp32: coarse values (exact in fp32, none zero), so that a sum with 0 changes nothing."""
    gen = torch.Generator().manual_seed(seed)
    g = torch.round((torch.rand(S, generator=gen) + 0.25) * 64.0) / 64.0
    return g.float(), torch.tensor(1.75)
