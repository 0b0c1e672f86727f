"""The recorded MSC cases (tests/golden/msc_features*.npz, tools/gen_msc_golden.py), one seeded case of eight maps and their
float64 restatement, computed once and shared by tests/test_msc_cpu.py and tests/test_gpu_msc*.py.  Nothing here is modified by a
test."""
import functools

import numpy as np

import msc_restatement as MR
from support import load_cases

SHAPE_SETS = ("odd", "one_up", "pascal41", "pascal65", "wide")      # B = 2, C = 5, randn
SPECIAL = ("tie", "nan")
# "eight": as many maps as the kernels take (SPX_MSC_MAX_MAPS), generated here - a 1 x 1 source, a repeated grid, sources smaller
# and larger than the target.  Every map wins at least 45 of the 630 pixels and float64 decides them all (tests/test_msc_cpu.py).
# M = 880 with the maximum's segment (a multiple of 4: the vector path) and 754 without.  EIGHT_NEEDS leaves empty ranges of the
# backward's prefix sums at the front (map 1), in the middle (map 4) and next to the end (map 6).
EIGHT_GRIDS = ((7, 9), (1, 1), (4, 5), (6, 7), (9, 11), (3, 3), (7, 9), (8, 10))
EIGHT_NEEDS = (True, False, True, True, False, True, False, True)


@functools.lru_cache(maxsize=None)
def case(name):
    """The fixture's fields of one case plus ``maps`` (the list map0, map1, ...); "eight": ``maps`` and ``g`` alone."""
    if name == "eight":
        rng = np.random.default_rng(0)
        maps = [rng.standard_normal((2, 5, h, w)).astype(np.float32) for h, w in EIGHT_GRIDS]
        return {"maps": maps, "g": rng.standard_normal(maps[0].shape).astype(np.float32)}
    cases = dict(load_cases("msc_features"))
    cases.update(load_cases("msc_features_pascal65"))
    c = dict(cases[name])
    c["maps"] = [c[f"map{k}"] for k in range(sum(1 for f in c if f.startswith("map")))]
    return c


@functools.lru_cache(maxsize=None)
def restated(name):
    """MR.forward of the case's maps: (z, index, bound of z, u, bound of every candidate)."""
    return MR.forward(case(name)["maps"])
