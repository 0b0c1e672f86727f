"""The recorded MSC cases (tests/golden/msc_features*.npz, tools/gen_msc_golden.py) and their float64 restatement, computed once
and shared by tests/test_msc_cpu.py and tests/test_gpu_msc.py.  Nothing here is modified by a test."""
import functools

import msc_restatement as MR
from support import load_cases

SHAPE_SETS = ("odd", "one_up", "pascal41", "pascal65", "wide")      # B = 2, C = 5, randn
SPECIAL = ("tie", "nan")


@functools.lru_cache(maxsize=None)
def case(name):
    """The fixture's fields of one case plus ``maps`` (the list map0, map1, ...)."""
    cases = dict(load_cases("msc_features"))
    cases.update(load_cases("msc_features_pascal65"))
    c = dict(cases[name])
    c["maps"] = [c[f"map{k}"] for k in range(sum(1 for f in c if f.startswith("map")))]
    return c


@functools.lru_cache(maxsize=None)
def restated(name):
    """MR.forward of the case's maps: (z, index, bound of z, u, bound of every candidate)."""
    return MR.forward(case(name)["maps"])
