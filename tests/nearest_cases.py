"""The reference-recorded cases of the nearest-image / nearest-prototype analysis (tools/gen_nearest_golden.py), shared by
tests/test_nearest_cpu.py and tests/test_gpu_nearest.py.  The crop-chain cases extend those of tests/golden/push_boxes.npz: the
planes, labels and flat indices come from that fixture, the third label image and the recorded rows from nearest_analysis.npz."""
import functools

import numpy as np

from support import load_cases, planes_of

NEAREST = load_cases("nearest_analysis")
PUSH_BOX = load_cases("push_boxes")
CROP_CASES = sorted(name for name in NEAREST if name not in ("images", "protos"))


@functools.lru_cache(maxsize=None)
def crop_case(name):
    """dict: planes fp32 [3, P, h, w] (image 2 holds every prototype's winning plane again), labels uint8 [3, H, W], rows int64
    [R, 5] = (label image = plane image, prototype, label value L, flat latent index, masking) and the recorded fields."""
    rec, base = NEAREST[name], PUSH_BOX[name]
    planes = planes_of(base)
    img = base["img"]
    third = np.stack([planes[img[p], p] for p in range(planes.shape[1])])
    out = dict(rec)
    out["planes"] = np.concatenate([planes, third[None]]).astype(np.float32)
    out["labels"] = np.concatenate([base["labels"], rec["third"][None]])
    out["exact"] = name.startswith("exact")
    return out
