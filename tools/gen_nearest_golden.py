"""Write tests/golden/nearest_analysis.npz by driving the reference's own ``nearest_img.min_across_dataset``,
``nearest_proto.min_on_sample`` (segmentation/analysis) and ``helpers.find_continuous_high_activation_crop`` (CPU only).

    SPX_REFERENCE=/path/to/ScaleProtoSeg python tools/gen_nearest_golden.py [output.npz]

The functions are loaded from the reference checkout with the stand-ins of tools/reference_stubs.py around them, a fake
``ppnet`` that returns prepared bf16-representable distances and a fake dataset whose "image files" carry a size and an index.
Data only is recorded, keys ``<case>__<field>``:

* ``images``: 5 images, P = 8, grid 9 x 11: the distances, the reference's ``top_n_idx`` [n, P] and per-image indices.
* ``protos``: ``min_on_sample`` twice under a fixed ``torch.manual_seed``: the distances [1, P, 9, 11], the sampled pixels, the
  include lists (the second drops most of the near prototypes, so a list comes back short) and the lists, padded with -1.
* the crop chain over the cases of tests/golden/push_boxes.npz (the four ``log_*`` shapes and the identity case; planes, labels
  and flat indices are read from that fixture and not stored again) plus a third label image per case with a void block under
  one patch and a class of exactly one pixel.  Per row = (label image, prototype, masking) the reference's expressions
  ``np.bincount(...).argmax()``, ``np.percentile(u32, 95)``, ``np.percentile(u32[y_mask], 95)`` (``np.inf`` on an empty mask) and
  ``find_continuous_high_activation_crop(u32 * y_mask, rf, threshold)`` for both thresholds, with the robustness flags of
  tests/nearest_restatement.py.  The maskings: the prototype's own class (the push, :476-484) and the patch's majority class
  (nearest_img.py:260-300).

The tool asserts that the restatement equals the reference in every recorded row, that no two of the n + 1 smallest values of
a column tie, that each case has at most 1 non-robust row in 8 per masking (none in the identity case), and that between them
the cases hold an absent class (+inf), a class of exactly one pixel, a void-majority patch and a gt crop that differs from the
all-pixel crop."""
from __future__ import annotations

import os
import tempfile

import numpy as np
import torch

import reference_stubs as S
import nearest_restatement as NR
import overlap_restatement as R
import push_boxes_restatement as PB

N_NEAR = 3
EPS = 1e-4


class _Net:
    def __init__(self, distances):
        self.distances = distances
        self.num_prototypes = distances.shape[1]

    def to(self, _):
        return self

    def eval(self):
        return self

    def __call__(self, x, return_activations=False):
        return None, self.distances[x.n:x.n + 1]


class _Data:
    image_margin_size = 0
    convert_targets = None

    def __init__(self, root, count, H, W):
        self.annotations_dir = root
        self.img_ids = [f"img{n}" for n in range(count)]
        for n, i in enumerate(self.img_ids):
            np.save(os.path.join(root, i + ".npy"), np.zeros((H, W), np.int64))
            with open(self.get_img_path(i), "w") as fp:
                fp.write(f"{H} {W} {n}")

    def __len__(self):
        return len(self.img_ids)

    def get_img_path(self, i):
        return os.path.join(self.annotations_dir, i + ".img")


def _pool(lo, hi):
    """Every bf16 value in [lo, hi), ascending."""
    return S.bf16(torch.linspace(lo, hi, 1 << 16)).unique()


def _image_distances(g, N, P, h, w):
    """bf16-representable distances in [0.5, 3.5) with one distinct minimum below 0.5 per (image, prototype): no two minima tie."""
    d = S.bf16(0.5 + 3.0 * torch.rand(N, P, h * w, generator=g))
    low = _pool(0.0625, 0.5)
    low = low[torch.randperm(low.numel(), generator=g)[:N * P]].reshape(N, P, 1)
    d.scatter_(2, torch.randint(0, h * w, (N, P, 1), generator=g), low)
    return d.reshape(N, P, h, w).contiguous()


def _pixel_distances(g, P, h, w):
    """[1, P, h, w]: at every pixel P distinct bf16 values, so no two prototypes tie anywhere."""
    pool = _pool(0.25, 3.9)
    cols = [pool[torch.randperm(pool.numel(), generator=g)[:P]] for _ in range(h * w)]
    return torch.stack(cols, dim=1).reshape(1, P, h, w).contiguous()


def _images_case(IMG):
    g = torch.Generator().manual_seed(20250301)
    N, P, h, w = 5, 8, 9, 11
    d = _image_distances(g, N, P, h, w)
    with tempfile.TemporaryDirectory() as root:
        top, list_idx = IMG.min_across_dataset(_Data(root, N, 36, 44), _Net(d), device="cpu", n=N_NEAR)
    minima = d.flatten(2).min(-1).values.numpy()                              # [N, P]
    for p in range(P):
        col = np.sort(minima[:, p])[:N_NEAR + 1]
        assert len(set(col.tolist())) == len(col), "a tie among the n + 1 smallest minima"
    want, _ = NR.topk_images(minima, N_NEAR)
    assert np.array_equal(want, top.numpy().T), "topk_images != the reference"
    flat = torch.cat(list_idx, 0).numpy()
    assert np.array_equal(flat, d.flatten(2).numpy().argmin(-1))
    return {"images__distances": d.numpy(), "images__top": top.numpy().astype(np.int64), "images__flat": flat.astype(np.int64)}


def _protos_case(PRO):
    g = torch.Generator().manual_seed(20250302)
    P, h, w = 40, 9, 11
    d = _pixel_distances(g, P, h, w)
    out = {"protos__distances": d.numpy()}
    includes = (list(range(0, P, 2)) + [1, 7], [3, 11, 19, 38])
    with tempfile.TemporaryDirectory() as root:
        data = _Data(root, 1, 36, 44)
        for t, include in enumerate(includes):
            torch.manual_seed(78 + t)             # seeds whose pixels have a nearest prototype outside the include list
            lists, (ys, xs) = PRO.min_on_sample(data, _Net(d), 0, device="cpu", n=N_NEAR, include_list=include)
            padded = np.full((N_NEAR, N_NEAR), -1, np.int64)
            for r, (lst, y, x) in enumerate(zip(lists, ys.tolist(), xs.tolist())):
                col = d[0, :, y, x].numpy()
                assert len(set(np.sort(col)[:N_NEAR + 11].tolist())) == N_NEAR + 11
                assert lst == NR.nearest_protos(col, N_NEAR, include, N_NEAR + 10), "nearest_protos != the reference"
                padded[r, :len(lst)] = lst
            out[f"protos__include{t}"] = np.array(include, np.int64)
            out[f"protos__pixels{t}"] = np.stack([np.zeros(N_NEAR, np.int64), ys.numpy(), xs.numpy()], axis=1)
            out[f"protos__lists{t}"] = padded
    assert (out["protos__lists1"] == -1).any(), "the short include list must leave a list short"
    near = [NR.nearest_protos(d[0, :, y, x].numpy(), 1)[0] for _, y, x in out["protos__pixels0"]]
    assert any(p not in includes[0] for p in near), "the include list must drop a nearest prototype"
    return out


def third_labels(labels):
    """Image 0's labels with a void block under the peak of prototype 2 and exactly one pixel of class 3 (label 4)."""
    lab = labels[0].copy()
    H, W = lab.shape
    lab[int(0.3 * H):int(0.7 * H), int(0.08 * W):int(0.45 * W)] = 0
    lab[1, W // 2] = 4
    return lab


def _crop_case(name, case, HELP, feats):
    d = case["distances"]
    kind = str(case["kind"])
    planes = (np.float32(4.0) - d) if kind == "linear" else np.log((d + 1) / (d + EPS))
    assert planes.dtype == np.float32
    labels = np.concatenate([case["labels"], third_labels(case["labels"])[None]])
    img, flat, cls = case["img"], case["flat"], case["ident"].argmax(1)
    P, (h, w), (H, W) = len(img), planes.shape[2:], labels.shape[1:]
    worst = 0.0
    rows, rec = [], {k: [] for k in ("majority", "threshold", "threshold_gt", "box", "box_gt", "robust", "robust_gt")}
    for masking in (0, 1):                                                    # 0: the prototype's class, 1: the patch majority
        for n in (None, 2):                                                   # the winning image's labels, the third image's
            for p in range(P):
                lab = labels[img[p] if n is None else n]
                plane = planes[img[p], p]
                u32 = R.upsample(plane, (H, W)).astype(np.float32)            # the stubs' cv2.resize
                rf = PB.rf_box(int(flat[p]), h, w, H, W)
                major = int(np.bincount(lab[rf[0]:rf[1], rf[2]:rf[3]].flatten().astype(np.int64)).argmax())
                assert major == NR.patch_majority(lab, rf)
                L = int(cls[p]) + 1 if masking == 0 else major
                y_mask = lab == L
                T = np.percentile(u32, 95)
                T_gt = np.inf if np.sum(y_mask) == 0 else np.percentile(u32[y_mask], 95)
                box = HELP.find_continuous_high_activation_crop(u32 * y_mask, rf, threshold=T)
                box_gt = HELP.find_continuous_high_activation_crop(u32 * y_mask, rf, threshold=T_gt)
                mine = NR.gt_boxes(plane, lab, L, int(flat[p]), threshold=np.float32(T), u32=u32)
                mine_gt = NR.gt_boxes(plane, lab, L, int(flat[p]), threshold=np.float32(T_gt), u32=u32)
                assert mine["rf"] == rf and mine["box"] == list(box) and mine_gt["box"] == list(box_gt), (name, masking, n, p)
                # the definition's form of the quantile (rank and gamma in float64, as np.percentile of the float64 copy gives
                # them) against numpy on float32 input, which forms gamma from a float32 virtual index: (count / 2^24) of the
                # gap between the two order statistics apart, a fraction of the margin here and nothing on the identity grid
                restated = NR.masked_threshold(u32, y_mask)
                gap = 0.0 if restated == np.float32(T_gt) else abs(float(restated) - float(T_gt))
                worst = max(worst, gap / max(R.margin(plane), 1e-30))
                assert gap <= (0.0 if kind == "linear" else R.margin(plane) / 4), (name, masking, n, p, restated, T_gt)
                count = int(y_mask.sum())
                feats |= {f for f, hit in (("absent", count == 0), ("one_pixel", count == 1), ("void_majority", major == 0),
                                           ("gt_differs", list(box) != list(box_gt))) if hit}
                rows.append([img[p] if n is None else n, p, L, int(flat[p]), masking])
                for k, v in (("majority", major), ("threshold", np.float32(T)), ("threshold_gt", np.float32(T_gt)), ("box", box),
                             ("box_gt", box_gt), ("robust", mine["robust"]), ("robust_gt", mine_gt["robust"])):
                    rec[k].append(v)
    rows = np.array(rows, np.int64)
    robust, robust_gt = np.array(rec["robust"]), np.array(rec["robust_gt"])
    exact = kind == "linear"
    for masking in (0, 1):
        sel = rows[:, 4] == masking
        for flags in (robust[sel], robust_gt[sel]):
            bad = int((~flags).sum())
            assert bad <= (0 if exact else int(sel.sum()) // 8), (name, masking, bad)
    differ = int(sum(list(a) != list(b) for a, b in zip(rec["box"], rec["box_gt"])))
    print(name, "rows", len(rows), "non-robust", int((~robust).sum()), int((~robust_gt).sum()), "gt crop differs in", differ,
          "restated threshold within", worst, "of the margin")
    out = dict(third=labels[2], rows=rows, majority=np.array(rec["majority"], np.int64), threshold=np.array(rec["threshold"], np.float32),
               threshold_gt=np.array(rec["threshold_gt"], np.float32), box=np.array(rec["box"], np.int64),
               box_gt=np.array(rec["box_gt"], np.int64), robust=robust, robust_gt=robust_gt)
    return {f"{name}__{k}": v for k, v in out.items()}


def main():
    S.stub_modules()
    S.mod("segmentation.utils", non_zero_proto=None)
    HELP = S.load("helpers.py", "helpers")
    IMG = S.load(os.path.join("segmentation", "analysis", "nearest_img.py"), "ref_nearest_img")
    PRO = S.load(os.path.join("segmentation", "analysis", "nearest_proto.py"), "ref_nearest_proto")
    cases = {}
    cases.update(_images_case(IMG))
    cases.update(_protos_case(PRO))
    z = np.load(os.path.join(S.HERE, "..", "tests", "golden", "push_boxes.npz"))
    feats = set()
    for name in ("log_s5x7", "log_s9x11", "log_s17x17", "log_s33x65", "exact_70x85"):
        case = {k.split("__")[1]: z[k] for k in z.files if k.startswith(name + "__")}
        cases.update(_crop_case(name, case, HELP, feats))
    want = {"absent", "one_pixel", "void_majority", "gt_differs"}
    assert want <= feats, want - feats
    out = S.out_path("nearest_analysis.npz")
    np.savez_compressed(out, **cases)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
