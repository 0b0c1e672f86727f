"""The definition of the training-batch preparation (scaleprotoseg_amd/batch.py, include/spx_hip.h) in NumPy: a helper of the batch
tests and of tools/gen_batch_golden.py, not a test file.

* the label path through PIL itself, written as the reference writes it (segmentation/data/dataset.py:134-186 and resize_label of
  dataset.py:22-30): id table, int32, ``Image.resize(NEAREST)``, zero pad, crop, flip, and ``resize_label`` per latent grid;
* the image path in float32, operation by operation as include/spx_hip.h states it (the library is built with -ffp-contract=off,
  so this matches the kernel bit for bit), and the normalisation of the same bytes once more in float64."""
from __future__ import annotations

import numpy as np
from PIL import Image

F = np.float32


def convert(label: np.ndarray, id_map) -> np.ndarray:
    """``convert_targets`` as a table: raw value -> class id, 0 for a raw value outside the table."""
    label = np.asarray(label).astype(np.int64)
    if id_map is None:
        return label
    table = np.asarray(id_map, dtype=np.int64)
    ok = (label >= 0) & (label < table.size)
    return np.where(ok, table[np.clip(label, 0, table.size - 1)], 0)


def resize_label(label: np.ndarray, size) -> np.ndarray:
    """dataset.py:22-30; size is (W, H)."""
    return np.asarray(Image.fromarray(label.astype(float)).resize(size, resample=Image.NEAREST)).astype(np.int64)


def window_label(label_raw, id_map, scaled, origin, flip, window) -> np.ndarray:
    """dataset.py:134-136, 152-153, 158-186 for the label."""
    label = convert(label_raw, id_map).astype(np.int32)
    hs, ws = scaled
    label = np.asarray(Image.fromarray(label).resize((ws, hs), resample=Image.NEAREST), dtype=np.int64)
    pad_h, pad_w = max(window[0] - hs, 0), max(window[1] - ws, 0)
    if pad_h > 0 or pad_w > 0:
        label = np.pad(label, ((0, pad_h), (0, pad_w)), constant_values=0)
    label = label[origin[0]:origin[0] + window[0], origin[1]:origin[1] + window[1]]
    if flip:
        label = np.fliplr(label).copy()
    return label


def latent_labels(window_lab: np.ndarray, grids):
    return [resize_label(window_lab, (w, h)) for h, w in grids]


def shifted_i32(lab: np.ndarray) -> np.ndarray:
    """functional.shifted_labels_i32: v - 1, and -1 where that leaves int32."""
    w = lab.astype(np.int64) - 1
    return np.where((w < -2147483647) | (w > 2147483647), -1, w).astype(np.int32)


def _axis(d: np.ndarray, n_in: int, n_out: int):
    """Source indices and weight of OpenCV's INTER_LINEAR sample position along one axis, in float32."""
    r = F(n_in) / F(n_out)
    f = (d.astype(F) + F(0.5)) * r - F(0.5)
    f = np.where(f < 0, F(0), f).astype(F)
    fl = np.floor(f)
    i0 = fl.astype(np.int64)
    frac = (f - fl).astype(F)
    i1 = np.minimum(i0 + 1, n_in - 1)
    edge = i0 >= n_in - 1
    i0 = np.where(edge, n_in - 1, i0)
    i1 = np.where(edge, n_in - 1, i1)
    frac = np.where(edge, F(0), frac).astype(F)
    return i0, i1, frac


def window_bytes(image: np.ndarray, scaled, origin, flip, window, round_u8: bool = True):
    """(r float32 [3, Hc, Wc], inside bool [Hc, Wc]): the bilinear value of every window pixel inside the scaled image (rounded to a
    byte level with ``round_u8``), 0 in the pad."""
    h, w = image.shape[:2]
    hs, ws = scaled
    Hc, Wc = window
    x = np.arange(Wc)
    sx = origin[1] + (Wc - 1 - x if flip else x)
    sy = origin[0] + np.arange(Hc)
    inside = (sy < hs)[:, None] & (sx < ws)[None, :]
    x0, x1, a = _axis(np.minimum(sx, ws - 1), w, ws)
    y0, y1, b = _axis(np.minimum(sy, hs - 1), h, hs)
    img = image.astype(F)
    a, b = a[None, :, None], b[:, None, None]
    ia, ib = F(1) - a, F(1) - b
    p00, p01 = img[y0][:, x0], img[y0][:, x1]
    p10, p11 = img[y1][:, x0], img[y1][:, x1]
    v = ((p00 * ia + p01 * a) * ib + (p10 * ia + p11 * a) * b).astype(F)
    r = np.rint(v) if round_u8 else v
    r = np.where(inside[:, :, None], r, F(0)).astype(F)
    return np.ascontiguousarray(r.transpose(2, 0, 1)), inside


def window_image_f32(image, scaled, origin, flip, window, mean, std, normalize=True, round_u8=True) -> np.ndarray:
    """The kernel's fp32 output, [3, Hc, Wc]: every operation rounded to float32."""
    r, inside = window_bytes(image, scaled, origin, flip, window, round_u8)
    m = np.asarray(mean, dtype=F)[:, None, None]
    s = np.asarray(std, dtype=F)[:, None, None]
    v = (r / F(255.0)).astype(F)
    if normalize:
        v = ((v - m).astype(F) / s).astype(F)
        return np.where(inside[None], v, F(0)).astype(F)
    return np.where(inside[None], v, np.broadcast_to(m, v.shape)).astype(F)


def window_image_f64(image, scaled, origin, flip, window, mean, std, normalize=True, round_u8=True) -> np.ndarray:
    """The same bytes normalised in float64, as the reference does (dataset.py:156, transforms.Normalize on a float64 tensor)."""
    r, inside = window_bytes(image, scaled, origin, flip, window, round_u8)
    m = np.asarray(mean, dtype=np.float64)[:, None, None]
    s = np.asarray(std, dtype=np.float64)[:, None, None]
    v = r.astype(np.float64) / 255.0
    if normalize:
        return np.where(inside[None], (v - m) / s, 0.0)
    return np.where(inside[None], v, np.broadcast_to(m, v.shape))


def window_image_u8(image, scaled, origin, flip, window, mean) -> np.ndarray:
    """The uint8 output: the byte itself, rint(mean * 255) saturated in the pad."""
    r, inside = window_bytes(image, scaled, origin, flip, window, True)
    pad = np.clip(np.rint(np.asarray(mean, dtype=F) * F(255.0)), 0, 255).astype(F)[:, None, None]
    return np.where(inside[None], r, np.broadcast_to(pad, r.shape)).astype(np.uint8)


def image_bound(ref64: np.ndarray, mean, std, normalize=True) -> np.ndarray:
    """|fp32 output - float64 restatement| allowed: the three fp32 roundings of r / 255, - mean and / std (and of mean and std
    themselves): 2^-23 (1 + |mean_c|) / std_c + 2^-23 |ref|.  Without normalisation one rounding of r / 255 <= 1: 2^-24."""
    if not normalize:
        return np.full(ref64.shape, 2.0 ** -24)
    m = np.abs(np.asarray(mean, dtype=np.float64))[:, None, None]
    s = np.abs(np.asarray(std, dtype=np.float64))[:, None, None]
    return 2.0 ** -23 * (1.0 + m) / s + 2.0 ** -23 * np.abs(ref64)
