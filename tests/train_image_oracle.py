"""CPU oracle of the training dataloader's transform (pdm/utils/data_utils.py:61-82) -- TEST INFRASTRUCTURE ONLY.

A numpy restatement for CPU tests and for machines without PIL:

  * ``resize``: PIL's 8-bit resampler (Resample.c: ``ImagingResampleHorizontal_8bpc`` / ``Vertical_8bpc``) in numpy integers,
    driven by a coefficient table builder -- ``ops.pil_bilinear_table`` in the tests that check that builder, or this module's
    own ``bilinear_table`` (``precompute_coeffs`` + ``normalize_coeffs_8bpc`` with the triangle filter, vectorised).
    ``tests/golden/train_image_tiny.npz`` pins both against the PIL that generated the fixture, on every pixel.
  * ``crop_flip_normalize``: the crop window, the horizontal flip, ToTensor (``/ 255``) and Normalize (``(v - 0.5) / 0.5``) in
    float32, one IEEE operation each, as torchvision computes them.
  * ``pixel_values``: the two together for a ragged batch.
"""
from __future__ import annotations

import math

import numpy as np
import torch

PRECISION_BITS = 32 - 8 - 2


def bilinear_table(in_size: int, out_size: int):
    """(bounds int32 [out, 2] = (xmin, count), weights int32 [out, ksize]) of PIL's BILINEAR for one axis: the triangle filter
    1 - |x| of support max(in / out, 1) around c = (i + 0.5) in / out over [max(int(c - s + 0.5), 0), min(int(c + s + 0.5), in)),
    normalised to sum 1 and rounded to PRECISION_BITS fractional bits"""
    scale = in_size / out_size
    fscale = max(scale, 1.0)
    support = 1.0 * fscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    weights = np.zeros((out_size, ksize), np.int32)
    for i in range(out_size):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        x = np.abs((np.arange(xmin, xmax).astype(np.float64) - center + 0.5) * (1.0 / fscale))
        w = np.where(x < 1.0, 1.0 - x, 0.0)
        ww = 0.0
        for v in w:                                  # the C loop's summation order
            ww += float(v)
        if ww != 0.0:
            w = w / ww
        fixed = w * float(1 << PRECISION_BITS)
        weights[i, :xmax - xmin] = np.where(w < 0, np.trunc(fixed - 0.5), np.trunc(fixed + 0.5)).astype(np.int32)
        bounds[i] = (xmin, xmax - xmin)
    return bounds, weights


def _resample_axis0(img: np.ndarray, out_size: int, table) -> np.ndarray:
    """one pass along axis 0 of a uint8 array: int32 accumulators starting at one half, arithmetic shift, clamp, uint8"""
    bounds, weights = table(img.shape[0], out_size)
    src = img.astype(np.int64)
    out = np.empty((out_size,) + img.shape[1:], np.uint8)
    tail = (1,) * (img.ndim - 1)
    for i, (x0, n) in enumerate(bounds):
        acc = (src[x0:x0 + n] * weights[i, :n].astype(np.int64).reshape((n,) + tail)).sum(0) + (1 << (PRECISION_BITS - 1))
        assert np.abs(acc).max() < 2 ** 31                # PIL accumulates in int32: nothing here may need more
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize(img: np.ndarray, out_h: int, out_w: int, table=bilinear_table) -> np.ndarray:
    """``PIL.Image.fromarray(img).resize((out_w, out_h), BILINEAR)`` of a uint8 [H, W, C] array: the horizontal pass, then the
    vertical one, each skipped when its size does not change"""
    assert img.dtype == np.uint8 and img.ndim == 3
    if out_w != img.shape[1]:
        img = np.swapaxes(_resample_axis0(np.swapaxes(img, 0, 1), out_w, table), 0, 1)
    if out_h != img.shape[0]:
        img = _resample_axis0(img, out_h, table)
    return np.ascontiguousarray(img)


def resized_size(h: int, w: int, size: int):
    """torchvision's Resize(size) on an (h, w) image: the shorter side to size, the longer to int(size * long / short)"""
    return (size, int(size * w / h)) if h <= w else (int(size * h / w), size)


def crop_flip_normalize(resized: np.ndarray, R: int, top: int, left: int, flip: int) -> torch.Tensor:
    """uint8 [H1, W1, 3] -> float32 [3, R, R]: crop, hflip, ToTensor (uint8 -> float32, / 255), Normalize ((v - 0.5) / 0.5)"""
    assert 0 <= top <= resized.shape[0] - R and 0 <= left <= resized.shape[1] - R
    win = resized[top:top + R, left:left + R]
    if flip:
        win = win[:, ::-1]
    x = torch.from_numpy(np.ascontiguousarray(win)).permute(2, 0, 1).to(torch.float32).div(255)
    return x.sub(0.5).div(0.5).contiguous()


def pixel_values(images, R: int, tops, lefts, flips, table=bilinear_table, resized=None) -> torch.Tensor:
    """a list of uint8 [H, W, 3] arrays -> float32 [B, 3, R, R]; ``resized``: the resized images to use instead of this module's
    own (the fixture's PIL output)"""
    out = []
    for i, im in enumerate(images):
        r = resized[i] if resized is not None else resize(im, *resized_size(im.shape[0], im.shape[1], R), table=table)
        out.append(crop_flip_normalize(r, R, int(tops[i]), int(lefts[i]), int(flips[i])))
    return torch.stack(out)
