"""Antialiased bilinear resampling of uint8 images as ``resize_image`` defines it (torchvision's ``Resize(image_hw, antialias=True)``:
``torch._upsample_bilinear2d_aa`` with ``align_corners=False``, then round-half-even and a clamp to 0 .. 255), in the form the device
kernel takes (csrc/resize_aa.hip, ``yogo_resize_aa_u8``): per axis one tap table made here, on the host.

``aa_taps(n_in, n_out)``: for output ``i`` the first source index ``start[i]`` and ``K`` weights, zero-padded; in fp64, normalised,
then rounded to fp32.  ``scale = n_in / n_out``, ``support = max(scale, 1)``, ``c = scale * (i + 0.5)``, the taps are
``lo = max(0, int(c - support + 0.5)) <= j < hi = min(n_in, int(c + support + 0.5))`` with the triangle weights
``max(0, 1 - |(j - c + 0.5) / support|)`` divided by their sum.  ``K`` is the longest run ``hi - lo`` of the axis: 4 for an exact 2 x
down-scale, 2 or 3 for an up-scale, at most 2 * scale + 1 otherwise (17 at 8 x).  Every ``start[i] + j`` with a non-zero weight lies in
``[0, n_in)`` by construction.

``resize_aa_host`` is the numpy twin of the kernel: the same tables, the horizontal pass first into an fp32 intermediate, then the
vertical one, each sum in ascending tap order, every step rounded to fp32 (a fused multiply-add: the product is exact in fp64, the sum
is rounded to fp64 and then to fp32), then ``rint`` (half-even) and the clamp.  It is what the tests without a GPU hold to the
definition; nothing on the hot path runs it.

The device serves down-scaling up to ``MAX_DOWNSCALE`` per axis (``K <= MAX_TAPS``) and any up-scaling; ``device_serves`` says so.
"""
from __future__ import annotations

from functools import lru_cache
from typing import Tuple

import numpy as np

MAX_DOWNSCALE = 8
MAX_TAPS = 18


def device_serves(n_in: int, n_out: int) -> bool:
    """one axis n_in -> n_out is within what yogo_resize_aa_u8 takes"""
    return 1 <= n_in <= 65535 and 1 <= n_out <= 65535 and n_in <= MAX_DOWNSCALE * n_out


@lru_cache(maxsize=64)
def aa_taps(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray]:
    """-> (start int32 [n_out], weights float32 [n_out, K]) of one axis; cached per size pair, read-only"""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"aa_taps: sizes {n_in} -> {n_out} must be at least 1")
    scale = n_in / n_out
    support = max(scale, 1.0)
    inv = 1.0 / support
    c = scale * (np.arange(n_out, dtype=np.float64) + 0.5)
    lo = np.maximum(0, (c - support + 0.5).astype(np.int64))   # (astype truncates towards zero, as C's int() does)
    hi = np.minimum(n_in, (c + support + 0.5).astype(np.int64))
    K = int((hi - lo).max())
    j = lo[:, None] + np.arange(K, dtype=np.int64)[None, :]
    w = np.maximum(0.0, 1.0 - np.abs((j - c[:, None] + 0.5) * inv))
    w[j >= hi[:, None]] = 0.0
    w /= w.sum(axis=1, keepdims=True)
    start, weights = lo.astype(np.int32), w.astype(np.float32)
    start.setflags(write=False)
    weights.setflags(write=False)
    return start, weights


def _fma32(w: np.ndarray, v: np.ndarray, acc: np.ndarray) -> np.ndarray:
    """fmaf(w, v, acc) on fp32 arrays: the product of two fp32 numbers is exact in fp64"""
    return (w.astype(np.float64) * v.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def _pass(x: np.ndarray, start: np.ndarray, weights: np.ndarray) -> np.ndarray:
    """fp32 [..., n_in] -> fp32 [..., n_out] along the last axis, taps in ascending order"""
    n_in = x.shape[-1]
    acc = np.zeros(x.shape[:-1] + (len(start),), dtype=np.float32)
    for j in range(weights.shape[1]):
        idx = np.minimum(start.astype(np.int64) + j, n_in - 1)   # (a padded tap: weight 0, any index in range)
        acc = _fma32(weights[:, j], x[..., idx], acc)
    return acc


def resize_aa_host(img: np.ndarray, hw: Tuple[int, int]) -> np.ndarray:
    """uint8 [..., Hs, Ws] -> uint8 [..., hw[0], hw[1]]: what yogo_resize_aa_u8 computes, in numpy"""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim < 2:
        raise ValueError(f"resize_aa_host: a uint8 [..., H, W] array, got {img.shape} {img.dtype}")
    sy, wy = aa_taps(img.shape[-2], int(hw[0]))
    sx, wx = aa_taps(img.shape[-1], int(hw[1]))
    mid = _pass(img.astype(np.float32), sx, wx)                                # [..., Hs, Wd]
    out = np.swapaxes(_pass(np.swapaxes(mid, -1, -2), sy, wy), -1, -2)         # [..., Hd, Wd]
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)
