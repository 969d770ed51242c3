"""Host restatement of the blob generator (yogo_amd/csrc/blobgen.hip) in numpy: the same counter hash, the same draws, the same
placement rule -- for bit-exact comparison with the device.  Also the reference's expressions the device must reproduce
(background value, fp32 label rows, img / 255)."""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

M64 = (1 << 64) - 1
TRIES = 100
KIND_THUMB, KIND_HFLIP, KIND_VFLIP, KIND_Y, KIND_X = 0, 1, 2, 3, 4


def mix64(z: np.ndarray) -> np.ndarray:
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def key_of(seed: int, epoch: int) -> np.uint64:
    return mix64(np.array([((seed & 0xFFFFFFFF) << 32) | (epoch & 0xFFFFFFFF)], dtype=np.uint64))[0]


def draw32(key, index: int, slot: int, kind: int, tries) -> np.ndarray:
    ctr = (np.uint64(index) << np.uint64(24)) | np.uint64(slot << 16) | np.uint64(kind << 8) | np.asarray(tries, dtype=np.uint64)
    return (mix64(np.uint64(key) ^ ctr) >> np.uint64(32)).astype(np.uint64)


def uniform(d, m: int) -> np.ndarray:
    return ((np.asarray(d, dtype=np.uint64) * np.uint64(m)) >> np.uint64(32)).astype(np.int64)


def place(table: np.ndarray, index: int, seed: int, epoch: int, n: int, H: int, W: int) -> Dict:
    """one image: boxes [(t, x, y, flips)], rows [count, 5] fp32, background, plus the statistics of the search (the try
    index that each placed slot accepted, the number of slots that exhausted every try)"""
    key = key_of(seed, epoch)
    T = table.shape[0]
    ts = [int(uniform(draw32(key, index, k, KIND_THUMB, 0), T)) for k in range(n)]
    shades = [int(table[t, 4]) for t in ts]
    # the reference's expression (blobgen.py:214-220): np.mean -> fill a float32 image -> uint8
    background = int(np.array([np.float32(np.mean(shades))], dtype=np.float32).astype(np.uint8)[0])
    acc: List[Tuple[int, int, int, int]] = []
    boxes, rows, accepted_tries, exhausted = [], [], [], 0
    tries = np.arange(TRIES)
    for k, t in enumerate(ts):
        h, w, cls = int(table[t, 1]), int(table[t, 2]), int(table[t, 3])
        ys = uniform(draw32(key, index, k, KIND_Y, tries), H - h)
        xs = uniform(draw32(key, index, k, KIND_X, tries), W - w)
        ok = np.ones(TRIES, dtype=bool)
        for (x0, y0, x1, y1) in acc:
            ok &= ~((xs < x1) & (x0 < xs + w) & (ys < y1) & (y0 < ys + h))
        if not ok.any():
            exhausted += 1
            continue
        j = int(np.argmax(ok))
        x, y = int(xs[j]), int(ys[j])
        fl = int(draw32(key, index, k, KIND_HFLIP, 0) >> np.uint64(31)) | int(draw32(key, index, k, KIND_VFLIP, 0) >> np.uint64(31)) << 1
        acc.append((x, y, x + w, y + h))
        boxes.append((t, x, y, fl))
        # the reference's label row: Python double quotients, then a float32 tensor
        rows.append(np.array([cls, x / W, y / H, (x + w) / W, (y + h) / H], dtype=np.float64).astype(np.float32))
        accepted_tries.append(j)
    return {"boxes": boxes, "rows": np.array(rows, dtype=np.float32).reshape(-1, 5), "background": background,
            "accepted_tries": accepted_tries, "exhausted": exhausted}


def compose(atlas: np.ndarray, table: np.ndarray, placed: Dict, H: int, W: int) -> np.ndarray:
    img = np.full((H, W), placed["background"], dtype=np.uint8)
    for t, x, y, fl in placed["boxes"]:
        off, h, w = int(table[t, 0]), int(table[t, 1]), int(table[t, 2])
        th = atlas[off:off + h * w].reshape(h, w)
        if fl & 1:
            th = th[:, ::-1]
        if fl & 2:
            th = th[::-1, :]
        img[y:y + h, x:x + w] = th
    return img


def generate(atlas: np.ndarray, table: np.ndarray, indices, seed: int, epoch: int, n: int, H: int, W: int):
    """-> (images [S, H, W] uint8, rows [S, n, 5] fp32 zero-padded, counts [S], per-image placement dicts)"""
    S = len(indices)
    imgs = np.zeros((S, H, W), dtype=np.uint8)
    rows = np.zeros((S, n, 5), dtype=np.float32)
    counts = np.zeros(S, dtype=np.int32)
    placed = []
    for s, i in enumerate(indices):
        p = place(table, int(i), seed, epoch, n, H, W)
        imgs[s] = compose(atlas, table, p, H, W)
        c = len(p["boxes"])
        rows[s, :c] = p["rows"]
        counts[s] = c
        placed.append(p)
    return imgs, rows, counts, placed
