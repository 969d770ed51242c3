"""The rules of ``yogo_draw_boxes`` (yogo_amd/csrc/draw_boxes.hip) restated in numpy, and the cases both are held to.

``render`` is what ``yogo_amd.utils.utils.draw_yogo_prediction`` makes PIL draw, written out as arithmetic: the background, per kept
row an outline (``ImageDraw.rectangle``) and then its label (``ImageDraw.text``), in row order.  tests/test_draw_host.py holds it to
PIL itself; tests/test_gpu_draw_boxes.py holds the kernel to it."""
from __future__ import annotations

import numpy as np

CLASS_NAMES = ["ring", "t", "schizont", "gametocyte", "wbc", "misc", "healthy cell"]


def background(img: np.ndarray, normalised: bool) -> np.ndarray:
    """[1|3, H, W] uint8, or float32 (x 255 in fp32 and truncated when `normalised`) -> [H, W, 4] uint8, alpha 255"""
    if img.dtype != np.uint8:
        v = img.astype(np.float32)
        if normalised:
            v = v * np.float32(255.0)
        img = v.astype(np.int32).astype(np.uint8)
    C, H, W = img.shape
    out = np.empty((H, W, 4), dtype=np.uint8)
    for c in range(3):
        out[:, :, c] = img[c if C == 3 else 0]
    out[:, :, 3] = 255
    return out


def box_pixels(row: np.ndarray, H: int, W: int):
    """the four fp32 pixel coordinates of a kept row (xyxy in image fractions), multiplied in fp32"""
    row = row.astype(np.float32)
    return np.float32(W) * row[0], np.float32(H) * row[1], np.float32(W) * row[2], np.float32(H) * row[3]


def render(img: np.ndarray, rows: np.ndarray, atlas, colours: np.ndarray, normalised: bool = False) -> np.ndarray:
    """img [1|3, H, W], rows [n, 5 + C] float32 -> [H, W, 4] uint8"""
    out = background(img, normalised)
    H, W = out.shape[:2]

    def put(x, y, colour):
        if 0 <= x < W and 0 <= y < H:
            out[y, x] = colour

    for row in rows:
        xf0, yf0, xf1, yf1 = box_pixels(row, H, W)
        cls = int(np.argmax(row[5:]))                      # the first maximum
        x0, y0, x1, y1 = int(xf0), int(yf0), int(xf1), int(yf1)   # truncated toward zero
        if y0 > y1:
            y0, y1 = y1, y0
        xa, xb = min(x0, x1), max(x0, x1)
        for x in range(max(xa, 0), min(xb, W - 1) + 1):
            put(x, y0, colours[cls])
            put(x, y1, colours[cls])
        for y in range(max(min(y0 + 1, y1), 0), min(max(y0 + 1, y1), H - 1) + 1):
            put(x0, y, colours[cls])
            put(x1, y, colours[cls])
        tx, ty = int(xf0), int(yf0)
        fx, fy = float(xf0) - tx, float(yf0) - ty          # the fractions carry the coordinate's sign
        w, h, ox, oy, data = atlas.lookup(cls, fx, fy)
        if w == 0 or h == 0:
            continue
        mask = np.frombuffer(data, dtype=np.uint8).reshape(h, w)
        for my in range(h):
            y = ty + oy + my
            if not 0 <= y < H:
                continue
            for mx in range(w):
                x = tx + ox + mx
                if not 0 <= x < W:
                    continue
                m = int(mask[my, mx])
                for c, ink in enumerate((0, 0, 0, 255)):
                    t = m * ink + (255 - m) * int(out[y, x, c]) + 128
                    out[y, x, c] = ((t >> 8) + t) >> 8
    return out


def random_rows(rng, n: int, C: int, kind: str = "any") -> np.ndarray:
    """n rows [5 + C]: xyxy in image fractions, centres in -0.1 .. 1.1, sides up to 0.5; `kind` forces an edge case"""
    cx, cy = rng.uniform(-0.1, 1.1, n), rng.uniform(-0.1, 1.1, n)
    w, h = rng.uniform(0, 0.5, n), rng.uniform(0, 0.5, n)
    if kind == "flat":
        h[:] = 0
    elif kind == "thin":
        w[:] = 0
    elif kind == "outside":
        cx, cy = cx + 2.0, cy - 2.0
    elif kind == "negative":
        cx, cy = rng.uniform(-0.3, 0.05, n), rng.uniform(-0.3, 0.05, n)
    elif kind == "corner":     # text clipped at the right and bottom edges
        cx, cy, w, h = rng.uniform(0.9, 1.0, n), rng.uniform(0.9, 1.0, n), rng.uniform(0, 0.1, n), rng.uniform(0, 0.1, n)
    rows = np.zeros((n, 5 + C), dtype=np.float32)
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2
    rows[:, 4] = rng.uniform(0.5, 1.0, n)
    rows[:, 5:] = rng.uniform(0, 1, (n, C))
    return rows


KINDS = ("any", "any", "any", "flat", "thin", "outside", "negative", "corner")


def make_cases(seed: int, n_cases: int, H: int, W: int, channels: int, C: int = len(CLASS_NAMES), max_boxes: int = 6):
    """[(img uint8 [channels, H, W], rows [n, 5 + C])]: case 0 has no boxes, the edge cases of KINDS come round in turn"""
    rng = np.random.default_rng(seed)
    cases = []
    for k in range(n_cases):
        img = rng.integers(0, 256, (channels, H, W), dtype=np.uint8)
        n = 0 if k == 0 else int(rng.integers(1, max_boxes + 1))
        cases.append((img, random_rows(rng, n, C, KINDS[k % len(KINDS)])))
    return cases


def encoder_cases(rendered: np.ndarray):
    """{name: [H, W, 4] uint8}: what the PNG encoder and its twin are held to.  `rendered` is a drawn frame."""
    rng = np.random.default_rng(11)
    few = rng.integers(0, 8, (40, 50, 4), dtype=np.uint8)   # differences in -7 .. 7: 15 distinct filtered values
    return {
        "noise": rng.integers(0, 256, (48, 64, 4), dtype=np.uint8),
        "constant": np.full((48, 64, 4), 77, dtype=np.uint8),
        "rendered": np.ascontiguousarray(rendered),
        "one_pixel": rng.integers(0, 256, (1, 1, 4), dtype=np.uint8),
        "ragged_height": (rng.integers(0, 6, (37, 53, 4), dtype=np.uint8) * 40).astype(np.uint8),   # 37 rows: two bands and five rows
        "wide_band": np.concatenate([rng.integers(0, 256, (16, 1030, 4), dtype=np.uint8),               # 16 x 4121 > 65 535 bytes:
                                     rng.integers(0, 8, (4, 1030, 4), dtype=np.uint8)]),                  # stored in two blocks; coded
        "few_values": few,
    }
