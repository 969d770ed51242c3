"""The cases level 1 of the PNG encoder (literals and LZ77 matches: yogo_amd/png_encode.py) and its twin are held to, shared by
tests/test_png_encode_matches_host.py and tests/test_gpu_png_encode_matches.py.  Each is the smallest shape at which its part of the
coder can go wrong; the host test asserts from the twin's tokens that each exercises what its name says."""
from __future__ import annotations

import numpy as np

from yogo_amd import png_encode as E

# a run of R equal bytes is a literal and a match of R - 1 at distance 1 when the row keeps filter 0, and a literal, a zero and a match
# of R - 2 when it takes Sub (one more where the filler before it ends in a zero): R = T + 1 .. T + 3 are planted for every length T
# on either side of a length-symbol boundary
RUN_TARGETS = sorted(set(E.LEN_BASE) | {b - 1 for b in E.LEN_BASE if b > E.MIN_MATCH})
# distances on either side of every distance-symbol boundary the candidates bpp * k, k = 1 .. WINDOW, reach: bpp 1 and bpp 4
DISTANCES_BPP1 = sorted({d for b in E.DIST_BASE for d in (b - 1, b) if 1 <= d <= E.WINDOW})
DISTANCES_BPP4 = sorted({d for b in E.DIST_BASE for d in ((b - 1) // 4 * 4, (b + 3) // 4 * 4) if E.WINDOW <= d <= 4 * E.WINDOW})


def _filler(rng, n: int) -> np.ndarray:
    """compressible bytes (16 values) that never equal a planted byte (those are 128 and up)"""
    return rng.integers(0, 16, n, dtype=np.uint8)


def runs_row() -> np.ndarray:
    """[1, W, 1]: the runs one behind the other, WINDOW + 8 filler bytes apart (no candidate reaches the run before), none across the end of a piece (positions count the scanline's
    bytes: its first is the filter type)"""
    rng = np.random.default_rng(21)
    runs = [t + extra for t in RUN_TARGETS for extra in (1, 2, 3)]
    gap = E.WINDOW + 8
    places, at = [], 8
    for r in runs:
        if at % E.PIECE + r + 8 > E.PIECE:
            at = (at // E.PIECE + 1) * E.PIECE + 8
        places.append(at)
        at += r + gap
    scanline = _filler(rng, (at + E.PIECE - 1) // E.PIECE * E.PIECE)
    for k, (at, r) in enumerate(zip(places, runs)):
        scanline[at: at + r] = 128 + k % 120
    return scanline[1:].reshape(1, -1, 1)


def distances_row(bpp: int) -> np.ndarray:
    """[1, W, bpp]: per distance d, d + 8 bytes of period d (d random bytes, and the first 8 of them again), in a piece of their own"""
    rng = np.random.default_rng(22 + bpp)
    dists = DISTANCES_BPP1 if bpp == 1 else DISTANCES_BPP4
    row = _filler(rng, len(dists) * E.PIECE)
    for k, d in enumerate(dists):
        at = k * E.PIECE + 4 * bpp
        row[at: at + d + 8] = np.resize(rng.integers(128, 256, d, dtype=np.uint8), d + 8)   # d < 8: the match overlaps itself
    return row.reshape(1, -1, bpp)


def single_match() -> np.ndarray:
    """[1, 600, 1]: 32 values in an order that repeats no triple within reach (the host test asserts it), five bits each so that
    the band is coded, and ONE planted repeat of six bytes"""
    row = (np.random.default_rng(0).integers(0, 32, 600, dtype=np.uint8) * 8).astype(np.uint8)
    row[300: 306] = [250, 130, 190, 160, 220, 140]
    row[320: 326] = row[300: 306]
    return row.reshape(1, -1, 1)


def match_cases() -> dict:
    """{name: [H, W, bpp] uint8}"""
    rng = np.random.default_rng(12)
    yy, xx = np.mgrid[0:40, 0:50]
    smooth = (120 + 40 * np.sin(xx / 9.0) * np.cos(yy / 7.0)).astype(np.uint8)
    cases = {
        "constant": np.full((48, 64, 4), 77, dtype=np.uint8),                       # overlapping copies one pixel back, cut at piece ends
        "one_pixel": rng.integers(0, 256, (1, 1, 4), dtype=np.uint8),               # no token but the filter type and four literals
        "runs": runs_row(),
        "distances_bpp1": distances_row(1),
        "distances_bpp4": distances_row(4),
        "single_match": single_match(),
        "ragged_height": (rng.integers(0, 6, (37, 53, 4), dtype=np.uint8) * 40).astype(np.uint8),   # two bands and five rows
        "last_band_one_row": (rng.integers(0, 4, (17, 40, 4), dtype=np.uint8) * 60).astype(np.uint8),
        "wide_band": np.concatenate([rng.integers(0, 256, (16, 1030, 4), dtype=np.uint8),          # 16 x 4121 > 65 535 bytes: stored
                                     rng.integers(0, 8, (4, 1030, 4), dtype=np.uint8)]),             # in two blocks; then a coded band
        "long_rows": (rng.integers(0, 3, (2, 8200, 4), dtype=np.uint8) * 90).astype(np.uint8),     # a scanline above 32 768 bytes
        "grey": (rng.integers(0, 5, (21, 33, 1), dtype=np.uint8) * 50).astype(np.uint8),
        "grey_alpha": (rng.integers(0, 5, (21, 33, 2), dtype=np.uint8) * 50).astype(np.uint8),
        "rgb": (rng.integers(0, 5, (21, 33, 3), dtype=np.uint8) * 50).astype(np.uint8),
        "smooth": np.stack([smooth, smooth, smooth, np.full_like(smooth, 255)], axis=-1),         # what a drawn frame looks like
        "noise": rng.integers(0, 256, (48, 64, 4), dtype=np.uint8),                                # stored: the file of level 0
    }
    return cases


def bench_frame_rows(rows: int = 64) -> np.ndarray:
    """rows 0 .. `rows` - 1 of the first frame of tools/bench_draw_boxes.make_frames(seed=0) as RGBA [rows, 1032, 4] (the generator
    restated: a smooth bright field, 200 dark round cells, Gaussian noise of sigma 2)"""
    H, W = 772, 1032
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    f = 190 + 20 * np.cos(xx / W * rng.uniform(1, 3) + rng.uniform(0, 6)) * np.cos(yy / H * rng.uniform(1, 3) + rng.uniform(0, 6))
    for _ in range(200):
        cx, cy, r = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(12, 22)
        x0, x1, y0, y1 = int(max(cx - r, 0)), int(min(cx + r + 1, W)), int(max(cy - r, 0)), int(min(cy + r + 1, H))
        d = np.hypot(xx[y0:y1, x0:x1] - cx, yy[y0:y1, x0:x1] - cy)
        f[y0:y1, x0:x1] -= 60 * np.clip(r - d, 0, 3) / 3
    grey = np.clip(f + rng.normal(0, 2, (H, W)), 0, 255).astype(np.uint8)[:rows]
    return np.ascontiguousarray(np.stack([grey, grey, grey, np.full_like(grey, 255)], axis=-1))
