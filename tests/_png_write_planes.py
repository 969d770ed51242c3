"""The PNG writer of tests/_png_write.py at 1 or 3 bytes per pixel (8-bit greyscale, 8-bit RGB), after the PNG specification: a file
from given pixels with a chosen filter type per row.  The filters act on BYTES: the byte to the left of a byte is the one
``bpp`` bytes before it -- the same channel of the pixel to the left.

The decoder under test (csrc/png_unpack_planes.hip) and this writer share an author; tests/test_png_write_planes.py holds every
file written here against PIL (``read_image``)."""
import numpy as np

from _png_write import paeth, png_bytes


def _as_rows(img):
    """uint8 [H, W] or [H, W, 3] -> (uint8 [H, W * bpp] row bytes, bpp)"""
    img = np.asarray(img, dtype=np.uint8)
    if img.ndim == 2:
        return img, 1
    if img.ndim == 3 and img.shape[2] == 3:
        return img.reshape(img.shape[0], -1), 3
    raise ValueError(f"an [H, W] or [H, W, 3] image is expected, got {img.shape}")


def filter_rows_bpp(img, types):
    """uint8 [H, W] / [H, W, 3] pixels -> uint8 [H, 1 + W * bpp] scanlines, row y under filter types[y] (0 .. 4)"""
    rows, bpp = _as_rows(img)
    H, n = rows.shape
    out = np.zeros((H, 1 + n), dtype=np.uint8)
    for y in range(H):
        cur = rows[y].astype(np.int64)
        up = rows[y - 1].astype(np.int64) if y else np.zeros(n, np.int64)
        left = np.concatenate((np.zeros(bpp, np.int64), cur[:-bpp]))[:n]
        upleft = np.concatenate((np.zeros(bpp, np.int64), up[:-bpp]))[:n]
        t = int(types[y])
        pred = {0: np.zeros(n, np.int64), 1: left, 2: up, 3: (left + up) // 2, 4: paeth(left, up, upleft)}[t]
        out[y, 0] = t
        out[y, 1:] = (cur - pred) & 255
    return out


def png_planes_bytes(img, types=None, **kw):
    """One 8-bit file: colour type 0 for an [H, W] image, 2 for an [H, W, 3] one; types: filter type per row (default 0); the other
    arguments are ``_png_write.png_bytes``'s (idat_sizes, level, before, after)."""
    rows, bpp = _as_rows(img)
    H, W = rows.shape[0], rows.shape[1] // bpp
    scan = filter_rows_bpp(img, [0] * H if types is None else types)
    return png_bytes(np.zeros((H, W), np.uint8), scan=scan.tobytes(), ihdr=(W, H, 8, 0 if bpp == 1 else 2, 0, 0, 0), **kw)
