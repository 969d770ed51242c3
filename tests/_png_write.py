"""A small PNG writer for the tests, after the PNG specification (nothing but numpy and the standard library): a file from given
pixel rows with a chosen filter type per row, any split of the zlib stream over IDAT chunks, any IHDR fields and ancillary chunks
before and after the IDAT chunks; 8-bit greyscale from an [H, W] image, 8-bit RGB from an [H, W, 3] one.  `filter_rows` is the numpy
restatement of the five filters at 1 or 3 bytes per pixel -- they act on BYTES: the byte to the left of a byte is the one ``bpp``
bytes before it, the same channel of the pixel to the left -- and `unfilter_rows` their reverse at one byte per pixel.

The decoders under test (yogo_amd/png.py, csrc/png_unfilter.h behind csrc/png_unpack.hip and csrc/png_unpack_planes.hip) and this
writer share an author; PIL reads the files it writes (tests/test_png_host.py, tests/test_png_write_planes.py)."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def chunk(ctype: bytes, data: bytes, crc=None) -> bytes:
    return struct.pack(">I", len(data)) + ctype + data + struct.pack(">I", zlib.crc32(ctype + data) if crc is None else crc)


def paeth(a, b, c):
    """the predictor on int arrays: whichever of a, b, c is nearest a + b - c, ties in that order"""
    pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def _as_rows(img):
    """uint8 [H, W] or [H, W, 3] -> (uint8 [H, W * bpp] row bytes, bpp)"""
    img = np.asarray(img, dtype=np.uint8)
    if img.ndim == 2:
        return img, 1
    if img.ndim == 3 and img.shape[2] == 3:
        return img.reshape(img.shape[0], -1), 3
    raise ValueError(f"an [H, W] or [H, W, 3] image is expected, got {img.shape}")


def filter_rows(img, types):
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


def unfilter_rows(scan):
    """uint8 [H, 1 + W] scanlines -> uint8 [H, W] pixels (pixel by pixel where the filter is serial)"""
    scan = np.asarray(scan, dtype=np.uint8)
    H, W = scan.shape[0], scan.shape[1] - 1
    out = np.zeros((H, W), dtype=np.int64)
    for y in range(H):
        t, raw = int(scan[y, 0]), scan[y, 1:].astype(np.int64)
        up = out[y - 1] if y else np.zeros(W, np.int64)
        if t == 0:
            out[y] = raw
        elif t == 2:
            out[y] = (raw + up) & 255
        else:
            for x in range(W):
                a = out[y, x - 1] if x else 0
                c = up[x - 1] if x else 0
                pred = a if t == 1 else (a + up[x]) // 2 if t == 3 else int(paeth(np.int64(a), up[x], np.int64(c)))
                out[y, x] = (raw[x] + pred) & 255
    return out.astype(np.uint8)


ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))   # x0, y0, dx, dy per pass


def adam7_scan(img):
    """the scanlines of an interlaced 8-bit greyscale file: the seven reduced images one after the other, every row unfiltered"""
    img = np.asarray(img, dtype=np.uint8)
    out = bytearray()
    for x0, y0, dx, dy in ADAM7:
        sub = img[y0::dy, x0::dx]
        if sub.size:
            out += filter_rows(sub, [0] * sub.shape[0]).tobytes()
    return bytes(out)


def png_bytes(img, types=None, *, idat_sizes=None, level=6, ihdr=None, before=(), after=(), scan=None, stream=None):
    """One file.  img: uint8 [H, W] (colour type 0) or [H, W, 3] (colour type 2); types: filter type per row (default 0); idat_sizes: lengths of the IDAT payloads (the last
    chunk takes the rest; default one chunk); ihdr: (width, height, bit depth, colour type, compression, filter, interlace) when
    it is to differ from the image; before / after: ancillary chunks [(type, data)] between IHDR and the first IDAT / between the
    last IDAT and IEND (IDAT chunks are consecutive by the specification); scan: the scanline bytes to compress instead of the
    filtered image; stream: the zlib stream itself."""
    rows, bpp = _as_rows(img)
    H, W = rows.shape[0], rows.shape[1] // bpp
    scan = filter_rows(img, [0] * H if types is None else types).tobytes() if scan is None else scan
    z = zlib.compress(scan, level) if stream is None else stream
    parts, at = [], 0
    for n in (idat_sizes or []):
        parts.append(z[at:at + n])
        at += n
    parts.append(z[at:])
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", *(ihdr or (W, H, 8, 0 if bpp == 1 else 2, 0, 0, 0))))
    out += b"".join(chunk(*c) for c in before) + b"".join(chunk(b"IDAT", p) for p in parts) + b"".join(chunk(*c) for c in after)
    return out + chunk(b"IEND", b"")
