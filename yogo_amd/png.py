"""The host side of PNG files for the device image decoder (standard library and numpy, no PIL), written from the PNG specification.

A PNG file is an 8-byte signature and a sequence of chunks -- big-endian uint32 length, 4-byte type, the data, the CRC-32 of type
and data.  IHDR comes first (width, height, bit depth, colour type, compression, filter, interlace), the IDAT chunks' data
concatenated are ONE zlib stream of the filtered scanlines (``height`` rows of one filter-type byte and the row's bytes), IEND is
last.  ``parse_png`` lists what the device routes (yogo_amd/png_batch.py, for yogo_amd/png_feed.py and yogo_amd/png_prefill.py) need: the header fields and where the IDAT payloads lie, so that they are
copied back to back into the staging buffer and the device sees one zlib stream (csrc/inflate.hip), whose inflated rows
csrc/png_unpack.hip unfilters (csrc/png_unfilter.h).  Only 8-bit greyscale, non-interlaced files without transparency go that way
(``PngInfo.device_decodable``); everything else is read by ``yogo_amd.yogo_dataset.read_image`` on the host.  The prefill of the
device image cache (yogo_amd/png_prefill.py, csrc/png_unpack_planes.hip) parses files the same way and also takes 8-bit RGB ones
(``PngInfo.prefill_decodable``, ``PngInfo.bytes_per_pixel``).

With ``--device-image-decode-all`` both routes hand every colour type, bit depth and Adam7 to csrc/png_unpack_any.hip
(``PngInfo.any_decodable``, ``PngInfo.inflated_bytes``, ``PngInfo.format_code``, ``palette_table``).  ``decode_any`` is that
kernel's twin in numpy and states the rules: how the scanlines of each format are laid out and unfiltered, and how PIL's
``Image.open(...).convert("L" | "RGB")`` -- ``read_image`` -- turns their samples into 8-bit planes.
"""
from __future__ import annotations

import struct
import zlib
from dataclasses import dataclass, field
from typing import Iterator, List, Optional, Tuple

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}   # samples per pixel of a colour type
DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}   # the bit depths the specification allows it
ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))   # x0, y0, dx, dy per pass
FMT_PLANAR = 1      # yogo_png_unpack_any's format code of pixels the host decoded (no colour type is 1)
PALETTE_BYTES = 768


class NotPng(ValueError):
    """the file does not start with the PNG signature: another format under a .png name, which the host decoder may still read"""


@dataclass
class PngInfo:
    width: int
    height: int
    bit_depth: int
    color_type: int
    interlace: int
    idat: List[Tuple[int, int]] = field(default_factory=list)   # (offset, length) of every IDAT payload, in file order
    has_trns: bool = False
    plte: Optional[Tuple[int, int]] = None   # (offset, length) of the PLTE payload: the first one before IDAT, if its CRC-32 is right

    @property
    def device_decodable(self) -> bool:
        """8-bit greyscale, not interlaced, no tRNS: the scanlines are 1 + width bytes and a pixel is a byte"""
        return self.bit_depth == 8 and self.color_type == 0 and self.interlace == 0 and not self.has_trns

    @property
    def prefill_decodable(self) -> bool:
        """8-bit greyscale or 8-bit RGB, not interlaced, no tRNS: what csrc/png_unpack_planes.hip unfilters for the device image
        cache (yogo_amd/png_prefill.py) -- scanlines of 1 + width * bytes_per_pixel bytes"""
        return self.bit_depth == 8 and self.color_type in (0, 2) and self.interlace == 0 and not self.has_trns

    @property
    def bytes_per_pixel(self) -> int:
        """of an 8-bit file: 1 (grey), 3 (RGB); the other colour types are not decoded on the device"""
        return 3 if self.color_type == 2 else 1

    @property
    def idat_bytes(self) -> int:
        return sum(n for _, n in self.idat)

    @property
    def scanline_bytes(self) -> int:
        """what the zlib stream of a device-decodable file inflates to"""
        return self.height * (1 + self.width)

    @property
    def format_known(self) -> bool:
        """a colour type at a bit depth the specification allows it, interlace method 0 or 1"""
        return self.bit_depth in DEPTHS.get(self.color_type, ()) and self.interlace in (0, 1)

    @property
    def any_decodable(self) -> bool:
        """what csrc/png_unpack_any.hip takes (--device-image-decode-all): every known format, tRNS or not; a palette file only with
        a PLTE chunk of 1 .. 256 whole entries"""
        if not self.format_known:
            return False
        return self.color_type != 3 or (self.plte is not None and self.plte[1] % 3 == 0 and 0 < self.plte[1] <= PALETTE_BYTES)

    @property
    def bits_per_pixel(self) -> int:
        return CHANNELS[self.color_type] * self.bit_depth

    @property
    def filter_bpp(self) -> int:
        """how many bytes back the filters' byte "to the left" lies: 1, 2, 3, 4, 6 or 8"""
        return max(1, self.bits_per_pixel // 8)

    @property
    def format_code(self) -> int:
        """the format as yogo_png_unpack_any's table names it"""
        return self.color_type | self.bit_depth << 8 | self.interlace << 16

    def passes(self) -> Iterator[Tuple[int, int, int, int, int, int]]:
        """(x0, y0, dx, dy, width, height) of every reduced image that has pixels, in the order of their scanlines: the seven Adam7
        passes, or the whole image"""
        for x0, y0, dx, dy in (ADAM7 if self.interlace else ((0, 0, 1, 1),)):
            if self.width > x0 and self.height > y0:
                yield x0, y0, dx, dy, -(-(self.width - x0) // dx), -(-(self.height - y0) // dy)

    @property
    def inflated_bytes(self) -> int:
        """what the zlib stream of a file of a known format inflates to: per reduced image its rows of one filter-type byte and
        ceil(width * bits_per_pixel / 8) bytes; a pass without pixels has no scanlines"""
        return sum(h * (1 + (w * self.bits_per_pixel + 7) // 8) for _, _, _, _, w, h in self.passes())


def parse_png(buf) -> PngInfo:
    """The header fields and IDAT payload ranges of one file.  ValueError naming what is wrong: the signature (NotPng), a chunk that
    passes the end of the file, a first chunk that is not IHDR (an IDAT before it included), a bad CRC-32 of IHDR or of an IDAT
    chunk, an IHDR of another size than 13 bytes or with a zero dimension, no IDAT, no IEND."""
    mv = memoryview(buf).cast("B")
    if bytes(mv[:8]) != SIGNATURE:
        raise NotPng("PNG: bad signature")
    pos, info, n = 8, None, len(mv)
    while True:
        if pos + 12 > n:
            raise ValueError("PNG: the file ends without an IEND chunk")
        length, = struct.unpack_from(">I", mv, pos)
        ctype = bytes(mv[pos + 4:pos + 8])
        if pos + 12 + length > n:
            raise ValueError(f"PNG: chunk {ctype!r} at {pos} passes the end of the file")
        if info is None and ctype != b"IHDR":
            raise ValueError(f"PNG: the first chunk is {ctype!r}, not IHDR")
        if ctype in (b"IHDR", b"IDAT"):
            crc, = struct.unpack_from(">I", mv, pos + 8 + length)
            if zlib.crc32(mv[pos + 4:pos + 8 + length]) != crc:
                raise ValueError(f"PNG: bad CRC-32 of the {ctype.decode()} chunk at {pos}")
        if ctype == b"IHDR":
            if info is not None or length != 13:
                raise ValueError("PNG: a second IHDR chunk, or one that is not 13 bytes long")
            w, h, depth, ctyp, comp, filt, lace = struct.unpack_from(">IIBBBBB", mv, pos + 8)
            if w == 0 or h == 0 or comp != 0 or filt != 0:
                raise ValueError(f"PNG: IHDR with width {w}, height {h}, compression {comp}, filter {filt}")
            info = PngInfo(w, h, depth, ctyp, lace)
        elif ctype == b"IDAT":
            info.idat.append((pos + 8, length))
        elif ctype == b"PLTE":
            crc, = struct.unpack_from(">I", mv, pos + 8 + length)
            if info.plte is None and not info.idat and zlib.crc32(mv[pos + 4:pos + 8 + length]) == crc:
                info.plte = (pos + 8, length)
        elif ctype == b"tRNS":
            info.has_trns = True
        elif ctype == b"IEND":
            if not info.idat:
                raise ValueError("PNG: no IDAT chunk")
            return info
        pos += 12 + length


def palette_table(buf, info: PngInfo) -> np.ndarray:
    """the 256 x 3 bytes R G B of a palette file (``info.any_decodable``), a shorter PLTE padded with zeros"""
    table = np.zeros(PALETTE_BYTES, dtype=np.uint8)
    o, n = info.plte
    table[:n] = np.frombuffer(buf, dtype=np.uint8, count=n, offset=o)
    return table


def _paeth(a: int, b: int, c: int) -> int:
    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def unfilter_bytes(scan: np.ndarray, height: int, row_bytes: int, bpp: int) -> np.ndarray:
    """``height`` scanlines of 1 + row_bytes bytes -> uint8 [height, row_bytes].  The filters act on bytes, mod 256: 0 None, 1 Sub
    (+ the byte bpp back), 2 Up (+ the byte above; zeros above row 0), 3 Average (+ floor((left + above) / 2)), 4 Paeth.
    ValueError for a filter type above 4."""
    rows = np.asarray(scan, dtype=np.uint8).reshape(height, 1 + row_bytes)
    out = np.zeros((height, row_bytes), dtype=np.uint8)
    for y in range(height):
        t, raw = int(rows[y, 0]), rows[y, 1:]
        up = out[y - 1] if y else np.zeros(row_bytes, np.uint8)
        if t == 0:
            out[y] = raw
        elif t == 2:
            out[y] = raw + up
        elif t in (1, 3, 4):
            r, u, cur = raw.tolist(), up.tolist(), [0] * row_bytes
            for i in range(row_bytes):
                a = cur[i - bpp] if i >= bpp else 0
                c = u[i - bpp] if i >= bpp else 0
                pred = a if t == 1 else (a + u[i]) >> 1 if t == 3 else _paeth(a, u[i], c)
                cur[i] = (r[i] + pred) & 255
            out[y] = cur
        else:
            raise ValueError(f"PNG: filter type {t} in row {y}")
    return out


def _samples(rows: np.ndarray, width: int, info: PngInfo) -> np.ndarray:
    """unfiltered row bytes -> [height, width, channels]: 16-bit samples as (high byte, low byte) pairs in uint16, depths below 8
    expanded most significant bits first, the padding bits of a row's last byte dropped"""
    h, depth, ch = rows.shape[0], info.bit_depth, CHANNELS[info.color_type]
    if depth == 16:
        return (rows[:, 0::2].astype(np.uint16) << 8 | rows[:, 1::2]).reshape(h, width, ch)
    if depth == 8:
        return rows.reshape(h, width, ch).astype(np.uint16)
    per = 8 // depth
    shifts = np.arange(per - 1, -1, -1, dtype=np.uint16) * depth
    v = (rows[:, :, None].astype(np.uint16) >> shifts) & ((1 << depth) - 1)
    return v.reshape(h, -1)[:, :width, None]


def decode_any(data, rgb: bool = False) -> np.ndarray:
    """One PNG file of any known format -> uint8 [1, H, W] (rgb False) or [3, H, W], the pixels of
    ``yogo_amd.yogo_dataset.read_image(path, rgb)``, with nothing but zlib and numpy: what csrc/png_unpack_any.hip computes.
      grey 1 / 2 / 4     v * 255 / (2^depth - 1)
      grey 8             as it is
      grey 16            min(v, 255): PIL's I;16 -> L clips, it does not shift
      grey+alpha 8 / 16  the grey sample's high byte; alpha dropped
      RGB, RGBA 8 / 16   the high byte of each sample; alpha dropped
      palette            PLTE[index], a table shorter than the index range padded with zeros
    tRNS, gAMA, sBIT and a PLTE in a file of another colour type change nothing.  One plane from colour is
    L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16, three planes from grey are the plane three times.
    ValueError for what the device does not take either (``PngInfo.any_decodable``), a stream of the wrong length, a bad filter."""
    info = parse_png(data)
    if not info.any_decodable:
        raise ValueError(f"PNG: colour type {info.color_type} at {info.bit_depth} bits, interlace {info.interlace}"
                         + (", without a usable PLTE chunk" if info.format_known else ""))
    scan = np.frombuffer(zlib.decompress(b"".join(bytes(memoryview(data)[o:o + n]) for o, n in info.idat)), dtype=np.uint8)
    if scan.size != info.inflated_bytes:
        raise ValueError(f"PNG: the stream inflates to {scan.size} bytes, the header says {info.inflated_bytes}")
    ch = CHANNELS[info.color_type]
    full = np.zeros((info.height, info.width, ch), dtype=np.uint16)
    at = 0
    for x0, y0, dx, dy, w, h in info.passes():
        row_bytes = (w * info.bits_per_pixel + 7) // 8
        rows = unfilter_bytes(scan[at:at + h * (1 + row_bytes)], h, row_bytes, info.filter_bpp)
        at += h * (1 + row_bytes)
        full[y0::dy, x0::dx] = _samples(rows, w, info)
    if info.color_type == 3:
        colour = palette_table(data, info).reshape(256, 3)[full[:, :, 0]]
    elif info.color_type in (2, 6):
        colour = (full[:, :, :3] >> (info.bit_depth - 8)).astype(np.uint8)
    else:
        colour = None
        if info.color_type == 4:
            grey = full[:, :, 0] >> (info.bit_depth - 8)
        elif info.bit_depth == 16:
            grey = np.minimum(full[:, :, 0], 255)
        else:
            grey = full[:, :, 0] * (255 // ((1 << info.bit_depth) - 1))
        grey = grey.astype(np.uint8)
    if colour is None:
        return np.ascontiguousarray(np.broadcast_to(grey[None], (3 if rgb else 1,) + grey.shape))
    if rgb:
        return np.ascontiguousarray(colour.transpose(2, 0, 1))
    c = colour.astype(np.uint32)
    return ((19595 * c[:, :, 0] + 38470 * c[:, :, 1] + 7471 * c[:, :, 2] + 0x8000) >> 16).astype(np.uint8)[None]
