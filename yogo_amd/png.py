"""The host side of PNG files for the device image decoder (standard library only, no PIL), written from the PNG specification.

A PNG file is an 8-byte signature and a sequence of chunks -- big-endian uint32 length, 4-byte type, the data, the CRC-32 of type
and data.  IHDR comes first (width, height, bit depth, colour type, compression, filter, interlace), the IDAT chunks' data
concatenated are ONE zlib stream of the filtered scanlines (``height`` rows of one filter-type byte and the row's bytes), IEND is
last.  ``parse_png`` lists what yogo_amd/png_feed.py needs: the header fields and where the IDAT payloads lie, so that they are
copied back to back into the staging buffer and the device sees one zlib stream (csrc/inflate.hip), whose inflated rows
csrc/png_unpack.hip unfilters (csrc/png_unfilter.h).  Only 8-bit greyscale, non-interlaced files without transparency go that way
(``PngInfo.device_decodable``); everything else is read by ``yogo_amd.yogo_dataset.read_image`` on the host.  The prefill of the
device image cache (yogo_amd/png_prefill.py, csrc/png_unpack_planes.hip) parses files the same way and also takes 8-bit RGB ones
(``PngInfo.prefill_decodable``, ``PngInfo.bytes_per_pixel``).
"""
from __future__ import annotations

import struct
import zlib
from dataclasses import dataclass, field
from typing import List, Tuple

SIGNATURE = b"\x89PNG\r\n\x1a\n"


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
        elif ctype == b"tRNS":
            info.has_trns = True
        elif ctype == b"IEND":
            if not info.idat:
                raise ValueError("PNG: no IDAT chunk")
            return info
        pos += 12 + length
