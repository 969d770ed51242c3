"""The host side of Blosc 1 chunks of uint8 data (standard library only), written from the published chunk layout.

A chunk is a 16-byte header -- version (2), the inner codec's version, flags, typesize, then little-endian uint32 ``nbytes``,
``blocksize``, ``cbytes`` -- followed, unless the ``memcpyed`` flag says that the ``nbytes`` raw bytes come next, by
``nblocks = ceil(nbytes / blocksize)`` little-endian int32 ``bstarts`` (offsets from the start of the chunk).  With
``typesize == 1`` a block is never split: at ``bstarts[i]`` lies one int32 ``csize`` and ``csize`` bytes, the block's raw bytes
when ``csize`` equals the block's decoded size and one stream of the inner codec otherwise.  zarr 2.17 writes its arrays with
``Blosc(cname="lz4", clevel=5, shuffle=1)`` by default; for uint8 the byte shuffle is the identity.

``parse_chunk`` lists the blocks (what yogo_amd/zarr_feed.py hands to ``yogo_blosc_lz4_decode``), ``lz4_block_decode`` is the
LZ4 block format with the checks and the status codes of the kernel (csrc/blosc_lz4.hip), ``decompress`` decodes a chunk on
the host (inner format 4, one Zstandard frame per block, with the frame decoder it is given: yogo_amd/zstd.py).  The LZ4 block format is pinned to liblz4 by tests/golden/lz4_blocks.npz; the framing is not pinned to c-blosc.
"""
from __future__ import annotations

import ctypes
import ctypes.util
import struct
import zlib
from typing import Callable, List, Optional, Tuple

HEADER = 16
FLAG_SHUFFLE, FLAG_MEMCPYED, FLAG_BITSHUFFLE, FLAG_DONT_SPLIT = 0x01, 0x02, 0x04, 0x10
FORMATS = {0: "blosclz", 1: "lz4", 2: "snappy", 3: "zlib", 4: "zstd"}   # bits 5-7 of the flags (lz4hc writes 1 as well)

# status of one LZ4 block, the same numbers in csrc/blosc_lz4.hip
LZ4_OK = 0
LZ4_LITERALS_PAST_SOURCE = 1    # a literal run longer than what is left of the source
LZ4_SOURCE_ENDS_IN_SEQUENCE = 2  # the source ends inside a length extension, before a token, or inside the 2-byte offset
LZ4_BAD_OFFSET = 3              # offset 0, or larger than what the block has produced so far
LZ4_PAST_DESTINATION = 4        # a literal run or a match that would pass dst_len
LZ4_ENDS_EARLY = 5              # the block ends before dst_len
LZ4_BAD_ENTRY = 6               # (kernel only) a table entry that does not lie inside the buffers
LZ4_STATUS = {
    LZ4_LITERALS_PAST_SOURCE: "a literal run passes the end of the source",
    LZ4_SOURCE_ENDS_IN_SEQUENCE: "the source ends inside a sequence",
    LZ4_BAD_OFFSET: "a match offset is 0 or larger than what the block has produced",
    LZ4_PAST_DESTINATION: "a copy passes the end of the destination",
    LZ4_ENDS_EARLY: "the block ends before the destination is full",
    LZ4_BAD_ENTRY: "a table entry lies outside the buffers",
}

Entry = Tuple[int, int, int, int, int]   # (src_off, src_len, dst_off, dst_len, raw)


class LZ4Error(ValueError):
    """a malformed LZ4 block; ``status`` is the code of the check that failed"""

    def __init__(self, status: int):
        super().__init__(f"LZ4 block: {LZ4_STATUS[status]} (status {status})")
        self.status = status


def lz4_block_status(src, dst_len: int) -> Tuple[int, bytearray]:
    """Decode one LZ4 block of exactly ``dst_len`` bytes -> (status, what was produced up to the failing check).  Every check
    comes in the order of the kernel's, so that the two name the same defect."""
    src = memoryview(src).cast("B")
    n, sp = len(src), 0
    out = bytearray()
    while True:
        if sp >= n:
            return LZ4_SOURCE_ENDS_IN_SEQUENCE, out
        token = src[sp]
        sp += 1
        lit = token >> 4
        if lit == 15:
            while True:
                if sp >= n:
                    return LZ4_SOURCE_ENDS_IN_SEQUENCE, out
                b = src[sp]
                sp += 1
                lit += b
                if b != 255:
                    break
        if lit > n - sp:
            return LZ4_LITERALS_PAST_SOURCE, out
        if lit > dst_len - len(out):
            return LZ4_PAST_DESTINATION, out
        out += src[sp:sp + lit]
        sp += lit
        if sp == n:
            return (LZ4_OK if len(out) == dst_len else LZ4_ENDS_EARLY), out
        if n - sp < 2:
            return LZ4_SOURCE_ENDS_IN_SEQUENCE, out
        off = src[sp] | (src[sp + 1] << 8)
        sp += 2
        ml = token & 15
        if ml == 15:
            while True:
                if sp >= n:
                    return LZ4_SOURCE_ENDS_IN_SEQUENCE, out
                b = src[sp]
                sp += 1
                ml += b
                if b != 255:
                    break
        ml += 4
        if off == 0 or off > len(out):
            return LZ4_BAD_OFFSET, out
        if ml > dst_len - len(out):
            return LZ4_PAST_DESTINATION, out
        start = len(out) - off
        if off >= ml:
            out += out[start:start + ml]
        else:   # periodic: byte i of the match is byte i % off of the last `off` bytes
            period = bytes(out[start:])
            out += (period * (ml // off + 1))[:ml]


def lz4_block_decode(src, dst_len: int) -> bytes:
    """one LZ4 block -> its ``dst_len`` bytes; LZ4Error (a ValueError) naming the check that failed"""
    status, out = lz4_block_status(src, dst_len)
    if status != LZ4_OK:
        raise LZ4Error(status)
    return bytes(out)


_liblz4: Optional[ctypes.CDLL] = None
_liblz4_tried = False


def liblz4() -> Optional[ctypes.CDLL]:
    """the system's liblz4, or None"""
    global _liblz4, _liblz4_tried
    if not _liblz4_tried:
        _liblz4_tried = True
        name = ctypes.util.find_library("lz4")
        if name:
            try:
                L = ctypes.CDLL(name)
                L.LZ4_decompress_safe.restype = ctypes.c_int
                L.LZ4_decompress_safe.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
                _liblz4 = L
            except (OSError, AttributeError):
                _liblz4 = None
    return _liblz4


def _lz4_block(src: bytes, dst_len: int) -> bytes:
    """one block through liblz4 where it is installed, else through lz4_block_decode.  (LZ4_decompress_safe keeps inside both
    buffers but lets a match offset of 0 pass, with undefined bytes as its result; lz4_block_decode and the kernel refuse it.)"""
    L = liblz4()
    if L is None:
        return lz4_block_decode(src, dst_len)
    dst = ctypes.create_string_buffer(max(dst_len, 1))
    got = L.LZ4_decompress_safe(src, dst, len(src), dst_len)
    if got != dst_len:
        raise ValueError(f"LZ4 block: LZ4_decompress_safe returned {got}, {dst_len} bytes expected")
    return dst.raw[:dst_len]


def parse_header(buf) -> dict:
    mv = memoryview(buf).cast("B")
    if len(mv) < HEADER:
        raise ValueError(f"Blosc chunk: {len(mv)} bytes, shorter than the {HEADER}-byte header")
    version, versionlz, flags, typesize = mv[0], mv[1], mv[2], mv[3]
    nbytes, blocksize, cbytes = struct.unpack_from("<III", mv, 4)
    return {"version": version, "versionlz": versionlz, "flags": flags, "typesize": typesize, "nbytes": nbytes,
            "blocksize": blocksize, "cbytes": cbytes, "format": flags >> 5, "memcpyed": bool(flags & FLAG_MEMCPYED)}


def parse_chunk(buf, expect_nbytes: int) -> Tuple[int, List[Entry]]:
    """Validate a chunk -> (flags, [(src_off, src_len, dst_off, dst_len, raw)]): where each block's bytes lie in the chunk,
    where its decoded bytes belong, and whether they are stored raw.  ValueError naming the check that failed;
    NotImplementedError for ``typesize > 1`` (blocks split into streams)."""
    mv = memoryview(buf).cast("B")
    h = parse_header(mv)
    if h["version"] != 2:
        raise ValueError(f"Blosc chunk: format version {h['version']}, only 2 is read")
    nbytes, blocksize, flags = h["nbytes"], h["blocksize"], h["flags"]
    if nbytes != expect_nbytes:
        raise ValueError(f"Blosc chunk: nbytes {nbytes}, {expect_nbytes} expected")
    if h["cbytes"] != len(mv):
        raise ValueError(f"Blosc chunk: cbytes {h['cbytes']}, the chunk has {len(mv)} bytes")
    if blocksize < 1:
        raise ValueError("Blosc chunk: blocksize 0")
    if h["memcpyed"]:
        if len(mv) != HEADER + nbytes:
            raise ValueError(f"Blosc chunk: memcpyed with {len(mv) - HEADER} bytes after the header, {nbytes} expected")
        return flags, ([(HEADER, nbytes, 0, nbytes, 1)] if nbytes else [])
    if h["typesize"] != 1:
        raise NotImplementedError(f"Blosc chunk: typesize {h['typesize']} (blocks split into streams), only 1 is read")
    nblocks = -(-nbytes // blocksize)
    if HEADER + 4 * nblocks > len(mv):
        raise ValueError(f"Blosc chunk: the table of {nblocks} block starts passes the end of the chunk ({len(mv)} bytes)")
    bstarts = struct.unpack_from(f"<{nblocks}i", mv, HEADER)
    entries: List[Entry] = []
    for i, bs in enumerate(bstarts):
        dst_off = i * blocksize
        dst_len = min(blocksize, nbytes - dst_off)
        if bs < HEADER + 4 * nblocks or bs + 4 > len(mv):
            raise ValueError(f"Blosc chunk: bstart {bs} of block {i} lies outside the chunk ({len(mv)} bytes)")
        csize = struct.unpack_from("<i", mv, bs)[0]
        if not 1 <= csize <= dst_len:
            raise ValueError(f"Blosc chunk: csize {csize} of block {i} outside [1, {dst_len}]")
        if bs + 4 + csize > len(mv):
            raise ValueError(f"Blosc chunk: block {i} ({csize} bytes at {bs + 4}) passes the end of the chunk ({len(mv)} bytes)")
        entries.append((bs + 4, csize, dst_off, dst_len, 1 if csize == dst_len else 0))
    return flags, entries


def device_decodable(flags: int) -> bool:
    """the blocks ``parse_chunk`` listed can go to yogo_blosc_lz4_decode: raw bytes (memcpyed) or LZ4 blocks, not bit-shuffled"""
    if flags & FLAG_MEMCPYED:
        return True
    return (flags >> 5) == 1 and not flags & FLAG_BITSHUFFLE


def device_decodable_zstd(flags: int) -> bool:
    """the blocks ``parse_chunk`` listed can go to yogo_zstd_decode: raw bytes (memcpyed) or one Zstandard frame per block, not
    bit-shuffled"""
    if flags & FLAG_MEMCPYED:
        return True
    return (flags >> 5) == 4 and not flags & FLAG_BITSHUFFLE


def decompress(buf, expect_nbytes: int, zstd: Optional[Callable[[bytes, int], bytes]] = None) -> bytes:
    """a whole chunk on the host.  NotImplementedError naming what was found for bit-shuffle, ``typesize > 1`` and inner
    formats other than lz4 / lz4hc and zlib; ValueError for a malformed chunk.  ``zstd``: a decoder of one Zstandard frame
    ``(bytes, decoded size) -> bytes`` (yogo_amd.zstd.frame_decoder()); with it, inner format 4 (one frame per block) is read."""
    mv = memoryview(buf).cast("B")
    flags, entries = parse_chunk(mv, expect_nbytes)
    if flags & FLAG_MEMCPYED:
        return bytes(mv[HEADER:HEADER + expect_nbytes])
    if flags & FLAG_BITSHUFFLE:
        raise NotImplementedError("Blosc chunk: bit-shuffle (flag 0x04) is not read")
    fmt = flags >> 5
    if fmt not in (1, 3) and not (fmt == 4 and zstd is not None):
        raise NotImplementedError(f"Blosc chunk: inner format {fmt} ({FORMATS.get(fmt, 'unknown')}) is not read (lz4, lz4hc and zlib are)")
    out = bytearray(expect_nbytes)
    for src_off, src_len, dst_off, dst_len, raw in entries:
        data = mv[src_off:src_off + src_len]
        if raw:
            out[dst_off:dst_off + dst_len] = data
        elif fmt == 1:
            out[dst_off:dst_off + dst_len] = _lz4_block(bytes(data), dst_len)
        elif fmt == 4:
            block = zstd(bytes(data), dst_len)
            if len(block) != dst_len:
                raise ValueError(f"Blosc chunk: a zstd block of {len(block)} bytes, {dst_len} expected")
            out[dst_off:dst_off + dst_len] = block
        else:
            block = zlib.decompress(data)
            if len(block) != dst_len:
                raise ValueError(f"Blosc chunk: a zlib block of {len(block)} bytes, {dst_len} expected")
            out[dst_off:dst_off + dst_len] = block
    return bytes(out)
