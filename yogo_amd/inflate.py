"""The host side of zlib streams (standard library only), written from RFC 1950 (the wrapper) and RFC 1951 (DEFLATE).

``split_zlib`` takes the wrapper off a stream -- what yogo_amd/zarr_feed.py does per chunk before it hands the raw DEFLATE bytes
to ``yogo_inflate_zlib`` (csrc/inflate.hip) -- and ``inflate_status`` is a pure-Python inflater with the checks, the order of
the checks and the status codes of the kernel: the twin the tests hold both against ``zlib`` with.  It decodes every code by
the canonical walk (per-length counts, symbols sorted by code), which the kernel's primary tables are built from and fall back
to; code-length sets are held to zlib's rule (inflate_table): over-subscribed sets are refused, incomplete ones too, except a
literal / length or distance set whose only code has length 1 and a distance set without any code.
"""
from __future__ import annotations

import struct
import zlib
from typing import List, Optional, Sequence, Tuple

# status of one stream, the same numbers in csrc/inflate.hip
INF_OK = 0
INF_BAD_ROW = 1            # (kernel only) a table row that does not lie inside the buffers
INF_BAD_BLOCK_TYPE = 2     # block type 3
INF_STORED_LEN = 3         # a stored block whose NLEN is not the complement of its LEN
INF_SOURCE_ENDS = 4        # the source ends inside a block header, a code, its extra bits or a stored block's bytes
INF_BAD_LENGTHS = 5        # a dynamic header: too many codes, a repeat with nothing before it or past the end, no end-of-block
#                            code, an over-subscribed or an incomplete set
INF_BAD_SYMBOL = 6         # a bit pattern no code owns, literal / length symbol 286 or 287, distance code 30 or 31
INF_BAD_DISTANCE = 7       # a distance larger than what the stream has produced
INF_PAST_DESTINATION = 8   # a literal, a match or a stored block that would pass dst_len
INF_ENDS_EARLY = 9         # the final block ends before dst_len
INF_ADLER = 10             # dst_len bytes came out and their Adler-32 is not the trailer's
INF_STATUS = {
    INF_BAD_ROW: "a table row lies outside the buffers",
    INF_BAD_BLOCK_TYPE: "block type 3",
    INF_STORED_LEN: "a stored block's LEN and NLEN do not match",
    INF_SOURCE_ENDS: "the source ends inside a token",
    INF_BAD_LENGTHS: "a dynamic block's code lengths are invalid",
    INF_BAD_SYMBOL: "a code or symbol that the format does not define",
    INF_BAD_DISTANCE: "a match distance larger than what the stream has produced",
    INF_PAST_DESTINATION: "the stream passes the end of the destination",
    INF_ENDS_EARLY: "the stream ends before the destination is full",
    INF_ADLER: "the Adler-32 of the inflated bytes is not the trailer's",
}

MAX_BITS = 15
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LIT_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST_LENS = [5] * 32


def split_zlib(stream) -> Tuple[int, int, int]:
    """(deflate_off, deflate_len, adler32) of one zlib stream: where its raw DEFLATE bytes lie and what its trailer says.
    ValueError on a wrapper the device route does not take: too short, CM != 8, CINFO > 7, a bad FCHECK, a preset dictionary."""
    mv = memoryview(stream).cast("B")
    if len(mv) < 6:
        raise ValueError(f"zlib stream: {len(mv)} bytes, shorter than header and trailer")
    cmf, flg = mv[0], mv[1]
    if cmf & 15 != 8:
        raise ValueError(f"zlib stream: compression method {cmf & 15}, only 8 (deflate) is read")
    if cmf >> 4 > 7:
        raise ValueError(f"zlib stream: window size code {cmf >> 4} above 7")
    if (cmf * 256 + flg) % 31:
        raise ValueError("zlib stream: the header check (FCHECK) fails")
    if flg & 0x20:
        raise ValueError("zlib stream: a preset dictionary (FDICT) is not read")
    return 2, len(mv) - 6, struct.unpack_from(">I", mv, len(mv) - 4)[0]


class _Code:
    """one canonical Huffman code: count[l] codes of length l, the symbols sorted by code"""

    def __init__(self, lens: Sequence[int]):
        self.count = [0] * (MAX_BITS + 1)
        for l in lens:
            self.count[l] += 1
        self.count[0] = 0
        self.sorted = [s for l in range(1, MAX_BITS + 1) for s, sl in enumerate(lens) if sl == l]
        left = 1
        self.over = False
        for l in range(1, MAX_BITS + 1):
            left = (left << 1) - self.count[l]
            if left < 0:
                self.over = True
                break
        self.left = left
        self.longest = max((l for l in range(1, MAX_BITS + 1) if self.count[l]), default=0)

    def usable(self, codes: bool) -> bool:
        """zlib's rule; codes: the code-length code, which must be complete"""
        if self.over:
            return False
        return not (self.left > 0 if codes else (self.left > 0 and self.longest > 1))

    def decode(self, bits: int) -> Tuple[int, int]:
        """one code off the low bits -> (length, symbol); (15, -1) where no code owns the pattern"""
        code = first = index = 0
        for l in range(1, MAX_BITS + 1):
            code |= (bits >> (l - 1)) & 1
            c = self.count[l]
            if code - c < first:
                return l, self.sorted[index + code - first]
            index += c
            first = (first + c) << 1
            code <<= 1
        return MAX_BITS, -1


def inflate_status(deflate, dst_len: int, adler32: Optional[int] = None) -> Tuple[int, bytes]:
    """Inflate one raw DEFLATE stream of exactly ``dst_len`` bytes -> (status, what was produced up to the failing check).
    Every check comes in the order of the kernel's, so that the two name the same defect.  ``adler32``: the trailer's value
    (None: not compared)."""
    src = memoryview(deflate).cast("B")
    n = len(src)
    nbits = 8 * n
    padded = bytes(src) + bytes(9)
    bp = 0
    out = bytearray()

    def peek(at: int) -> int:   # the 64 bits from `at` on; zero past the end
        return (int.from_bytes(padded[at >> 3:(at >> 3) + 9], "little") >> (at & 7)) & 0xFFFFFFFFFFFFFFFF

    def body() -> int:
        nonlocal bp
        while True:
            if bp + 3 > nbits:
                return INF_SOURCE_ENDS
            hdr = peek(bp)
            bfinal, btype = hdr & 1, (hdr >> 1) & 3
            bp += 3
            if btype == 3:
                return INF_BAD_BLOCK_TYPE
            if btype == 0:
                bp = (bp + 7) & ~7
                if bp + 32 > nbits:
                    return INF_SOURCE_ENDS
                v = peek(bp)
                ln = v & 0xFFFF
                bp += 32
                if ln != ((v >> 16) & 0xFFFF) ^ 0xFFFF:
                    return INF_STORED_LEN
                if ln > n - (bp >> 3):
                    return INF_SOURCE_ENDS
                if ln > dst_len - len(out):
                    return INF_PAST_DESTINATION
                out.extend(src[bp >> 3:(bp >> 3) + ln])
                bp += 8 * ln
            else:
                if btype == 1:
                    lit_lens: List[int] = FIXED_LIT_LENS
                    dist_lens: List[int] = FIXED_DIST_LENS
                else:
                    if bp + 14 > nbits:
                        return INF_SOURCE_ENDS
                    v = peek(bp)
                    nl, nd, nc = (v & 31) + 257, ((v >> 5) & 31) + 1, ((v >> 10) & 15) + 4
                    bp += 14
                    if nl > 286 or nd > 30:
                        return INF_BAD_LENGTHS
                    if bp + 3 * nc > nbits:
                        return INF_SOURCE_ENDS
                    v = peek(bp)
                    bp += 3 * nc
                    cl = [0] * 19
                    for k in range(nc):
                        cl[CL_ORDER[k]] = (v >> (3 * k)) & 7
                    cc = _Code(cl)
                    if not cc.usable(True):
                        return INF_BAD_LENGTHS
                    total = nl + nd
                    lens: List[int] = []
                    prev = 0
                    while len(lens) < total:
                        v = peek(bp)
                        l, sym = cc.decode(v)
                        if bp + l > nbits:
                            return INF_SOURCE_ENDS
                        if sym < 0:
                            return INF_BAD_LENGTHS
                        bp += l
                        v >>= l
                        if sym < 16:
                            lens.append(sym)
                            prev = sym
                            continue
                        if sym == 16 and not lens:
                            return INF_BAD_LENGTHS
                        eb = 2 if sym == 16 else 3 if sym == 17 else 7
                        val = prev if sym == 16 else 0
                        if bp + eb > nbits:
                            return INF_SOURCE_ENDS
                        rep = (11 if sym == 18 else 3) + (v & ((1 << eb) - 1))
                        bp += eb
                        if len(lens) + rep > total:
                            return INF_BAD_LENGTHS
                        lens.extend([val] * rep)
                        prev = val
                    if lens[256] == 0:
                        return INF_BAD_LENGTHS
                    lit_lens, dist_lens = lens[:nl], lens[nl:]
                lc, dc = _Code(lit_lens), _Code(dist_lens)
                if not lc.usable(False) or not dc.usable(False):
                    return INF_BAD_LENGTHS
                while True:
                    v = peek(bp)
                    l, sym = lc.decode(v)
                    if bp + l > nbits:
                        return INF_SOURCE_ENDS
                    if sym < 0:
                        return INF_BAD_SYMBOL
                    bp += l
                    v >>= l
                    if sym < 256:
                        if len(out) >= dst_len:
                            return INF_PAST_DESTINATION
                        out.append(sym)
                        continue
                    if sym == 256:
                        break
                    if sym >= 286:
                        return INF_BAD_SYMBOL
                    sym -= 257
                    eb = 0 if sym < 8 or sym == 28 else (sym >> 2) - 1
                    if bp + eb > nbits:
                        return INF_SOURCE_ENDS
                    ln = (3 + sym if sym < 8 else 258 if sym == 28 else 3 + ((4 + (sym & 3)) << eb)) + (v & ((1 << eb) - 1))
                    bp += eb
                    v >>= eb
                    l, sym = dc.decode(v)
                    if bp + l > nbits:
                        return INF_SOURCE_ENDS
                    if sym < 0 or sym >= 30:
                        return INF_BAD_SYMBOL
                    bp += l
                    v >>= l
                    eb = 0 if sym < 4 else (sym >> 1) - 1
                    if bp + eb > nbits:
                        return INF_SOURCE_ENDS
                    dist = (1 + sym if sym < 4 else 1 + ((2 + (sym & 1)) << eb)) + (v & ((1 << eb) - 1))
                    bp += eb
                    if dist > len(out):
                        return INF_BAD_DISTANCE
                    if ln > dst_len - len(out):
                        return INF_PAST_DESTINATION
                    start = len(out) - dist
                    if dist >= ln:
                        out.extend(out[start:start + ln])
                    else:   # periodic: byte i of the match is byte i % dist of the last `dist` bytes
                        out.extend((bytes(out[start:]) * (ln // dist + 1))[:ln])
            if bfinal:
                return INF_OK

    status = body()
    if status == INF_OK and len(out) != dst_len:
        status = INF_ENDS_EARLY
    if status == INF_OK and adler32 is not None and zlib.adler32(out) != adler32:
        status = INF_ADLER
    return status, bytes(out)
