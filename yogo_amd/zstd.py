"""The host side of Zstandard frames (standard library only), written from the published format (RFC 8878).

``zstd_frame_status`` is a pure-Python decoder of ONE frame with the checks, the order of the checks and the status codes of the
kernel (csrc/zstd.hip, ``yogo_zstd_decode``): the twin the tests hold both against libzstd's own frames with
(tests/golden/zstd_frames.npz).  ``zstd_decode`` is the same with an exception, ``frame_decoder`` picks what the host route decodes a
frame with (libzstd through ctypes where it loads, else this module), ``libzstd`` is the system's library or None.

What is read: one frame -- magic, frame header with or without window descriptor and frame content size (which must equal the
expected size); raw, RLE and compressed blocks of at most 128 KB; literals sections raw, RLE, Huffman-compressed (1 or 4 streams,
weights direct or FSE-compressed) and treeless; sequences sections with every table predefined, RLE, FSE-compressed or repeated;
the three repeat offsets; offset codes up to 31.  A match may reach back over everything the frame has produced: the window size is
parsed and otherwise NOT enforced.  A content checksum, when the header flags one, must be present (4 bytes) and is NOT verified.
Refused with a status: a dictionary id, a skippable frame, a set reserved bit, anything after the frame's end (a second frame too).
"""
from __future__ import annotations

import ctypes
import ctypes.util
from typing import Callable, List, Optional, Set, Tuple

MAGIC = 0xFD2FB528
BLOCK_MAX = 1 << 17          # bytes of a block, and of a block's literals
HUF_MAX_BITS = 11
LL_MAX_LOG, ML_MAX_LOG, OF_MAX_LOG, HUF_MAX_LOG = 9, 9, 8, 6
LL_MAX_SYM, ML_MAX_SYM, OF_MAX_SYM, HUF_MAX_SYM = 35, 52, 31, 11

# status of one frame, the same numbers in csrc/zstd.hip and include/yogo_hip.h
ZSTD_OK = 0
ZSTD_BAD_ROW = 1             # (kernel only) a table row that does not lie inside the buffers
ZSTD_SOURCE_ENDS = 2         # the source, or a block, ends inside a header, a section or a table description
ZSTD_BAD_MAGIC = 3           # the first four bytes are not the frame magic (a skippable frame's magic included)
ZSTD_UNSUPPORTED_HEADER = 4  # a set reserved bit or a dictionary id in the frame header
ZSTD_CONTENT_SIZE = 5        # the header's frame content size is not the expected size
ZSTD_BAD_BLOCK = 6           # block type 3, or a block size above 128 KB
ZSTD_BAD_LITERALS = 7        # a literals section: above 128 KB, stream sizes past the section, treeless without a table
ZSTD_BAD_HUFFMAN = 8         # Huffman weights that describe no code of at most 11 bits
ZSTD_BAD_FSE_TABLE = 9       # an FSE table: accuracy log or symbol above the limit, probabilities that do not sum up, repeat without a table
ZSTD_BAD_BITSTREAM = 10      # a backward bitstream that is empty, lacks its marker bit, or is not consumed exactly
ZSTD_BAD_SEQUENCES = 11      # a sequences section: reserved mode bits, bytes after zero sequences, a literal length past the block's literals
ZSTD_BAD_OFFSET = 12         # a match offset of 0 or larger than what the frame has produced
ZSTD_PAST_DESTINATION = 13   # a block, literals or a match that would pass the expected size
ZSTD_ENDS_EARLY = 14         # the last block ends before the expected size
ZSTD_TRAILING = 15           # bytes after the frame's end
ZSTD_STATUS = {
    ZSTD_BAD_ROW: "a table row lies outside the buffers",
    ZSTD_SOURCE_ENDS: "the source ends inside a header or a section",
    ZSTD_BAD_MAGIC: "no Zstandard frame magic",
    ZSTD_UNSUPPORTED_HEADER: "a reserved bit or a dictionary id in the frame header",
    ZSTD_CONTENT_SIZE: "the frame content size is not the expected size",
    ZSTD_BAD_BLOCK: "a reserved block type or a block above 128 KB",
    ZSTD_BAD_LITERALS: "an invalid literals section",
    ZSTD_BAD_HUFFMAN: "invalid Huffman weights",
    ZSTD_BAD_FSE_TABLE: "an invalid FSE table",
    ZSTD_BAD_BITSTREAM: "a bitstream without its end marker or not consumed exactly",
    ZSTD_BAD_SEQUENCES: "an invalid sequences section",
    ZSTD_BAD_OFFSET: "a match offset is 0 or larger than what the frame has produced",
    ZSTD_PAST_DESTINATION: "the frame passes the end of the destination",
    ZSTD_ENDS_EARLY: "the frame ends before the destination is full",
    ZSTD_TRAILING: "bytes after the end of the frame",
}

LL_DEFAULT = (4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1)
ML_DEFAULT = (1, 4, 3, 2, 2, 2, 2, 2, 2) + (1,) * 37 + (-1,) * 7
OF_DEFAULT = (1, 1, 1, 1, 1, 1, 2, 2, 2) + (1,) * 15 + (-1,) * 5
LL_BASE = tuple(range(16)) + (16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536)
LL_BITS = (0,) * 16 + (1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16)
ML_BASE = tuple(range(3, 35)) + (35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539)
ML_BITS = (0,) * 32 + (1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16)


class ZstdError(ValueError):
    """a malformed or unsupported Zstandard frame; ``status`` is the code of the check that failed"""

    def __init__(self, status: int):
        super().__init__(f"Zstandard frame: {ZSTD_STATUS[status]} (status {status})")
        self.status = status


class _Stop(Exception):
    def __init__(self, status: int):
        self.status = status


class FseTable:
    """one FSE decoding table: per state its symbol, the bits to read and the base of the next state"""

    def __init__(self, log: int, symbol: List[int], nbits: List[int], base: List[int]):
        self.log, self.symbol, self.nbits, self.base = log, symbol, nbits, base


def fse_build(freq, log: int) -> FseTable:
    """the decoding table of normalised counts (-1: "less than one") that sum to ``1 << log``"""
    size = 1 << log
    symbol = [0] * size
    high = size
    nxt = [0] * len(freq)
    for s, f in enumerate(freq):
        if f == -1:
            high -= 1
            symbol[high] = s
            nxt[s] = 1
    step, mask, pos = (size >> 1) + (size >> 3) + 3, size - 1, 0
    for s, f in enumerate(freq):
        if f > 0:
            nxt[s] = f
            for _ in range(f):
                symbol[pos] = s
                pos = (pos + step) & mask
                while pos >= high:
                    pos = (pos + step) & mask
    nbits, base = [0] * size, [0] * size
    for i in range(size):
        x = nxt[symbol[i]]
        nxt[symbol[i]] += 1
        nbits[i] = log - (x.bit_length() - 1)
        base[i] = (x << nbits[i]) - size
    return FseTable(log, symbol, nbits, base)


def fse_rle(sym: int) -> FseTable:
    return FseTable(0, [sym], [0], [0])


class _Forward:
    """bits of src[lo:hi], least significant first; a peek past the end reads zeros, ``take`` refuses to pass it"""

    def __init__(self, src, lo: int, hi: int):
        self.v = int.from_bytes(bytes(src[lo:hi]), "little")
        self.lo, self.nbits, self.pos = lo, 8 * (hi - lo), 0

    def peek(self, k: int) -> int:
        return (self.v >> self.pos) & ((1 << k) - 1)

    def take(self, k: int) -> None:
        self.pos += k
        if self.pos > self.nbits:
            raise _Stop(ZSTD_SOURCE_ENDS)

    def end(self) -> int:
        """the byte after the last one used"""
        return self.lo + (self.pos + 7) // 8


def read_fse_description(src, lo: int, hi: int, max_log: int, max_sym: int, trace: Optional[Set[str]] = None) -> Tuple[FseTable, int]:
    """an FSE table description at src[lo:hi] -> (table, the byte after it)"""
    f = _Forward(src, lo, hi)
    log = 5 + f.peek(4)
    f.take(4)
    if log > max_log:
        raise _Stop(ZSTD_BAD_FSE_TABLE)
    if trace is not None and log == max_log:
        trace.add(f"accuracy_log_at_limit_{max_log}")
    remaining = 1 << log
    freq: List[int] = []
    while remaining > 0:
        if len(freq) > max_sym:
            raise _Stop(ZSTD_BAD_FSE_TABLE)
        bits = (remaining + 1).bit_length()
        val = f.peek(bits)
        lower = (1 << (bits - 1)) - 1
        threshold = (1 << bits) - 1 - (remaining + 1)
        if (val & lower) < threshold:
            f.take(bits - 1)
            val &= lower
        else:
            f.take(bits)
            if val > lower:
                val -= threshold
        p = val - 1
        if p == -1 and trace is not None:
            trace.add("less_than_one_probability")
        remaining -= abs(p)
        if remaining < 0:
            raise _Stop(ZSTD_BAD_FSE_TABLE)
        freq.append(p)
        if p == 0:
            while True:
                rep = f.peek(2)
                f.take(2)
                freq.extend([0] * rep)
                if rep != 3:
                    break
                if len(freq) > max_sym + 1:
                    raise _Stop(ZSTD_BAD_FSE_TABLE)
    if len(freq) > max_sym + 1:
        raise _Stop(ZSTD_BAD_FSE_TABLE)
    return fse_build(freq, log), f.end()


def _bits(data: bytes, p: int, k: int) -> int:
    """the k bits (k <= 32) from bit p of `data`, least significant first; zeros below bit 0.  Five bytes at the most are touched:
    the cost does not grow with the stream"""
    if p >= 0:
        return (int.from_bytes(data[p >> 3:(p >> 3) + 5], "little") >> (p & 7)) & ((1 << k) - 1)
    if k + p <= 0:
        return 0
    return (int.from_bytes(data[:5], "little") << -p) & ((1 << k) - 1)


class _Backward:
    """a backward bitstream src[lo:hi]: the last byte holds the 1 marker bit above the first bits to read"""

    def __init__(self, src, lo: int, hi: int):
        if hi <= lo or src[hi - 1] == 0:
            raise _Stop(ZSTD_BAD_BITSTREAM)
        self.data = bytes(src[lo:hi])
        self.pos = 8 * (hi - lo - 1) + src[hi - 1].bit_length() - 1   # bits left to read

    def read(self, k: int) -> int:
        """k bits; below the stream's start zeros are read and ``pos`` goes negative (the caller's to judge)"""
        self.pos -= k
        return _bits(self.data, self.pos, k)


class HufTable:
    """a Huffman decoding table of 1 << log entries: symbol and bits of the code that owns each pattern"""

    def __init__(self, log: int, symbol: List[int], nbits: List[int]):
        self.log, self.symbol, self.nbits = log, symbol, nbits


def huf_build(weights: List[int]) -> HufTable:
    """weights of the symbols 0 .. len - 1, the last one still to be implied"""
    total = sum((1 << (w - 1)) for w in weights if w)
    if total == 0:
        raise _Stop(ZSTD_BAD_HUFFMAN)
    log = total.bit_length()
    if log > HUF_MAX_BITS:
        raise _Stop(ZSTD_BAD_HUFFMAN)
    left = (1 << log) - total
    if left & (left - 1):
        raise _Stop(ZSTD_BAD_HUFFMAN)
    weights = list(weights) + [left.bit_length()]
    symbol, nbits = [0] * (1 << log), [0] * (1 << log)
    at = 0
    for w in range(1, log + 1):
        for s, ws in enumerate(weights):
            if ws == w:
                n = 1 << (w - 1)
                symbol[at:at + n] = [s] * n
                nbits[at:at + n] = [log + 1 - w] * n
                at += n
    return HufTable(log, symbol, nbits)


def read_huffman_description(src, lo: int, hi: int, trace: Optional[Set[str]] = None) -> Tuple[HufTable, int]:
    """a Huffman tree description at src[lo:hi] -> (table, the byte after it)"""
    if lo >= hi:
        raise _Stop(ZSTD_SOURCE_ENDS)
    hb = src[lo]
    weights: List[int] = []
    if hb >= 128:
        n = hb - 127
        end = lo + 1 + (n + 1) // 2
        if end > hi:
            raise _Stop(ZSTD_SOURCE_ENDS)
        for i in range(n):
            b = src[lo + 1 + i // 2]
            weights.append((b >> 4) if i % 2 == 0 else (b & 15))
        if max(weights) > HUF_MAX_BITS:
            raise _Stop(ZSTD_BAD_HUFFMAN)
        if trace is not None:
            trace.add("huffman_direct_weights")
    else:
        end = lo + 1 + hb
        if end > hi:
            raise _Stop(ZSTD_SOURCE_ENDS)
        table, at = read_fse_description(src, lo + 1, end, HUF_MAX_LOG, HUF_MAX_SYM, trace)
        bs = _Backward(src, at, end)
        s1 = bs.read(table.log)
        s2 = bs.read(table.log)
        if bs.pos < 0:
            raise _Stop(ZSTD_BAD_BITSTREAM)
        while True:   # the two states take turns until one's update passes the start of the stream
            if len(weights) >= 254:
                raise _Stop(ZSTD_BAD_HUFFMAN)
            weights.append(table.symbol[s1])
            s1 = table.base[s1] + bs.read(table.nbits[s1])
            if bs.pos < 0:
                weights.append(table.symbol[s2])
                break
            weights.append(table.symbol[s2])
            s2 = table.base[s2] + bs.read(table.nbits[s2])
            if bs.pos < 0:
                weights.append(table.symbol[s1])
                break
        if trace is not None:
            trace.add("huffman_fse_weights")
    t = huf_build(weights)
    if trace is not None and t.log == HUF_MAX_BITS:
        trace.add("huffman_11_bit_code")
    return t, end


def _huf_stream(src, lo: int, hi: int, count: int, t: HufTable, out: bytearray) -> None:
    bs = _Backward(src, lo, hi)
    data, pos, log, symbol, nbits = bs.data, bs.pos, t.log, t.symbol, t.nbits
    for _ in range(count):
        e = _bits(data, pos - log, log)    # (zeros below the start)
        out.append(symbol[e])
        pos -= nbits[e]
        if pos < 0:
            break
    if pos != 0:
        raise _Stop(ZSTD_BAD_BITSTREAM)


class _Frame:
    def __init__(self, src, dst_len: int, trace: Optional[Set[str]]):
        self.src = memoryview(src).cast("B")
        self.n = len(self.src)
        self.dst_len = dst_len
        self.out = bytearray()
        self.trace = trace
        self.huf: Optional[HufTable] = None
        self.tables: List[Optional[FseTable]] = [None, None, None]   # literal length, offset, match length
        self.rep = [1, 4, 8]
        self.window = 0

    def note(self, what: str) -> None:
        if self.trace is not None:
            self.trace.add(what)

    def run(self) -> None:
        src, n = self.src, self.n
        if n < 4:
            raise _Stop(ZSTD_SOURCE_ENDS)
        if int.from_bytes(bytes(src[0:4]), "little") != MAGIC:
            raise _Stop(ZSTD_BAD_MAGIC)
        if n < 5:
            raise _Stop(ZSTD_SOURCE_ENDS)
        fhd = src[4]
        p = 5
        if fhd & 0x08 or fhd & 0x03:
            raise _Stop(ZSTD_UNSUPPORTED_HEADER)
        single, checksum, fcs_flag = (fhd >> 5) & 1, (fhd >> 2) & 1, fhd >> 6
        if not single:
            if p >= n:
                raise _Stop(ZSTD_SOURCE_ENDS)
            wd = src[p]
            p += 1
            base = 1 << (10 + (wd >> 3))
            self.window = base + (base >> 3) * (wd & 7)    # parsed, not enforced
            self.note("window_descriptor")
        fcs_bytes = (1 if single else 0, 2, 4, 8)[fcs_flag]
        if fcs_bytes:
            if n - p < fcs_bytes:
                raise _Stop(ZSTD_SOURCE_ENDS)
            fcs = int.from_bytes(bytes(src[p:p + fcs_bytes]), "little") + (256 if fcs_bytes == 2 else 0)
            p += fcs_bytes
            if fcs != self.dst_len:
                raise _Stop(ZSTD_CONTENT_SIZE)
            self.note("frame_content_size")
        blocks = 0
        while True:
            if n - p < 3:
                raise _Stop(ZSTD_SOURCE_ENDS)
            bh = src[p] | (src[p + 1] << 8) | (src[p + 2] << 16)
            p += 3
            last, btype, size = bh & 1, (bh >> 1) & 3, bh >> 3
            if btype == 3 or size > BLOCK_MAX:
                raise _Stop(ZSTD_BAD_BLOCK)
            blocks += 1
            if btype == 0:
                if size > n - p:
                    raise _Stop(ZSTD_SOURCE_ENDS)
                if size > self.dst_len - len(self.out):
                    raise _Stop(ZSTD_PAST_DESTINATION)
                self.out += src[p:p + size]
                p += size
                self.note("raw_block")
            elif btype == 1:
                if n - p < 1:
                    raise _Stop(ZSTD_SOURCE_ENDS)
                if size > self.dst_len - len(self.out):
                    raise _Stop(ZSTD_PAST_DESTINATION)
                self.out += bytes([src[p]]) * size
                p += 1
                self.note("rle_block")
            else:
                if size > n - p:
                    raise _Stop(ZSTD_SOURCE_ENDS)
                self.block(p, p + size)
                p += size
                self.note("compressed_block")
            if last:
                break
        if blocks > 1:
            self.note("several_blocks")
        if checksum:
            if n - p < 4:
                raise _Stop(ZSTD_SOURCE_ENDS)
            p += 4    # present, not verified
            self.note("content_checksum")
        if p != n:
            raise _Stop(ZSTD_TRAILING)
        if len(self.out) != self.dst_len:
            raise _Stop(ZSTD_ENDS_EARLY)

    def literals(self, lo: int, hi: int) -> Tuple[bytes, int]:
        """the literals section at the start of the block src[lo:hi] -> (the literals, the byte after the section)"""
        src = self.src
        if lo >= hi:
            raise _Stop(ZSTD_SOURCE_ENDS)
        b0 = src[lo]
        ltype, sf = b0 & 3, (b0 >> 2) & 3
        if ltype < 2:
            hdr = (1, 2, 1, 3)[sf]
            if hdr > hi - lo:
                raise _Stop(ZSTD_SOURCE_ENDS)
            v = int.from_bytes(bytes(src[lo:lo + hdr]), "little")
            regen = v >> (3 if hdr == 1 else 4)
            if regen > BLOCK_MAX:
                raise _Stop(ZSTD_BAD_LITERALS)
            at = lo + hdr
            if ltype == 0:
                if regen > hi - at:
                    raise _Stop(ZSTD_SOURCE_ENDS)
                self.note("raw_literals")
                return bytes(src[at:at + regen]), at + regen
            if hi - at < 1:
                raise _Stop(ZSTD_SOURCE_ENDS)
            self.note("rle_literals")
            return bytes([src[at]]) * regen, at + 1
        hdr, bits = ((3, 10), (3, 10), (4, 14), (5, 18))[sf]
        if hdr > hi - lo:
            raise _Stop(ZSTD_SOURCE_ENDS)
        v = int.from_bytes(bytes(src[lo:lo + hdr]), "little")
        regen, comp = (v >> 4) & ((1 << bits) - 1), (v >> (4 + bits)) & ((1 << bits) - 1)
        if regen > BLOCK_MAX:
            raise _Stop(ZSTD_BAD_LITERALS)
        at = lo + hdr
        if comp > hi - at:
            raise _Stop(ZSTD_SOURCE_ENDS)
        end = at + comp
        if ltype == 2:
            self.huf, at = read_huffman_description(src, at, end, self.trace)
        else:
            if self.huf is None:
                raise _Stop(ZSTD_BAD_LITERALS)
            self.note("treeless_literals")
        out = bytearray()
        if sf == 0:
            self.note("huffman_1_stream")
            _huf_stream(src, at, end, regen, self.huf, out)
            if len(out) != regen:
                raise _Stop(ZSTD_BAD_BITSTREAM)
        else:
            self.note("huffman_4_streams")
            if end - at < 6:
                raise _Stop(ZSTD_SOURCE_ENDS)
            sizes = [src[at + 2 * i] | (src[at + 2 * i + 1] << 8) for i in range(3)]
            at += 6
            if sum(sizes) > end - at:
                raise _Stop(ZSTD_BAD_LITERALS)
            sizes.append(end - at - sum(sizes))
            seg = (regen + 3) // 4
            if regen < 3 * seg:
                raise _Stop(ZSTD_BAD_LITERALS)
            for i, sz in enumerate(sizes):
                part = bytearray()
                want = seg if i < 3 else regen - 3 * seg
                _huf_stream(src, at, at + sz, want, self.huf, part)
                if len(part) != want:
                    raise _Stop(ZSTD_BAD_BITSTREAM)
                out += part
                at += sz
        return bytes(out), end

    def block(self, lo: int, hi: int) -> None:
        src, out = self.src, self.out
        block_start = len(out)
        lits, q = self.literals(lo, hi)
        if q >= hi:
            raise _Stop(ZSTD_SOURCE_ENDS)
        b0 = src[q]
        if b0 == 0:
            nseq, q = 0, q + 1
            if q != hi:
                raise _Stop(ZSTD_BAD_SEQUENCES)
            self.note("zero_sequences")
        elif b0 < 128:
            nseq, q = b0, q + 1
        elif b0 < 255:
            if hi - q < 2:
                raise _Stop(ZSTD_SOURCE_ENDS)
            nseq, q = ((b0 - 128) << 8) + src[q + 1], q + 2
        else:
            if hi - q < 3:
                raise _Stop(ZSTD_SOURCE_ENDS)
            nseq, q = src[q + 1] + (src[q + 2] << 8) + 0x7F00, q + 3
        lp = 0
        if nseq:
            if q >= hi:
                raise _Stop(ZSTD_SOURCE_ENDS)
            modes = src[q]
            q += 1
            if modes & 3:
                raise _Stop(ZSTD_BAD_SEQUENCES)
            spec = (("ll", modes >> 6, LL_DEFAULT, 6, LL_MAX_LOG, LL_MAX_SYM), ("of", (modes >> 4) & 3, OF_DEFAULT, 5, OF_MAX_LOG, OF_MAX_SYM),
                    ("ml", (modes >> 2) & 3, ML_DEFAULT, 6, ML_MAX_LOG, ML_MAX_SYM))
            for i, (name, mode, default, dlog, max_log, max_sym) in enumerate(spec):
                self.note(f"{name}_table_{('predefined', 'rle', 'fse', 'repeat')[mode]}")
                if mode == 0:
                    self.tables[i] = fse_build(default, dlog)
                elif mode == 1:
                    if q >= hi:
                        raise _Stop(ZSTD_SOURCE_ENDS)
                    if src[q] > max_sym:
                        raise _Stop(ZSTD_BAD_FSE_TABLE)
                    self.tables[i] = fse_rle(src[q])
                    q += 1
                elif mode == 2:
                    self.tables[i], q = read_fse_description(src, q, hi, max_log, max_sym, self.trace)
                elif self.tables[i] is None:
                    raise _Stop(ZSTD_BAD_FSE_TABLE)
            ll_t, of_t, ml_t = self.tables
            bs = _Backward(src, q, hi)
            ll_s, of_s, ml_s = bs.read(ll_t.log), bs.read(of_t.log), bs.read(ml_t.log)
            if bs.pos < 0:
                raise _Stop(ZSTD_BAD_BITSTREAM)
            rep = self.rep
            for i in range(nseq):
                ofc, mlc, llc = of_t.symbol[of_s], ml_t.symbol[ml_s], ll_t.symbol[ll_s]
                ofv = (1 << ofc) + bs.read(ofc)
                ml = ML_BASE[mlc] + bs.read(ML_BITS[mlc])
                ll = LL_BASE[llc] + bs.read(LL_BITS[llc])
                if i != nseq - 1:
                    ll_s = ll_t.base[ll_s] + bs.read(ll_t.nbits[ll_s])
                    ml_s = ml_t.base[ml_s] + bs.read(ml_t.nbits[ml_s])
                    of_s = of_t.base[of_s] + bs.read(of_t.nbits[of_s])
                if bs.pos < 0:
                    raise _Stop(ZSTD_BAD_BITSTREAM)
                if ofv > 3:
                    off = ofv - 3
                    rep[:] = [off, rep[0], rep[1]]
                else:
                    idx = ofv - 1 + (1 if ll == 0 else 0)
                    self.note(f"repeat_offset_{ofv}" + ("_ll0" if ll == 0 else ""))
                    if idx == 0:
                        off = rep[0]
                    elif idx == 1:
                        off = rep[1]
                        rep[:] = [rep[1], rep[0], rep[2]]
                    elif idx == 2:
                        off = rep[2]
                        rep[:] = [rep[2], rep[0], rep[1]]
                    else:
                        off = rep[0] - 1
                        rep[:] = [off, rep[0], rep[1]]
                if ll > len(lits) - lp:
                    raise _Stop(ZSTD_BAD_SEQUENCES)
                if ll > self.dst_len - len(out):
                    raise _Stop(ZSTD_PAST_DESTINATION)
                out += lits[lp:lp + ll]
                lp += ll
                if off == 0 or off > len(out):
                    raise _Stop(ZSTD_BAD_OFFSET)
                if ml > self.dst_len - len(out):
                    raise _Stop(ZSTD_PAST_DESTINATION)
                if ofc >= 17:
                    self.note("offset_code_17_or_more")
                start = len(out) - off
                if start < block_start:
                    self.note("match_into_earlier_block")
                if off >= ml:
                    out += out[start:start + ml]
                else:
                    self.note("overlapping_match")
                    if off == 1 and ml > 64:
                        self.note("offset_1_match_over_64")
                    period = bytes(out[start:])
                    out += (period * (ml // off + 1))[:ml]
            if bs.pos != 0:
                raise _Stop(ZSTD_BAD_BITSTREAM)
        rest = len(lits) - lp
        if rest > self.dst_len - len(out):
            raise _Stop(ZSTD_PAST_DESTINATION)
        out += lits[lp:]


def zstd_frame_status(src, dst_len: int, trace: Optional[Set[str]] = None) -> Tuple[int, bytes]:
    """Decode one frame of exactly ``dst_len`` bytes -> (status, what was produced up to the failing check).  Every check comes in
    the order of the kernel's, so that the two name the same defect.  The content checksum is not verified and the window size is
    not enforced (module docstring).  ``trace``: a set that receives the names of the format's features the frame uses."""
    f = _Frame(src, int(dst_len), trace)
    try:
        f.run()
    except _Stop as stop:
        return stop.status, bytes(f.out)
    return ZSTD_OK, bytes(f.out)


def zstd_decode(src, dst_len: int) -> bytes:
    """one frame -> its ``dst_len`` bytes; ZstdError (a ValueError) naming the check that failed"""
    status, out = zstd_frame_status(src, dst_len)
    if status != ZSTD_OK:
        raise ZstdError(status)
    return out


_libzstd: Optional[ctypes.CDLL] = None
_libzstd_tried = False


def libzstd() -> Optional[ctypes.CDLL]:
    """the system's libzstd, or None"""
    global _libzstd, _libzstd_tried
    if not _libzstd_tried:
        _libzstd_tried = True
        name = ctypes.util.find_library("zstd")
        if name:
            try:
                L = ctypes.CDLL(name)
                L.ZSTD_decompress.restype = ctypes.c_size_t
                L.ZSTD_decompress.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
                L.ZSTD_compress.restype = ctypes.c_size_t
                L.ZSTD_compress.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
                L.ZSTD_compressBound.restype = ctypes.c_size_t
                L.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
                L.ZSTD_isError.restype = ctypes.c_uint
                L.ZSTD_isError.argtypes = [ctypes.c_size_t]
                L.ZSTD_versionString.restype = ctypes.c_char_p
                _libzstd = L
            except (OSError, AttributeError):
                _libzstd = None
    return _libzstd


def lib_decode(src: bytes, dst_len: int) -> bytes:
    """one frame through libzstd; ValueError where the library refuses it or the size differs"""
    L = libzstd()
    dst = ctypes.create_string_buffer(max(dst_len, 1))
    got = L.ZSTD_decompress(dst, dst_len, bytes(src), len(src))
    if L.ZSTD_isError(got) or got != dst_len:
        raise ValueError(f"Zstandard frame: ZSTD_decompress returned {got}, {dst_len} bytes expected")
    return dst.raw[:dst_len]


def lib_compress(data: bytes, level: int = 1) -> bytes:
    """one frame written by libzstd (tools and fixtures; the library must load)"""
    L = libzstd()
    cap = L.ZSTD_compressBound(len(data))
    buf = ctypes.create_string_buffer(cap)
    n = L.ZSTD_compress(buf, cap, bytes(data), len(data), level)
    if L.ZSTD_isError(n):
        raise ValueError("ZSTD_compress failed")
    return buf.raw[:n]


def frame_decoder() -> Callable[[bytes, int], bytes]:
    """what the host route decodes one frame with: libzstd where it loads, else the pure-Python decoder"""
    return lib_decode if libzstd() is not None else zstd_decode
