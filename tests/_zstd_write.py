"""A writer of Zstandard frames for the tests, after the published format (RFC 8878; libzstd is not needed): it emits exactly the
blocks, literals sections, Huffman weights, FSE tables, table modes and sequences it is given.

* `frame(blocks, ...)`: a frame of the blocks `raw_block` / `rle_block` / `compressed_block` describe; a compressed block is
  `Literals` (raw, RLE, Huffman-coded in 1 or 4 streams with direct or FSE-compressed weights, or treeless) plus sequences
  `(literal length, match length, offset value)` -- offset values 1-3 are the repeat codes, above that `offset + 3` -- under three
  `Table`s (predefined, RLE, FSE-compressed from given normalised counts, or repeat);
* `zstd_expand(blocks)`: what the blocks decode to, byte by byte from the sequences' meaning (no decoder of the package is involved);
* `features(frame_bytes, size)`: the format's features a frame uses (the names yogo_amd.zstd's decoder notes while it decodes);
* `hand_written()`: the frames of the cases the library did not produce;
* `corrupt_frame(defect)`: a valid frame with exactly one defect per status;
* `compress(data)`: a small compressor (greedy matches, predefined tables, Huffman-coded or raw literals) whose frames libzstd decodes.

The FSE decoding tables (yogo_amd.zstd.fse_build, which the encoder here walks backwards) and the code tables are the package's:
the decoders under test and this writer share an author; tests/golden/zstd_frames.npz holds frames written by libzstd itself."""
import heapq
import struct

from yogo_amd import zstd as Z

MAGIC = struct.pack("<I", Z.MAGIC)
CANARY = 0xA5


class Bits:
    """fields in the order the DECODER reads them"""

    def __init__(self):
        self.fields = []

    def add(self, value, k):
        assert 0 <= value < (1 << k) or k == 0 and value == 0, (value, k)
        self.fields.append((value, k))

    def forward(self) -> bytes:
        v = n = 0
        for value, k in self.fields:
            v |= value << n
            n += k
        return v.to_bytes((n + 7) // 8, "little")

    def backward(self, marker=True, slack=0) -> bytes:
        """the first field read lies just below the marker bit; slack: zero bits nobody reads below the last field"""
        v, n = 0, slack
        for value, k in reversed(self.fields):
            v |= value << n
            n += k
        if not marker:
            return v.to_bytes((n + 7) // 8, "little") + b"\0"
        v |= 1 << n
        return v.to_bytes((n + 8) // 8, "little")


def fse_description(freq, log) -> bytes:
    """normalised counts (-1: "less than one") that sum to 1 << log, as the format describes them; trailing zeros are not written"""
    assert sum(abs(f) for f in freq) == 1 << log
    b = Bits()
    b.add(log - 5, 4)
    remaining, s = 1 << log, 0
    while remaining > 0:
        p = freq[s]
        s += 1
        bits = (remaining + 1).bit_length()
        lower, threshold = (1 << (bits - 1)) - 1, (1 << bits) - 1 - (remaining + 1)
        val = p + 1
        if val < threshold:
            b.add(val, bits - 1)
        elif val <= lower:
            b.add(val, bits)
        else:
            b.add(val + threshold, bits)
        remaining -= abs(p)
        if p == 0:
            zeros = 0
            while remaining > 0 and s < len(freq) and freq[s] == 0:
                zeros += 1
                s += 1
            while zeros >= 3:
                b.add(3, 2)
                zeros -= 3
            b.add(zeros, 2)
    return b.forward()


def fse_states(table, symbols):
    """the states an FSE decoder walks through while it emits `symbols`, and the bits of each update: found backwards"""
    if not symbols:
        return [], []
    by_symbol = {}
    for st, sym in enumerate(table.symbol):
        by_symbol.setdefault(sym, []).append(st)
    states = [by_symbol[symbols[-1]][0]]
    updates = []
    for sym in reversed(symbols[:-1]):
        nxt = states[0]
        st = next(c for c in by_symbol[sym] if table.base[c] <= nxt < table.base[c] + (1 << table.nbits[c]))
        states.insert(0, st)
        updates.insert(0, (nxt - table.base[st], table.nbits[st]))
    return states, updates


class Table:
    """one of the three tables of a sequences section: mode "predefined", "rle" (symbol), "fse" (freq, log) or "repeat" (the Table kept)"""

    def __init__(self, mode, symbol=None, freq=None, log=None, kept=None):
        self.mode, self.symbol, self.freq, self.log, self.kept = mode, symbol, freq, log, kept

    def resolve(self, which):
        if self.mode == "predefined":
            return Z.fse_build({"ll": Z.LL_DEFAULT, "of": Z.OF_DEFAULT, "ml": Z.ML_DEFAULT}[which], 5 if which == "of" else 6)
        if self.mode == "rle":
            return Z.fse_rle(self.symbol)
        if self.mode == "fse":
            return Z.fse_build(self.freq, self.log)
        return self.kept.resolve(which)

    def header(self) -> bytes:
        if self.mode == "rle":
            return bytes([self.symbol])
        return fse_description(self.freq, self.log) if self.mode == "fse" else b""


PREDEFINED = Table("predefined")
MODE = {"predefined": 0, "rle": 1, "fse": 2, "repeat": 3}


def _code(value, bases):
    c = max(i for i, b in enumerate(bases) if b <= value)
    return c, value - bases[c]


def sequences_section(seqs, ll=PREDEFINED, of=PREDEFINED, ml=PREDEFINED, *, marker=True, slack=0, modes_or=0) -> bytes:
    """the sequences section of [(literal length, match length, offset value)]"""
    n = len(seqs)
    if n == 0:
        return b"\0"
    head = bytes([n]) if n < 128 else (bytes([128 + (n >> 8), n & 255]) if n < 0x7F00 else b"\xff" + struct.pack("<H", n - 0x7F00))
    head += bytes([(MODE[ll.mode] << 6) | (MODE[of.mode] << 4) | (MODE[ml.mode] << 2) | modes_or])
    head += ll.header() + of.header() + ml.header()
    codes = []
    for lit, mlen, ofv in seqs:
        llc, lle = _code(lit, Z.LL_BASE)
        mlc, mle = _code(mlen, Z.ML_BASE)
        ofc = ofv.bit_length() - 1
        codes.append((llc, lle, mlc, mle, ofc, ofv - (1 << ofc)))
    tl, to, tm = ll.resolve("ll"), of.resolve("of"), ml.resolve("ml")
    sl, ul = fse_states(tl, [c[0] for c in codes])
    so, uo = fse_states(to, [c[4] for c in codes])
    sm, um = fse_states(tm, [c[2] for c in codes])
    b = Bits()
    b.add(sl[0], tl.log)
    b.add(so[0], to.log)
    b.add(sm[0], tm.log)
    for i, (llc, lle, mlc, mle, ofc, ofe) in enumerate(codes):
        b.add(ofe, ofc)
        b.add(mle, Z.ML_BITS[mlc])
        b.add(lle, Z.LL_BITS[llc])
        if i != n - 1:
            b.add(*ul[i])
            b.add(*um[i])
            b.add(*uo[i])
    return head + b.backward(marker, slack)


def huffman_codes(weights):
    """weights of the symbols 0 .. n - 1, the last one included -> {symbol: (code, bits)} as the decoder's table lays them out"""
    total = sum(1 << (w - 1) for w in weights if w)
    log = total.bit_length() - 1
    assert total == 1 << log, "the weights do not fill a table"
    codes, at = {}, 0
    for w in range(1, log + 1):
        for s, ws in enumerate(weights):
            if ws == w:
                nb = log + 1 - w
                codes[s] = (at >> (log - nb), nb)
                at += 1 << (w - 1)
    return codes


def huffman_stream(data, codes) -> bytes:
    b = Bits()
    for s in data:
        b.add(*codes[s])
    return b.backward()


def huffman_description(weights, fse=None) -> bytes:
    """the tree description of `weights` (the last one is implied, not written).  fse: (freq, log) to write them FSE-compressed"""
    w = list(weights[:-1])
    if fse is None:
        assert len(w) <= 128
        w2 = w + [0]
        return bytes([127 + len(w)]) + bytes((w2[i] << 4) | w2[i + 1] for i in range(0, len(w), 2))
    freq, log = fse
    table = Z.fse_build(freq, log)
    assert len(w) >= 2
    s1, u1 = fse_states(table, w[0::2])
    s2, u2 = fse_states(table, w[1::2])
    b = Bits()
    b.add(s1[0], log)
    b.add(s2[0], log)
    for k in range(len(w) - 2):
        b.add(*(u1 if k % 2 == 0 else u2)[k // 2])
    last = (s1 if (len(w) - 2) % 2 == 0 else s2)[(len(w) - 2) // 2]
    assert table.nbits[last] > 0, "the decoder would not see the stream's end"
    body = fse_description(freq, log) + b.backward()
    assert len(body) < 128
    return bytes([len(body)]) + body


class Literals:
    """kind "raw", "rle", "huffman" (weights, streams 1 or 4, fse=(freq, log) for FSE-compressed weights) or "treeless" (the weights
    of the table kept, streams)"""

    def __init__(self, data, kind="raw", weights=None, streams=1, fse=None):
        self.data, self.kind, self.weights, self.streams, self.fse = bytes(data), kind, weights, streams, fse

    def section(self) -> bytes:
        n = len(self.data)
        if self.kind in ("raw", "rle"):
            t = 0 if self.kind == "raw" else 1
            body = self.data if t == 0 else self.data[:1]
            assert t == 0 or self.data == self.data[:1] * n
            if n < 32:
                return bytes([t | (n << 3)]) + body
            if n < 4096:
                return struct.pack("<H", t | (1 << 2) | (n << 4)) + body
            return struct.pack("<I", t | (3 << 2) | (n << 4))[:3] + body
        t = 2 if self.kind == "huffman" else 3
        codes = huffman_codes(self.weights)
        body = huffman_description(self.weights, self.fse) if t == 2 else b""
        if self.streams == 1:
            body += huffman_stream(self.data, codes)
        else:
            seg = (n + 3) // 4
            parts = [huffman_stream(self.data[i * seg:(i + 1) * seg], codes) for i in range(4)]
            body += struct.pack("<HHH", *(len(p) for p in parts[:3])) + b"".join(parts)
        c = len(body)
        if self.streams == 1:
            assert n < 1024 and c < 1024
            return struct.pack("<I", t | (n << 4) | (c << 14))[:3] + body
        if n < 1024 and c < 1024:
            return struct.pack("<I", t | (1 << 2) | (n << 4) | (c << 14))[:3] + body
        if n < 16384 and c < 16384:
            return struct.pack("<I", t | (2 << 2) | (n << 4) | (c << 18)) + body
        return struct.pack("<Q", t | (3 << 2) | (n << 4) | (c << 22))[:5] + body


def raw_block(data):
    return {"type": 0, "data": bytes(data)}


def rle_block(byte, count):
    return {"type": 1, "byte": byte, "count": count}


def compressed_block(literals, seqs=(), ll=PREDEFINED, of=PREDEFINED, ml=PREDEFINED, **kw):
    return {"type": 2, "literals": literals, "seqs": list(seqs), "tables": (ll, of, ml), "kw": kw}


def block_bytes(b, last) -> bytes:
    if b["type"] == 0:
        body, size = b["data"], len(b["data"])
    elif b["type"] == 1:
        body, size = bytes([b["byte"]]), b["count"]
    else:
        body = b["literals"].section() + sequences_section(b["seqs"], *b["tables"], **b["kw"])
        size = len(body)
    assert size <= Z.BLOCK_MAX
    return struct.pack("<I", (1 if last else 0) | (b.get("wire_type", b["type"]) << 1) | (size << 3))[:3] + body


def frame(blocks, *, size=None, single=True, checksum=False, fhd_or=0, dict_id=None, magic=MAGIC) -> bytes:
    """size None: no frame content size (a window descriptor instead)"""
    fhd = (0x04 if checksum else 0) | fhd_or
    out = bytearray(magic)
    if size is None:
        out += bytes([fhd, 0x78])    # window 1 << 25
    else:
        flag = 0 if size < 256 else 1 if size < 65536 + 256 else 2
        if not single and flag == 0:
            flag = 2
        out += bytes([fhd | (flag << 6) | (0x20 if single else 0)])
        if not single:
            out += bytes([0x78])
    if dict_id is not None:
        out += bytes([dict_id])
    if size is not None:
        out += bytes([size]) if flag == 0 else struct.pack("<H", size - 256) if flag == 1 else struct.pack("<I", size)
    for i, b in enumerate(blocks):
        out += block_bytes(b, i == len(blocks) - 1)
    if checksum:
        out += b"\xde\xad\xbe\xef"
    return bytes(out)


def zstd_expand(blocks) -> bytes:
    """what the blocks decode to, byte by byte from their meaning"""
    out = bytearray()
    rep = [1, 4, 8]
    for b in blocks:
        if b["type"] == 0:
            out += b["data"]
        elif b["type"] == 1:
            out += bytes([b["byte"]]) * b["count"]
        else:
            lits, lp = b["literals"].data, 0
            for lit, mlen, ofv in b["seqs"]:
                out += lits[lp:lp + lit]
                lp += lit
                if ofv > 3:
                    off = ofv - 3
                    rep = [off, rep[0], rep[1]]
                else:
                    idx = ofv - 1 + (lit == 0)
                    if idx == 0:
                        off = rep[0]
                    elif idx == 1:
                        off, rep = rep[1], [rep[1], rep[0], rep[2]]
                    elif idx == 2:
                        off, rep = rep[2], [rep[2], rep[0], rep[1]]
                    else:
                        off = rep[0] - 1
                        rep = [off, rep[0], rep[1]]
                assert 1 <= off <= len(out), (off, len(out))
                for _ in range(mlen):
                    out.append(out[-off])
            out += lits[lp:]
    return bytes(out)


def features(frame_bytes, size):
    """the names of the format's features a well-formed frame uses"""
    seen = set()
    status, _ = Z.zstd_frame_status(frame_bytes, size, seen)
    assert status == 0, status
    return seen


# ---- hand-written frames: what the library's frames do not hold

def _weights_for(nbits_of):
    """{symbol: code bits} of a complete prefix code -> the weights list up to the largest symbol"""
    log = max(nbits_of.values())
    w = [0] * (max(nbits_of) + 1)
    for s, nb in nbits_of.items():
        w[s] = log + 1 - nb
    return w


def hand_written():
    """name -> (frame, what it decodes to)"""
    out = {}

    def put(name, blocks, **kw):
        want = zstd_expand(blocks)
        out[name] = (frame(blocks, size=len(want), **kw), want)

    text = b"abcdefghijklmnopqrstuvwxyz0123456789"
    # RLE literals; an offset-1 match longer than 64; the repeat codes with a literal length above 0
    put("rle_literals", [compressed_block(Literals(b"Q" * 40, "rle"), [(10, 100, 1 + 3), (10, 5, 7 + 3), (5, 4, 20 + 3), (3, 6, 1), (2, 5, 2), (4, 7, 3), (1, 9, 3)])])
    # the repeat codes with a literal length of 0: 1 -> second, 2 -> third, 3 -> first minus 1
    put("repeat_ll0", [compressed_block(Literals(text), [(20, 4, 5 + 3), (4, 4, 9 + 3), (2, 5, 16 + 3), (0, 6, 1), (0, 4, 2), (0, 5, 3), (3, 3, 1)])],
        single=False)
    # RLE-mode tables (every sequence the same codes), then repeat mode keeps them; a content checksum
    rl, ro, rm = Table("rle", symbol=4), Table("rle", symbol=3), Table("rle", symbol=5)
    put("rle_tables", [raw_block(b"0123456789"), compressed_block(Literals(text), [(4, 8, 8 + 1), (4, 8, 8 + 3), (4, 8, 8 + 6)], rl, ro, rm),
                       compressed_block(Literals(text[:12]), [(4, 8, 8 + 2), (4, 8, 8 + 0)], Table("repeat", kept=rl), Table("repeat", kept=ro),
                                        Table("repeat", kept=rm))], checksum=True)
    # FSE tables at the accuracy limits 9 / 8 / 9 with "less than one" counts
    fl = [200, 100, 100, 50, 30, 20, -1, -1, -1, -1, 8]
    fo = [100, 60, 40, 30, 10, 8, 4, -1, -1, -1, -1]
    fm = [256, 128, 64, 32, 16, 8, 4, -1, -1, -1, -1]
    seqs = [(i % 6, 3 + (i * 5) % 7, (1 << (2 + i % 5)) + i % 3) for i in range(40)]
    seqs = [(6, 4, 4 + 3)] + seqs
    lit = bytes((i * 37 + 11) & 255 for i in range(sum(s[0] for s in seqs) + 9))
    put("fse_at_limits", [raw_block(bytes(range(100))), compressed_block(Literals(lit), seqs, Table("fse", freq=fl, log=9), Table("fse", freq=fo, log=8), Table("fse", freq=fm, log=9))])
    # a maximal 11-bit Huffman code, direct weights, 1 stream: code lengths 1, 2, ..., 10, 11, 11
    lens = {s: min(s + 1, 11) for s in range(12)}
    w11 = _weights_for(lens)
    data = bytes([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 11, 10, 0, 0, 3] * 9)
    put("huffman_11_bits", [compressed_block(Literals(data, "huffman", weights=w11, streams=1))])
    # FSE-compressed weights at the accuracy limit 6 with a "less than one" count, 4 streams, then a treeless block
    lens = {s: 3 for s in range(6)}
    lens.update({200: 3, 255: 3})    # the last symbol above 128: direct weights could not say it
    wf = _weights_for(lens)          # weights 1 at eight symbols, 0 elsewhere
    freq = [32, 31, -1]              # weights 0 and 1 (no count above half the table: every state reads a bit); weight 2 never occurs
    data = bytes([0, 1, 2, 3, 4, 5, 200, 255] * 30 + [255, 200, 0])
    put("huffman_fse_weights_limit", [compressed_block(Literals(data, "huffman", weights=wf, streams=4, fse=(freq, 6))),
                                      compressed_block(Literals(data[:50], "treeless", weights=wf, streams=1), [(10, 30, 243 + 3)])])
    # a match that spans a 128 KB block boundary: it starts in the first block's bytes and is copied in the second; offset code 17
    first = bytes((i * 7 + (i >> 8)) & 255 for i in range(1 << 17))
    put("match_over_block_boundary", [raw_block(first), compressed_block(Literals(b"xyz"), [(3, 300, (1 << 17) + 3 + 3), (0, 200, 1 + 3)])])
    # RLE and raw blocks in one frame, a last block that is empty
    put("block_kinds", [rle_block(0x33, 1000), raw_block(b"between"), rle_block(0x44, 70), raw_block(b"")])
    return out


# ---- one defect per status

def _good(size_known=True):
    blocks = [compressed_block(Literals(b"0123456789abcdefXYZthe end..", "raw"), [(16, 40, 16 + 3), (3, 12, 5 + 3)])]
    want = zstd_expand(blocks)
    return blocks, want, frame(blocks, size=len(want) if size_known else None)


def _frame_of_body(body, size) -> bytes:
    """a frame of one compressed block with the given bytes"""
    return frame([], size=size) + struct.pack("<I", 1 | (2 << 1) | (len(body) << 3))[:3] + body


DEFECTS = ["truncated", "magic", "skippable", "reserved_bit", "dictionary", "content_size", "block_type3", "treeless_first", "literals_size",
           "huffman_weights", "fse_log", "repeat_first", "rle_symbol", "no_marker", "bits_left", "huffman_overrun", "mode_reserved", "literals_short",
           "after_zero_sequences", "offset0", "offset_far", "match_past_dst", "early", "trailing", "two_frames", "header_only"]


def corrupt_frame(defect):
    """(frame, dst_len, expected status, the truth its output must be a prefix of)"""
    blocks, want, good = _good()
    lit = blocks[0]["literals"]
    n = len(want)
    if defect == "truncated":
        return good[:-3], n, Z.ZSTD_SOURCE_ENDS, want
    if defect == "header_only":
        return good[:5], n, Z.ZSTD_SOURCE_ENDS, want
    if defect == "magic":
        return b"\x29" + good[1:], n, Z.ZSTD_BAD_MAGIC, want
    if defect == "skippable":
        return struct.pack("<II", 0x184D2A50, 4) + b"skip" + good, n, Z.ZSTD_BAD_MAGIC, want
    if defect == "reserved_bit":
        return frame(blocks, size=n, fhd_or=0x08), n, Z.ZSTD_UNSUPPORTED_HEADER, want
    if defect == "dictionary":
        return frame(blocks, size=n, fhd_or=0x01, dict_id=7), n, Z.ZSTD_UNSUPPORTED_HEADER, want
    if defect == "content_size":
        return frame(blocks, size=n + 1), n, Z.ZSTD_CONTENT_SIZE, want
    if defect == "block_type3":
        return frame([dict(blocks[0], wire_type=3)], size=n), n, Z.ZSTD_BAD_BLOCK, want
    if defect == "treeless_first":
        b = compressed_block(Literals(bytes([0, 1, 0, 1]), "treeless", weights=[1, 1], streams=1))
        return frame([b], size=4), 4, Z.ZSTD_BAD_LITERALS, b""
    if defect == "literals_size":     # four streams whose three sizes pass the section
        sec = Literals(bytes([0, 1] * 40), "huffman", weights=[1, 1], streams=4).section()
        at = 3 + 2    # behind the section header and the tree description
        return _frame_of_body(sec[:at] + struct.pack("<H", 500) + sec[at + 2:] + b"\0", 80), 80, Z.ZSTD_BAD_LITERALS, b""
    if defect == "huffman_weights":   # weights 3, 1 and an implied one: 5 of 8 slots are taken, and 3 is no power of two
        sec = Literals(bytes([0, 1] * 8), "huffman", weights=[1, 1], streams=1).section()
        assert sec[3:5] == bytes([128, 0x10])
        return _frame_of_body(sec[:3] + bytes([129, 0x31]) + sec[5:] + b"\0", 16), 16, Z.ZSTD_BAD_HUFFMAN, b""
    if defect in ("fse_log", "repeat_first", "rle_symbol"):
        t = {"fse_log": Table("fse", freq=[32], log=5), "repeat_first": Table("repeat", kept=PREDEFINED), "rle_symbol": Table("rle", symbol=2)}[defect]
        if defect == "fse_log":
            t.header = lambda: b"\x0f\xff"          # accuracy log 20
        if defect == "rle_symbol":
            t.header = lambda: bytes([36])          # literal-length code 36
            b = compressed_block(lit, [(2, 40, 16 + 3), (2, 12, 5 + 3)], ll=t)
        else:
            b = compressed_block(lit, blocks[0]["seqs"], of=t) if defect == "repeat_first" else compressed_block(lit, blocks[0]["seqs"], ll=_FakeFse(t))
        return frame([b], size=n), n, Z.ZSTD_BAD_FSE_TABLE, want
    if defect == "no_marker":
        return frame([compressed_block(lit, blocks[0]["seqs"], marker=False)], size=n), n, Z.ZSTD_BAD_BITSTREAM, want
    if defect == "bits_left":
        return frame([compressed_block(lit, blocks[0]["seqs"], slack=8)], size=n), n, Z.ZSTD_BAD_BITSTREAM, want
    if defect == "huffman_overrun":   # a Huffman stream one symbol short of its count
        sec = Literals(bytes([0, 1] * 8), "huffman", weights=[1, 1], streams=1).section()
        v = struct.unpack("<I", sec[:3] + b"\0")[0] + (1 << 4)     # regenerated size 17
        return _frame_of_body(struct.pack("<I", v)[:3] + sec[3:] + b"\0", 17), 17, Z.ZSTD_BAD_BITSTREAM, b""
    if defect == "mode_reserved":
        return frame([compressed_block(lit, blocks[0]["seqs"], modes_or=1)], size=n), n, Z.ZSTD_BAD_SEQUENCES, want
    if defect == "literals_short":
        return frame([compressed_block(lit, [(16, 40, 16 + 3), (13, 12, 5 + 3)])], size=n), n, Z.ZSTD_BAD_SEQUENCES, want
    if defect == "after_zero_sequences":
        return _frame_of_body(lit.section() + b"\0\0", len(lit.data)), len(lit.data), Z.ZSTD_BAD_SEQUENCES, b""
    if defect == "offset0":           # repeat code 3 with a literal length of 0 at the frame's start: first repeat offset 1, minus 1
        return frame([compressed_block(lit, [(0, 5, 3)])], size=n), n, Z.ZSTD_BAD_OFFSET, b""
    if defect == "offset_far":
        return frame([compressed_block(lit, [(16, 40, 17 + 3), (3, 12, 5 + 3)])], size=n), n, Z.ZSTD_BAD_OFFSET, want
    if defect == "match_past_dst":
        return _good(False)[2], n - 10, Z.ZSTD_PAST_DESTINATION, want
    if defect == "early":
        return _good(False)[2], n + 1, Z.ZSTD_ENDS_EARLY, want
    if defect == "trailing":
        return good + b"\0", n, Z.ZSTD_TRAILING, want
    if defect == "two_frames":
        return good + good, n, Z.ZSTD_TRAILING, want
    raise KeyError(defect)


class _FakeFse(Table):
    """a table whose description is the given one's and whose states are the predefined ones (the description is refused first)"""

    def __init__(self, t):
        super().__init__("fse")
        self._t = t

    def header(self):
        return self._t.header()

    def resolve(self, which):
        return PREDEFINED.resolve(which)


# ---- a small compressor

def _huffman_lengths(counts):
    heap = [(c, i, (s,)) for i, (s, c) in enumerate(sorted(counts.items()))]
    heapq.heapify(heap)
    lens = {s: 0 for s in counts}
    tie = len(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            lens[s] += 1
        heapq.heappush(heap, (a[0] + b[0], tie, a[2] + b[2]))
        tie += 1
    return lens


def _literals(data) -> Literals:
    counts = {}
    for x in data:
        counts[x] = counts.get(x, 0) + 1
    if len(data) >= 64 and len(counts) >= 2 and max(counts) <= 128:
        lens = _huffman_lengths(counts)
        if max(lens.values()) <= Z.HUF_MAX_BITS:
            lit = Literals(data, "huffman", weights=_weights_for(lens), streams=1 if len(data) < 1000 else 4)
            if len(lit.section()) < len(data):
                return lit
    return Literals(data)


def compress(data) -> bytes:
    """greedy: the most recent earlier occurrence of the next 4 bytes, extended as far as it goes; blocks of at most 64 KB of input"""
    data = bytes(data)
    blocks = []
    table = {}
    for lo in range(0, max(len(data), 1), 1 << 16):
        hi = min(lo + (1 << 16), len(data))
        seqs, lits, anchor, i = [], bytearray(), lo, lo
        while i + 4 <= hi:
            key = data[i:i + 4]
            cand = table.get(key)
            table[key] = i
            if cand is None:
                i += 1
                continue
            ml = 4
            while i + ml < hi and data[cand + ml] == data[i + ml] and ml < 60000:
                ml += 1
            seqs.append((i - anchor, ml, i - cand + 3))
            lits += data[anchor:i]
            i += ml
            anchor = i
        lits += data[anchor:hi]
        b = compressed_block(_literals(bytes(lits)), seqs)
        body = block_bytes(b, False)
        blocks.append(b if len(body) - 3 < hi - lo else raw_block(data[lo:hi]))
    return frame(blocks, size=len(data))


def golden_frames():
    """name -> (frame written by libzstd, what it decodes to) from tests/golden/zstd_frames.npz"""
    import os

    import numpy as np

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zstd_frames.npz"))
    return {k[:-2]: (z[k].tobytes(), z[k[:-2] + "_d"].tobytes()) for k in z.files if k.endswith("_c") and k[:-2] + "_d" in z.files}


def decode_on_device(entries, extra_rows=()):
    """One yogo_zstd_decode launch over `entries` = [(stored bytes, dst_len, raw)].  Sources and destinations are packed at offsets
    of every alignment with gaps between them; the destination and the workspace start out as CANARY bytes.  extra_rows: table rows
    appended as they are (rows that do not lie inside the buffers; None stands for the buffer's size).
    -> (status list, what each entry's destination range holds, True when every destination byte outside the ranges is still CANARY,
    True when every workspace byte beyond the rows' 128 KB each is still CANARY)"""
    import numpy as np
    import torch

    from yogo_amd.device_decode import zstd_frames, zstd_work_bytes

    rows, src, dpos = [], bytearray(), 16
    for i, (data, dst_len, raw) in enumerate(entries):
        pad = (5 * i + 3) % 16 if i % 4 else (16 - len(src) % 16) % 16    # every fourth source starts on a multiple of 16
        src += bytes([0x5A]) * pad
        soff = len(src)
        src += data
        doff = dpos + ((7 * i + 1) % 16 if i % 3 else 0)                   # every third destination likewise
        rows.append((soff, len(data), doff, dst_len, 1 if raw else 0))
        dpos = -(-(doff + dst_len + 16) // 16) * 16
    src += bytes([0x5A]) * 16
    total = dpos + 16
    n_inside = len(rows)
    for r in extra_rows:
        rows.append(tuple({"src": len(src), "dst": total}.get(v, v) for v in r))
    need = zstd_work_bytes(len(rows))
    dst = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    work = torch.full((need + 4096,), CANARY, dtype=torch.uint8, device="cuda")
    status = torch.full((len(rows),), -1, dtype=torch.int32, device="cuda")
    zstd_frames(torch.frombuffer(src, dtype=torch.uint8).cuda(), torch.tensor(rows, dtype=torch.int64).reshape(-1, 5).cuda(), dst, status, work)
    host = dst.cpu().numpy()
    outside = np.ones(host.size, dtype=bool)
    got = []
    for _, _, doff, dst_len, _ in rows[:n_inside]:
        outside[doff:doff + dst_len] = False
        got.append(host[doff:doff + dst_len].tobytes())
    return status.cpu().tolist(), got, bool((host[outside] == CANARY).all()), bool((work[need:] == CANARY).all())


# ---- zarr stores of Zstandard frames (the host and the feed tests)

BLOSC_ZSTD_DOC = {"id": "blosc", "cname": "zstd", "clevel": 5, "shuffle": 1, "blocksize": 0}
ZSTD_DOC = {"id": "zstd", "level": 1}
FLAGS_ZSTD = 0x01 | (4 << 5)      # byte-shuffle (a no-op at typesize 1), inner format zstd


def store_stack():
    """[48, 64, 8]: the golden stack's six frames, one of noise (no codec shrinks it: raw blocks) and one of four values"""
    import os

    import numpy as np

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zstd_frames.npz"))
    rng = np.random.default_rng(5)
    extra = [rng.integers(0, 256, (48, 64), dtype=np.uint8), rng.integers(0, 4, (48, 64), dtype=np.uint8) * 70]
    return np.concatenate([z["stack_d"], np.stack(extra, axis=2)], axis=2)


def library_encoder():
    """bytes -> one frame: libzstd's own frame where the golden file holds one for exactly these bytes (the six frames of the golden
    stack, whole and in blocks of 1 000 bytes), else this module's compressor"""
    import os

    import numpy as np

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zstd_frames.npz"))
    known = {}
    for name, pieces in (("stack_chunks", [z["stack_d"][:, :, i].tobytes() for i in range(6)]),
                         ("stack_blocks", [z["stack_d"][:, :, i].tobytes()[at:at + 1000] for i in range(6) for at in range(0, 3072, 1000)])):
        blob, at = z[name + "_c"].tobytes(), 0
        for raw, n in zip(pieces, z[name + "_n"].tolist()):
            known[raw] = blob[at:at + n]
            at += n
    used = {"library": 0, "writer": 0}

    def encode(raw):
        raw = bytes(raw)
        used["library" if raw in known else "writer"] += 1
        return known[raw] if raw in known else compress(raw)

    encode.used = used
    return encode


def zstd_members(a, chunks, kind, *, encode, blocksize=1000, memcpyed=(), replace=None, prefix="", **kw):
    """{key: bytes} of one array under Blosc-zstd (kind "blosc-zstd": one frame per block of `blocksize`, a block stored raw when
    its frame is no shorter, the keys in `memcpyed` as memcpyed chunks) or under the zstd codec (kind "zstd": one frame per chunk).
    replace: {key: f(stored bytes) -> stored bytes}"""
    import _blosc_write as BW
    import _zarr_write as ZW

    doc = dict(BLOSC_ZSTD_DOC if kind == "blosc-zstd" else ZSTD_DOC)
    members = ZW.array_members(a, chunks, compressor=doc, prefix=prefix, **kw)
    out = {}
    for k, v in members.items():
        if k.endswith(".zarray"):
            out[k] = v
            continue
        enc = BW.blosc_frame(v, blocksize, flags=FLAGS_ZSTD, compress=encode, memcpyed=k in memcpyed) if kind == "blosc-zstd" else encode(v)
        out[k] = replace[k](enc) if replace and k in replace else enc
    return out


def zstd_group_members(frames, chunks, kind, **kw):
    import json

    members = {".zgroup": json.dumps({"zarr_format": 2}).encode()}
    for i, f in enumerate(frames):
        members.update(zstd_members(f, chunks, kind, prefix=f"{i}/", **kw))
    return members
