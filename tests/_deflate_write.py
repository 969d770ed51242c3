"""Writers for the DEFLATE tests, after RFC 1951 / RFC 1950 (nothing but the standard library):
* `Bits` writes bit fields LSB first and Huffman codes MSB first; `stored`, `fixed` and `dynamic` emit exactly the block they are
  given -- tokens, code lengths, the code-length symbols of a dynamic header, its three counts -- so that a test builds every
  shape of the format, and every defect, by hand;
* `expand` is what a token list means, byte by byte (no decoder of the package is involved);
* `describe` lists what a well-formed stream holds, for the tests to assert that a case contains what it is named after;
* `zlib_wrap` puts the two-byte header and the Adler-32 trailer round a raw stream;
* `CASES` / `DEFECTS`: the hand-built streams the host and the device tests share.

The decoders under test (yogo_amd/inflate.py, csrc/inflate.hip) and these writers share an author; zlib itself is the reference
the tests hold both to."""
import struct
import zlib

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def bits(self, value, n):
        assert 0 <= value < (1 << n)
        self.acc |= value << self.n
        self.n += n

    def code(self, code, length):
        """a Huffman code: its most significant bit first"""
        for k in range(length - 1, -1, -1):
            self.bits((code >> k) & 1, 1)

    def align(self):
        self.n = -(-self.n // 8) * 8

    def raw(self, data):
        assert self.n % 8 == 0
        self.acc |= int.from_bytes(data, "little") << self.n
        self.n += 8 * len(data)

    def bytes(self):
        return self.acc.to_bytes(-(-self.n // 8), "little")


def canonical(lens):
    """{symbol: (code, length)} of the canonical code with these lengths (RFC 1951 3.2.2; it need not be complete)"""
    out, code = {}, 0
    for l in range(1, 16):
        for s, sl in enumerate(lens):
            if sl == l:
                out[s] = (code, l)
                code += 1
        code <<= 1
    return out


def complete_lens(k):
    """lengths of a complete code over k >= 2 symbols: 2^m - k of length m - 1, the rest of length m"""
    assert k >= 2
    m = (k - 1).bit_length()
    short = (1 << m) - k
    return [m - 1] * short + [m] * (k - short)


def spread(symbols, size, lens=None):
    """a length list of `size` entries that gives `symbols` (in this order) the lengths `lens` (default: a complete code)"""
    symbols = list(symbols)
    lens = lens or complete_lens(len(symbols))
    out = [0] * size
    for s, l in zip(symbols, lens):
        out[s] = l
    return out


def len_symbol(n):
    s = max(i for i, b in enumerate(LEN_BASE) if b <= n) if n < 258 else 28
    return 257 + s, LEN_EXTRA[s], n - LEN_BASE[s]


def dist_symbol(d):
    s = max(i for i, b in enumerate(DIST_BASE) if b <= d)
    return s, DIST_EXTRA[s], d - DIST_BASE[s]


def stored(w, data, final=False, nlen=None):
    w.bits(1 if final else 0, 1)
    w.bits(0, 2)
    w.align()
    w.bits(len(data), 16)
    w.bits((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
    w.raw(data)


def _tokens(w, tokens, lit_lens, dist_lens, end=True):
    """tokens: an int is a literal, (length, distance) a match, ("sym", s) a bare literal / length symbol,
    ("dsym", length, d, extra) a match whose distance code and extra bits are given"""
    lc, dc = canonical(lit_lens), canonical(dist_lens)
    for t in tokens:
        if isinstance(t, int):
            w.code(*lc[t])
        elif t[0] == "sym":
            w.code(*lc[t[1]])
        else:
            ln = t[1] if t[0] == "dsym" else t[0]
            s, eb, ev = len_symbol(ln)
            w.code(*lc[s])
            w.bits(ev, eb)
            if t[0] == "dsym":
                w.code(*dc[t[2]])
                w.bits(t[3], DIST_EXTRA[t[2]] if t[2] < 30 else 0)
            else:
                s, eb, ev = dist_symbol(t[1])
                w.code(*dc[s])
                w.bits(ev, eb)
    if end:
        w.code(*lc[256])


def fixed(w, tokens, final=False, end=True):
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    _tokens(w, tokens, FIXED_LIT, FIXED_DIST, end)


def plain_ops(lens):
    return [(l, None) for l in lens]


def dynamic(w, tokens, lit_lens, dist_lens, final=False, ops=None, cl_lens=None, nc=None, nl=None, nd=None, end=True):
    """a dynamic block.  ops: the code-length symbols of the header, [(symbol 0..18, value of its extra bits or None)] (default:
    every length plain); cl_lens: the 19 lengths of the code-length code (default: a complete code over the symbols in use);
    nc / nl / nd: the three counts as announced (default: what the lists hold)."""
    ops = plain_ops(list(lit_lens) + list(dist_lens)) if ops is None else ops
    if cl_lens is None:
        used = sorted({s for s, _ in ops})
        if len(used) == 1:
            used.append(used[0] ^ 1)
        cl_lens = spread(used, 19)
    if nc is None:
        nc = max(4, max(k + 1 for k in range(19) if cl_lens[CL_ORDER[k]]))
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits((len(lit_lens) if nl is None else nl) - 257, 5)
    w.bits((len(dist_lens) if nd is None else nd) - 1, 5)
    w.bits(nc - 4, 4)
    for k in range(nc):
        w.bits(cl_lens[CL_ORDER[k]], 3)
    cc = canonical(cl_lens)
    for s, extra in ops:
        w.code(*cc[s])
        if s >= 16:
            w.bits(extra, {16: 2, 17: 3, 18: 7}[s])
    if tokens is not None:
        _tokens(w, tokens, lit_lens, dist_lens, end)


def expand(tokens):
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            ln, d = t
            assert 1 <= d <= len(out)
            for _ in range(ln):
                out.append(out[-d])
    return bytes(out)


def zlib_wrap(raw, data):
    return b"\x78\x9c" + raw + struct.pack(">I", zlib.adler32(data))


def describe(raw):
    """the blocks of a well-formed raw stream: [{"type", "final", "stored" (bytes of a stored block), "nc", "nl", "nd", "ops"
    ([(code-length symbol, repeat count or None)]), "lit_lens", "dist_lens", "tokens" ([literal | (length, distance)])}]"""
    padded, pos = bytes(raw) + bytes(4), 0

    def take(n):
        nonlocal pos
        v = (int.from_bytes(padded[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << n) - 1)
        pos += n
        return v

    def table(lens):
        return {(c, l): s for s, (c, l) in canonical(lens).items()}

    def sym(codes):
        code = 0
        for l in range(1, 16):
            code = (code << 1) | take(1)
            if (code, l) in codes:
                return codes[(code, l)]
        raise ValueError("no code")

    blocks = []
    while True:
        b = {"final": take(1), "type": take(2)}
        blocks.append(b)
        if b["type"] == 0:
            pos = -(-pos // 8) * 8
            n = take(16)
            assert take(16) == n ^ 0xFFFF
            b["stored"] = raw[pos // 8:pos // 8 + n]
            pos += 8 * n
        else:
            if b["type"] == 1:
                lit_lens, dist_lens = FIXED_LIT, FIXED_DIST
            else:
                b["nl"], b["nd"], b["nc"] = take(5) + 257, take(5) + 1, take(4) + 4
                cl = [0] * 19
                for k in range(b["nc"]):
                    cl[CL_ORDER[k]] = take(3)
                lens, ops, clc = [], [], table(cl)
                while len(lens) < b["nl"] + b["nd"]:
                    s = sym(clc)
                    if s < 16:
                        ops.append((s, None))
                        lens.append(s)
                    else:
                        rep = {16: 3, 17: 3, 18: 11}[s] + take({16: 2, 17: 3, 18: 7}[s])
                        ops.append((s, rep))
                        lens += [lens[-1] if s == 16 else 0] * rep
                b["ops"], b["cl_lens"] = ops, cl
                lit_lens, dist_lens = lens[:b["nl"]], lens[b["nl"]:]
            b["lit_lens"], b["dist_lens"], b["tokens"] = lit_lens, dist_lens, []
            lc, dc = table(lit_lens), table(dist_lens)
            while True:
                s = sym(lc)
                if s == 256:
                    break
                if s < 256:
                    b["tokens"].append(s)
                    continue
                ln = LEN_BASE[s - 257] + take(LEN_EXTRA[s - 257])
                d = sym(dc)
                b["tokens"].append((ln, DIST_BASE[d] + take(DIST_EXTRA[d])))
        if b["final"]:
            return blocks


def matches(blocks):
    return [t for b in blocks for t in b.get("tokens", ()) if not isinstance(t, int)]


# ---- the hand-built streams: name -> (raw stream, what it inflates to) -----------------------------------------------------------

def _one(build):
    w = Bits()
    data = build(w)
    return w.bytes(), data


def _fixed_case(tokens):
    def build(w):
        fixed(w, tokens, final=True)
        return expand(tokens)
    return _one(build)


def _dynamic_case(tokens, lit_lens, dist_lens, **kw):
    def build(w):
        dynamic(w, tokens, lit_lens, dist_lens, final=True, **kw)
        return expand(tokens)
    return _one(build)


def _lit_lens_15():
    """literals 0..14 and the end-of-block code with lengths 1, 2, ..., 14, 15, 15: a complete code with two 15-bit codes"""
    return spread(list(range(14)) + [14, 256], 257, list(range(1, 15)) + [15, 15])


def _repeat_ops():
    """257 literal / length lengths and one distance length, written with each repeat code at its minimum and its maximum count:
    8 | 16 x3 | 16 x6 | 17 x3 | 17 x10 | 18 x11 | 18 x138, then plain lengths that complete the code (10 + 24 codes of length 8,
    11 of length 7, 50 of length 6: 34 + 22 + 200 = 256 / 256)"""
    ops = [(8, None), (16, 0), (16, 3), (17, 0), (17, 7), (18, 0), (18, 127)]
    lens = [8] * 10 + [0] * (3 + 10 + 11 + 138) + [8] * 24 + [7] * 11 + [6] * 50 + [0]
    assert len(lens) == 258
    return ops + plain_ops(lens[172:]), lens[:257], lens[257:]


def _fill(tokens, total, dist):
    """`tokens` plus matches at `dist` (and literals at the very end) that bring the output to exactly `total` bytes"""
    tokens = list(tokens)
    have = len(expand(tokens))
    while total - have >= 3:
        ln = min(258, total - have)
        tokens.append((ln, dist))
        have += ln
    return tokens + [1] * (total - have)


def _cross_case():
    """266 literal / length lengths whose last eight are zero and four distance lengths 0 0 0 1: one code 18 (eleven zeros) runs
    from the first set into the second"""
    lit = spread([65, 66, 256, 257], 266, [2, 2, 2, 2])
    dist = [0, 0, 0, 1]
    tokens = [65, 66, 66, 65, (3, 4)]
    return _dynamic_case(tokens, lit, dist, ops=plain_ops(lit[:258]) + [(18, 0), (1, None)])


def _cases():
    c = {}
    big = bytes((i * 7 + 3) & 0xFF for i in range(65535))
    c["stored-len0"] = _one(lambda w: (stored(w, b"", final=True), b"")[1])
    c["stored-len65535"] = _one(lambda w: (stored(w, big, final=True), big)[1])
    c["stored-two"] = _one(lambda w: (stored(w, b"first,"), stored(w, b" second", final=True), b"first, second")[2])
    c["stored-sync-flush"] = _one(lambda w: (fixed(w, [65, 66]), stored(w, b""), fixed(w, [67], final=True), b"ABC")[3])
    head = list(b"0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ+-*")   # 65 literals
    c["fixed-len3"] = _fixed_case(head + [(3, 10)])
    c["fixed-len258"] = _fixed_case(head + [(258, 65)])
    for ln in (3, 64, 65, 258):      # the periodic copy at its shortest period (a match is at least 3 bytes long)
        c[f"fixed-dist1-len{ln}"] = _fixed_case([90, (ln, 1)])
    for d in (63, 64, 65):
        c[f"fixed-dist{d}"] = _fixed_case(head[:d] + [(100, d), (40, d)])
    far = [(i * 11 + (i >> 8)) & 0xFF for i in range(300)]
    c["fixed-dist32768"] = _fixed_case(_fill(far, 32768, 300) + [(200, 32768), 7, (258, 32768)])
    c["dynamic-hclen5"] = _dynamic_case(list(range(1, 40)), spread(range(1, 257), 257, [8] * 256), [0])
    c["dynamic-hclen19-15bit"] = _dynamic_case([0, 1, 13, 14, 14, 2, 14], _lit_lens_15(), [0])
    ops, ll, dl = _repeat_ops()
    c["dynamic-repeats"] = _dynamic_case([0, 9, 200, 255, 9], ll, dl, ops=ops)
    c["dynamic-repeat-crosses"] = _cross_case()
    c["dynamic-one-distance"] = _dynamic_case([7, 7, 7, (20, 1), 8, (5, 1)], spread([7, 8, 256, 257 + 2, 257 + 12], 270), [1])
    c["dynamic-no-distance"] = _dynamic_case([5, 6, 5, 5], spread([5, 6, 256], 257), [0])
    # tokens of every width, so that they straddle the edges of the decoder's source window wherever it is refilled: literals of
    # 8 and 9 bits and matches with 0 to 13 extra bits, 2 000 of them
    mix, n = list(range(256)), 256
    for i in range(2000):
        if i % 3 == 0 and n > 40:
            d = (1, 5, 97, 1000, 9000, 30000)[i // 3 % 6]
            t = (3 + i % 256, min(d, n))
        else:
            t = (i * 37) & 0xFF
        mix.append(t)
        n += 1 if isinstance(t, int) else t[0]
    c["fixed-mixed-tokens"] = _fixed_case(mix)
    return c


def _defects():
    """name -> (raw stream, dst_len, the status inflate_status must give: an INF_* name).  Where the status is about dst_len
    (past the destination, ends early) the stream itself is well formed."""
    d = {}
    good = [72, 101, 108, 108, 111, 32, (8, 3), 33, 10]
    data = expand(good)

    def one(name, status, build, dst_len=len(data)):
        w = Bits()
        build(w)
        d[name] = (w.bytes(), dst_len, status)

    one("block-type-3", "INF_BAD_BLOCK_TYPE", lambda w: (fixed(w, good[:3], end=True), w.bits(1, 1), w.bits(3, 2), w.bits(0, 8)))
    one("stored-nlen", "INF_STORED_LEN", lambda w: stored(w, data, final=True, nlen=0x1234))
    d["stored-cut"] = (d_cut(lambda w: stored(w, data, final=True), 5), len(data), "INF_SOURCE_ENDS")
    d["stored-header-cut"] = (d_cut(lambda w: stored(w, data, final=True), len(data) + 2), len(data), "INF_SOURCE_ENDS")
    d["fixed-cut-in-code"] = (d_cut(lambda w: fixed(w, good, final=True), 6), len(data), "INF_SOURCE_ENDS")
    d["empty-source"] = (b"", 0, "INF_SOURCE_ENDS")
    one("symbol-286", "INF_BAD_SYMBOL", lambda w: fixed(w, good[:6] + [("sym", 286)], final=True))
    one("symbol-287", "INF_BAD_SYMBOL", lambda w: fixed(w, good[:6] + [("sym", 287)], final=True))
    one("distance-code-30", "INF_BAD_SYMBOL", lambda w: fixed(w, good[:6] + [("dsym", 8, 30, 0)], final=True))
    one("distance-code-31", "INF_BAD_SYMBOL", lambda w: fixed(w, good[:6] + [("dsym", 8, 31, 0)], final=True))
    one("distance-too-far", "INF_BAD_DISTANCE", lambda w: fixed(w, good[:6] + [(8, 7)], final=True))
    one("match-past-dst", "INF_PAST_DESTINATION", lambda w: fixed(w, good, final=True), dst_len=len(data) - 4)
    one("literal-past-dst", "INF_PAST_DESTINATION", lambda w: fixed(w, good, final=True), dst_len=len(data) - 1)
    one("stored-past-dst", "INF_PAST_DESTINATION", lambda w: stored(w, data, final=True), dst_len=len(data) - 1)
    one("ends-early", "INF_ENDS_EARLY", lambda w: fixed(w, good, final=True), dst_len=len(data) + 1)
    lit3 = spread([65, 66, 256], 257)
    one("hclen4", "INF_BAD_LENGTHS",     # four code-length codes reach 16, 17, 18 and 0 alone: every length is zero, no end-of-block code
        lambda w: dynamic(w, None, [0] * 257, [0], final=True, ops=[(18, 127), (18, 109)], cl_lens=spread([18, 0], 19), nc=4))
    one("repeat16-first", "INF_BAD_LENGTHS",
        lambda w: dynamic(w, None, lit3, [0], final=True, ops=[(16, 0)] + plain_ops(lit3[3:] + [0]), cl_lens=spread([0, 1, 2, 16], 19)))
    one("repeat-past-end", "INF_BAD_LENGTHS",
        lambda w: dynamic(w, None, lit3, [0], final=True, ops=plain_ops(lit3) + [(17, 0)]))
    one("no-end-of-block", "INF_BAD_LENGTHS", lambda w: dynamic(w, None, spread([65, 66], 257), [0], final=True))
    one("hlit-287", "INF_BAD_LENGTHS", lambda w: dynamic(w, None, lit3, [0], final=True, nl=287))
    one("hdist-31", "INF_BAD_LENGTHS", lambda w: dynamic(w, None, lit3, [0], final=True, nd=31))
    one("lengths-over-subscribed", "INF_BAD_LENGTHS", lambda w: dynamic(w, None, spread([65, 66, 256], 257, [1, 1, 1]), [0], final=True))
    one("lengths-incomplete", "INF_BAD_LENGTHS", lambda w: dynamic(w, None, spread([65, 66, 256], 257, [2, 2, 2]), [0], final=True))
    one("distances-incomplete", "INF_BAD_LENGTHS", lambda w: dynamic(w, None, lit3, [2, 2], final=True))
    one("code-length-code-incomplete", "INF_BAD_LENGTHS",
        lambda w: dynamic(w, None, lit3, [0], final=True, cl_lens=spread([0, 1, 2], 19, [2, 2, 2])))
    one("unused-distance-code", "INF_BAD_SYMBOL",      # a single distance code of length 1 owns the pattern 0; 1 belongs to no code
        lambda w: (dynamic(w, [65, 65, 65, ("sym", 257)], spread([65, 256, 257], 258), [1], final=True, end=False), w.bits(1, 1), w.bits(0, 16)))
    one("no-distance-code-but-a-match", "INF_BAD_SYMBOL",
        lambda w: (dynamic(w, [65, 65, 65, ("sym", 257)], spread([65, 256, 257], 258), [0], final=True, end=False), w.bits(0, 16)))
    return d


def d_cut(build, drop):
    w = Bits()
    build(w)
    return w.bytes()[:-drop]


CASES = _cases()
DEFECTS = _defects()


# ---- streams made by zlib itself ------------------------------------------------------------------------------------------------

def zlib_datas():
    import random

    rnd = random.Random(11)
    half = rnd.randbytes(32768)
    return {"empty": b"", "one-byte": b"y", "zeros": bytes(3000), "period3": b"abc" * 1000,
            "low-entropy": bytes(rnd.choice(b"aaaabbbcd") for _ in range(3000)), "random": rnd.randbytes(3000),
            "repeat-at-32768": half + half + rnd.randbytes(70000 - 65536),      # (farther than deflate() itself looks back)
            "repeat-at-32500": half[:32500] + half[:32500]}


ZLIB_CONFIGS = {"stored": (0, zlib.Z_DEFAULT_STRATEGY), "fixed": (6, zlib.Z_FIXED), "huffman-only": (6, zlib.Z_HUFFMAN_ONLY),
                "rle": (6, zlib.Z_RLE), "level1": (1, zlib.Z_DEFAULT_STRATEGY), "level6": (6, zlib.Z_DEFAULT_STRATEGY),
                "level9": (9, zlib.Z_DEFAULT_STRATEGY), "full-flush": (6, zlib.Z_DEFAULT_STRATEGY)}


def zlib_stream(data, config):
    """`data` as a zlib stream made by zlib.compressobj under ZLIB_CONFIGS[config]; "full-flush": a Z_FULL_FLUSH in the middle"""
    level, strategy = ZLIB_CONFIGS[config]
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    if config == "full-flush":
        return c.compress(data[:len(data) // 2]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(data[len(data) // 2:]) + c.flush()
    return c.compress(data) + c.flush()


CANARY = 0xA5


def inflate_on_device(entries):
    """One yogo_inflate_zlib launch over `entries` = [(raw stream, dst_len, adler32)].  Sources and destinations are packed at
    offsets of every alignment with gaps between them; the destination starts out as CANARY bytes.
    -> (status list, what each entry's destination range holds, True when every byte outside the ranges is still CANARY)"""
    import numpy as np
    import torch

    from yogo_amd.device_decode import inflate_streams

    rows, src, dpos = [], bytearray(), 16
    for i, (data, dst_len, adler) in enumerate(entries):
        pad = (5 * i + 3) % 16 if i % 4 else (16 - len(src) % 16) % 16    # every fourth source starts on a multiple of 16
        src += bytes([0x5A]) * pad
        soff = len(src)
        src += data
        doff = dpos + ((7 * i + 1) % 16 if i % 3 else 0)                   # every third destination likewise
        rows.append((soff, len(data), doff, dst_len, adler))
        dpos = -(-(doff + dst_len + 16) // 16) * 16
    src += bytes([0x5A]) * 16
    dst = torch.full((dpos + 16,), CANARY, dtype=torch.uint8, device="cuda")
    status = torch.full((len(rows),), -1, dtype=torch.int32, device="cuda")
    inflate_streams(torch.frombuffer(src, dtype=torch.uint8).cuda(), torch.tensor(rows, dtype=torch.int64).reshape(-1, 5).cuda(), dst, status)
    host = dst.cpu().numpy()
    outside = np.ones(host.size, dtype=bool)
    got = []
    for _, _, doff, dst_len, _ in rows:
        outside[doff:doff + dst_len] = False
        got.append(host[doff:doff + dst_len].tobytes())
    return status.cpu().tolist(), got, bool((host[outside] == CANARY).all())
