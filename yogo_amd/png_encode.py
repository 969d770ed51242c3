"""PNG files written on the device (yogo_amd/csrc/png_encode.hip) and their restatement on the host.

``encode_png_host`` is the twin of ``yogo_png_encode``, as ``yogo_amd.inflate`` is of the device inflate: it takes the same
decisions in the same order and gives the same bytes, runs without a GPU and is what the device is held to.  The file it writes is
an ordinary PNG (8 bits per sample; grey, grey+alpha, RGB or RGBA by the pixel size 1 .. 4; no interlace) whose choices are made so
that every part is independent work:

* **filter** -- per scanline the filter type 0 .. 4 with the smallest sum of absolute values of the filtered bytes read as signed;
  ties go to the lowest type.  The raw rows are all there, so every row filters on its own.
* **bands** -- the filtered scanlines are cut into bands of ``BAND_ROWS`` rows.  A band is ONE dynamic-Huffman DEFLATE block of
  literals only (257 literal/length codes, one distance code of length zero: what zlib's ``Z_HUFFMAN_ONLY`` emits), closed with an
  empty stored block so that the next band starts on a byte boundary; the last band's closing block carries BFINAL.
* **code lengths** -- a Huffman tree over the used symbols sorted by (count, symbol), built with two queues (a leaf wins a tie
  against an internal node); lengths above the limit (15, and 7 for the code-length alphabet) are folded into the limit and the
  Kraft sum is brought back by, per unit of excess, taking one code off the limit and splitting the longest shorter code; the
  lengths go back to the symbols longest first, from the rarest.  The header spells every one of the 258 lengths out as its own
  symbol (no repeat codes 16 .. 18) and sends all 19 code-length code lengths.
* **stored fallback** -- a band that does not come out smaller than stored blocks (at most 65 535 bytes each) is written as stored
  blocks, which is what makes ``encode_bound`` exact and small.
* **chunks** -- every band is its own IDAT chunk; the zlib header opens the first, the Adler-32 closes the last.

That is level 0, the default.  **Level 1** (``yogo_png_encode_level``, ``--device-draw-level 1``) keeps the filter, the bands, the
chunks, the closing stored block, the stored fallback and the bound, and codes a band as one dynamic-Huffman block of literals AND
matches.  Every choice is a pure function of the band's filtered bytes, position by position, so no lane waits for another:

* **pieces** -- the band's filtered bytes are cut into pieces of ``PIECE`` bytes, counted from the band's first byte.  No match
  passes the end of its piece (or of the band), and no match reaches back before the band's first byte.
* **candidates** -- at position i the ``WINDOW`` distances ``bpp * k``, k = 1 .. ``WINDOW``, that do not pass the band's first byte
  (so at most 256 back: the same channel of the pixels before).  The length of a candidate is the number of bytes from i on that
  equal the byte `distance` before them (the copy may overlap itself: distance < length is what codes a constant row), at most
  ``MAX_MATCH`` and at most up to the piece's end.  The longest candidate wins, ties go to the nearest.  A length below
  ``MIN_MATCH`` is no match.
* **parse** -- greedy from the piece's first byte: a position with a match gives a length/distance pair and the parse goes on
  behind it, any other position gives a literal.  Pieces do not depend on each other.
* **block** -- 286 literal/length code lengths and 30 distance code lengths (limit 15, the rule of *code lengths* above), each
  spelled out as its own symbol; a band without a match sends ONE distance code of length zero instead, a band whose matches use
  one distance symbol gives it a one-bit code.  The bit count -- header, codes, extra bits -- is known before anything is written,
  and the band is stored blocks when it is not smaller (the comparison of level 0: an incompressible image is the same file at
  both levels).
"""
from __future__ import annotations

import struct
import zlib
from typing import List, Tuple

import numpy as np

BAND_ROWS = 16
MAX_STORED = 65535
LIT_SYMBOLS = 257          # literals 0 .. 255 and end-of-block
LIT_LIMIT = 15
CL_LIMIT = 7
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
ZLIB_HEADER = b"\x78\x01"
SIGNATURE = b"\x89PNG\r\n\x1a\n"
COLOUR_TYPE = {1: 0, 2: 4, 3: 2, 4: 6}

LEVELS = (0, 1)
PIECE = 512                # level 1: bytes of a band parsed on their own; no match passes a piece's end
WINDOW = 64                # level 1: the candidates of a position are the distances bpp * k, k = 1 .. WINDOW
MIN_MATCH = 3
MAX_MATCH = 258
LEN_SYMBOLS = 286          # literals, end-of-block and the 29 length symbols
DIST_SYMBOLS = 30
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)

ST_OK = 0
ST_SLOT = 1        # the file does not fit the slot: nothing of it was written
ST_BAND = 2        # a band passed its part of the work buffer (cannot happen: the stored fallback bounds it)


def stored_bytes(n: int) -> int:
    """n bytes as stored blocks: 5 bytes of header per block of at most 65 535"""
    return n + 5 * ((n + MAX_STORED - 1) // MAX_STORED)


def band_bound(rows: int, row_bytes: int, first: bool, last: bool) -> int:
    """the most bytes the IDAT chunk of a band of `rows` scanlines takes: length, type, [zlib header], stored blocks, [Adler], CRC"""
    return 12 + stored_bytes(rows * (row_bytes + 1)) + (2 if first else 0) + (4 if last else 0)


def encode_bound(H: int, W: int, bpp: int = 4) -> int:
    """the size of a slot: no H x W image of `bpp` bytes per pixel encodes to more (``yogo_png_encode_bound``)"""
    nb = (H + BAND_ROWS - 1) // BAND_ROWS
    total = len(SIGNATURE) + 25 + 12
    for k in range(nb):
        rows = min(BAND_ROWS, H - k * BAND_ROWS)
        total += band_bound(rows, W * bpp, k == 0, k == nb - 1)
    return total


def filter_scanlines(pixels: np.ndarray) -> np.ndarray:
    """[H, W, bpp] uint8 -> [H, 1 + W * bpp] uint8: per row the filter type and the filtered bytes (the rule above)"""
    H, W, bpp = pixels.shape
    rb = W * bpp
    cur = pixels.reshape(H, rb).astype(np.int32)
    left = np.zeros_like(cur)
    left[:, bpp:] = cur[:, :-bpp] if rb > bpp else 0
    up = np.zeros_like(cur)
    up[1:] = cur[:-1]
    ul = np.zeros_like(cur)
    ul[1:, bpp:] = cur[:-1, :-bpp] if rb > bpp else 0
    p = left + up - ul
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    cands = np.stack([cur, cur - left, cur - up, cur - ((left + up) >> 1), cur - paeth]) & 255     # [5, H, rb]
    signed = np.where(cands >= 128, 256 - cands, cands)
    types = np.argmin(signed.sum(axis=2), axis=0)                                                     # first minimum
    out = np.empty((H, 1 + rb), dtype=np.uint8)
    out[:, 0] = types
    out[:, 1:] = cands[types, np.arange(H)]
    return out


def huffman_lengths(freqs, limit: int) -> List[int]:
    """code lengths of at most `limit` bits for the symbols with a count above zero (0 for the others); the rule above"""
    used = sorted((int(f), s) for s, f in enumerate(freqs) if f)
    n = len(used)
    lengths = [0] * len(freqs)
    if n == 0:
        return lengths
    if n == 1:
        lengths[used[0][1]] = 1
        return lengths
    leaf = [f for f, _ in used]
    node: List[int] = []                    # the counts of the internal nodes, in the order they are made (never decreasing)
    leaf_parent, node_parent = [0] * n, [0] * (n - 1)
    li = ni = 0
    for k in range(n - 1):
        total = 0
        for _ in range(2):
            if li < n and (ni >= len(node) or leaf[li] <= node[ni]):
                total += leaf[li]
                leaf_parent[li] = k
                li += 1
            else:
                total += node[ni]
                node_parent[ni] = k
                ni += 1
        node.append(total)
    depth = [0] * (n - 1)
    for k in range(n - 3, -1, -1):
        depth[k] = depth[node_parent[k]] + 1
    count = [0] * (limit + 1)
    for i in range(n):
        count[min(depth[leaf_parent[i]] + 1, limit)] += 1
    kraft = sum(count[b] << (limit - b) for b in range(1, limit + 1))
    while kraft > (1 << limit):
        count[limit] -= 1
        b = limit - 1
        while count[b] == 0:
            b -= 1
        count[b] -= 1
        count[b + 1] += 2
        kraft -= 1
    i = 0
    for b in range(limit, 0, -1):
        for _ in range(count[b]):
            lengths[used[i][1]] = b
            i += 1
    return lengths


def canonical_codes(lengths, limit: int) -> List[int]:
    """the canonical code of every symbol, bit-reversed: DEFLATE sends Huffman codes most significant bit first into a stream that
    fills bytes from the least significant bit"""
    count = [0] * (limit + 2)
    for b in lengths:
        count[b] += 1
    count[0] = 0
    nxt, code = [0] * (limit + 2), 0
    for b in range(1, limit + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for b in lengths:
        if b == 0:
            out.append(0)
            continue
        c = nxt[b]
        nxt[b] += 1
        out.append(int(format(c, f"0{b}b")[::-1], 2))
    return out


def _pack(codes: np.ndarray, lens: np.ndarray) -> Tuple[np.ndarray, int]:
    """the bits of codes[i] (lens[i] of them, least significant first) one after the other -> (bit array, total)"""
    ends = np.cumsum(lens)
    total = int(ends[-1]) if len(ends) else 0
    starts = ends - lens
    bits = np.zeros(total, dtype=np.uint8)
    for k in range(int(lens.max()) if len(lens) else 0):
        m = lens > k
        bits[starts[m] + k] = (codes[m] >> k) & 1
    return bits, total


def encode_band(data: bytes, final: bool) -> Tuple[bytes, bool]:
    """the DEFLATE blocks of one band's filtered scanlines -> (bytes, stored?)"""
    sym = np.frombuffer(data, dtype=np.uint8).astype(np.int64)
    n = len(sym)
    freqs = np.bincount(sym, minlength=LIT_SYMBOLS)
    freqs[256] = 1
    lit_len = huffman_lengths(freqs, LIT_LIMIT)
    header_lens = lit_len + [0]                          # ... and the one distance code, of length zero
    cl_freq = np.bincount(np.asarray(header_lens), minlength=19)
    cl_len = huffman_lengths(cl_freq, CL_LIMIT)
    bits = 17 + 3 * 19 + sum(cl_len[b] for b in header_lens) + sum(int(freqs[s]) * lit_len[s] for s in range(LIT_SYMBOLS)) + 3
    huff = (bits + 7) // 8 + 4
    if huff >= stored_bytes(n):
        out = bytearray()
        nblk = (n + MAX_STORED - 1) // MAX_STORED
        for k in range(nblk):
            piece = data[k * MAX_STORED: (k + 1) * MAX_STORED]
            out += bytes([1 if (final and k == nblk - 1) else 0]) + struct.pack("<HH", len(piece), len(piece) ^ 0xFFFF) + piece
        return bytes(out), True
    lit_code, cl_code = canonical_codes(lit_len, LIT_LIMIT), canonical_codes(cl_len, CL_LIMIT)
    # BFINAL 0, BTYPE 2, HLIT 0 (257), HDIST 0 (1), HCLEN 15 (19)
    codes = [0, 2, 0, 0, 15] + [cl_len[s] for s in CL_ORDER] + [cl_code[b] for b in header_lens]
    lens = [1, 2, 5, 5, 4] + [3] * 19 + [cl_len[b] for b in header_lens]
    ll, lc = np.asarray(lit_len, dtype=np.int64), np.asarray(lit_code, dtype=np.int64)
    codes = np.concatenate([np.asarray(codes, dtype=np.int64), lc[sym], [lc[256]], [1 if final else 0]])
    lens = np.concatenate([np.asarray(lens, dtype=np.int64), ll[sym], [ll[256]], [3]])
    stream, total = _pack(codes, lens)
    assert total == bits
    return np.packbits(stream, bitorder="little").tobytes() + b"\x00\x00\xff\xff", False


def _stored_blocks(data: bytes, final: bool) -> bytes:
    out = bytearray()
    nblk = (len(data) + MAX_STORED - 1) // MAX_STORED
    for k in range(nblk):
        piece = data[k * MAX_STORED: (k + 1) * MAX_STORED]
        out += bytes([1 if (final and k == nblk - 1) else 0]) + struct.pack("<HH", len(piece), len(piece) ^ 0xFFFF) + piece
    return bytes(out)


def length_symbol(length: int) -> int:
    """the index 0 .. 28 of the length symbol (257 + index) that codes a match of `length` bytes"""
    if length == MAX_MATCH:
        return 28
    return max(k for k in range(28) if LEN_BASE[k] <= length)


def distance_symbol(dist: int) -> int:
    return max(k for k in range(DIST_SYMBOLS) if DIST_BASE[k] <= dist)


def find_matches(data: np.ndarray, bpp: int) -> Tuple[np.ndarray, np.ndarray]:
    """per position of a band's filtered bytes the winning candidate (the rule above) -> (length, distance); length 0: no match"""
    n = len(data)
    pos = np.arange(n, dtype=np.int64)
    room = np.minimum(np.minimum((pos // PIECE + 1) * PIECE, n) - pos, MAX_MATCH)      # up to the piece's end
    best_len, best_dist = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for k in range(1, WINDOW + 1):
        d = bpp * k
        if d >= n:
            break
        eq = data[d:] == data[:-d]                                   # eq[j]: byte d + j equals the byte d before it
        m = len(eq)
        stop = np.where(eq, m, np.arange(m))                         # the first mismatch at or behind j
        run = np.minimum.accumulate(stop[::-1])[::-1] - np.arange(m)
        cand = np.minimum(run, room[d:])
        better = cand > best_len[d:]                                 # strictly: a tie stays with the nearer one
        best_len[d:][better] = cand[better]
        best_dist[d:][better] = d
    best_len[best_len < MIN_MATCH] = 0
    best_dist[best_len == 0] = 0
    return best_len, best_dist


def parse_band(data: np.ndarray, bpp: int) -> np.ndarray:
    """the tokens of a band -> int64 [t, 3]: (position, length, distance), a literal as (position, 1, 0).  Greedy from position 0 is
    greedy per piece: no match passes a piece's end, so every piece's first byte starts a token."""
    length, dist = find_matches(data, bpp)
    tokens, i, n = [], 0, len(data)
    while i < n:
        if length[i]:
            tokens.append((i, int(length[i]), int(dist[i])))
            i += int(length[i])
        else:
            tokens.append((i, 1, 0))
            i += 1
    return np.asarray(tokens, dtype=np.int64).reshape(len(tokens), 3)


def encode_band_matches(data: bytes, bpp: int, final: bool) -> Tuple[bytes, bool, np.ndarray]:
    """level 1: the DEFLATE blocks of one band's filtered scanlines -> (bytes, stored?, tokens [t, 3])"""
    raw = np.frombuffer(data, dtype=np.uint8)
    n = len(raw)
    tok = parse_band(raw, bpp)
    is_match = tok[:, 2] > 0
    lits = raw[tok[~is_match, 0]].astype(np.int64)
    mlen, mdist = tok[is_match, 1], tok[is_match, 2]
    len_sym_of = np.zeros(MAX_MATCH + 1, dtype=np.int64)
    for v in range(MIN_MATCH, MAX_MATCH + 1):
        len_sym_of[v] = length_symbol(v)
    dist_sym_of = np.zeros(4 * WINDOW + 1, dtype=np.int64)
    for v in range(1, 4 * WINDOW + 1):
        dist_sym_of[v] = distance_symbol(v)
    ls, ds = len_sym_of[mlen], dist_sym_of[mdist]
    freqs = np.bincount(lits, minlength=LEN_SYMBOLS) + np.bincount(257 + ls, minlength=LEN_SYMBOLS)
    freqs[256] = 1
    dfreqs = np.bincount(ds, minlength=DIST_SYMBOLS)
    lit_len = huffman_lengths(freqs, LIT_LIMIT)
    dist_len = huffman_lengths(dfreqs, LIT_LIMIT) if len(ds) else [0]      # no match: one distance code of length zero
    header_lens = lit_len + dist_len
    cl_freq = np.bincount(np.asarray(header_lens), minlength=19)
    cl_len = huffman_lengths(cl_freq, CL_LIMIT)
    len_extra, dist_extra = np.asarray(LEN_EXTRA, dtype=np.int64), np.asarray(DIST_EXTRA, dtype=np.int64)
    bits = (17 + 3 * 19 + sum(cl_len[b] for b in header_lens) + sum(int(freqs[s]) * lit_len[s] for s in range(LEN_SYMBOLS))
            + sum(int(dfreqs[s]) * dist_len[s] for s in range(len(dist_len))) + int(len_extra[ls].sum()) + int(dist_extra[ds].sum()) + 3)
    if (bits + 7) // 8 + 4 >= stored_bytes(n):
        return _stored_blocks(data, final), True, np.zeros((0, 3), dtype=np.int64)
    lit_code, dist_code, cl_code = canonical_codes(lit_len, LIT_LIMIT), canonical_codes(dist_len, LIT_LIMIT), canonical_codes(cl_len, CL_LIMIT)
    # BFINAL 0, BTYPE 2, HLIT 29 (286), HDIST 29 (30) or 0 (1), HCLEN 15 (19)
    codes = [0, 2, LEN_SYMBOLS - 257, len(dist_len) - 1, 15] + [cl_len[s] for s in CL_ORDER] + [cl_code[b] for b in header_lens]
    lens = [1, 2, 5, 5, 4] + [3] * 19 + [cl_len[b] for b in header_lens]
    ll, lc = np.asarray(lit_len, dtype=np.int64), np.asarray(lit_code, dtype=np.int64)
    dl, dc = np.asarray(dist_len, dtype=np.int64), np.asarray(dist_code, dtype=np.int64)
    # per token up to four fields: the literal or length code, the length's extra bits, the distance code, its extra bits
    t = len(tok)
    fc, fl = np.zeros((t, 4), dtype=np.int64), np.zeros((t, 4), dtype=np.int64)
    fc[~is_match, 0], fl[~is_match, 0] = lc[lits], ll[lits]
    if len(ds):
        base_l, base_d = np.asarray(LEN_BASE, dtype=np.int64), np.asarray(DIST_BASE, dtype=np.int64)
        fc[is_match] = np.stack([lc[257 + ls], mlen - base_l[ls], dc[ds], mdist - base_d[ds]], axis=1)
        fl[is_match] = np.stack([ll[257 + ls], len_extra[ls], dl[ds], dist_extra[ds]], axis=1)
    codes = np.concatenate([np.asarray(codes, dtype=np.int64), fc.reshape(-1), [lc[256]], [1 if final else 0]])
    lens = np.concatenate([np.asarray(lens, dtype=np.int64), fl.reshape(-1), [ll[256]], [3]])
    stream, total = _pack(codes, lens)
    assert total == bits
    return np.packbits(stream, bitorder="little").tobytes() + b"\x00\x00\xff\xff", False, tok


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode_png_host(pixels: np.ndarray, level: int = 0, return_bands: bool = False, return_tokens: bool = False):
    """[H, W, bpp] (or [H, W]) uint8 -> the bytes of the PNG file ``yogo_png_encode_level`` writes for it at `level`; with
    `return_bands` also the list of booleans "band k is stored blocks", with `return_tokens` also per band the tokens of
    ``parse_band`` (level 1; none for a stored band and at level 0).  The extras follow the bytes in that order."""
    if level not in LEVELS:
        raise ValueError(f"level must be one of {LEVELS}, got {level!r}")
    pixels = np.ascontiguousarray(pixels, dtype=np.uint8)
    if pixels.ndim == 2:
        pixels = pixels[:, :, None]
    H, W, bpp = pixels.shape
    if H < 1 or W < 1 or bpp not in COLOUR_TYPE:
        raise ValueError(f"cannot encode pixels of shape {pixels.shape}: [H, W, 1 .. 4] with H, W >= 1")
    scan = filter_scanlines(pixels)
    nb = (H + BAND_ROWS - 1) // BAND_ROWS
    out = bytearray(SIGNATURE + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, COLOUR_TYPE[bpp], 0, 0, 0)))
    stored, tokens = [], []
    for k in range(nb):
        band = scan[k * BAND_ROWS: (k + 1) * BAND_ROWS].tobytes()
        if level == 0:
            body, st = encode_band(band, k == nb - 1)
            tok = np.zeros((0, 3), dtype=np.int64)
        else:
            body, st, tok = encode_band_matches(band, bpp, k == nb - 1)
        stored.append(st)
        tokens.append(tok)
        if k == 0:
            body = ZLIB_HEADER + body
        if k == nb - 1:
            body += struct.pack(">I", zlib.adler32(scan.tobytes()) & 0xFFFFFFFF)
        out += _chunk(b"IDAT", body)
    out += _chunk(b"IEND", b"")
    extras = ([stored] if return_bands else []) + ([tokens] if return_tokens else [])
    return (bytes(out), *extras) if extras else bytes(out)
