"""PNG files of every colour type and bit depth for the tests, on top of tests/_png_write.py (which stays the 8-bit grey / RGB
writer): random samples, a chosen filter type per row at any ``bpp``, optionally Adam7, optionally a tRNS chunk, a PLTE of any
length.  The container comes from ``_png_write.png_bytes(ihdr=..., scan=..., before=...)``.

The decoders under test (yogo_amd/png.py: decode_any; csrc/png_unpack_any.hip) and this writer share an author; PIL reads the files
it writes, and the tests compare with PIL's pixels (``read_image``)."""
import struct

import numpy as np

import _png_write as PW

CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
FORMATS = ((0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16))
SHAPES = ((67, 37), (9, 5), (5, 3), (1, 1))   # H x W


def format_id(fmt) -> str:
    return f"ct{fmt[0]}d{fmt[1]}"


def filter_bytes(rows, types, bpp):
    """uint8 [h, n] row bytes -> uint8 [h, 1 + n] scanlines, row y under filter types[y]; the byte to the left is ``bpp`` back"""
    rows = np.asarray(rows, dtype=np.uint8)
    h, n = rows.shape
    out = np.zeros((h, 1 + n), dtype=np.uint8)
    for y in range(h):
        cur = rows[y].astype(np.int64)
        up = rows[y - 1].astype(np.int64) if y else np.zeros(n, np.int64)
        left = np.concatenate((np.zeros(bpp, np.int64), cur))[:n]
        upleft = np.concatenate((np.zeros(bpp, np.int64), up))[:n]
        t = int(types[y])
        pred = {0: np.zeros(n, np.int64), 1: left, 2: up, 3: (left + up) // 2, 4: PW.paeth(left, up, upleft)}.get(t, np.zeros(n, np.int64))
        out[y, 0] = t
        out[y, 1:] = (cur - pred) & 255
    return out


def pack_samples(samples, depth):
    """[h, w, channels] samples below 2^depth -> uint8 [h, ceil(w * channels * depth / 8)] row bytes: 16-bit samples big-endian,
    depths below 8 most significant bits first, the last byte of a row padded with zero bits"""
    s = np.asarray(samples).astype(np.uint16)
    h = s.shape[0]
    flat = s.reshape(h, -1)
    if depth == 16:
        return np.stack((flat >> 8, flat & 255), axis=2).reshape(h, -1).astype(np.uint8)
    if depth == 8:
        return flat.astype(np.uint8)
    per = 8 // depth
    pad = (-flat.shape[1]) % per
    flat = np.concatenate((flat, np.zeros((h, pad), np.uint16)), axis=1).reshape(h, -1, per)
    shifts = np.arange(per - 1, -1, -1, dtype=np.uint16) * depth
    return (flat << shifts).sum(axis=2).astype(np.uint8)


def random_samples(rng, H, W, ct, depth):
    """[H, W, channels] uint16; 16-bit greyscale: half of the samples below 300, around PIL's clip at 255"""
    ch = CHANNELS[ct]
    s = rng.integers(0, 1 << depth, size=(H, W, ch), dtype=np.uint16 if depth < 16 else np.uint32).astype(np.uint16)
    if ct == 0 and depth == 16:
        s = np.where(rng.random((H, W, ch)) < 0.5, rng.integers(0, 300, size=(H, W, ch)), s).astype(np.uint16)
    return s


def scanlines(samples, depth, types=None, interlace=False, bad=None):
    """the bytes a file's zlib stream holds.  types: filter type per row, indexed by the row's number among ALL scanlines of the file
    (default: 0 1 2 3 4 0 ... from the first row on, so that every band of rows mixes all five); bad: (pass, row, value) puts
    ``value`` in the filter-type byte of that row of that pass (pass 0 when not interlaced) without filtering it"""
    s = np.asarray(samples)
    H, W, ch = s.shape
    bpp = max(1, ch * depth // 8)
    out, n = bytearray(), 0
    for p, (x0, y0, dx, dy) in enumerate(PW.ADAM7 if interlace else ((0, 0, 1, 1),)):
        sub = s[y0::dy, x0::dx]
        if sub.size == 0:
            continue
        h = sub.shape[0]
        t = [(n + y) % 5 if types is None else int(types[n + y]) for y in range(h)]
        n += h
        if bad is not None and bad[0] == p:
            t[bad[1]] = bad[2]
        out += filter_bytes(pack_samples(sub, depth), t, bpp).tobytes()
    return bytes(out)


def trns_chunk(rng, ct, depth, entries=0):
    """a tRNS chunk as the colour type has it (a grey level, an RGB triple, alpha per palette entry); for colour types 4 and 6, which
    carry alpha themselves, two bytes that a decoder ignores"""
    if ct == 3:
        return (b"tRNS", bytes(rng.integers(0, 256, size=max(1, entries), dtype=np.uint8).tolist()))
    return (b"tRNS", b"".join(struct.pack(">H", int(rng.integers(0, 1 << depth))) for _ in range(3 if ct in (2, 6) else 1)))


def make_png(rng, H, W, ct, depth, *, interlace=False, trns=False, types=None, plte_entries=None, bad=None, extra=(), samples=None):
    """-> (file bytes, samples [H, W, channels] uint16, palette uint8 [entries, 3] or None).  plte_entries: the length of the PLTE
    chunk of a palette file (default 2^depth; 0: no PLTE chunk); a file of another colour type gets a PLTE chunk when it is > 0"""
    s = random_samples(rng, H, W, ct, depth) if samples is None else samples
    n = (1 << depth if ct == 3 else 0) if plte_entries is None else plte_entries
    palette = rng.integers(0, 256, size=(n, 3), dtype=np.uint8) if n else None
    before = list(extra)
    if palette is not None:
        before.append((b"PLTE", palette.tobytes()))
    if trns:
        before.append(trns_chunk(rng, ct, depth, n))
    data = PW.png_bytes(np.zeros((H, W), np.uint8), ihdr=(W, H, depth, ct, 0, 0, 1 if interlace else 0),
                        scan=scanlines(s, depth, types, interlace, bad), before=before)
    return data, s, palette
