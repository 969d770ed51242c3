"""The host side of baseline JPEG files (numpy only, no PIL), written from ITU-T T.81 and the arithmetic of libjpeg's jidctint.c
(JDCT_ISLOW), jdsample.c (fancy upsampling) and jdcolor.c, whose defaults PIL decodes with.

``parse_jpeg`` reads the marker segments up to SOS into a ``JpegInfo``; ``JpegInfo.device_decodable`` says whether
``yogo_jpeg_decode`` (csrc/jpeg_decode.hip) takes the file; ``table_row`` is that kernel's table row; ``jpeg_status`` makes the
kernel's checks in the kernel's order and returns its status; ``decode`` is the numpy twin, bit for bit what
``read_image(path, rgb)`` gives for the files the predicate accepts.

Anything libjpeg would repair with a warning -- bytes in front of a marker, a scan that ends early, a run past coefficient 63 --
is a nonzero status here and in the kernel, so that the device never disagrees with PIL about a damaged file: it hands it over.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

# status of one file, the same numbers in csrc/jpeg_decode.hip
JPG_OK = 0
JPG_BAD_ROW = 1          # the row does not lie inside src / dst, or its frame is not one the kernel takes
JPG_NO_TABLE = 2         # the scan names a quantisation or Huffman table that was never defined (or that ends behind the file)
JPG_BAD_HUFFMAN = 3      # a DHT whose counts describe no prefix code (libjpeg: no all-ones code either), or more than 256 symbols
JPG_SOURCE_ENDS = 4      # the source ends inside a code, inside extra bits or in front of a restart marker
JPG_BAD_CODE = 5         # a bit pattern without a code
JPG_BAD_CATEGORY = 6     # a DC category above 11, an AC category above 10, an AC symbol r/0 with r in 1 .. 14
JPG_RUN_PAST_63 = 7      # a run that passes coefficient 63
JPG_BAD_MARKER = 8       # a marker inside a restart interval, FF followed by neither 00 nor an allowed marker, bytes left over in
#                          front of a restart marker, a restart marker that is not the expected RSTm
JPG_NO_EOI = 9           # behind the last MCU stands no EOI (bytes left over, another marker, the end of the file)
JPG_MCU_COUNT = 10       # EOI stands in front of the frame's last MCU
JPG_COEF_RANGE = 11      # a dequantised coefficient outside +-COEF_MAX: more than 8-bit samples give at any quantiser (|DCT| <= 1024
#                          plus half a quantiser step of at most 255), and where libjpeg's scalar and vector IDCTs part ways
JPG_STATUS = {
    JPG_BAD_ROW: "a table row lies outside the buffers or describes no frame the kernel takes",
    JPG_NO_TABLE: "the scan names a table that was never defined",
    JPG_BAD_HUFFMAN: "a Huffman table's counts describe no prefix code",
    JPG_SOURCE_ENDS: "the source ends inside the scan",
    JPG_BAD_CODE: "a bit pattern without a code",
    JPG_BAD_CATEGORY: "a coefficient category the format does not define",
    JPG_RUN_PAST_63: "a zero run passes coefficient 63",
    JPG_BAD_MARKER: "a marker that does not belong where it stands",
    JPG_NO_EOI: "no EOI behind the last MCU",
    JPG_MCU_COUNT: "EOI in front of the last MCU",
    JPG_COEF_RANGE: "a dequantised coefficient larger than 8-bit samples give",
}

MAX_WIDTH = 1040         # the widest frame the kernel's LDS band serves (130 blocks of grey / 4:4:4, 65 MCUs of 4:2:2 / 4:2:0)
COEF_MAX = 2047
TABLE_COLS = 18          # int64 per table row (``table_row``)

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63], dtype=np.int64)   # zigzag position -> natural (row-major) position
_ZZ = ZIGZAG.tolist()


class NotJpeg(ValueError):
    """the bytes do not start with SOI (FFD8): another format under the name"""


class Component(NamedTuple):
    id: int
    h: int
    v: int
    tq: int


class JpegInfo(NamedTuple):
    sof: int                                # the SOFn marker's n (0 baseline, 1 extended, 2 progressive, 9 arithmetic ...); -1: no frame
    precision: int
    height: int
    width: int
    components: Tuple[Component, ...]
    quant: Dict[int, Tuple[int, int]]       # table id -> (offset of its 64 entries in the file, 1 where they are 16-bit)
    huffman: Dict[Tuple[int, int], int]     # (class: 0 DC / 1 AC, table id) -> offset of its 16 counts in the file
    restart_interval: int
    jfif: bool
    adobe_transform: Optional[int]          # the Adobe APP14 segment's transform byte, None without the segment
    scan_components: Tuple[Tuple[int, int, int], ...]   # SOS: (component id, DC table id, AC table id)
    scan_params: Tuple[int, int, int, int]  # SOS: Ss, Se, Ah, Al
    scan_offset: int                        # where the entropy-coded bytes start
    scans: int                              # SOS markers in the file (counted without decoding: FFDA behind the first scan)

    @property
    def ycbcr(self) -> bool:
        """three components that libjpeg treats as YCbCr (jdapimin.c: default_decompress_parms)"""
        if len(self.components) != 3:
            return False
        if self.jfif:
            return True
        if self.adobe_transform is not None:
            return self.adobe_transform != 0
        return tuple(c.id for c in self.components) != (0x52, 0x47, 0x42)

    @property
    def sampling(self) -> Optional[Tuple[int, int]]:
        """(1, 1) for grey, the luma factors (h, v) of a 4:4:4 / 4:2:2 / 4:2:0 file, None for anything else"""
        if len(self.components) == 1:
            return (1, 1)
        if len(self.components) != 3:
            return None
        y, cb, cr = self.components
        if (cb.h, cb.v, cr.h, cr.v) != (1, 1, 1, 1) or (y.h, y.v) not in ((1, 1), (2, 1), (2, 2)):
            return None
        return (y.h, y.v)

    @property
    def device_decodable(self) -> bool:
        """what yogo_jpeg_decode takes: Huffman sequential, 8 bits, ONE interleaved scan over all components, grey or YCbCr at
        4:4:4 / 4:2:2 / 4:2:0, a width the kernel's band serves"""
        n = len(self.components)
        return (self.sof in (0, 1) and self.precision == 8 and self.height > 0 and 0 < self.width <= MAX_WIDTH
                and self.scans == 1 and self.scan_params == (0, 63, 0, 0) and n in (1, 3) and self.sampling is not None
                and (n == 1 or self.ycbcr)
                and tuple(s[0] for s in self.scan_components) == tuple(c.id for c in self.components))


def parse_jpeg(data) -> JpegInfo:
    """the marker segments of one file up to its first SOS.  NotJpeg without SOI, ValueError for a JPEG that does not parse."""
    d = bytes(data) if not isinstance(data, bytes) else data
    n = len(d)
    if n < 2 or d[0] != 0xFF or d[1] != 0xD8:
        raise NotJpeg("no SOI marker")
    sof, precision, height, width, comps = -1, 0, 0, 0, ()
    quant: Dict[int, Tuple[int, int]] = {}
    huff: Dict[Tuple[int, int], int] = {}
    dri, jfif, adobe = 0, False, None
    p = 2
    while True:
        if p + 4 > n:
            raise ValueError("JPEG: the file ends in front of SOS")
        if d[p] != 0xFF:
            raise ValueError(f"JPEG: no marker at byte {p}")
        m = d[p + 1]
        if m == 0xFF:
            p += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD8:
            p += 2
            continue
        if m == 0xD9:
            raise ValueError("JPEG: EOI in front of SOS")
        ln = (d[p + 2] << 8) | d[p + 3]
        seg, end = p + 4, p + 2 + ln
        if ln < 2 or end > n:
            raise ValueError(f"JPEG: the segment of marker {m:02X} at byte {p} does not lie inside the file")
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            if sof >= 0:
                raise ValueError("JPEG: two frame headers")
            if ln < 8 or ln != 8 + 3 * d[seg + 5]:
                raise ValueError("JPEG: a frame header of the wrong length")
            sof, precision = m - 0xC0, d[seg]
            height, width = (d[seg + 1] << 8) | d[seg + 2], (d[seg + 3] << 8) | d[seg + 4]
            comps = tuple(Component(d[seg + 6 + 3 * i], d[seg + 7 + 3 * i] >> 4, d[seg + 7 + 3 * i] & 15, d[seg + 8 + 3 * i])
                          for i in range(d[seg + 5]))
            if width == 0 or not comps or any(not (1 <= c.h <= 4 and 1 <= c.v <= 4) for c in comps):
                raise ValueError("JPEG: an empty frame or a sampling factor outside 1 .. 4")
        elif m == 0xDB:
            q = seg
            while q < end:
                pq, tq = d[q] >> 4, d[q] & 15
                size = 128 if pq else 64
                if pq > 1 or tq > 3 or q + 1 + size > end:
                    raise ValueError("JPEG: a malformed DQT segment")
                quant[tq] = (q + 1, pq)
                q += 1 + size
        elif m == 0xC4:
            q = seg
            while q < end:
                tc, th = d[q] >> 4, d[q] & 15
                if tc > 1 or th > 3 or q + 17 > end:
                    raise ValueError("JPEG: a malformed DHT segment")
                total = sum(d[q + 1:q + 17])
                if q + 17 + total > end:
                    raise ValueError("JPEG: a DHT table longer than its segment")
                huff[(tc, th)] = q + 1
                q += 17 + total
        elif m == 0xDD:
            if ln != 4:
                raise ValueError("JPEG: a DRI segment of the wrong length")
            dri = (d[seg] << 8) | d[seg + 1]
        elif m == 0xE0:
            if ln >= 7 and d[seg:seg + 5] == b"JFIF\0":
                jfif = True
        elif m == 0xEE:
            if ln >= 14 and d[seg:seg + 5] == b"Adobe":
                adobe = d[seg + 11]
        elif m == 0xDA:
            if sof < 0:
                raise ValueError("JPEG: SOS in front of the frame header")
            ns = d[seg]
            if ns < 1 or ns > 4 or ln != 6 + 2 * ns:
                raise ValueError("JPEG: a scan header of the wrong length")
            sc = tuple((d[seg + 1 + 2 * i], d[seg + 2 + 2 * i] >> 4, d[seg + 2 + 2 * i] & 15) for i in range(ns))
            q = seg + 1 + 2 * ns
            params = (d[q], d[q + 1], d[q + 2] >> 4, d[q + 2] & 15)
            scans = 1 + d.count(b"\xff\xda", end)
            return JpegInfo(sof, precision, height, width, comps, quant, huff, dri, jfif, adobe, sc, params, end, scans)
        p = end


def table_row(info: JpegInfo, src_off: int, src_len: int, dst_off: int, planes: int) -> List[int]:
    """the kernel's table row of one accepted file (TABLE_COLS int64): { src_off, src_len, dst_off, dst_len = planes * H * W, H, W,
    components | luma h << 8 | luma v << 16, restart interval, offset of the entropy-coded bytes, then per component (three slots, a
    grey file fills the first of each) the offset of its quantisation table's entries * 2 + (1 where they are 16-bit), of its DC
    table's 16 counts and of its AC table's 16 counts; offsets from the file's first byte, -1 for a table never defined }"""
    hs, vs = info.sampling
    ids = {c.id: c for c in info.components}
    q, dc, ac = [-1] * 3, [-1] * 3, [-1] * 3
    for i, (cid, td, ta) in enumerate(info.scan_components[:3]):
        tq = ids[cid].tq
        if tq in info.quant:
            q[i] = info.quant[tq][0] * 2 + info.quant[tq][1]
        dc[i] = info.huffman.get((0, td), -1)
        ac[i] = info.huffman.get((1, ta), -1)
    return [int(src_off), int(src_len), int(dst_off), planes * info.height * info.width, info.height, info.width,
            len(info.components) | hs << 8 | vs << 16, info.restart_interval, info.scan_offset] + q + dc + ac


# ---- the scan: the kernel's serial part, check for check ---------------------------------------------------------------------
_LOOK: Dict[bytes, object] = {}


def _huffman(d: bytes, off: int):
    """the DHT table at ``off`` (16 counts, then the symbols) -> a list of 65536 entries symbol << 5 | code length for the 16 bits
    a code starts with (0: no code), or a status"""
    if off < 0 or off + 16 > len(d):
        return JPG_NO_TABLE
    counts = d[off:off + 16]
    total = sum(counts)
    if off + 16 + total > len(d):
        return JPG_NO_TABLE
    key = d[off:off + 16 + total]
    got = _LOOK.get(key)
    if got is not None:
        return got
    if total > 256:
        return JPG_BAD_HUFFMAN
    look = np.zeros(65536, dtype=np.int32)
    code, k = 0, off + 16
    for ln in range(1, 17):
        c = counts[ln - 1]
        if c and code + c >= (1 << ln):
            _LOOK[key] = JPG_BAD_HUFFMAN
            return JPG_BAD_HUFFMAN
        for _ in range(c):
            look[code << (16 - ln):(code + 1) << (16 - ln)] = (d[k] << 5) | ln
            code += 1
            k += 1
        code <<= 1
    got = look.tolist()
    if len(_LOOK) > 64:
        _LOOK.clear()
    _LOOK[key] = got
    return got


def _segment(d: bytes, pos: int) -> Tuple[bytes, int, int]:
    """the entropy-coded bytes from ``pos`` up to the first marker or the end -> (the bytes with the stuffing taken out, where the
    marker's FF stands -- or the source ended --, the marker's second byte or -1 at the end of the source)"""
    q = pos
    while True:
        q = d.find(b"\xff", q)
        if q < 0 or q + 1 >= len(d):
            stop, marker = (len(d) if q < 0 else q), -1
            break
        if d[q + 1] != 0:
            stop, marker = q, d[q + 1]
            break
        q += 2
    return d[pos:stop].replace(b"\xff\x00", b"\xff"), stop, marker


def _geometry(info: JpegInfo):
    """-> (blocks per MCU of every component as (h, v), MCUs across, MCU rows)"""
    if len(info.components) == 1:
        return [(1, 1)], -(-info.width // 8), -(-info.height // 8)
    hs, vs = info.sampling
    return [(hs, vs), (1, 1), (1, 1)], -(-info.width // (8 * hs)), -(-info.height // (8 * vs))


def _scan(d: bytes, info: JpegInfo) -> Tuple[int, Optional[List[np.ndarray]]]:
    """the whole scan -> (status, per component the dequantised coefficients int32 [block rows, blocks across, 64] in natural order)"""
    n = len(d)
    if not info.device_decodable or info.scan_offset > n:
        return JPG_BAD_ROW, None
    ids = {c.id: c for c in info.components}
    quants, dcs, acs = [], [], []
    for cid, td, ta in info.scan_components:
        tq = ids[cid].tq
        if tq not in info.quant:
            return JPG_NO_TABLE, None
        qo, wide = info.quant[tq]
        if qo + (128 if wide else 64) > n:
            return JPG_NO_TABLE, None
        quants.append([(d[qo + 2 * k] << 8) | d[qo + 2 * k + 1] for k in range(64)] if wide else list(d[qo:qo + 64]))
    for cid, td, ta in info.scan_components:
        for store, key in ((dcs, (0, td)), (acs, (1, ta))):
            t = _huffman(d, info.huffman.get(key, -1))
            if isinstance(t, int):
                return t, None
            store.append(t)
    blocks, mx, my = _geometry(info)
    coefs = [np.zeros((my * v, mx * h, 64), dtype=np.int32) for h, v in blocks]
    ri, total = info.restart_interval, mx * my
    pred = [0] * len(blocks)
    buf, stop, marker = _segment(d, info.scan_offset)
    acc, have, at, real = 0, 0, 0, 8 * len(buf)   # `have` bits in acc (real ones first, then zeros); `real`: real bits not yet consumed
    expected = 0

    def ended() -> int:   # the status of a read past the last real bit
        if marker < 0:
            return JPG_SOURCE_ENDS
        return JPG_MCU_COUNT if marker == 0xD9 else JPG_BAD_MARKER

    for mcu in range(total):
        if ri and mcu and mcu % ri == 0:
            if real >= 8:
                return JPG_BAD_MARKER, None
            if marker < 0:
                return JPG_SOURCE_ENDS, None
            if marker != 0xD0 + expected:
                return JPG_BAD_MARKER, None
            expected = (expected + 1) & 7
            buf, stop, marker = _segment(d, stop + 2)
            acc, have, at, real = 0, 0, 0, 8 * len(buf)
            pred = [0] * len(blocks)
        my_, mx_ = divmod(mcu, mx)
        for c, (h, v) in enumerate(blocks):
            q, dct, act, plane = quants[c], dcs[c], acs[c], coefs[c]
            for by in range(v):
                for bx in range(h):
                    out = [0] * 64
                    k = 0
                    while k < 64:
                        if have < 32:
                            acc = (acc << 48) | int.from_bytes(buf[at:at + 6].ljust(6, b"\0"), "big")
                            at += 6
                            have += 48
                        e = (dct if k == 0 else act)[(acc >> (have - 16)) & 0xFFFF]
                        ln = e & 31
                        if (ln or 16) > real:
                            return ended(), None
                        if ln == 0:
                            return JPG_BAD_CODE, None
                        have -= ln
                        real -= ln
                        r, s = (e >> 9) & 15, (e >> 5) & 15
                        if k == 0:
                            if e >> 5 > 11:
                                return JPG_BAD_CATEGORY, None
                            r = 0
                        elif s == 0:
                            if r == 15:
                                if k + 16 > 64:
                                    return JPG_RUN_PAST_63, None
                                k += 16
                                continue
                            if r:
                                return JPG_BAD_CATEGORY, None
                            break
                        elif s > 10:
                            return JPG_BAD_CATEGORY, None
                        k += r
                        if k > 63:
                            return JPG_RUN_PAST_63, None
                        val = 0
                        if s:
                            if s > real:
                                return ended(), None
                            val = (acc >> (have - s)) & ((1 << s) - 1)
                            have -= s
                            real -= s
                            if val < (1 << (s - 1)):
                                val -= (1 << s) - 1
                        acc &= (1 << have) - 1
                        if k == 0:
                            pred[c] += val
                            val = pred[c]
                        val *= q[k]
                        if val < -COEF_MAX or val > COEF_MAX:
                            return JPG_COEF_RANGE, None
                        out[_ZZ[k]] = val
                        k += 1
                    plane[my_ * v + by, mx_ * h + bx] = out
    if real >= 8 or marker != 0xD9:
        return JPG_NO_EOI, None
    return JPG_OK, coefs


def jpeg_status(data) -> int:
    """the status yogo_jpeg_decode gives the file: 0, or the number of the first check that fails.  A file that does not parse, or
    that the predicate refuses, is JPG_BAD_ROW (the routes never hand one over)."""
    d = bytes(data)
    try:
        info = parse_jpeg(d)
    except ValueError:
        return JPG_BAD_ROW
    return _scan(d, info)[0]


# ---- the parallel part: IDCT, upsampling, colour ------------------------------------------------------------------------------
def _idct_pass(x: np.ndarray, shift: int) -> np.ndarray:
    """jidctint.c's one-dimensional pass over axis 1 of int32 [n, 8, 8] (13-bit constants), descaled by ``shift`` with rounding"""
    i0, i1, i2, i3, i4, i5, i6, i7 = (x[:, k, :] for k in range(8))
    z1 = (i2 + i6) * 4433
    t2 = z1 + i6 * -15137
    t3 = z1 + i2 * 6270
    t0 = (i0 + i4) << 13
    t1 = (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    z1, z2, z3, z4 = i7 + i1, i5 + i3, i7 + i3, i5 + i1
    z5 = (z3 + z4) * 9633
    o0, o1, o2, o3 = i7 * 2446, i5 * 16819, i3 * 25172, i1 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    half = np.int32(1 << (shift - 1))
    rows = (t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3)
    return np.stack([(r + half) >> shift for r in rows], axis=1)


def _idct(coef: np.ndarray) -> np.ndarray:
    """dequantised coefficients int32 [rows, across, 64] -> the component's samples uint8 [rows * 8, across * 8]"""
    rows, across, _ = coef.shape
    x = coef.reshape(-1, 8, 8).astype(np.int32)
    with np.errstate(over="ignore"):
        x = np.clip(_idct_pass(x, 11), -32768, 32767)                 # columns (the vector units keep 16 bits between the passes)
        x = _idct_pass(x.transpose(0, 2, 1), 18).transpose(0, 2, 1)   # rows
    x = np.clip(x + 128, 0, 255).astype(np.uint8)
    return x.reshape(rows, across, 8, 8).transpose(0, 2, 1, 3).reshape(rows * 8, across * 8)


def _upsample_h2v1(c: np.ndarray) -> np.ndarray:
    """jdsample.c h2v1_fancy_upsample over the real samples [h, cw] -> int32 [h, 2 * cw]; replication at cw <= 2, as jinit_upsampler
    chooses"""
    c = c.astype(np.int32)
    out = np.empty((c.shape[0], 2 * c.shape[1]), dtype=np.int32)
    if c.shape[1] <= 2:
        out[:, 0::2] = out[:, 1::2] = c
        return out
    left = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
    right = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
    out[:, 0::2] = (3 * c + left + 1) >> 2
    out[:, 1::2] = (3 * c + right + 2) >> 2
    out[:, 0], out[:, -1] = c[:, 0], c[:, -1]
    return out


def _upsample_h2v2(c: np.ndarray) -> np.ndarray:
    """jdsample.c h2v2_fancy_upsample over the real samples [ch, cw] -> int32 [2 * ch, 2 * cw]; replication at cw <= 2"""
    c = c.astype(np.int32)
    ch, cw = c.shape
    out = np.empty((2 * ch, 2 * cw), dtype=np.int32)
    if cw <= 2:
        for dy in (0, 1):
            out[dy::2, 0::2] = out[dy::2, 1::2] = c
        return out
    above = np.concatenate([c[:1], c[:-1]], axis=0)
    below = np.concatenate([c[1:], c[-1:]], axis=0)
    for dy, far in ((0, above), (1, below)):
        s = 3 * c + far
        left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
        right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
        out[dy::2, 0::2] = (3 * s + left + 8) >> 4
        out[dy::2, 1::2] = (3 * s + right + 7) >> 4
        out[dy::2, 0] = (4 * s[:, 0] + 8) >> 4
        out[dy::2, -1] = (4 * s[:, -1] + 7) >> 4
    return out


def pixels(info: JpegInfo, coefs: List[np.ndarray], rgb: bool) -> np.ndarray:
    """the dequantised coefficients of every component -> uint8 [1 | 3, H, W] as ``read_image`` converts"""
    H, W = info.height, info.width
    planes = [_idct(c) for c in coefs]
    if len(planes) == 1:
        y = planes[0][:H, :W]
        return np.stack([y] * 3) if rgb else y[None].copy()
    hs, vs = info.sampling
    ch, cw = -(-H // vs), -(-W // hs)
    up = {(1, 1): lambda c: c.astype(np.int32), (2, 1): _upsample_h2v1, (2, 2): _upsample_h2v2}[(hs, vs)]
    y = planes[0][:H, :W].astype(np.int32)
    cb, cr = (up(p[:ch, :cw])[:H, :W] - 128 for p in planes[1:])
    r = np.clip(y + ((91881 * cr + 32768) >> 16), 0, 255)
    g = np.clip(y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0, 255)
    b = np.clip(y + ((116130 * cb + 32768) >> 16), 0, 255)
    if rgb:
        return np.stack([r, g, b]).astype(np.uint8)
    return ((19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16).astype(np.uint8)[None]


def decode(data, rgb: bool) -> np.ndarray:
    """the numpy twin of yogo_jpeg_decode: uint8 [1 | 3, H, W], bit for bit ``read_image(path, rgb)``.  ValueError with the status
    for a file the kernel would hand to the host."""
    d = bytes(data)
    info = parse_jpeg(d)
    status, coefs = _scan(d, info)
    if status:
        raise ValueError(f"JPEG: {JPG_STATUS[status]} (status {status})")
    return pixels(info, coefs, rgb)
