"""Writers for the Blosc / LZ4 tests, after the published formats (neither c-blosc nor liblz4 is needed):
* LZ4 blocks: `lz4_build` emits exactly the sequences it is given, `lz4_compress` is a small greedy compressor that keeps the
  format's end-of-block rules (the last 5 bytes are literals, no match starts in the last 12), so that liblz4 decodes its output;
* `lz4_sequences` lists what a block holds (for the tests to assert that a case contains what it is named after);
* Blosc 1 framing of uint8 data with a chosen blocksize and flags byte, a block stored raw when LZ4 does not shrink it, and the
  memcpyed variant;
* `blosc_members`: tests/_zarr_write.py's array with every chunk value re-encoded.

The decoders under test (yogo_amd/blosc.py, csrc/blosc_lz4.hip) and these writers share an author; tests/golden/lz4_blocks.npz
holds blocks written by liblz4 itself."""
import struct

import _zarr_write as ZW

BLOSC_DOC = {"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1, "blocksize": 0}
FLAGS_LZ4 = 0x01 | (1 << 5)      # byte-shuffle (a no-op at typesize 1), inner format lz4


def _length(n: int) -> bytes:
    """the extension bytes of a length whose nibble is 15: n = value - 15"""
    out = bytearray()
    while n >= 255:
        out.append(255)
        n -= 255
    out.append(n)
    return bytes(out)


def lz4_sequence(literals: bytes, offset=None, match_len=None) -> bytes:
    """one sequence; offset None: the last one (it ends after its literals)"""
    lit = len(literals)
    ml = 0 if offset is None else match_len - 4
    assert offset is None or (match_len >= 4 and 0 <= offset <= 65535)
    out = bytearray([(min(lit, 15) << 4) | min(ml, 15)])
    if lit >= 15:
        out += _length(lit - 15)
    out += literals
    if offset is not None:
        out += struct.pack("<H", offset)
        if ml >= 15:
            out += _length(ml - 15)
    return bytes(out)


def lz4_build(seqs) -> bytes:
    """a block of exactly the sequences [(literals, offset, match_len), ..., (literals, None, None)]"""
    assert seqs and seqs[-1][1] is None and all(s[1] is not None for s in seqs[:-1])
    return b"".join(lz4_sequence(*s) for s in seqs)


def lz4_expand(seqs) -> bytes:
    """what the sequences decode to, straight from their meaning (byte by byte: no decoder of the package is involved)"""
    out = bytearray()
    for literals, offset, match_len in seqs:
        out += literals
        if offset is not None:
            assert 1 <= offset <= len(out)
            for _ in range(match_len):
                out.append(out[-offset])
    return bytes(out)


def lz4_sequences(block: bytes):
    """[(literal length, offset or None, match length or None)] of a well-formed block"""
    out, sp, n = [], 0, len(block)
    while True:
        token = block[sp]
        sp += 1
        lit = token >> 4
        if lit == 15:
            while True:
                b = block[sp]
                sp += 1
                lit += b
                if b != 255:
                    break
        sp += lit
        if sp == n:
            out.append((lit, None, None))
            return out
        off = block[sp] | (block[sp + 1] << 8)
        sp += 2
        ml = token & 15
        if ml == 15:
            while True:
                b = block[sp]
                sp += 1
                ml += b
                if b != 255:
                    break
        out.append((lit, off, ml + 4))


def corrupt_block(defect):
    """(block, dst_len): a valid block with exactly one defect (the host and the kernel tests run the same ones)"""
    good = [(b"0123456789abcdef", 16, 40), (b"XYZ", 5, 12), (b"the end..", None, None)]
    dst_len = len(lz4_expand(good))
    if defect == "offset0":
        return lz4_sequence(b"0123456789abcdef", 0, 40) + lz4_build(good[1:]), dst_len
    if defect == "offset_far":
        return lz4_sequence(b"0123456789abcdef", 17, 40) + lz4_build(good[1:]), dst_len
    if defect == "literals":     # the last sequence announces 9 literals, 4 follow
        return lz4_build(good)[:-5], dst_len
    if defect == "extension":    # a match length whose extension bytes run into the end of the source
        return lz4_sequence(*good[0]) + bytes([0x1F]) + b"Q" + struct.pack("<H", 4) + b"\xff\xff", dst_len
    if defect == "match_past_dst":
        return lz4_build(good), dst_len - 10
    if defect == "early":
        return lz4_build(good), dst_len + 1
    raise KeyError(defect)


def lz4_compress(data: bytes) -> bytes:
    """greedy: the most recent earlier occurrence of the next 4 bytes (one table entry per hash), extended as far as it goes"""
    data = bytes(data)
    n = len(data)
    seqs, anchor, i = [], 0, 0
    table = {}
    limit = n - 12    # no match starts after this
    while i < limit:
        key = data[i:i + 4]
        cand = table.get(key)
        table[key] = i
        if cand is None or i - cand > 65535:
            i += 1
            continue
        ml = 4
        end = n - 5   # the last 5 bytes stay literals
        while i + ml < end and data[cand + ml] == data[i + ml]:
            ml += 1
        seqs.append((data[anchor:i], i - cand, ml))
        i += ml
        anchor = i
    seqs.append((data[anchor:], None, None))
    return lz4_build(seqs)


def blosc_frame(raw: bytes, blocksize: int, *, flags: int = FLAGS_LZ4, memcpyed: bool = False, compress=lz4_compress,
                typesize: int = 1, version: int = 2) -> bytes:
    """one Blosc 1 chunk.  A block is stored raw when `compress` does not shrink it; memcpyed: flag 0x02 and the raw bytes."""
    raw = bytes(raw)
    nbytes = len(raw)
    if memcpyed:
        return struct.pack("<BBBBIII", version, 1, flags | 0x02, typesize, nbytes, blocksize, 16 + nbytes) + raw
    nblocks = -(-nbytes // blocksize)
    body, bstarts = bytearray(), []
    pos = 16 + 4 * nblocks
    for b in range(nblocks):
        block = raw[b * blocksize:(b + 1) * blocksize]
        enc = compress(block)
        if len(enc) >= len(block):
            enc = block
        bstarts.append(pos)
        body += struct.pack("<i", len(enc)) + enc
        pos += 4 + len(enc)
    return struct.pack("<BBBBIII", version, 1, flags, typesize, nbytes, blocksize, pos) + struct.pack(f"<{nblocks}i", *bstarts) + bytes(body)


def blosc_raw_share(chunk: bytes) -> tuple:
    """(blocks stored raw, LZ4 blocks) of a framed chunk; a memcpyed chunk counts as one raw block"""
    flags, nbytes, blocksize = chunk[2], *struct.unpack_from("<II", chunk, 4)
    if flags & 0x02:
        return 1, 0
    nblocks = -(-nbytes // blocksize)
    raw = 0
    for b, bs in enumerate(struct.unpack_from(f"<{nblocks}i", chunk, 16)):
        raw += struct.unpack_from("<i", chunk, bs)[0] == min(blocksize, nbytes - b * blocksize)
    return raw, nblocks - raw


def blosc_members(a, chunks, *, blocksize, doc=None, frame=None, **kw):
    """{key: bytes} of one array whose compressor document is Blosc's and whose chunk values are framed by
    `frame(key, raw_chunk_bytes)` (default: blosc_frame at `blocksize`)"""
    members = ZW.array_members(a, chunks, compressor=dict(doc or BLOSC_DOC), **kw)
    frame = frame or (lambda key, raw: blosc_frame(raw, blocksize))
    return {k: (v if k.endswith(".zarray") else frame(k, v)) for k, v in members.items()}


CANARY = 0xA5


def decode_on_device(entries):
    """One yogo_blosc_lz4_decode launch over `entries` = [(stored bytes, dst_len, raw)].  Sources and destinations are packed at
    offsets of every alignment with gaps between them; the destination starts out as CANARY bytes.
    -> (status list, what each entry's destination range holds, True when every byte outside the ranges is still CANARY)"""
    import numpy as np
    import torch

    from yogo_amd.device_decode import decode_blocks

    rows, src, spos, dpos = [], bytearray(), 0, 16
    for i, (data, dst_len, raw) in enumerate(entries):
        pad = (5 * i + 3) % 16 if i % 4 else (16 - len(src) % 16) % 16    # every fourth source starts on a multiple of 16
        src += bytes([0x5A]) * pad
        soff = len(src)
        src += data
        doff = dpos + ((7 * i + 1) % 16 if i % 3 else 0)                   # every third destination likewise
        rows.append((soff, len(data), doff, dst_len, 1 if raw else 0))
        dpos = -(-(doff + dst_len + 16) // 16) * 16
    src += bytes([0x5A]) * 16
    dst = torch.full((dpos + 16,), CANARY, dtype=torch.uint8, device="cuda")
    status = torch.full((len(rows),), -1, dtype=torch.int32, device="cuda")
    decode_blocks(torch.frombuffer(src, dtype=torch.uint8).cuda(), torch.tensor(rows, dtype=torch.int64).reshape(-1, 5).cuda(), dst, status)
    host = dst.cpu().numpy()
    outside = np.ones(host.size, dtype=bool)
    got = []
    for _, _, doff, dst_len, _ in rows:
        outside[doff:doff + dst_len] = False
        got.append(host[doff:doff + dst_len].tobytes())
    return status.cpu().tolist(), got, bool((host[outside] == CANARY).all())
