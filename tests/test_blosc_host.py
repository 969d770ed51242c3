"""The host half of Blosc input (yogo_amd/blosc.py, yogo_amd/zarr_store.py): the pure-Python LZ4 block decoder against blocks
written by liblz4 (tests/golden/lz4_blocks.npz) and against liblz4 itself where it loads, the chunk parser's refusals, and a
Blosc-compressed store read without numcodecs."""
import ctypes
import os
import struct
import sys
import zlib

import numpy as np
import pytest

import _blosc_write as BW
import _zarr_write as ZW
from yogo_amd import blosc
from yogo_amd.zarr_store import open_zarr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lz4_blocks.npz")
NAMES = ["zeros", "period3", "low_entropy", "incompressible", "far_match"]


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {n: (z[n + "_c"].tobytes(), z[n + "_d"].tobytes()) for n in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_python_decoder_reproduces_the_liblz4_blocks(golden, name):
    comp, want = golden[name]
    assert blosc.lz4_block_decode(comp, len(want)) == want
    assert blosc.lz4_block_status(comp, len(want))[0] == blosc.LZ4_OK


def test_the_fixtures_hold_what_they_are_named_after(golden):
    far = BW.lz4_sequences(golden["far_match"][0])
    assert max(o or 0 for _, o, _ in far) > 65000
    assert BW.lz4_sequences(golden["incompressible"][0]) == [(2048, None, None)]
    assert any(o == 3 and m > 3 for _, o, m in BW.lz4_sequences(golden["period3"][0]))   # a periodic match
    assert any(o == 1 and m > 64 for _, o, m in BW.lz4_sequences(golden["zeros"][0]))


@pytest.mark.parametrize("name", NAMES)
def test_writer_round_trips(golden, name):
    want = golden[name][1]
    mine = BW.lz4_compress(want)
    assert blosc.lz4_block_decode(mine, len(want)) == want
    if name != "incompressible":
        assert len(mine) < len(want) and any(o is not None for _, o, _ in BW.lz4_sequences(mine))
    seqs = [(b"abcdefgh", 8, 20), (b"", 3, 4), (b"xy" * 20, 1, 300), (b"tail!", None, None)]
    assert blosc.lz4_block_decode(BW.lz4_build(seqs), len(BW.lz4_expand(seqs))) == BW.lz4_expand(seqs)
    assert BW.lz4_sequences(BW.lz4_build(seqs)) == [(8, 8, 20), (0, 3, 4), (40, 1, 300), (5, None, None)]


@pytest.mark.skipif(blosc.liblz4() is None, reason="liblz4 is not installed")
@pytest.mark.parametrize("name", NAMES)
def test_both_directions_agree_with_liblz4(golden, name):
    L = blosc.liblz4()
    want = golden[name][1]
    cap = L.LZ4_compressBound(len(want))
    buf = ctypes.create_string_buffer(cap)
    n = L.LZ4_compress_default(want, buf, len(want), cap)
    assert n > 0 and blosc.lz4_block_decode(buf.raw[:n], len(want)) == want          # liblz4 compresses, ours decodes
    mine = BW.lz4_compress(want)
    back = ctypes.create_string_buffer(len(want))
    assert L.LZ4_decompress_safe(mine, back, len(mine), len(want)) == len(want) and back.raw == want   # ours compresses, liblz4 decodes


def test_decompress_uses_either_block_decoder(golden, monkeypatch):
    raw = golden["low_entropy"][1] + golden["incompressible"][1] + golden["zeros"][1][:100]
    chunk = BW.blosc_frame(raw, 1000)
    assert min(BW.blosc_raw_share(chunk)) > 0
    assert blosc.decompress(chunk, len(raw)) == raw
    monkeypatch.setattr(blosc, "liblz4", lambda: None)
    assert blosc.decompress(chunk, len(raw)) == raw
    assert blosc.decompress(BW.blosc_frame(raw, 1000, memcpyed=True), len(raw)) == raw
    zl = BW.blosc_frame(raw, 1000, flags=0x01 | (3 << 5), compress=lambda b: zlib.compress(b, 1))
    assert blosc.decompress(zl, len(raw)) == raw


@pytest.mark.parametrize("defect,code", [
    ("offset0", blosc.LZ4_BAD_OFFSET), ("offset_far", blosc.LZ4_BAD_OFFSET), ("literals", blosc.LZ4_LITERALS_PAST_SOURCE),
    ("extension", blosc.LZ4_SOURCE_ENDS_IN_SEQUENCE), ("match_past_dst", blosc.LZ4_PAST_DESTINATION), ("early", blosc.LZ4_ENDS_EARLY)])
def test_python_decoder_names_each_defect(defect, code):
    block, dst_len = BW.corrupt_block(defect)
    status, _ = blosc.lz4_block_status(block, dst_len)
    assert status == code
    with pytest.raises(ValueError, match=f"status {code}") as e:
        blosc.lz4_block_decode(block, dst_len)
    assert e.value.status == code


def test_parse_chunk_lists_the_blocks(golden):
    raw = golden["low_entropy"][1][:2500]
    chunk = BW.blosc_frame(raw, 1000)
    flags, entries = blosc.parse_chunk(chunk, 2500)
    assert flags == BW.FLAGS_LZ4 and [(e[2], e[3], e[4]) for e in entries] == [(0, 1000, 0), (1000, 1000, 0), (2000, 500, 0)]
    assert b"".join(blosc.lz4_block_decode(chunk[so:so + sl], dl) for so, sl, _, dl, _ in entries) == raw
    flags, entries = blosc.parse_chunk(BW.blosc_frame(raw, 1000, memcpyed=True), 2500)
    assert flags & blosc.FLAG_MEMCPYED and entries == [(16, 2500, 0, 2500, 1)]
    assert blosc.device_decodable(flags) and blosc.device_decodable(BW.FLAGS_LZ4)
    assert not blosc.device_decodable(0x01 | (3 << 5)) and not blosc.device_decodable(BW.FLAGS_LZ4 | blosc.FLAG_BITSHUFFLE)


def test_parse_chunk_refuses_each_malformed_header(golden):
    raw = golden["low_entropy"][1][:2500]
    good = BW.blosc_frame(raw, 1000)

    def patched(at, fmt, value):
        b = bytearray(good)
        struct.pack_into(fmt, b, at, value)
        return bytes(b)

    bstart1 = struct.unpack_from("<i", good, 20)[0]
    for chunk, expect, msg in [
        (good[:10], 2500, "shorter than the 16-byte header"),
        (patched(0, "<B", 3), 2500, "format version 3"),
        (good, 2501, "nbytes 2500, 2501 expected"),
        (good + b"\0", 2500, "cbytes"),
        (patched(8, "<I", 0), 2500, "blocksize 0"),
        (patched(20, "<i", len(good) - 2), 2500, "bstart"),
        (patched(20, "<i", 4), 2500, "bstart"),
        (patched(bstart1, "<i", 0), 2500, "csize 0"),
        (patched(bstart1, "<i", 1001), 2500, "csize 1001"),
        (patched(struct.unpack_from("<i", good, 24)[0], "<i", 499), 2500, "passes the end"),   # the last block, longer than what is left
        (patched(8, "<I", 1), 2500, "table of 2500 block starts"),
        (BW.blosc_frame(raw, 1000, memcpyed=True)[:-1], 2500, "cbytes"),
    ]:
        with pytest.raises(ValueError, match=msg):
            blosc.parse_chunk(chunk, expect)


def test_unsupported_chunks_name_what_was_found(golden):
    raw = golden["zeros"][1]
    with pytest.raises(NotImplementedError, match="bit-shuffle"):
        blosc.decompress(BW.blosc_frame(raw, 1000, flags=BW.FLAGS_LZ4 | 0x04), len(raw))
    with pytest.raises(NotImplementedError, match=r"inner format 4 \(zstd\)"):
        blosc.decompress(BW.blosc_frame(raw, 1000, flags=0x01 | (4 << 5)), len(raw))
    with pytest.raises(NotImplementedError, match=r"inner format 6 \(unknown\)"):
        blosc.decompress(BW.blosc_frame(raw, 1000, flags=0x01 | (6 << 5)), len(raw))
    with pytest.raises(NotImplementedError, match="typesize 4"):
        blosc.decompress(BW.blosc_frame(raw, 1000, typesize=4), len(raw))


def _stack():
    rng = np.random.default_rng(11)
    s = rng.integers(0, 4, size=(24, 48, 7), dtype=np.uint8) * 60        # LZ4 shrinks these frames
    s[:, :, 2] = rng.integers(0, 256, size=(24, 48), dtype=np.uint8)     # ... and not this one
    return s


@pytest.mark.parametrize("as_zip", [False, True], ids=["dir", "zip"])
@pytest.mark.parametrize("chunks", [(24, 48, 1), (24, 48, 3)], ids=["cn1", "cn3"])
def test_blosc_store_opens_without_numcodecs(tmp_path, monkeypatch, chunks, as_zip):
    monkeypatch.setitem(sys.modules, "numcodecs", None)   # `import numcodecs` raises ImportError
    stack = _stack()
    absent = (0, 0, 1)
    members = BW.blosc_members(stack, chunks, blocksize=500, fill_value=9, skip=[absent])
    kinds = [BW.blosc_raw_share(v) for k, v in members.items() if not k.endswith(".zarray")]
    assert sum(r for r, _ in kinds) > 0 and sum(c for _, c in kinds) > 0   # raw and LZ4 blocks both occur
    p = ZW.write_members(tmp_path / ("s.zip" if as_zip else "s.zarr"), members, as_zip=as_zip)
    a = open_zarr(p)
    assert a.device_decodable and not a.raw
    want = stack.copy()
    want[:, :, chunks[2]:2 * chunks[2]] = 9
    for i in range(7):
        assert np.array_equal(a.frame(i), want[:, :, i]), i
    # the stored bytes as they are
    buf = np.zeros(a.chunk_nbytes + 4096, np.uint8)
    got = a.read_stored_into((0, 0, 0), buf)
    assert bytes(buf[:got]) == members["0.0.0"]
    with pytest.raises(KeyError):
        a.read_stored_into(absent, buf)


def test_device_decodable_query(tmp_path):
    stack = _stack()
    for doc, want in [({"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1, "blocksize": 0}, True),
                      ({"id": "blosc", "cname": "lz4hc", "clevel": 5, "shuffle": 0, "blocksize": 0}, True),
                      ({"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 2, "blocksize": 0}, False),
                      ({"id": "blosc", "cname": "zstd", "clevel": 5, "shuffle": 1, "blocksize": 0}, False)]:
        p = ZW.write_members(tmp_path / f"{doc['cname']}{doc['shuffle']}.zarr", BW.blosc_members(stack, (24, 48, 1), blocksize=500, doc=doc))
        assert open_zarr(p).device_decodable is want
    assert open_zarr(ZW.write_stack(tmp_path / "z.zarr", stack, (24, 48, 1), compressor="zlib")).device_decodable is False
    assert open_zarr(ZW.write_stack(tmp_path / "r.zarr", stack, (24, 48, 1))).device_decodable is False


def test_stager_table_decodes_to_what_the_host_route_stages(tmp_path, monkeypatch):
    """the host half of the device route (ChunkStager.stage_stored): its table, applied here with the Python decoder, fills the
    staging buffer exactly as the host route does -- LZ4 and raw blocks, a memcpyed chunk cut into pieces, a zlib-inside chunk
    decoded on the host, and a chunk taken over from the previous batch"""
    from yogo_amd.zarr_feed import RAW_PIECE, ChunkStager, FrameSource, plan_batch

    monkeypatch.setitem(sys.modules, "numcodecs", None)
    rng = np.random.default_rng(4)
    stack = (rng.integers(0, 3, size=(300, 300, 6), dtype=np.uint8) * 100)
    stack[150:, :, :] = rng.integers(0, 256, size=(150, 300, 6), dtype=np.uint8)
    n = 300 * 300 * 2
    assert n > RAW_PIECE

    def frame(key, raw):
        if key == "0.0.0":
            return BW.blosc_frame(raw, 32768, memcpyed=True)
        if key == "0.0.1":
            return BW.blosc_frame(raw, 32768, flags=0x01 | (3 << 5), compress=lambda b: zlib.compress(b, 1))
        return BW.blosc_frame(raw, 32768)

    p = ZW.write_members(tmp_path / "s.zarr", BW.blosc_members(stack, (300, 300, 2), blocksize=32768, frame=frame))
    src = FrameSource(open_zarr(p))
    stager = ChunkStager(src, threads=2)
    try:
        prev, kinds = None, []
        for lo, hi in ((0, 3), (3, 6)):     # chunk 0.0.1 (frames 2, 3) is shared
            plan = plan_batch(src, lo, hi)
            want = np.zeros(plan.nbytes, np.uint8)
            stager.stage(plan, want)
            sbuf = np.zeros(len(plan.keys) * src.stored_stride, np.uint8)
            table = stager.stage_stored(plan, sbuf, prev)
            got = np.full(plan.nbytes, 0xEE, np.uint8)
            for so, sl, do, dl, raw in table.tolist():
                data = bytes(sbuf[so:so + sl])
                got[do:do + dl] = np.frombuffer(data if raw else blosc.lz4_block_decode(data, dl), np.uint8)
            used = np.zeros(plan.nbytes, bool)
            for k in plan.keys:
                used[plan.offsets[k]:plan.offsets[k] + n] = True
            assert np.array_equal(got[used], want[used]) and (got[~used] == 0xEE).all()
            assert len(plan.row_chunk) == len(table) and table[:, 1].max() <= max(RAW_PIECE, 32768)
            kinds += table[:, 4].tolist()
            prev = (plan, sbuf)
        assert 0 in kinds and 1 in kinds      # LZ4 and raw rows both occurred
        assert stager.reads["0.0.1"] == 3     # twice by the host route above (no `prev` there), once by the device route
    finally:
        stager.close()


def test_an_incomplete_blosc_document_is_left_to_numcodecs(tmp_path, monkeypatch):
    """only a document with every key numcodecs writes is read here; the defaults of a shorter one are numcodecs' to choose"""
    monkeypatch.setitem(sys.modules, "numcodecs", None)
    doc = {k: v for k, v in BW.BLOSC_DOC.items() if k != "blocksize"}
    p = ZW.write_members(tmp_path / "s.zarr", BW.blosc_members(_stack(), (24, 48, 1), blocksize=500, doc=doc))
    with pytest.raises(NotImplementedError, match="numcodecs"):
        open_zarr(p)
