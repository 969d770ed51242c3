"""The host half of Zstandard input (yogo_amd/zstd.py, yogo_amd/blosc.py, yogo_amd/zarr_store.py): the pure-Python frame decoder
against frames written by libzstd (tests/golden/zstd_frames.npz), against the hand-written frames of tests/_zstd_write.py and
against libzstd itself where it loads; one status per defect; a mutation fuzz; Blosc-zstd and zstd-codec stores read without
numcodecs."""
import sys

import numpy as np
import pytest

import _blosc_write as BW
import _zarr_write as ZW
import _zstd_write as W
from yogo_amd import blosc
from yogo_amd import zstd as Z
from yogo_amd.zarr_store import open_zarr

GOLDEN = W.golden_frames()
HAND = W.hand_written()
# what tests/golden/make_zstd_frames.py guarantees of the library's frames (it fails where libzstd stops producing one of them) ...
GOLDEN_FEATURES = {"raw_block", "rle_block", "raw_literals", "ll_table_predefined", "of_table_predefined", "ml_table_predefined",
                   "huffman_4_streams", "huffman_direct_weights", "huffman_fse_weights", "zero_sequences", "huffman_1_stream",
                   "several_blocks", "treeless_literals", "ll_table_fse", "of_table_fse", "ml_table_fse", "compressed_block"}
# ... and everything the decoder reads
ALL_FEATURES = GOLDEN_FEATURES | {
    "rle_literals", "window_descriptor", "frame_content_size", "content_checksum",
    "ll_table_rle", "of_table_rle", "ml_table_rle", "ll_table_repeat", "of_table_repeat", "ml_table_repeat",
    "repeat_offset_1", "repeat_offset_2", "repeat_offset_3", "repeat_offset_1_ll0", "repeat_offset_2_ll0", "repeat_offset_3_ll0",
    "overlapping_match", "offset_1_match_over_64", "match_into_earlier_block", "offset_code_17_or_more", "huffman_11_bit_code",
    "accuracy_log_at_limit_6", "accuracy_log_at_limit_8", "accuracy_log_at_limit_9", "less_than_one_probability"}


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_python_decoder_reproduces_the_libzstd_frames(name):
    comp, want = GOLDEN[name]
    status, out = Z.zstd_frame_status(comp, len(want))
    assert status == Z.ZSTD_OK and out == want
    if name == "sentence":
        assert Z.zstd_decode(comp, len(want)) == want


@pytest.mark.parametrize("name", sorted(HAND))
def test_python_decoder_reproduces_the_hand_written_frames(name):
    comp, want = HAND[name]
    status, out = Z.zstd_frame_status(comp, len(want))
    assert status == Z.ZSTD_OK and out == want


def test_the_frames_hold_every_feature_the_decoder_reads():
    golden = set().union(*(W.features(c, len(d)) for c, d in GOLDEN.values()))
    assert GOLDEN_FEATURES <= golden, sorted(GOLDEN_FEATURES - golden)
    assert any(f.endswith("_table_repeat") for f in golden)
    both = golden.union(*(W.features(c, len(d)) for c, d in HAND.values()))
    assert ALL_FEATURES <= both, sorted(ALL_FEATURES - both)
    hand = set().union(*(W.features(c, len(d)) for c, d in HAND.values()))
    assert {"ll_table_rle", "rle_literals", "huffman_11_bit_code", "accuracy_log_at_limit_6", "accuracy_log_at_limit_8",
            "accuracy_log_at_limit_9", "less_than_one_probability", "offset_1_match_over_64", "match_into_earlier_block"} <= hand


@pytest.mark.parametrize("defect", W.DEFECTS)
def test_python_decoder_names_each_defect(defect):
    comp, n, code, truth = W.corrupt_frame(defect)
    status, out = Z.zstd_frame_status(comp, n)
    assert status == code != Z.ZSTD_OK
    assert truth.startswith(out) or (not truth and not out)
    with pytest.raises(ValueError, match=f"status {code}") as e:
        Z.zstd_decode(comp, n)
    assert e.value.status == code and isinstance(e.value, Z.ZstdError)


def test_every_status_has_a_defect_and_a_text():
    reached = {W.corrupt_frame(d)[2] for d in W.DEFECTS}
    assert reached == set(Z.ZSTD_STATUS) - {Z.ZSTD_BAD_ROW}     # (a row outside the buffers is the kernel's alone)
    assert sorted(Z.ZSTD_STATUS) == list(range(1, 16))


def test_single_byte_mutations_end_in_a_status_or_in_bytes():
    """fixed seed; the decoder returns (status, bytes), never another exception, and never more than dst_len bytes -- every loop of
    it consumes source bits or counts down a length checked against the source or dst_len; where libzstd loads and both accept, the
    bytes agree"""
    rng = np.random.default_rng(1234)
    frames = [GOLDEN[n] for n in ("sentence", "text", "noisy_frame")] + [HAND[n] for n in ("rle_literals", "repeat_ll0", "rle_tables",
                                                                                          "fse_at_limits", "huffman_11_bits", "huffman_fse_weights_limit")]
    lib = Z.libzstd()
    accepted = compared = 0
    for i in range(3000):
        comp, want = frames[i % len(frames)]
        b = bytearray(comp)
        at = int(rng.integers(0, min(len(b), 400) if i % 3 else len(b)))     # (two in three land in the headers and tables)
        b[at] ^= 1 << int(rng.integers(0, 8)) if i % 2 else int(rng.integers(1, 256))
        status, out = Z.zstd_frame_status(bytes(b), len(want))
        assert 0 <= status <= 15 and len(out) <= len(want)
        if status == 0:
            accepted += 1
            assert len(out) == len(want)
            if lib is not None and not (b[4] & 0x04):     # (a frame with a content checksum: the library verifies it, the decoder here does not)
                try:
                    theirs = Z.lib_decode(bytes(b), len(want))
                except ValueError:
                    continue
                compared += 1
                assert theirs == out, (i, at)
    assert accepted > 0 and (lib is None or compared > 0)


@pytest.mark.skipif(Z.libzstd() is None, reason="libzstd is not installed")
def test_both_directions_agree_with_libzstd():
    rng = np.random.default_rng(8)
    for data in [b"", b"abc", bytes(1000), rng.integers(0, 4, 20000, dtype=np.uint8).tobytes(), b"hello world, " * 20000,
                 rng.integers(0, 100, 3000, dtype=np.uint8).tobytes(), GOLDEN["noisy_frame"][1]]:
        assert Z.lib_decode(W.compress(data), len(data)) == data                   # ours compresses, libzstd decodes
        for level in (1, 19):
            assert Z.zstd_decode(Z.lib_compress(data, level), len(data)) == data   # libzstd compresses, ours decodes
    for name, (comp, want) in HAND.items():
        if "content_checksum" not in W.features(comp, len(want)):                  # (the writer's checksum bytes are not one)
            assert Z.lib_decode(comp, len(want)) == want, name


def test_blosc_decompress_reads_format_4_only_with_a_frame_decoder():
    raw = GOLDEN["noisy_frame"][1]
    chunk = BW.blosc_frame(raw, 1000, flags=W.FLAGS_ZSTD, compress=W.compress)
    with pytest.raises(NotImplementedError, match=r"inner format 4 \(zstd\)"):
        blosc.decompress(chunk, len(raw))
    assert blosc.decompress(chunk, len(raw), zstd=Z.zstd_decode) == raw
    assert blosc.decompress(chunk, len(raw), zstd=Z.frame_decoder()) == raw
    flags, _ = blosc.parse_chunk(chunk, len(raw))
    assert blosc.device_decodable_zstd(flags) and not blosc.device_decodable(flags)
    assert not blosc.device_decodable_zstd(flags | blosc.FLAG_BITSHUFFLE) and not blosc.device_decodable_zstd(BW.FLAGS_LZ4)
    assert blosc.device_decodable_zstd(BW.FLAGS_LZ4 | blosc.FLAG_MEMCPYED)


@pytest.mark.parametrize("python_decoder", [False, True], ids=["frame_decoder", "pure-python"])
@pytest.mark.parametrize("as_zip", [False, True], ids=["dir", "zip"])
@pytest.mark.parametrize("kind", ["blosc-zstd", "zstd"])
def test_zstd_stores_open_without_numcodecs(tmp_path, monkeypatch, kind, as_zip, python_decoder):
    monkeypatch.setitem(sys.modules, "numcodecs", None)   # `import numcodecs` raises ImportError
    if python_decoder:
        monkeypatch.setattr(Z, "libzstd", lambda: None)
    stack = W.store_stack()
    encode = W.library_encoder()
    ext = ".zip" if as_zip else ".zarr"
    # an [H, W, N] array, one frame per chunk: libzstd's own frames, a memcpyed chunk, raw blocks (the noise frame), an absent chunk
    members = W.zstd_members(stack, (48, 64, 1), kind, encode=encode, memcpyed={"0.0.1"}, fill_value=9, skip=[(0, 0, 4)])
    assert encode.used["library"] >= 4
    if kind == "blosc-zstd":
        kinds = [BW.blosc_raw_share(v) for k, v in members.items() if not k.endswith(".zarray")]
        assert sum(r for r, _ in kinds) > 1 and sum(c for _, c in kinds) > 0 and members["0.0.1"][2] & 0x02
    a = open_zarr(ZW.write_members(tmp_path / ("a" + ext), members, as_zip=as_zip))
    raw = open_zarr(ZW.write_stack(tmp_path / ("raw" + ext), stack, (48, 64, 1), as_zip=as_zip, fill_value=9, skip=[(0, 0, 4)]))
    assert a.device_codec == kind and a.device_decodable is False and not a.raw
    for i in range(8):
        assert np.array_equal(a.frame(i), raw.frame(i)), i
    assert np.array_equal(a.frame(4), np.full((48, 64), 9, np.uint8)) and np.array_equal(a.frame(0), stack[:, :, 0])
    # three frames per chunk, tiles of 32 x 40
    b = open_zarr(ZW.write_members(tmp_path / ("b" + ext), W.zstd_members(stack, (32, 40, 3), kind, encode=encode), as_zip=as_zip))
    for i in range(8):
        assert np.array_equal(b.frame(i), stack[:, :, i]), i
    # a group of 2-D members
    g = open_zarr(ZW.write_members(tmp_path / ("g" + ext), W.zstd_group_members([stack[:, :, i] for i in range(3)], (48, 64), kind, encode=encode),
                                   as_zip=as_zip))
    assert len(g) == 3 and g[0].device_codec == kind
    for i in range(3):
        assert np.array_equal(g[i][:], stack[:, :, i])


def test_a_corrupt_zstd_chunk_names_its_key(tmp_path, monkeypatch):
    monkeypatch.setitem(sys.modules, "numcodecs", None)
    stack = W.store_stack()
    members = W.zstd_members(stack, (48, 64, 1), "zstd", encode=W.library_encoder(), replace={"0.0.2": lambda f: f[:-9]})
    a = open_zarr(ZW.write_members(tmp_path / "s.zarr", members))
    assert np.array_equal(a.frame(1), stack[:, :, 1])
    with pytest.raises(RuntimeError, match=r"0\.0\.2"):
        a.frame(2)


def test_the_zstd_codec_goes_to_the_host_by_default():
    """profiles/zstd_feed.log: one frame per chunk is one wavefront per chunk, which lost to the host's 16 threads"""
    from yogo_amd import zarr_feed

    assert zarr_feed.DEVICE_DECODE_ZSTD is False and zarr_feed.DEVICE_DECODE_ZLIB is False


@pytest.mark.parametrize("kind", ["blosc-zstd", "zstd"])
def test_stager_table_decodes_to_what_the_host_route_stages(tmp_path, monkeypatch, kind):
    """the host half of the device route (ChunkStager.stage_stored): its table, applied here with the Python decoder, fills the
    staging buffer exactly as the host route does -- libzstd's frames, raw blocks (the noise frame), a memcpyed chunk"""
    from yogo_amd.zarr_feed import ChunkStager, FrameSource, plan_batch

    monkeypatch.setitem(sys.modules, "numcodecs", None)
    stack = W.store_stack()
    members = W.zstd_members(stack, (48, 64, 1), kind, encode=W.library_encoder(), memcpyed={"0.0.1"})
    src = FrameSource(open_zarr(ZW.write_members(tmp_path / "s.zarr", members)))
    assert src.first.device_codec == kind
    stager = ChunkStager(src, threads=2)
    try:
        prev, kinds = None, []
        for lo, hi in ((0, 3), (3, 8)):
            plan = plan_batch(src, lo, hi)
            want = np.zeros(plan.nbytes, np.uint8)
            stager.stage(plan, want)
            sbuf = np.zeros(len(plan.keys) * src.stored_stride, np.uint8)
            table = stager.stage_stored(plan, sbuf, prev)
            got = np.full(plan.nbytes, 0xEE, np.uint8)
            for so, sl, do, dl, raw in table.tolist():
                data = bytes(sbuf[so:so + sl])
                got[do:do + dl] = np.frombuffer(data if raw else Z.zstd_decode(data, dl), np.uint8)
            used = np.zeros(plan.nbytes, bool)
            for k in plan.keys:
                used[plan.offsets[k]:plan.offsets[k] + src.chunk_nbytes] = True
            assert np.array_equal(got[used], want[used]) and (got[~used] == 0xEE).all()
            assert len(plan.row_chunk) == len(table)
            kinds += table[:, 4].tolist()
            prev = (plan, sbuf)
        assert 0 in kinds and (kind == "zstd" or 1 in kinds)
    finally:
        stager.close()
