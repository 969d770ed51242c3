"""The host plumbing of the device-decode routes, without a GPU: the scanline-buffer layout and the tables of a PNG batch
(yogo_amd/png_batch.py), the stager's table of a store under the zlib codec and the registry of the zarr feed's device codecs
(yogo_amd/zarr_feed.py)."""
import inspect
import re
import sys
import zlib
from operator import attrgetter

import numpy as np
import pytest

import _deflate_write as DW
import _png_types_write as TW
import _zarr_write as ZW
from yogo_amd import inflate, png


def test_scan_layout_aligns_the_images_and_puts_the_palettes_behind_them():
    from yogo_amd.png_batch import SCAN_ALIGN, scan_layout

    assert SCAN_ALIGN == 16 and png.PALETTE_BYTES == 768
    lay = scan_layout([1, 16, 17], [0, 2])
    assert lay.at.tolist() == [0, 16, 32, 64] and lay.need == [1, 16, 17]
    assert all(a % 16 == 0 for a in lay.at.tolist())
    assert all(lay.at[i] + lay.need[i] <= lay.at[i + 1] for i in range(3))         # in order and without overlap
    assert lay.palette_at == {0: 64, 2: 64 + 768} and lay.total == 64 + 2 * 768    # 768 bytes each, directly behind the last image
    assert scan_layout([1, 16, 17]).total == 64 and scan_layout([1, 16, 17]).palette_at == {}
    lay = scan_layout([], [0])
    assert lay.at.tolist() == [0] and lay.palette_at == {0: 0} and lay.total == 768 and lay.need == []
    assert scan_layout([]).total == 0


def _stream_of(data):
    info = png.parse_png(data)
    return b"".join(data[o:o + n] for o, n in info.idat)


def test_the_table_builders_of_a_three_image_batch():
    """one 8-bit grey file, one image the host decoded, one palette file: the inflate rows and the three unpack tables, written out"""
    from yogo_amd.device_decode import ALIGN, png_unpack, png_unpack_any, png_unpack_planes
    from yogo_amd.png_batch import PngStream, Refused, batch_layout, inflate_rows, read_stream, slot_layout, unpack_table

    rng = np.random.default_rng(5)
    H, W = 3, 5
    grey, _, _ = TW.make_png(rng, H, W, 0, 8)
    pal, _, palette = TW.make_png(rng, H, W, 3, 8, plte_entries=7)
    rgb, _, _ = TW.make_png(rng, H, W, 2, 8)
    streams = [_stream_of(grey), None, _stream_of(pal)]
    src_at, slot_bytes = slot_layout([len(grey), 0, len(pal)])
    assert ALIGN == 256 and src_at.tolist() == [0, 256 * -(-len(grey) // 256), 256 * -(-len(grey) // 256)]
    slot = np.full(slot_bytes, 0xEE, np.uint8)
    any_png = attrgetter("any_decodable")
    records = [read_stream(grey, slot[:len(grey)], any_png),
               PngStream((H, W), host=True, pixels=np.arange(H * W, dtype=np.uint8).reshape(H, W)),
               read_stream(pal, slot[int(src_at[2]):int(src_at[2]) + len(pal)], any_png)]
    assert [(r.hw, r.host, r.stored, r.need) for r in records] == [((3, 5), False, len(streams[0]), 18), ((3, 5), True, 0, 0),
                                                                   ((3, 5), False, len(streams[2]), 18)]
    assert [r.code for r in records] == [0 | 8 << 8, png.FMT_PLANAR, 3 | 8 << 8] and [r.bpp for r in records] == [1, 1, 1]
    assert records[0].palette is None and records[2].palette.tolist() == palette.reshape(-1).tolist() + [0] * (768 - 21)
    assert slot[:len(streams[0])].tobytes() == streams[0] and slot[int(src_at[2]):int(src_at[2]) + len(streams[2])].tobytes() == streams[2]
    for r, s in zip(records, streams):
        if s is not None:
            assert (r.deflate, r.adler) == ((2, len(s) - 6), zlib.adler32(zlib.decompress(s))) and r.stream is None and r.pixels is None

    lay = batch_layout(records, 1 * H * W)
    assert lay.at.tolist() == [0, 32, 48, 80] and lay.need == [18, 15, 18] and lay.palette_at == {2: 80} and lay.total == 80 + 768
    assert inflate_rows(records, src_at, lay).tolist() == [
        [0 + 2, len(streams[0]) - 6, 0, 18, records[0].adler],
        [int(src_at[2]) + 2, len(streams[2]) - 6, 48, 18, records[2].adler]]
    assert unpack_table(png_unpack_any, records, lay).tolist() == [[0, 2048, 0], [32, 1, 0], [48, 2051, 80]]
    assert unpack_table(png_unpack_any, records, lay, rows=[2]).tolist() == [[48, 2051, 80]]
    assert unpack_table(png_unpack_any, records, lay, refused={0, 1}).tolist() == [[0, -1, 0], [32, -1, 0], [48, 2051, 80]]
    assert unpack_table(png_unpack, records[:2], lay).tolist() == [[0, 0], [32, 1]]                    # (offset, raw)
    colour = read_stream(rgb, np.zeros(len(rgb), np.uint8), attrgetter("prefill_decodable"))
    assert colour.bpp == 3 and colour.need == H * (1 + 3 * W)
    three = [records[0], records[1], colour]
    lay3 = batch_layout(three, 3 * H * W)
    assert lay3.at.tolist() == [0, 32, 80, 128] and lay3.palette_at == {} and lay3.total == 128
    assert unpack_table(png_unpack_planes, three, lay3).tolist() == [[0, 0], [32, 1], [80, 2]]           # (offset, kind)
    assert unpack_table(png_unpack_planes, three, lay3, refused={2}).tolist() == [[0, 0], [32, 1], [80, -1]]
    assert unpack_table(png_unpack_planes, [], batch_layout([], 0)).shape == (0, 2) and inflate_rows([], [], batch_layout([], 0)).shape == (0, 5)

    # what the predicate does not accept, and what is longer than its room, is refused before anything is copied
    room = np.full(len(pal), 0xEE, np.uint8)
    for data, accept, space in ((pal, attrgetter("prefill_decodable"), room), (pal, any_png, room[:len(streams[2]) - 1])):
        with pytest.raises(Refused):
            read_stream(data, space, accept)
        assert bool((room == 0xEE).all())
    kept = read_stream(pal, None, any_png)      # no room yet: the record keeps the stream
    assert kept.stream == streams[2] and (kept.stored, kept.deflate, kept.adler) == (records[2].stored, records[2].deflate, records[2].adler)


def test_zlib_stager_table_decodes_to_what_the_host_route_stages(tmp_path, monkeypatch):
    """the host half of the zlib codec's device route (ChunkStager.stage_stored): one coded row per chunk, the fifth field its
    Adler-32; a chunk whose wrapper ``split_zlib`` refuses (a preset dictionary, which the store's host decoder is given here) and a
    chunk longer than the room of a stored chunk arrive as raw rows, flagged raw, behind the coded ones"""
    from yogo_amd.zarr_feed import ChunkStager, FrameSource, plan_batch
    from yogo_amd.zarr_store import open_zarr

    monkeypatch.setitem(sys.modules, "numcodecs", None)
    rng = np.random.default_rng(9)
    stack = rng.integers(0, 4, size=(24, 48, 3), dtype=np.uint8) * 60
    members = ZW.array_members(stack, (24, 48, 1), compressor="zlib")
    raws = [stack[:, :, k].tobytes() for k in range(3)]
    zdict = bytes(range(64))
    c = zlib.compressobj(1, zdict=zdict)
    members["0.0.1"] = c.compress(raws[1]) + c.flush()
    w = DW.Bits()
    for at in range(0, len(raws[2]), 2):          # stored blocks of two bytes: seven stored bytes for two
        DW.stored(w, raws[2][at:at + 2], final=at + 2 >= len(raws[2]))
    members["0.0.2"] = DW.zlib_wrap(w.bytes(), raws[2])
    assert zlib.decompress(members["0.0.2"]) == raws[2]
    with pytest.raises(ValueError, match="preset dictionary"):
        inflate.split_zlib(members["0.0.1"])
    root = open_zarr(ZW.write_members(tmp_path / "s.zarr", members))
    plain = root._decode
    root._decode = lambda data: plain(data) if not data[1] & 0x20 else zlib.decompressobj(zdict=zdict).decompress(data)
    src = FrameSource(root)
    assert src.first.device_codec == "zlib" and len(members["0.0.2"]) > src.stored_stride
    stager = ChunkStager(src, threads=2)
    try:
        plan = plan_batch(src, 0, 3)
        want = np.zeros(plan.nbytes, np.uint8)
        stager.stage(plan, want)
        sbuf = np.zeros(len(plan.keys) * src.stored_stride, np.uint8)
        table = stager.stage_stored(plan, sbuf)
    finally:
        stager.close()
    n = src.chunk_nbytes
    assert table.dtype == np.int64 and table.shape == (3, 5) and len(plan.row_chunk) == 3 and plan.row_raw.tolist() == [False, True, True]
    assert [plan.keys[i] for i in plan.row_chunk] == ["0.0.0", "0.0.1", "0.0.2"]
    got = np.full(plan.nbytes, 0xEE, np.uint8)
    for (so, sl, do, dl, fifth), raw, owner in zip(table.tolist(), plan.row_raw, plan.row_chunk):
        if raw:
            assert fifth == 1 and sl == dl == n
            got[do:do + dl] = sbuf[so:so + sl]
        else:
            assert fifth == zlib.adler32(raws[owner]) and (so, sl) == (owner * src.stored_stride + 2, len(members[plan.keys[owner]]) - 6)
            status, data = inflate.inflate_status(bytes(sbuf[so:so + sl]), dl, fifth)
            assert status == inflate.INF_OK
            got[do:do + dl] = np.frombuffer(data, np.uint8)
    used = np.zeros(plan.nbytes, bool)
    for k in plan.keys:
        used[plan.offsets[k]:plan.offsets[k] + n] = True
    assert np.array_equal(got[used], want[used]) and (got[~used] == 0xEE).all()
    assert np.array_equal(want[used].reshape(3, 24, 48), stack.transpose(2, 0, 1))


def test_every_device_codec_has_its_record():
    from yogo_amd import zarr_feed
    from yogo_amd.zarr_store import ZarrArray

    names = set(re.findall(r'return "([\w-]+)"', inspect.getsource(ZarrArray.device_codec.fget)))
    assert names == {"blosc", "zlib", "blosc-zstd", "zstd"} == set(zarr_feed.CODECS)
    on = {k: (c.default_on, c.on()) for k, c in zarr_feed.CODECS.items()}
    assert on == {"blosc": (True, True), "blosc-zstd": (True, True), "zlib": (False, False), "zstd": (False, False)}
    assert [k for k, c in zarr_feed.CODECS.items() if c.copies_raw] == ["blosc"]
    assert {k for k, c in zarr_feed.CODECS.items() if c.workspace} == {"blosc-zstd", "zstd"}


def test_the_module_constants_switch_their_codecs_when_a_feed_is_built(monkeypatch):
    from yogo_amd import zarr_feed

    monkeypatch.setattr(zarr_feed, "DEVICE_DECODE_ZLIB", True)
    assert zarr_feed.CODECS["zlib"].on() and not zarr_feed.CODECS["zstd"].on() and zarr_feed.CODECS["zlib"].default_on is False
    monkeypatch.setattr(zarr_feed, "DEVICE_DECODE_ZSTD", True)
    assert zarr_feed.CODECS["zstd"].on() and zarr_feed.CODECS["blosc"].on()
