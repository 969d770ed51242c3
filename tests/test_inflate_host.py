"""The pure-Python inflater (yogo_amd/inflate.py: the twin of csrc/inflate.hip, check for check) against zlib: streams made by
zlib.compressobj at every strategy, hand-built streams of every block shape (tests/_deflate_write.py), and hand-built defective
streams, each of which gets its status here and an error from zlib.  Every case first shows that its bytes hold what it is named
after.  No GPU is needed."""
import struct
import zlib

import pytest

import _deflate_write as DW
from yogo_amd import inflate as I

DATAS = DW.zlib_datas()


def test_split_zlib():
    z = zlib.compress(b"hello hello hello", 6)
    off, ln, adler = I.split_zlib(z)
    assert (off, ln) == (2, len(z) - 6) and adler == zlib.adler32(b"hello hello hello")
    assert zlib.decompress(z[off:off + ln], -15) == b"hello hello hello"
    for bad, what in ((b"\x78\x9c\x03", "shorter"), (b"\x79\x9c" + z[2:], "method"), (b"\x88\x1c" + z[2:], "window"),
                      (b"\x78\x9d" + z[2:], "FCHECK"), (b"\x78\xbb" + z[2:], "dictionary")):
        with pytest.raises(ValueError, match=what):
            I.split_zlib(bad)
    assert (0x78 * 256 + 0xbb) % 31 == 0 and (0x88 * 256 + 0x1c) % 31 == 0     # (those two fail for what they are named after)


def test_status_numbers_are_distinct_and_named():
    codes = [getattr(I, n) for n in dir(I) if n.startswith("INF_") and n not in ("INF_OK", "INF_STATUS")]
    assert sorted(codes) == list(range(1, 11)) and set(I.INF_STATUS) == set(codes)


@pytest.mark.parametrize("config", list(DW.ZLIB_CONFIGS))
@pytest.mark.parametrize("name", list(DATAS))
def test_streams_made_by_zlib(name, config):
    data = DATAS[name]
    z = DW.zlib_stream(data, config)
    assert zlib.decompress(z) == data
    off, ln, adler = I.split_zlib(z)
    raw = z[off:off + ln]
    blocks = DW.describe(raw)
    types = {b["type"] for b in blocks}
    if config == "stored":
        assert types == {0}
    elif config == "fixed":
        assert 2 not in types and (1 in types or name.startswith(("random", "repeat-at")))    # (what does not shrink, zlib stores)
    elif config == "huffman-only":
        assert not DW.matches(blocks)
    elif config == "rle":
        assert all(d == 1 for _, d in DW.matches(blocks))
    elif config == "full-flush":
        assert any(b["type"] == 0 and b["stored"] == b"" for b in blocks[:-1])    # the flush's empty stored block
    elif data and name not in ("one-byte", "random", "repeat-at-32768"):
        assert DW.matches(blocks)
    if name == "repeat-at-32768":
        assert len(data) == 70000 and data[32768:65536] == data[:32768]
    if name == "repeat-at-32500" and config in ("level1", "level6", "level9"):
        assert any(d == 32500 for _, d in DW.matches(blocks))
    if name == "low-entropy" and config in ("level6", "huffman-only"):
        assert 2 in types
    assert I.inflate_status(raw, len(data), adler) == (I.INF_OK, data)
    assert I.inflate_status(raw, len(data), adler ^ 0x10000) == (I.INF_ADLER, data)


def _shows_its_name(name, raw, data):
    """the case holds what it is named after"""
    blocks = DW.describe(raw)
    m = DW.matches(blocks)
    if name.startswith("stored-len"):
        assert [len(b["stored"]) for b in blocks] == [int(name[10:])]
    elif name == "stored-two":
        assert [b["type"] for b in blocks] == [0, 0]
    elif name == "stored-sync-flush":
        assert [b["type"] for b in blocks] == [1, 0, 1] and blocks[1]["stored"] == b""
    elif name.startswith("fixed-len"):
        assert blocks[0]["type"] == 1 and [ln for ln, _ in m] == [int(name[9:])]
    elif name.startswith("fixed-dist1-len"):
        assert m == [(int(name[15:]), 1)]
    elif name.startswith("fixed-dist"):
        assert blocks[0]["type"] == 1 and int(name[10:]) in {d for _, d in m}
    elif name == "dynamic-hclen5":
        assert blocks[0]["nc"] == 5
    elif name == "dynamic-hclen19-15bit":
        assert blocks[0]["nc"] == 19 and blocks[0]["lit_lens"].count(15) == 2 and blocks[0]["lit_lens"][14] == 15 and 14 in blocks[0]["tokens"]
    elif name == "dynamic-repeats":
        assert {(16, 3), (16, 6), (17, 3), (17, 10), (18, 11), (18, 138)} <= set(blocks[0]["ops"])
    elif name == "dynamic-repeat-crosses":
        b = blocks[0]
        at, crossing = 0, []
        for s, rep in b["ops"]:
            n = 1 if rep is None else rep
            if at < b["nl"] < at + n:
                crossing.append(s)
            at += n
        assert crossing == [18]
    elif name == "dynamic-one-distance":
        assert [l for l in blocks[0]["dist_lens"] if l] == [1] and m
    elif name == "dynamic-no-distance":
        assert not any(blocks[0]["dist_lens"]) and not m
    elif name == "fixed-mixed-tokens":
        widths = {DW.LEN_EXTRA[DW.len_symbol(ln)[0] - 257] + DW.DIST_EXTRA[DW.dist_symbol(d)[0]] for ln, d in m}
        assert len(raw) > 12 * 256 and {0, 13} <= widths and len(widths) > 8
    else:
        raise KeyError(name)


@pytest.mark.parametrize("name", list(DW.CASES))
def test_hand_built_streams(name):
    raw, data = DW.CASES[name]
    assert zlib.decompress(DW.zlib_wrap(raw, data)) == data
    _shows_its_name(name, raw, data)
    assert I.inflate_status(raw, len(data), zlib.adler32(data)) == (I.INF_OK, data)


@pytest.mark.parametrize("name", list(DW.DEFECTS))
def test_defective_streams(name):
    raw, dst_len, want = DW.DEFECTS[name]
    status, out = I.inflate_status(raw, dst_len)
    assert status == getattr(I, want)
    if want in ("INF_PAST_DESTINATION", "INF_ENDS_EARLY"):     # a well-formed stream of another length than dst_len
        whole = zlib.decompress(raw, -15)
        assert len(whole) != dst_len and whole[:len(out)] == out
    else:
        with pytest.raises(zlib.error):
            zlib.decompress(raw, -15)
        with pytest.raises(zlib.error):
            zlib.decompress(b"\x78\x9c" + raw + struct.pack(">I", zlib.adler32(out)))
    assert len(out) <= dst_len
