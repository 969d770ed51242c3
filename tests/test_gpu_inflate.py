"""The device inflater (yogo_amd/csrc/inflate.hip) against zlib: the streams of tests/test_inflate_host.py -- made by zlib, built
by hand, and defective -- each group in ONE launch with many table rows, sources and destinations at every alignment, canary
bytes round every destination range.  The defective streams are bounds-checked decodes of bad input: the pure-Python twin
(yogo_amd.inflate.inflate_status) runs on every one of them first, and the device must name the same check, leave the same
bytes before it and touch nothing else.  What each case holds is shown in tests/test_inflate_host.py."""
import zlib

import pytest

import _deflate_write as DW
from yogo_amd import inflate as I

pytestmark = pytest.mark.gpu


def _check(names, entries, want):
    """entries through one launch; want: [(status, bytes that must lie at the front of the destination range)]"""
    for raw, dst_len, adler in entries:      # the twin first: nothing goes to the device that it has not been through
        I.inflate_status(raw, dst_len, adler)
    status, got, canaries = DW.inflate_on_device(entries)
    assert canaries
    for name, st, g, (wst, wbytes) in zip(names, status, got, want):
        assert st == wst, (name, st, wst)
        assert g[:len(wbytes)] == wbytes, name
        assert g[len(wbytes):] == bytes([DW.CANARY]) * (len(g) - len(wbytes)), name      # nothing behind what was produced


def test_streams_made_by_zlib():
    names, entries, want = [], [], []
    for name, data in DW.zlib_datas().items():
        for config in DW.ZLIB_CONFIGS:
            z = DW.zlib_stream(data, config)
            assert zlib.decompress(z) == data
            off, ln, adler = I.split_zlib(z)
            names.append(f"{name}-{config}")
            entries.append((z[off:off + ln], len(data), adler))
            want.append((I.INF_OK, data))
    _check(names, entries, want)


def test_hand_built_streams():
    names = list(DW.CASES)
    for raw, data in DW.CASES.values():
        assert zlib.decompress(DW.zlib_wrap(raw, data)) == data
    _check(names, [(raw, len(data), zlib.adler32(data)) for raw, data in DW.CASES.values()],
           [(I.INF_OK, data) for _, data in DW.CASES.values()])


def test_300_rows_in_one_launch():
    """short streams of every kind, 300 of them, their destinations at odd alignments (inflate_on_device's packing)"""
    cases = [v for k, v in DW.CASES.items() if len(v[1]) < 400]
    entries, want = [], []
    for i in range(300):
        if i % 3 == 2:
            data = bytes((i * j + (j >> 3)) & 0xFF for j in range(1 + i % 200))
            z = zlib.compress(data, 1 + i % 9)
            raw = z[2:-4]
        else:
            raw, data = cases[i % len(cases)]
        entries.append((raw, len(data), zlib.adler32(data)))
        want.append((I.INF_OK, data))
    assert len({len(d) % 16 for _, d in want}) == 16
    _check([str(i) for i in range(300)], entries, want)


def test_adler():
    ff = bytes([0xFF]) * 70000           # the largest sums: every byte 255
    z1, zf = zlib.compress(b"\x80", 6), zlib.compress(ff, 6)
    helo = zlib.compress(b"hello, hello, hello", 9)
    entries = [(z1[2:-4], 1, zlib.adler32(b"\x80")), (zf[2:-4], 70000, zlib.adler32(ff)),
               (helo[2:-4], 19, zlib.adler32(b"hello, hello, hello") ^ 1), (zf[2:-4], 70000, zlib.adler32(ff) ^ 0x80000000)]
    assert zlib.adler32(ff) >> 16 != 0 and zlib.adler32(ff) & 0xFFFF != 0
    # a wrong trailer: the Adler status, the bytes still zlib's
    _check(["n=1", "70000xFF", "wrong-trailer", "wrong-trailer-high-bit"], entries,
           [(I.INF_OK, b"\x80"), (I.INF_OK, ff), (I.INF_ADLER, b"hello, hello, hello"), (I.INF_ADLER, ff)])


def test_defective_streams():
    names, entries, want = [], [], []
    for name, (raw, dst_len, status) in DW.DEFECTS.items():
        st, out = I.inflate_status(raw, dst_len, 1)
        assert st == getattr(I, status)
        names.append(name)
        entries.append((raw, dst_len, 1))
        want.append((st, out))
    _check(names, entries, want)


def test_rows_outside_the_buffers():
    import torch

    from yogo_amd.device_decode import inflate_streams

    raw, data = DW.CASES["fixed-len3"]
    src = torch.frombuffer(bytearray(raw + bytes(16)), dtype=torch.uint8).cuda()
    n, S, D = len(raw), len(raw) + 16, 256
    rows = [(0, n, 16, len(data), zlib.adler32(data)),            # a good row among them
            (-1, n, 0, 8, 0), (0, -1, 0, 8, 0), (S + 1, 0, 0, 8, 0), (S - 4, 5, 0, 8, 0), (0, 1 << 62, 0, 8, 0),
            (0, n, -1, 8, 0), (0, n, 0, -1, 0), (0, n, D + 1, 0, 0), (0, n, D - 4, 5, 0), (0, n, 0, 1 << 62, 0), (1 << 62, 1 << 62, 0, 8, 0)]
    dst = torch.full((D,), DW.CANARY, dtype=torch.uint8, device="cuda")
    status = torch.full((len(rows),), -1, dtype=torch.int32, device="cuda")
    inflate_streams(src, torch.tensor(rows, dtype=torch.int64, device="cuda"), dst, status)
    assert status.cpu().tolist() == [I.INF_OK] + [I.INF_BAD_ROW] * (len(rows) - 1)
    host = dst.cpu().numpy().tobytes()
    assert host[16:16 + len(data)] == data
    assert host[:16] + host[16 + len(data):] == bytes([DW.CANARY]) * (D - len(data))


def test_entry_point_refuses_bad_arguments():
    import torch

    from yogo_amd.device_decode import inflate_streams

    src = torch.zeros(64, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(80, dtype=torch.uint8, device="cuda")
    table = torch.tensor([[0, 4, 0, 4, 1]], dtype=torch.int64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        inflate_streams(src, table, dst[8:], status)
    with pytest.raises(RuntimeError, match="overlap"):
        inflate_streams(dst[:48], table, dst, status)
    with pytest.raises(ValueError, match="table"):
        inflate_streams(src, table.to(torch.int32), dst, status)
