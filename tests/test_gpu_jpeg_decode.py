"""`yogo_jpeg_decode` (csrc/jpeg_decode.hip) on the MI355X through the C ABI: the grid of tests/_jpeg_files.py -- grey, 4:4:4, 4:2:2,
4:2:0; 1 x 1 up to 64 x 129 with partial blocks and odd chroma sizes; four qualities; noise, ramp, constant and checkerboard
content; optimised Huffman tables and restart intervals -- in ONE launch per number of output planes, the files at odd offsets, every
output range between 64 canary bytes: the planes are ``read_image``'s bit for bit and the status is 0.  The corrupted set: the
status is ``yogo_amd.jpeg.jpeg_status``'s for every file.  Rows outside the buffers, and the production frame (772 x 1032, grey) once."""
import os

import numpy as np
import pytest
import torch

import _jpeg_files as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CANARY, FILL = 64, 0xA5
REFUSED_ROW = [0, 0, 0, 0, 0, 0, 0, 0, 0] + [-1] * 9   # what stands in for a file the host would never hand over: H = 0


def _launch(files, planes, rows=None):
    """the files at odd offsets of one source buffer, their outputs between canaries of one destination buffer -> (dst on the
    host, status, [(offset, length) of every output])"""
    from yogo_amd import jpeg
    from yogo_amd.device_decode import jpeg_decode

    src, table, outs = bytearray(b"\x00"), [], []
    at = CANARY
    for data in files:
        if len(src) % 2 == 0:
            src += b"\x00"
        row = None
        try:
            info = jpeg.parse_jpeg(data)
            if info.device_decodable:
                row = jpeg.table_row(info, len(src), len(data), at, planes)
        except ValueError:
            pass
        if row is None:
            row = list(REFUSED_ROW)
            row[0], row[1], row[2] = len(src), len(data), at
        table.append(row)
        outs.append((at, row[3]))
        at += row[3] + CANARY
        src += data
    if rows is not None:
        table = rows(table)
    dst = torch.full((at,), FILL, dtype=torch.uint8, device=DEV)
    status = torch.full((len(table),), -1, dtype=torch.int32, device=DEV)
    jpeg_decode(torch.frombuffer(src, dtype=torch.uint8).to(DEV), torch.tensor(table, dtype=torch.int64, device=DEV), dst, planes, status)
    torch.cuda.synchronize()
    return dst.cpu().numpy(), status.cpu().numpy(), outs


def _canaries_untouched(dst, outs):
    mask = np.ones(dst.size, dtype=bool)
    for off, ln in outs:
        mask[off:off + ln] = False
    return bool((dst[mask] == FILL).all())


@pytest.fixture(scope="module")
def grid():
    return list(F.grid())


@pytest.mark.parametrize("planes", (1, 3))
def test_grid_is_read_image_bit_for_bit(grid, planes):
    dst, status, outs = _launch([d for _, d in grid], planes)
    assert _canaries_untouched(dst, outs)
    bad = [name for (name, _), st in zip(grid, status) if st != 0]
    assert not bad, (len(bad), bad[:5], status[status != 0][:5])
    wrong = []
    for (name, data), (off, ln) in zip(grid, outs):
        want = F.pil_pixels(data, planes == 3)
        if want.size != ln or not np.array_equal(dst[off:off + ln], want.reshape(-1)):
            wrong.append(name)
    assert not wrong, (len(wrong), wrong[:8])


@pytest.mark.parametrize("planes", (1, 3))
def test_corrupted_files_get_the_twins_status(planes):
    from yogo_amd import jpeg

    files = list(F.corrupted(0))
    dst, status, outs = _launch([d for _, d in files], planes)
    assert _canaries_untouched(dst, outs)
    want = np.array([jpeg.jpeg_status(d) for _, d in files])
    differ = [(name, int(g), int(w)) for (name, _), g, w in zip(files, status, want) if g != w]
    assert not differ, (len(differ), differ[:8])
    assert (want == 0).sum() > 100 and len(set(want.tolist())) >= 8   # (the set reaches the decoder and most of its checks)
    for (name, data), (off, ln), st in zip(files, outs, status):
        if st == 0:
            ref = F.pil_pixels(data, planes == 3)
            assert ref is None or np.array_equal(dst[off:off + ln], ref.reshape(-1)), name


def test_rows_outside_the_buffers_are_refused_and_write_nothing():
    data = F.write("grey", 16, 16, 75, "ramp", np.random.default_rng(1))

    def rows(table):
        good = table[0]
        out = [list(good) for _ in range(7)]
        out[1][0] = -1                 # the source starts in front of src
        out[2][1] = 1 << 40            # ... ends behind it
        out[3][2] = -1                 # the destination starts in front of dst
        out[4][2] = 1 << 40            # ... behind it
        out[5][3] += 1                 # dst_len is not planes * H * W
        out[6][5] = 1041               # a frame wider than the band
        return out

    dst, status, outs = _launch([data], 1, rows)
    assert status.tolist() == [0, 1, 1, 1, 1, 1, 1]
    assert _canaries_untouched(dst, outs)
    assert np.array_equal(dst[outs[0][0]:outs[0][0] + outs[0][1]], F.pil_pixels(data, False).reshape(-1))


def test_production_frame():
    rng = np.random.default_rng(3)
    data = F.write("grey", 772, 1032, 90, "noise", rng)
    dst, status, outs = _launch([data], 1)
    assert status.tolist() == [0] and _canaries_untouched(dst, outs)
    assert np.array_equal(dst[outs[0][0]:outs[0][0] + outs[0][1]], F.pil_pixels(data, False).reshape(-1))


def test_symbol_is_exported_and_declared():
    from yogo_amd import _hip

    assert "yogo_jpeg_decode" in _hip.prototypes()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "yogo_hip.h")).read()
    assert "int yogo_jpeg_decode(" in header
