"""yogo_amd/jpeg.py on the host: the numpy twin ``decode`` against ``read_image`` (PIL) bit for bit over the grid of
tests/_jpeg_files.py, the predicate ``device_decodable`` on what stays the host's, and ``jpeg_status`` over truncated and
byte-changed files: it never raises, and where it says 0 the twin gives PIL's pixels of the same bytes."""
import io

import numpy as np
import pytest
from PIL import Image

import _jpeg_files as F
from yogo_amd import jpeg


@pytest.mark.parametrize("size", F.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", F.FORMATS)
def test_twin_is_read_image_bit_for_bit(fmt, size, tmp_path):
    from yogo_amd.yogo_dataset import read_image

    H, W = size
    fi = F.FORMATS.index(fmt)
    n = 0
    for quality in F.QUALITIES:
        for ki, kind in enumerate(F.CONTENTS):
            for oi, options in enumerate(F.OPTIONS):
                rng = np.random.default_rng(((fi * 200 + H) * 200 + W) * 100 + quality + ki)
                data = F.write(fmt, H, W, quality, kind, rng, **options)
                info = jpeg.parse_jpeg(data)
                assert info.device_decodable and (info.height, info.width) == (H, W)
                assert (info.restart_interval > 0) == (oi >= 2)
                assert jpeg.jpeg_status(data) == 0
                path = tmp_path / "f.jpg"
                path.write_bytes(data)
                for rgb in (False, True):
                    want = read_image(path, rgb).numpy()
                    got = jpeg.decode(data, rgb)
                    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), (quality, kind, options, rgb)
                n += 1
    assert n == 100


def _grey(**kw):
    buf = io.BytesIO()
    Image.fromarray(F.content("ramp", 16, 24, 1, np.random.default_rng(0))[..., 0], "L").save(buf, format="JPEG", **kw)
    return buf.getvalue()


def _colour(mode="RGB", **kw):
    buf = io.BytesIO()
    planes = 4 if mode == "CMYK" else 3
    Image.fromarray(F.content("ramp", 16, 24, planes, np.random.default_rng(0)), mode).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def _patched(data, marker, offset, value):
    """the byte at ``offset`` behind the length of the first segment of ``marker`` replaced (offset -3: the marker's own byte)"""
    at = data.index(bytes([0xFF, marker]))
    out = bytearray(data)
    out[at + 4 + offset] = value
    return bytes(out)


def test_predicate_keeps_the_hosts_files():
    assert jpeg.parse_jpeg(_grey()).device_decodable and jpeg.parse_jpeg(_colour()).device_decodable
    progressive = jpeg.parse_jpeg(_grey(progressive=True))
    assert progressive.sof == 2 and not progressive.device_decodable
    cmyk = jpeg.parse_jpeg(_colour("CMYK"))
    assert len(cmyk.components) == 4 and not cmyk.device_decodable
    arithmetic = jpeg.parse_jpeg(_patched(_grey(), 0xC0, -3, 0xC9))
    assert arithmetic.sof == 9 and not arithmetic.device_decodable
    twelve = jpeg.parse_jpeg(_patched(_grey(), 0xC0, 0, 12))
    assert twelve.precision == 12 and not twelve.device_decodable
    wide = jpeg.parse_jpeg(_patched(_colour(subsampling=1), 0xC0, 7, 0x41))   # the luma component's sampling byte: 4 x 1
    assert (wide.components[0].h, wide.components[0].v) == (4, 1) and not wide.device_decodable
    with pytest.raises(jpeg.NotJpeg):
        buf = io.BytesIO()
        Image.new("L", (4, 4)).save(buf, format="PNG")
        jpeg.parse_jpeg(buf.getvalue())
    with pytest.raises(ValueError):
        jpeg.parse_jpeg(_grey()[:40])


def test_predicate_on_colour_transform_and_width():
    data = _colour()
    info = jpeg.parse_jpeg(data)
    assert info.jfif and info.ycbcr
    # without JFIF, an Adobe segment with transform 0 says RGB stored as RGB: the host's
    assert not info._replace(jfif=False, adobe_transform=0).device_decodable
    assert info._replace(jfif=False, adobe_transform=1).device_decodable
    assert not info._replace(width=jpeg.MAX_WIDTH + 1).device_decodable and info._replace(width=jpeg.MAX_WIDTH).device_decodable
    assert not info._replace(scans=2).device_decodable and not info._replace(height=0).device_decodable


def test_status_twin_over_corrupted_files():
    """seed 0: the share of status-0 files on which PIL raises or warns is printed and held to 25 %"""
    ok = skipped = 0
    seen = set()
    for name, data in F.corrupted(0):
        status = jpeg.jpeg_status(data)
        assert status in jpeg.JPG_STATUS or status == 0
        seen.add(status)
        if status:
            with pytest.raises(ValueError):
                jpeg.decode(data, False)
            continue
        ok += 1
        for rgb in (False, True):
            want = F.pil_pixels(data, rgb)
            if want is None:
                skipped += 1
                break
            assert np.array_equal(jpeg.decode(data, rgb), want), (name, rgb)
    print(f"status 0: {ok} files, PIL raised or warned on {skipped}; statuses seen: {sorted(seen)}")
    assert ok > 100 and skipped <= ok // 4
    assert {jpeg.JPG_SOURCE_ENDS, jpeg.JPG_BAD_MARKER, jpeg.JPG_NO_EOI, jpeg.JPG_MCU_COUNT} <= seen


def test_table_row_names_the_tables_in_the_file():
    data = F.write("420", 17, 33, 75, "ramp", np.random.default_rng(2), restart_marker_blocks=3)
    info = jpeg.parse_jpeg(data)
    row = jpeg.table_row(info, 5, len(data), 64, 3)
    assert len(row) == jpeg.TABLE_COLS and row[:6] == [5, len(data), 64, 3 * 17 * 33, 17, 33]
    assert row[6] == 3 | 2 << 8 | 2 << 16 and row[7] == 3 and row[8] == info.scan_offset
    assert data[info.scan_offset - 3:info.scan_offset] == bytes([0, 63, 0])
    for c, q in enumerate(row[9:12]):   # the Pq / Tq byte stands in front of a table's entries, Tc / Th in front of the counts
        assert data[q // 2 - 1] == (q % 2) << 4 | info.components[c].tq
    for c in range(3):
        assert data[row[12 + c] - 1] == info.scan_components[c][1] and data[row[15 + c] - 1] == 0x10 | info.scan_components[c][2]
    assert jpeg.table_row(info._replace(quant={}), 5, len(data), 64, 3)[9:12] == [-1, -1, -1]
