"""The host side of the device PNG route (yogo_amd/png.py): chunk parsing on PIL-written and hand-built files, the classification
of what the device takes, the errors, and the numpy restatement of the five filters (tests/_png_write.py, which the GPU test of
csrc/png_unpack.hip compares with) against PIL's pixels.  No GPU is needed."""
import io
import zlib

import numpy as np
import pytest
from PIL import Image

import _png_write as PW
from yogo_amd import png


def _pil_bytes(arr, mode=None, **kw):
    buf = io.BytesIO()
    Image.fromarray(arr, mode).save(buf, format="PNG", **kw)
    return buf.getvalue()


def _img(h=24, w=48, seed=3):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy * 3 + xx * 2) + rng.integers(0, 12, size=(h, w))).astype(np.uint8)


def _stream(data, info):
    return b"".join(data[o:o + n] for o, n in info.idat)


def test_pil_written_grey_file():
    img = _img(300, 400)
    data = _pil_bytes(img)
    info = png.parse_png(data)
    assert (info.width, info.height, info.bit_depth, info.color_type, info.interlace) == (400, 300, 8, 0, 0)
    assert info.device_decodable and info.scanline_bytes == 300 * 401
    scan = np.frombuffer(zlib.decompress(_stream(data, info)), dtype=np.uint8).reshape(300, 401)
    assert np.array_equal(PW.unfilter_rows(scan), img)
    assert len(set(scan[:, 0].tolist())) > 1            # PIL chose more than one filter type


@pytest.mark.parametrize("idat_sizes,ancillary", [(None, ()), ([7, 1, 30, 2], ()), ([10, 0, 10], ()),
                                                  ([40, 40], [(b"tEXt", b"k\0v"), (b"pHYs", bytes(9)), (b"tIME", bytes(7))])],
                         ids=["1-idat", "5-idat", "zero-length-idat", "ancillary-around"])
def test_hand_built_files(idat_sizes, ancillary):
    img = _img()
    types = [y % 5 for y in range(24)]
    data = PW.png_bytes(img, types, idat_sizes=idat_sizes, before=ancillary[:2], after=ancillary[2:])
    info = png.parse_png(data)
    assert len(info.idat) == len(idat_sizes or []) + 1 and info.device_decodable
    if idat_sizes:
        assert [n for _, n in info.idat][:-1] == idat_sizes
    scan = zlib.decompress(_stream(data, info))
    assert scan == PW.filter_rows(img, types).tobytes()
    # the numpy restatement of the filters equals PIL's pixels
    with Image.open(io.BytesIO(data)) as im:
        pil = np.asarray(im.convert("L"))
    assert np.array_equal(pil, img)
    assert np.array_equal(PW.unfilter_rows(np.frombuffer(scan, np.uint8).reshape(24, 49)), pil)


@pytest.mark.parametrize("t", range(5))
def test_each_filter_against_pil(t):
    img = np.random.default_rng(t).integers(0, 256, size=(9, 70), dtype=np.uint8)
    data = PW.png_bytes(img, [t] * 9)
    with Image.open(io.BytesIO(data)) as im:
        assert np.array_equal(np.asarray(im), img)
    scan = PW.filter_rows(img, [t] * 9)
    assert set(scan[:, 0].tolist()) == {t} and np.array_equal(PW.unfilter_rows(scan), img)


def test_kinds_the_device_does_not_take():
    rgb = np.random.default_rng(1).integers(0, 256, size=(8, 9, 3), dtype=np.uint8)
    grey16 = np.random.default_rng(2).integers(0, 65536, size=(8, 9), dtype=np.uint16)
    pal = Image.fromarray(_img(8, 9)).convert("P")
    buf = io.BytesIO()
    pal.save(buf, format="PNG")
    kinds = {"rgb": (_pil_bytes(rgb), 2, 8), "palette": (buf.getvalue(), 3, 8), "16-bit": (_pil_bytes(grey16), 0, 16)}
    for name, (data, ctype, depth) in kinds.items():
        info = png.parse_png(data)
        assert (info.color_type, info.bit_depth) == (ctype, depth) and not info.device_decodable, name
    laced = PW.png_bytes(_img(8, 9), ihdr=(9, 8, 8, 0, 0, 0, 1), scan=PW.adam7_scan(_img(8, 9)))
    with Image.open(io.BytesIO(laced)) as im:
        assert np.array_equal(np.asarray(im), _img(8, 9))          # an Adam7 file as PIL understands it
    lace = png.parse_png(laced)
    assert lace.interlace == 1 and not lace.device_decodable
    trns = png.parse_png(PW.png_bytes(_img(8, 9), before=[(b"tRNS", b"\0\7")]))
    assert trns.has_trns and not trns.device_decodable
    assert png.parse_png(PW.png_bytes(_img(8, 9))).device_decodable


def test_errors():
    good = PW.png_bytes(_img(), idat_sizes=[20])
    png.parse_png(good)
    with pytest.raises(png.NotPng, match="signature"):
        png.parse_png(b"\x89PNX" + good[4:])
    at = good.index(b"IDAT")
    with pytest.raises(ValueError, match="CRC-32 of the IDAT"):
        png.parse_png(good[:at + 6] + bytes([good[at + 6] ^ 1]) + good[at + 7:])
    with pytest.raises(ValueError, match="CRC-32 of the IHDR"):
        png.parse_png(good[:17] + bytes([good[17] ^ 1]) + good[18:])
    with pytest.raises(ValueError, match="IEND"):
        png.parse_png(good[:-12])
    with pytest.raises(ValueError, match="passes the end"):
        png.parse_png(good[:-20])
    idat_first = PW.SIGNATURE + PW.chunk(b"IDAT", b"abc") + good[8:]
    with pytest.raises(ValueError, match="not IHDR"):
        png.parse_png(idat_first)
    assert not isinstance(pytest.raises(ValueError, png.parse_png, idat_first).value, png.NotPng)
