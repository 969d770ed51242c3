"""The host side of ``--device-image-decode-all`` (yogo_amd/png.py): ``decode_any``, the numpy twin of csrc/png_unpack_any.hip,
against ``read_image`` (PIL) for every colour type and bit depth, plain and Adam7, with and without tRNS, under mixed filter types;
the inflated-size formula; the PLTE bookkeeping; the two earlier predicates, unchanged; the flag's argparse and ValueError checks.
No GPU is needed.

Shapes (H x W) as in tests/test_gpu_png_types.py: 67 x 37, 9 x 5, 5 x 3, 1 x 1."""
import zlib

import numpy as np
import pytest

import _png_types_write as TW
from yogo_amd import png

IDS = [TW.format_id(f) for f in TW.FORMATS]


def _inflated(data, info):
    return zlib.decompress(b"".join(data[o:o + n] for o, n in info.idat))


@pytest.mark.filterwarnings("ignore:Palette images with Transparency")
@pytest.mark.parametrize("trns", [False, True], ids=["", "trns"])
@pytest.mark.parametrize("lace", [False, True], ids=["plain", "adam7"])
@pytest.mark.parametrize("fmt", TW.FORMATS, ids=IDS)
def test_decode_any_equals_read_image(tmp_path, fmt, lace, trns):
    from yogo_amd.yogo_dataset import read_image

    for H, W in TW.SHAPES:
        rng = np.random.default_rng(H * 1000 + W + 7 * fmt[0] + fmt[1])
        data, _, _ = TW.make_png(rng, H, W, *fmt, interlace=lace, trns=trns)
        p = tmp_path / f"{H}x{W}.png"
        p.write_bytes(data)
        info = png.parse_png(data)
        assert info.any_decodable and info.has_trns is trns and (info.plte is not None) == (fmt[0] == 3)
        # the rows mix all five filter types (and every band of 64 rows does)
        assert info.inflated_bytes == len(_inflated(data, info)), (H, W)
        assert info.format_code == fmt[0] | fmt[1] << 8 | int(lace) << 16
        assert info.filter_bpp == max(1, TW.CHANNELS[fmt[0]] * fmt[1] // 8)
        for rgb in (False, True):
            want = read_image(p, rgb=rgb).numpy()
            got = png.decode_any(data, rgb=rgb)
            assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), (H, W, rgb)


def test_the_writer_mixes_filter_types():
    data, _, _ = TW.make_png(np.random.default_rng(0), 67, 37, 6, 16, interlace=True)
    info = png.parse_png(data)
    scan, at, seen = _inflated(data, info), 0, []
    for _, _, _, _, w, h in info.passes():
        rb = (w * info.bits_per_pixel + 7) // 8
        seen += [scan[at + y * (1 + rb)] for y in range(h)]
        at += h * (1 + rb)
    assert at == len(scan) and seen[:10] == [0, 1, 2, 3, 4, 0, 1, 2, 3, 4] and len(list(info.passes())) == 7


@pytest.mark.parametrize("hw,count", [((1, 1), 1), ((5, 3), 6), ((9, 5), 7), ((67, 37), 7)])
def test_adam7_passes_without_pixels_have_no_scanlines(hw, count):
    H, W = hw
    data, _, _ = TW.make_png(np.random.default_rng(1), H, W, 0, 8, interlace=True)
    info = png.parse_png(data)
    passes = list(info.passes())
    assert len(passes) == count and sum(w * h for *_, w, h in passes) == H * W
    assert info.inflated_bytes == sum(h * (1 + w) for *_, w, h in passes) == len(_inflated(data, info))


@pytest.mark.filterwarnings("ignore:Palette images with Transparency")
@pytest.mark.parametrize("depth", [1, 2, 4, 8])
@pytest.mark.parametrize("trns", [False, True])
def test_short_plte_is_padded_with_zeros(tmp_path, depth, trns):
    """a PLTE with fewer entries than the index range: the indices past it are black, as PIL has them"""
    from yogo_amd.yogo_dataset import read_image

    rng = np.random.default_rng(depth)
    entries = {1: 1, 2: 3, 4: 5, 8: 100}[depth]
    data, samples, palette = TW.make_png(rng, 9, 5, 3, depth, plte_entries=entries, trns=trns)
    assert int(samples.max()) >= entries and palette.shape == (entries, 3)
    info = png.parse_png(data)
    table = png.palette_table(data, info)
    assert info.any_decodable and info.plte[1] == 3 * entries and table.shape == (768,)
    assert np.array_equal(table[:3 * entries], palette.reshape(-1)) and not table[3 * entries:].any()
    p = tmp_path / "short.png"
    p.write_bytes(data)
    for rgb in (False, True):
        assert np.array_equal(png.decode_any(data, rgb=rgb), read_image(p, rgb=rgb).numpy())


def test_palette_file_without_a_usable_plte_stays_on_the_host():
    rng = np.random.default_rng(2)
    none = png.parse_png(TW.make_png(rng, 5, 3, 3, 8, plte_entries=0)[0])
    assert none.format_known and none.plte is None and not none.any_decodable
    with pytest.raises(ValueError, match="PLTE"):
        png.decode_any(TW.make_png(rng, 5, 3, 3, 8, plte_entries=0)[0])
    good = TW.make_png(rng, 5, 3, 3, 8)[0]
    at = good.index(b"PLTE")
    stale = good[:at + 10] + bytes([good[at + 10] ^ 1]) + good[at + 11:]      # the chunk's CRC-32 no longer fits
    assert png.parse_png(good).any_decodable and not png.parse_png(stale).any_decodable
    odd = png.parse_png(TW.PW.png_bytes(np.zeros((5, 3), np.uint8), ihdr=(3, 5, 8, 3, 0, 0, 0), before=[(b"PLTE", bytes(10))]))
    assert odd.plte == (odd.plte[0], 10) and not odd.any_decodable              # no whole number of entries
    # a PLTE chunk in a file of another colour type changes nothing
    rgb = TW.make_png(rng, 5, 3, 2, 8, plte_entries=4)[0]
    assert png.parse_png(rgb).plte is not None and png.parse_png(rgb).any_decodable and png.parse_png(rgb).prefill_decodable


@pytest.mark.parametrize("ihdr", [(3, 5, 3, 0), (3, 5, 4, 2), (3, 5, 16, 3), (3, 5, 8, 5), (3, 5, 8, 1), (3, 5, 2, 4)])
def test_formats_outside_the_specification_are_not_decodable(ihdr):
    W, H, depth, ct = ihdr
    for lace in (0, 1, 2):
        info = png.parse_png(TW.PW.png_bytes(np.zeros((H, W), np.uint8), ihdr=(W, H, depth, ct, 0, 0, lace)))
        assert not info.format_known and not info.any_decodable
    assert not png.parse_png(TW.PW.png_bytes(np.zeros((5, 3), np.uint8), ihdr=(3, 5, 8, 0, 0, 0, 2))).any_decodable


@pytest.mark.parametrize("trns", [False, True])
@pytest.mark.parametrize("lace", [False, True])
@pytest.mark.parametrize("fmt", TW.FORMATS, ids=IDS)
def test_the_two_earlier_predicates_are_unchanged(fmt, lace, trns):
    data, _, _ = TW.make_png(np.random.default_rng(3), 9, 5, *fmt, interlace=lace, trns=trns)
    info = png.parse_png(data)
    plain = fmt[1] == 8 and not lace and not trns
    assert info.device_decodable is (plain and fmt[0] == 0)
    assert info.prefill_decodable is (plain and fmt[0] in (0, 2))
    assert info.bytes_per_pixel == (3 if fmt[0] == 2 else 1)
    if fmt == (0, 8):
        assert info.scanline_bytes == 9 * (1 + 5)
        assert lace or info.inflated_bytes == info.scanline_bytes


def test_decode_any_refuses_a_bad_filter_byte_and_a_short_stream():
    rng = np.random.default_rng(4)
    data, _, _ = TW.make_png(rng, 9, 5, 2, 16, interlace=True, bad=(3, 1, 9))
    with pytest.raises(ValueError, match="filter type 9"):
        png.decode_any(data)
    whole, samples, _ = TW.make_png(rng, 9, 5, 0, 2)
    short = TW.PW.png_bytes(np.zeros((9, 5), np.uint8), ihdr=(5, 9, 2, 0, 0, 0, 0), scan=TW.scanlines(samples, 2)[:-3])
    with pytest.raises(ValueError, match="inflates to"):
        png.decode_any(short)


def test_the_flag_needs_device_image_decode(capsys):
    from yogo_amd.utils.argparsers import global_parser, infer_parser, train_parser

    infer = ["infer", "m.pth", "--path-to-images", "imgs"]
    train = ["train", "defn.yml", "--device-image-cache", "0.5"]
    for base in (infer, train):
        assert global_parser().parse_args(base).device_image_decode_all is False
        args = global_parser().parse_args(base + ["--device-image-decode", "--device-image-decode-all"])
        assert args.device_image_decode is True and args.device_image_decode_all is True
        with pytest.raises(SystemExit):
            global_parser().parse_args(base + ["--device-image-decode-all"])
        assert "--device-image-decode-all widens what --device-image-decode takes" in capsys.readouterr().err
    for parser, argv in ((infer_parser(), infer[1:]), (train_parser(), train[1:])):
        with pytest.raises(SystemExit):
            parser.parse_args(argv + ["--device-image-decode-all"])
        assert "needs --device-image-decode" in capsys.readouterr().err
        assert "--device-image-decode-all" in parser.format_help()


def test_the_python_entry_points_refuse_the_flag_alone(tmp_path):
    from yogo_amd.infer import predict
    from yogo_amd.yogo_dataloader import get_dataloader

    with pytest.raises(ValueError, match="needs device_image_decode"):
        predict(str(tmp_path / "m.pth"), path_to_images=tmp_path, device_image_decode_all=True)
    with pytest.raises(ValueError, match="needs --device-image-decode"):
        get_dataloader(None, 4, 12, 8, device_image_cache_gib=1.0, device_image_decode_all=True)
