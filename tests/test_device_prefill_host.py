"""Host side of the device-decoded prefill (`yogo train --device-image-cache GIB --device-image-decode`, yogo_amd/png_prefill.py):
the flag on the train parser and in the config, its error without a cache, the PNG predicate for what the device unfilters, and the
slot layout from file sizes."""
import struct

import numpy as np
import pytest

from _png_write import chunk, png_bytes


def test_train_parser_stores_the_flag():
    from yogo_amd.trainer import build_config
    from yogo_amd.utils.argparsers import global_parser, train_parser

    args = global_parser().parse_args(["train", "defn.yml", "--device-image-cache", "2", "--device-image-decode"])
    assert args.device_image_decode is True and build_config(args)["device_image_decode"] is True
    args = global_parser().parse_args(["train", "defn.yml", "--device-image-cache", "2"])
    assert args.device_image_decode is False and build_config(args)["device_image_decode"] is False
    args = global_parser().parse_args(["train", "defn.yml", "--device-image-cache", "2", "--no-device-image-decode"])
    assert args.device_image_decode is False
    assert global_parser().parse_args(["train", "defn.yml"]).device_image_decode is False
    assert train_parser().parse_args(["defn.yml", "--device-image-decode", "--device-image-cache", "0.5"]).device_image_decode is True
    # inference keeps its own flag of that name, which needs no cache
    assert global_parser().parse_args(["infer", "m.pth", "--path-to-images", "imgs", "--device-image-decode"]).device_image_decode is True
    assert "not counted in the GIB budget" in " ".join(train_parser().format_help().split())


@pytest.mark.parametrize("parser", ["global", "train"])
def test_the_flag_without_a_cache_is_a_parser_error(parser, capsys):
    from yogo_amd.utils.argparsers import global_parser, train_parser

    with pytest.raises(SystemExit) as e:
        if parser == "global":
            global_parser().parse_args(["train", "defn.yml", "--device-image-decode"])
        else:
            train_parser().parse_args(["defn.yml", "--device-image-decode"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "error: --device-image-decode fills the device image cache: it needs --device-image-cache GIB" in err


@pytest.mark.parametrize("color_type,depths", [(0, (1, 2, 4, 8, 16)), (2, (8, 16)), (3, (1, 2, 4, 8)), (4, (8, 16)), (6, (8, 16))])
@pytest.mark.parametrize("interlace", [0, 1])
def test_prefill_decodable(color_type, depths, interlace):
    from yogo_amd import png

    for depth in depths:
        data = png_bytes(np.zeros((3, 4), np.uint8), ihdr=(4, 3, depth, color_type, 0, 0, interlace))
        info = png.parse_png(data)
        want = depth == 8 and color_type in (0, 2) and interlace == 0
        assert info.prefill_decodable is want, (color_type, depth, interlace)
        assert info.device_decodable is (want and color_type == 0)           # inference's predicate is as it was
        if want:
            assert info.bytes_per_pixel == (3 if color_type == 2 else 1)


def test_trns_is_not_prefill_decodable():
    from yogo_amd import png

    rgb = np.zeros((3, 4, 3), np.uint8)
    assert png.parse_png(png_bytes(rgb)).prefill_decodable is True
    assert png.parse_png(png_bytes(rgb, before=[(b"tRNS", struct.pack(">HHH", 1, 2, 3))])).prefill_decodable is False
    assert png.parse_png(png_bytes(rgb[..., 0], before=[(b"tRNS", struct.pack(">H", 7))])).prefill_decodable is False
    assert png.parse_png(png_bytes(rgb, before=[(b"gAMA", struct.pack(">I", 45455))])).prefill_decodable is True
    assert chunk(b"IEND", b"")[-4:] == png_bytes(rgb)[-4:]


def test_slot_layout_packs_without_overlap_at_align():
    from yogo_amd.png_batch import slot_layout
    from yogo_amd.device_decode import ALIGN

    rng = np.random.default_rng(2)
    for sizes in ([1], [0, 5, 0], [ALIGN, ALIGN + 1, ALIGN - 1], list(rng.integers(0, 900_000, size=300)), [900_000, 10, 2_000_000, 3]):
        offsets, total = slot_layout(sizes)
        assert len(offsets) == len(sizes) and offsets[0] == 0
        assert all(int(o) % ALIGN == 0 for o in offsets) and total % ALIGN == 0
        ends = [int(o) + int(s) for o, s in zip(offsets, sizes)]
        assert all(ends[i] <= int(offsets[i + 1]) for i in range(len(sizes) - 1)) and ends[-1] <= total
        assert total <= sum(int(s) for s in sizes) + ALIGN * len(sizes)       # no room is wider than its file rounded up
    # a file's room does not depend on the files before it: a large file after small ones has its own size
    offsets, total = slot_layout([10, 10, 5_000_000])
    assert total - int(offsets[2]) >= 5_000_000
    offsets, total = slot_layout([])
    assert len(offsets) == 0 and total == 0


def test_decode_batch_is_checked():
    from yogo_amd.png_prefill import DEFAULT_DECODE_BATCH, check_decode_batch

    assert check_decode_batch(DEFAULT_DECODE_BATCH) == DEFAULT_DECODE_BATCH
    for bad in (0, -1, 65536):
        with pytest.raises(ValueError):
            check_decode_batch(bad)
