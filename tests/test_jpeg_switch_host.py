"""``--device-image-decode-jpeg`` without a GPU: what the parsers, ``get_dataloader``, ``predict`` and ``ImageCache`` say about the
switch (the rules of ``--device-image-decode-all``), the scope ``yogo test`` opens, and the batch steps of yogo_amd/png_batch.py on
a JPEG record."""
import numpy as np
import pytest

import _jpeg_files as F

INFER = ["infer", "m.pth", "--path-to-images", "imgs"]
TRAIN = ["train", "defn.yml", "--device-image-cache", "0.5"]
TEST = ["test", "m.pth", "defn.yml"]
NEEDS = "--device-image-decode-jpeg widens what --device-image-decode takes: it needs --device-image-decode"


def _error(parser, argv, capsys):
    with pytest.raises(SystemExit):
        parser.parse_args(argv)
    return capsys.readouterr().err


def test_train_and_infer_parsers(capsys):
    from yogo_amd.trainer import build_config
    from yogo_amd.utils.argparsers import global_parser, infer_parser, train_parser

    for base in (INFER, TRAIN):
        assert global_parser().parse_args(base).device_image_decode_jpeg is False
        ns = global_parser().parse_args(base + ["--device-image-decode", "--device-image-decode-jpeg"])
        assert ns.device_image_decode is True and ns.device_image_decode_jpeg is True and ns.device_image_decode_all is False
        assert _error(global_parser(), base + ["--device-image-decode-jpeg"], capsys).endswith(f"error: {NEEDS}\n")
    for parser, argv in ((infer_parser(), INFER[1:]), (train_parser(), TRAIN[1:])):
        assert NEEDS in _error(parser, argv + ["--device-image-decode-jpeg"], capsys)
        assert "--device-image-decode-jpeg" in parser.format_help()
    p = global_parser()
    assert build_config(p.parse_args(TRAIN))["device_image_decode_jpeg"] is False
    assert build_config(p.parse_args(TRAIN + ["--device-image-decode", "--device-image-decode-jpeg"]))["device_image_decode_jpeg"] is True
    ns = p.parse_args(["train", "defn.yml", "--device-image-stream", "--device-image-decode-jpeg"])   # the stream stands in for the cache's decode
    assert ns.device_image_stream and ns.device_image_decode_jpeg


def test_test_parser_needs_the_stream(capsys):
    from yogo_amd.utils.argparsers import global_parser, test_parser

    for p in (global_parser(), None):
        argv = TEST if p is not None else TEST[1:]
        p = p or test_parser()
        assert p.parse_args(argv).device_image_decode_jpeg is False
        assert p.parse_args(argv + ["--device-image-stream"]).device_image_decode_jpeg is False
        assert p.parse_args(argv + ["--device-image-stream", "--device-image-decode-jpeg"]).device_image_decode_jpeg is True
        assert ("--device-image-decode-jpeg widens what --device-image-stream decodes on the GPU: it needs --device-image-stream"
                in _error(p, argv + ["--device-image-decode-jpeg"], capsys))


def test_python_entry_points_refuse_the_flag_alone(tmp_path):
    from yogo_amd.image_cache import ImageCache
    from yogo_amd.infer import predict
    from yogo_amd.yogo_dataloader import get_dataloader

    with pytest.raises(ValueError, match="needs device_image_decode"):
        predict(str(tmp_path / "m.pth"), path_to_images=tmp_path, device_image_decode_jpeg=True)
    with pytest.raises(ValueError) as e:
        get_dataloader(None, 4, 12, 8, device_image_cache_gib=1.0, device_image_decode_jpeg=True)
    assert str(e.value) == NEEDS
    with pytest.raises(ValueError) as e:
        get_dataloader(None, 4, 12, 8, device_image_decode_jpeg=True)
    assert str(e.value) == NEEDS
    with pytest.raises(ValueError) as e:
        ImageCache([0] * 4, 4, (1, 8, 8), False, device_decode_jpeg=True)
    assert str(e.value) == NEEDS


def test_console_test_task_opens_the_jpeg_scope(monkeypatch):
    import yogo_amd.utils.test_model as tm
    import yogo_amd.yogo_dataloader as ydl
    from yogo_amd.__main__ import main

    seen = []
    monkeypatch.setattr(tm, "do_model_test", lambda args: seen.append((ydl._stream_scope, ydl._stream_jpeg)))
    main(TEST)
    main(TEST + ["--device-image-stream"])
    main(TEST + ["--device-image-stream", "--device-image-decode-jpeg"])
    assert seen == [((False, False, False), False), ((True, False, False), False), ((True, False, False), True)]
    assert ydl._stream_scope == (False, False, False) and ydl._stream_jpeg is False


def test_batch_steps_on_a_jpeg_record():
    """a JPEG record holds the file's bytes in its room, needs planes * H * W, takes no row of the inflate launch and is a planar
    entry of every unpack table"""
    from yogo_amd import jpeg, png
    from yogo_amd import png_batch as PB
    from yogo_amd.device_decode import png_unpack, png_unpack_any, png_unpack_planes

    data = F.write("420", 17, 33, 75, "ramp", np.random.default_rng(0))
    room = np.zeros(len(data) + 7, dtype=np.uint8)
    rec = PB.read_jpeg_stream(data, room, lambda info: info.device_decodable, 3)
    assert rec.jpeg is not None and rec.planar and not rec.host and rec.hw == (17, 33) and rec.stored == len(data) and rec.need == 3 * 17 * 33
    assert bytes(room[:len(data)]) == data and rec.stream is None
    assert PB.read_jpeg_stream(data, None, lambda info: True, 1).stream == data
    with pytest.raises(PB.Refused):
        PB.read_jpeg_stream(data, room[:10], lambda info: True, 1)
    with pytest.raises(PB.Refused):
        PB.read_jpeg_stream(data, room, lambda info: False, 1)
    with pytest.raises(jpeg.NotJpeg):
        PB.read_jpeg_stream(b"\x89PNG\r\n\x1a\n", room, lambda info: True, 1)
    host = PB.PngStream(host=True, pixels=np.zeros((3, 17, 33), np.uint8))
    layout = PB.batch_layout([host, rec], 3 * 17 * 33)
    assert layout.need == [3 * 17 * 33] * 2
    assert PB.inflate_rows([host, rec], [0, 256], layout).shape == (0, 5)
    assert PB.unpack_table(png_unpack, [host, rec], layout)[:, 1].tolist() == [1, 1]
    assert PB.unpack_table(png_unpack_planes, [host, rec], layout)[:, 1].tolist() == [PB.KIND_PLANAR] * 2
    assert PB.unpack_table(png_unpack_any, [host, rec], layout)[:, 1].tolist() == [png.FMT_PLANAR] * 2
