"""The device image stream without a GPU (yogo_amd/image_stream.py): how the sampler's order is cut into decode groups, and what the
parsers and ``get_dataloader`` say about ``--device-image-stream`` and the two flags that widen it."""
import pytest

from _image_cache_data import write_defn, write_images


def _check(order, batch_size, streamed, decode_batch):
    """groups() -> its groups, after the properties every result has: every batch once and in order, the DataLoader's boundaries, a
    group within decode_batch unless it is a single batch, and maximal (the next batch would not have fitted)"""
    from yogo_amd.image_stream import groups

    g = groups(order, batch_size, streamed, decode_batch)
    batches = [b for grp in g for b in grp]
    assert batches == [list(order[lo:lo + batch_size]) for lo in range(0, len(order), batch_size)]
    count = [sum(1 for b in grp for i in b if streamed(i)) for grp in g]
    for k, grp in enumerate(g):
        assert len(grp) >= 1 and (count[k] <= decode_batch or len(grp) == 1)
        if k + 1 < len(g):
            assert count[k] + sum(1 for i in g[k + 1][0] if streamed(i)) > decode_batch
    return g


def test_groups_at_every_decode_batch():
    order = [5, 3, 16, 0, 9, 12, 1, 14, 7, 2, 11, 4, 15, 8, 6, 10, 13]   # 17 samples: batches of 4, 4, 4, 4, 1
    everything = lambda i: True   # noqa: E731
    assert [len(g) for g in _check(order, 4, everything, 9)] == [2, 3]           # 8, then 8 + the partial last batch's 1 = 9 <= 9
    assert [len(g) for g in _check(order, 4, everything, 1)] == [1, 1, 1, 1, 1]  # a batch above decode_batch is a group of its own
    assert [len(g) for g in _check(order, 4, everything, 4)] == [1, 1, 1, 1, 1]
    assert [len(g) for g in _check(order, 4, everything, 8)] == [2, 2, 1]        # a partial last batch in a partial last group
    assert [len(g) for g in _check(order, 4, everything, 16)] == [4, 1]
    assert [len(g) for g in _check(order, 4, everything, 17)] == [5]             # the split's size
    assert [len(g) for g in _check(order, 4, everything, 1000)] == [5]
    assert _check([], 4, everything, 9) == []
    assert [len(g) for g in _check(order[:16], 4, everything, 9)] == [2, 2]
    assert [len(g) for g in _check(order, 17, everything, 3)] == [1]


def test_groups_count_streamed_samples_only():
    order = [5, 3, 16, 0, 9, 12, 1, 14, 7, 2, 11, 4, 15, 8, 6, 10, 13, 20, 18, 19, 17]
    # indices < 5 are resident, indices >= 17 are blob indices: neither is decoded.  Streamed per batch: 2, 3, 2, 4, 1, 0
    streamed = lambda i: 5 <= i < 17   # noqa: E731
    assert [len(g) for g in _check(order, 4, streamed, 5)] == [2, 1, 3]          # the blob batch rides with the last group
    assert [len(g) for g in _check(order, 4, streamed, 1000)] == [6]
    assert [len(g) for g in _check(order, 4, streamed, 1)] == [1, 1, 1, 1, 2]    # 1 + 0 streamed samples fit together
    # an all-resident batch inside a group: batches stream 2, 0, 2
    order2 = [5, 6, 0, 1, 2, 3, 4, 0, 7, 8, 1, 2]
    assert [len(g) for g in _check(order2, 4, streamed, 4)] == [3]
    assert [len(g) for g in _check(order2, 4, streamed, 3)] == [2, 1]
    assert [len(g) for g in _check(order2, 4, lambda i: False, 1)] == [3]


def test_groups_refuse_bad_sizes():
    from yogo_amd.image_stream import groups
    from yogo_amd.png_prefill import MAX_DECODE_BATCH

    for bad in (0, -1, MAX_DECODE_BATCH + 1):
        with pytest.raises(ValueError, match="decode_batch"):
            groups([0, 1], 2, lambda i: True, bad)
    with pytest.raises(ValueError, match="batch_size"):
        groups([0, 1], 0, lambda i: True, 4)


TRAIN = ["train", "tests/fake-data/defns/train_val_test.yml"]
TEST = ["test", "m.pth", "defn.yml"]


def _error(parser, argv, capsys):
    with pytest.raises(SystemExit):
        parser.parse_args(argv)
    return capsys.readouterr().err


def test_train_parser_takes_stream_in_decodes_place(capsys):
    from yogo_amd.trainer import build_config
    from yogo_amd.utils.argparsers import global_parser

    p = global_parser()
    assert p.parse_args(TRAIN).device_image_stream is False and build_config(p.parse_args(TRAIN))["device_image_stream"] is False
    ns = p.parse_args(TRAIN + ["--device-image-stream"])
    assert ns.device_image_stream is True and ns.device_image_cache is None and build_config(ns)["device_image_stream"] is True
    for widening in ("--device-image-resize", "--device-image-decode-all"):
        ns = p.parse_args(TRAIN + ["--device-image-stream", widening])
        assert getattr(ns, widening[2:].replace("-", "_")) is True
    ns = p.parse_args(TRAIN + ["--device-image-stream", "--device-image-cache", "2", "--device-image-decode", "--device-image-resize"])
    assert ns.device_image_stream and ns.device_image_decode and ns.device_image_cache == 2.0
    # without the stream: the texts of before, byte for byte
    assert _error(p, TRAIN + ["--device-image-resize"], capsys).endswith(
        "error: --device-image-resize resizes what the device decoded: it needs --device-image-decode\n")
    assert _error(p, TRAIN + ["--device-image-decode-all"], capsys).endswith(
        "error: --device-image-decode-all widens what --device-image-decode takes: it needs --device-image-decode\n")
    assert _error(p, TRAIN + ["--device-image-decode"], capsys).endswith(
        "error: --device-image-decode fills the device image cache: it needs --device-image-cache GIB\n")
    # the stream does not stand in for the cache that --device-image-decode fills
    assert _error(p, TRAIN + ["--device-image-decode", "--device-image-stream"], capsys).endswith(
        "error: --device-image-decode fills the device image cache: it needs --device-image-cache GIB\n")


def test_test_parser_accepts_the_three_flags(capsys):
    from yogo_amd.utils.argparsers import global_parser, test_parser

    for p in (global_parser(), None):
        argv = TEST if p is not None else TEST[1:]
        p = p or test_parser()
        ns = p.parse_args(argv)
        assert (ns.device_image_stream, ns.device_image_decode_all, ns.device_image_resize) == (False, False, False)
        ns = p.parse_args(argv + ["--device-image-stream", "--device-image-decode-all", "--device-image-resize"])
        assert (ns.device_image_stream, ns.device_image_decode_all, ns.device_image_resize) == (True, True, True)
        assert p.parse_args(argv + ["--device-image-stream"]).device_image_decode_all is False
        for widening in ("--device-image-resize", "--device-image-decode-all"):
            assert f"{widening} widens what --device-image-stream decodes on the GPU: it needs --device-image-stream" in _error(p, argv + [widening], capsys)


def test_help_says_what_the_stream_costs():
    from yogo_amd.utils.argparsers import test_parser, train_parser

    for p in (train_parser(), test_parser()):
        text = " ".join(p.format_help().split())
        assert "--device-image-stream" in text and "GPU memory" in text and "pinned host memory" in text and "first batch waits" in text


def test_get_dataloader_argument_errors(tmp_path):
    from yogo_amd.dataset_definition_file import DatasetDefinition
    from yogo_amd.yogo_dataloader import get_dataloader

    img_dir, lab_dir = write_images(tmp_path / "data", 8)
    defn = DatasetDefinition.from_yaml(write_defn(tmp_path, img_dir, lab_dir))
    kw = dict(image_hw=(64, 96))
    with pytest.raises(ValueError) as e:
        get_dataloader(defn, 4, 12, 8, device_image_resize=True, **kw)
    assert str(e.value) == "--device-image-resize resizes what the device decoded: it needs --device-image-decode"
    with pytest.raises(ValueError) as e:
        get_dataloader(defn, 4, 12, 8, device_image_decode_all=True, **kw)
    assert str(e.value) == "--device-image-decode-all widens what --device-image-decode takes: it needs --device-image-decode"
    for stream in (False, True):   # the stream is no cache: device_image_decode without one keeps raising
        with pytest.raises(ValueError) as e:
            get_dataloader(defn, 4, 12, 8, device_image_decode=True, device_image_stream=stream, **kw)
        assert str(e.value) == "--device-image-decode fills the device image cache: it needs --device-image-cache GIB"
    for bad in (0, 65536):
        with pytest.raises(ValueError, match="decode_batch"):
            get_dataloader(defn, 4, 12, 8, device_image_stream=True, stream_decode_batch=bad, **kw)


def test_stream_loaders_allocate_nothing_before_they_are_iterated(tmp_path):
    """with the switch on every split gets a stream over one shared scratch, with both widening switches passed on; the host loader
    is there for dataset / sampler / batch_size / len alone and has no workers; nothing touches a device before the first iteration"""
    from yogo_amd.dataset_definition_file import DatasetDefinition
    from yogo_amd.png_prefill import DEFAULT_DECODE_BATCH
    from yogo_amd.yogo_dataloader import get_dataloader

    img_dir, lab_dir = write_images(tmp_path / "data", 8)
    defn = DatasetDefinition.from_yaml(write_defn(tmp_path, img_dir, lab_dir))
    plain = get_dataloader(defn, 4, 12, 8, image_hw=(64, 96))
    assert all(dl.stream is None for dl in plain.values())
    dls = get_dataloader(defn, 4, 12, 8, image_hw=(64, 96), rgb=True, device_image_stream=True, device_image_resize=True, device_image_decode_all=True)
    sc = dls["train"].stream.scratch
    assert dls["val"].stream.scratch is sc and sc.filler is None and sc.staging == []
    assert (sc.decode_batch, sc.capacity, sc.image_shape, sc.device_resize, sc.decode_all) == (DEFAULT_DECODE_BATCH, DEFAULT_DECODE_BATCH, (3, 64, 96), True, True)
    assert 1 <= sc.max_threads <= 16
    for name in ("train", "val"):
        assert dls[name].loader.num_workers == 0 and len(dls[name]) == len(plain[name]) and dls[name].batch_size == 4
        assert dls[name].stream.stats["groups"] == 0 and dls[name].cache is None
    sc.close()   # (nothing to release: a no-op)
    assert get_dataloader(defn, 64, 12, 8, image_hw=(64, 96), device_image_stream=True, stream_decode_batch=9)["train"].stream.scratch.capacity == 64


def test_scope_turns_the_stream_on_for_get_dataloader(tmp_path):
    """`yogo test --device-image-stream`: inside the scope a ``get_dataloader`` call with the reference's arguments streams"""
    import yogo_amd.yogo_dataloader as ydl
    from yogo_amd.dataset_definition_file import DatasetDefinition

    img_dir, lab_dir = write_images(tmp_path / "data", 8)
    defn = DatasetDefinition.from_yaml(write_defn(tmp_path, img_dir, lab_dir))
    seen = []
    for scope in ((False, True, True), (True, False, False), (True, True, True)):
        with ydl.device_image_stream_scope(*scope):
            sc = ydl.get_dataloader(defn, 4, 12, 8, image_hw=(64, 96))["train"].stream
            seen.append(None if sc is None else (sc.scratch.decode_all, sc.scratch.device_resize))
    assert seen == [None, (False, False), (True, True)] and ydl._stream_scope == (False, False, False)
    assert ydl.get_dataloader(defn, 4, 12, 8, image_hw=(64, 96))["train"].stream is None


def test_console_test_task_opens_the_stream_scope(monkeypatch):
    import torch

    import yogo_amd.__main__ as main_mod
    import yogo_amd.utils.test_model as tm
    import yogo_amd.yogo_dataloader as ydl

    seen = []
    monkeypatch.setattr(tm, "do_model_test", lambda args: seen.append(ydl._stream_scope))
    monkeypatch.setattr(torch.multiprocessing, "set_start_method", lambda *a, **k: None)
    main_mod.main(TEST)
    main_mod.main(TEST + ["--device-image-stream"])
    main_mod.main(TEST + ["--device-image-stream", "--device-image-decode-all", "--device-image-resize"])
    assert seen == [(False, False, False), (True, False, False), (True, True, True)] and ydl._stream_scope == (False, False, False)
