"""The host half of `yogo infer --device-outputs` (yogo_amd/pred_sink.py): the flag, the keyword, the refusal of a CPU device, the
per-image split of drained records and the state-layout query -- none of which needs a device."""
import inspect

import numpy as np
import pytest
import torch


def test_parser_accepts_device_outputs_and_defaults_to_false():
    from yogo_amd.utils.argparsers import infer_parser

    p = infer_parser()
    assert p.parse_args(["m.pth", "--path-to-images", "x"]).device_outputs is False
    assert p.parse_args(["m.pth", "--path-to-images", "x", "--device-outputs"]).device_outputs is True
    assert p.parse_args(["m.pth", "--path-to-images", "x", "--no-device-outputs"]).device_outputs is False


def test_predict_has_the_keyword():
    from yogo_amd.infer import predict

    par = inspect.signature(predict).parameters["device_outputs"]
    assert par.default is False and par.kind is inspect.Parameter.KEYWORD_ONLY


def test_sink_on_a_cpu_device_raises_the_no_fallback_error():
    from yogo_amd.pred_sink import PredictionSink

    for mode, hw in (("npy", (64, 96)), ("rows", None)):
        with pytest.raises(RuntimeError, match="there is no CPU fallback"):
            PredictionSink(torch.device("cpu"), 4, mode, img_hw=hw)
        with pytest.raises(RuntimeError, match="there is no CPU fallback"):
            PredictionSink("cpu", 4, mode, img_hw=hw)


def test_split_records_by_image():
    from yogo_amd.pred_sink import split_records

    rec = np.arange(6 * 3, dtype=np.float32).reshape(6, 3)
    # zero rows at the start, in the middle and at the end
    counts = np.array([0, 2, 0, 0, 3, 1, 0], dtype=np.int32)
    parts = split_records(rec, counts)
    assert [p.shape for p in parts] == [(0, 3), (2, 3), (0, 3), (0, 3), (3, 3), (1, 3), (0, 3)]
    assert np.array_equal(parts[1], rec[0:2]) and np.array_equal(parts[4], rec[2:5]) and np.array_equal(parts[5], rec[5:6])
    assert all(p.dtype == np.float32 for p in parts)
    assert np.shares_memory(parts[4], rec)                       # views, not copies
    assert np.array_equal(np.concatenate(parts, axis=0), rec)
    # nothing at all, images without any record, one image holding everything
    assert split_records(np.zeros((0, 3), np.float32), np.zeros(0, np.int32)) == []
    assert [p.shape for p in split_records(np.zeros((0, 5), np.float32), [0, 0])] == [(0, 5), (0, 5)]
    assert np.array_equal(split_records(rec, [6])[0], rec)
    # counts that do not add up to the records are an error, not a silent truncation
    with pytest.raises(ValueError):
        split_records(rec, [1, 2])
    with pytest.raises(ValueError):
        split_records(rec, [7, -1])


def test_state_layout_query_answers_without_a_device():
    from yogo_amd.pred_sink import state_layout

    for C in (1, 4, 7, 255):
        off_rows, off_images, off_dropped, off_dropped_images, off_counts, words = state_layout(C)
        scalars = [off_rows, off_images, off_dropped, off_dropped_images]
        assert len(set(scalars)) == 4 and all(0 <= o < words for o in scalars)
        cls = set(range(off_counts, off_counts + C))
        assert off_counts + C <= words and not cls & set(scalars)
    from yogo_amd import _hip

    with pytest.raises(RuntimeError, match="code 1"):
        state_layout(0)
    with pytest.raises(RuntimeError, match="code 1"):
        _hip.call("yogo_pred_sink_state_layout", 4, None)


def test_npy_columns_equal_the_default_paths_hstack_bytes():
    """the saved array of the sink path against np.hstack over `_rows_xyxy_to_numpy` of the same rows, as np.save writes both (the
    header records the memory order, which numpy derives from the pieces: images without rows, with one row, with several)"""
    import io

    from yogo_amd.pred_sink import npy_columns
    from yogo_amd.utils.prediction_formatting import _rows_xyxy_to_numpy

    def saved(a):
        b = io.BytesIO()
        np.save(b, a)
        return b.getvalue()

    g = torch.Generator().manual_seed(0)
    for counts in ([0], [1], [2], [0, 0], [1, 1], [2, 2], [0, 5, 1], [3, 0, 7, 1, 6], [1, 1, 3], [0, 0, 3], [5, 1, 2, 4]):
        rows = [torch.rand(n, 9, generator=g) for n in counts]
        host = np.hstack([_rows_xyxy_to_numpy(10 + b, r, 772, 1032, np.float32) for b, r in enumerate(rows)])
        rec, per = np.ascontiguousarray(host.T), np.array(counts, dtype=np.int32)   # what a sink drains
        k = len(counts) // 2
        nk = int(per[:k].sum())
        for chunks in ([(rec, per)], [(rec[:nk].copy(), per[:k]), (rec[nk:].copy(), per[k:])]):   # one drain; a flush in between
            got = npy_columns(chunks, 4)
            assert got.dtype == np.float32 and np.array_equal(got, host) and saved(got) == saved(host), counts
    assert saved(npy_columns([], 4)) == saved(np.zeros((12, 0), dtype=np.float32))
