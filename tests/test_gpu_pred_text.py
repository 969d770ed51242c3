"""The text of `yogo infer --save-preds --device-outputs`, formatted on the device (yogo_amd/csrc/pred_text.hip, float_text.h,
`PredictionSink.drain_text`, `predict`): every comparison is bytes against the bytes of the host formatter `prediction_rows_to_text`
(Python's own `repr` of each float32) -- no tolerance anywhere.
* through the C ABI: records whose fields carry the structured float32 set of tests/_float_text_cases.py and 200 000 random bit
  patterns, images of 0 / 1 / many rows, runs of empty images, no records, no images;
* the class index (Python's `max(range(C), key=...)`: ties, equal scores, -inf, NaNs);
* the capacity check (guard bytes), inconsistent counts, argument errors without a launch;
* `drain_text` over several appends, drains in between and the growth path, against `drain()` + the host formatter;
* end to end: `predict(save_preds=True)` writes the same files with and without `device_outputs=True`, and the device route does not
  call the host formatter."""
import ctypes

import numpy as np
import pytest
import torch
from _float_text_cases import structured_bits

pytestmark = pytest.mark.gpu
CLASSES = ["you", "only", "glance", "once"]
GUARD = 64


# -----------------------------------------------------------------------------------------------------------------------------------
# the ABI and the host reference
# -----------------------------------------------------------------------------------------------------------------------------------
def _bound(n, images, P):
    from yogo_amd import _hip

    tb, wb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _hip.call("yogo_pred_text_bound", n, images, P, ctypes.addressof(tb), ctypes.addressof(wb))
    return int(tb.value), int(wb.value)


def _format(records, counts, cap=None, n=None, images=None):
    """yogo_pred_text_format on host arrays records [N, P] / counts [images]: (the whole text buffer with GUARD bytes behind `cap`, the
    offsets, the total, cap).  The buffers start as 0xAB / -5 / -7, so what the call did not write shows."""
    from yogo_amd import _hip

    P = records.shape[1]
    n = records.shape[0] if n is None else n
    images = len(counts) if images is None else images
    tb, wb = _bound(n, images, P)
    cap = tb if cap is None else cap
    text = torch.full((cap + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    offs = torch.full((images + 1,), -5, dtype=torch.int64, device="cuda")
    total = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    ws = torch.empty(max(wb, 8), dtype=torch.uint8, device="cuda")
    rec_d = torch.from_numpy(np.ascontiguousarray(records)).cuda() if records.shape[0] else None
    cnt_d = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).cuda() if len(counts) else None
    _hip.call("yogo_pred_text_format", rec_d, n, P, cnt_d, images, text, cap, offs, total, ws, _hip.stream_ptr())
    return text.cpu().numpy(), offs.cpu().numpy(), int(total), cap


def _reference(records, counts):
    """(the bytes of all images back to back, offsets [images + 1]) from prediction_rows_to_text per image"""
    from yogo_amd.pred_sink import split_records
    from yogo_amd.utils.prediction_formatting import prediction_rows_to_text

    texts = [prediction_rows_to_text(torch.from_numpy(np.ascontiguousarray(r))).encode("ascii") for r in split_records(records, counts)]
    return b"".join(texts), np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.int64)


def _check(records, counts):
    want_text, want_offs = _reference(records, counts)
    buf, offs, total, cap = _format(records, counts)
    assert total == len(want_text) and total <= cap
    assert np.array_equal(offs, want_offs)
    got = buf[:total].tobytes()
    if got != want_text:   # name the first image that differs
        for k in range(len(counts)):
            a, b = got[offs[k]: offs[k + 1]], want_text[want_offs[k]: want_offs[k + 1]]
            assert a == b, (k, a[:200], b[:200])
    assert bool((buf[total:] == 0xAB).all())   # nothing behind the text, guard included
    return want_text


def _field_values():
    """the structured set and 200 000 random bit patterns, as float32"""
    rnd = np.random.default_rng(31).integers(0, 1 << 32, size=200_000, dtype=np.uint64).astype(np.uint32)
    fractions = np.concatenate([np.arange(130, dtype=np.float32) / np.float32(129), np.arange(98, dtype=np.float32) / np.float32(97)])
    return np.concatenate([structured_bits(), rnd, fractions.view(np.uint32)]).view(np.float32)


def _image_counts(n):
    """counts that sum to n: first and last image empty, images of 1 row, of many rows (more than a workgroup's 256 records), runs of
    empty images, and more images (600 small ones) than the single-workgroup scan has lanes"""
    head = [0, 1, 300, 0, 0, 0, 5, 257, 0, 1, 1, 256, 0, 0]
    small = [k % 4 for k in range(600)]
    rest = n - sum(head) - sum(small)
    assert rest > 1000
    return np.array(head + small + [rest - 7, 0, 0, 7, 0], dtype=np.int32)


@pytest.mark.parametrize("C", [1, 7])
def test_text_through_the_abi(C):
    vals = _field_values()
    n = len(vals) // 4
    rng = np.random.default_rng(5 + C)
    rec = np.empty((n, 5 + C), dtype=np.float32)
    rec[:, :4] = vals[: 4 * n].reshape(n, 4)          # several values per record, in the order of the set
    rec[:, 4] = rng.random(n, dtype=np.float32)
    rec[:, 5:] = rng.random((n, C), dtype=np.float32)
    counts = _image_counts(n)
    text = _check(rec, counts)
    for s in (b"9.999999747378752e-05", b"9.999999747378752e-06", b"9999999198822400.0", b"1.0000000272564224e+16", b" inf", b" -inf", b" nan",
              b" -0.0", b"1.401298464324817e-45"):
        assert s in text, s
    if C == 7:
        assert {ln.split(b" ")[0] for ln in text.split(b"\n")} == {str(k).encode() for k in range(7)}


def test_empty_shapes():
    rec = np.random.default_rng(1).random((6, 9), dtype=np.float32)
    _check(rec[:1], np.array([1]))                                    # one image, one row
    _check(rec[:1], np.array([0, 0, 1, 0, 0]))
    _check(rec, np.array([0, 0, 0, 2, 0, 0, 0, 0, 4, 0, 0]))          # runs of empty images, at both ends too
    _check(rec, np.array([6]))
    # no records: every offset and the total are zero, nothing is launched
    from yogo_amd import _hip

    _hip.launch_log(True)
    try:
        buf, offs, total, _ = _format(rec[:0], np.zeros(5, dtype=np.int32))
        assert total == 0 and offs.tolist() == [0] * 6 and bool((buf == 0xAB).all())
        buf, offs, total, _ = _format(rec[:0], np.zeros(0, dtype=np.int32))   # no images either
        assert total == 0 and offs.tolist() == [0] and bool((buf == 0xAB).all())
        assert _hip.read_launch_log() == []
    finally:
        _hip.launch_log(False)
    assert _bound(0, 0, 9) == (0, 8)


def test_class_index_mirrors_python_max():
    """idx = 0; for k in 1 .. C - 1: if s[k] > s[idx]: idx = k -- the first maximum, and a NaN never displaces the current best (nor is
    displaced when it leads): not the NaN-is-the-maximum rule of the class counts"""
    nan, inf = float("nan"), float("inf")
    scores = [[0.2, 0.7, 0.7, 0.1, 0.7], [0.5] * 5, [0.0, -0.0, 0.0, -0.0, 0.0], [-inf] * 5, [-inf, -inf, -1e38, -inf, -inf],
              [nan, 0.5, 0.9, 0.1, 0.2], [0.3, nan, 0.9, 0.1, 0.2], [0.3, 0.1, nan, 0.2, 0.25], [nan] * 5, [0.1, 0.2, 0.3, 0.4, nan],
              [-inf, inf, inf, 0.0, 1.0], [0.1, 0.2, 0.3, 0.4, 0.5], [0.5, 0.4, 0.3, 0.2, 0.1]]
    rec = np.zeros((len(scores), 10), dtype=np.float32)
    rec[:, :4] = [0.25, 0.5, 0.125, 0.0625]
    rec[:, 5:] = np.array(scores, dtype=np.float32)
    text = _check(rec, np.array([len(scores)]))
    got = [int(ln.split(b" ")[0]) for ln in text.split(b"\n")]
    assert got == [1, 0, 0, 0, 2, 0, 2, 0, 0, 3, 1, 4, 0]            # what the reference is expected to say
    assert text.split(b"\n")[0] == b"1 0.25 0.5 0.125 0.0625"


def test_text_capacity_is_respected():
    rec = np.random.default_rng(2).random((700, 12), dtype=np.float32)
    counts = np.array([0, 300, 399, 1, 0])
    want, _ = _reference(rec, counts)
    buf, offs, total, cap = _format(rec, counts, cap=len(want))      # exactly enough
    assert total == len(want) and buf[:total].tobytes() == want and bool((buf[cap:] == 0xAB).all())
    buf, offs, total, cap = _format(rec, counts, cap=len(want) - 1)  # one byte short: reported, and nothing at or past text_cap
    assert total == len(want) and total > cap
    assert bool((buf[cap:] == 0xAB).all())
    assert buf[:cap].tobytes() == want[:cap]
    buf, offs, total, cap = _format(rec, counts, cap=0)              # a measuring run
    assert total == len(want) and bool((buf == 0xAB).all())


def test_inconsistent_counts_are_refused():
    rec = np.random.default_rng(3).random((20, 8), dtype=np.float32)
    for counts in ([5, 5, 5], [10, 11], [25, -5], [-1, 21], [0, 0, 0]):
        buf, offs, total, _ = _format(rec, np.array(counts))
        assert total == -1, counts
        assert bool((buf == 0xAB).all()) and bool((offs == -5).all()), counts
    buf, offs, total, _ = _format(rec, np.array([10, 10]), n=19)     # the records' count is the one that is off
    assert total == -1 and bool((buf == 0xAB).all())


def test_argument_errors_do_not_launch():
    from yogo_amd import _hip

    dev = torch.device("cuda")
    n, images, P = 6, 2, 9
    rec = torch.zeros(n, P, device=dev)
    counts = torch.tensor([2, 4], dtype=torch.int32, device=dev)
    text = torch.zeros(4096, dtype=torch.uint8, device=dev)
    offs = torch.zeros(images + 1, dtype=torch.int64, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.zeros(4096, dtype=torch.uint8, device=dev)
    good = dict(records=rec, n=n, P=P, img_counts=counts, images=images, text=text, text_cap=4096, img_offsets=offs, total=total, workspace=ws)

    def call(**kw):
        a = {**good, **kw}
        _hip.call("yogo_pred_text_format", a["records"], a["n"], a["P"], a["img_counts"], a["images"], a["text"], a["text_cap"], a["img_offsets"],
                  a["total"], a["workspace"], _hip.stream_ptr())

    _hip.launch_log(True)
    try:
        for bad in (dict(records=None), dict(img_counts=None), dict(text=None), dict(img_offsets=None), dict(total=None), dict(workspace=None),
                    dict(n=-1), dict(images=-1), dict(text_cap=-1), dict(P=5), dict(images=0), dict(n=1 << 31), dict(images=1 << 31)):
            with pytest.raises(RuntimeError, match="code 1"):
                call(**bad)
        out = (ctypes.c_size_t * 2)()
        for args in ((-1, 1, 9), (1, -1, 9), (1, 1, 5), (1 << 31, 1, 9)):
            with pytest.raises(RuntimeError, match="code 1"):
                _hip.call("yogo_pred_text_bound", *args, ctypes.addressof(out), ctypes.addressof(out) + 8)
        with pytest.raises(RuntimeError, match="code 1"):
            _hip.call("yogo_pred_text_bound", 1, 1, 9, None, ctypes.addressof(out))
        assert _hip.read_launch_log() == []
        call()
        assert len(_hip.read_launch_log()) == 1
    finally:
        _hip.launch_log(False)
    assert int(total) == len("0 0.0 0.0 0.0 0.0") * n + (n - images)


# -----------------------------------------------------------------------------------------------------------------------------------
# PredictionSink.drain_text
# -----------------------------------------------------------------------------------------------------------------------------------
def _batch(B, cap, P, counts, seed):
    """rows [B, cap, P] with NaN past counts[b]; boxes in [0, 1) with a few exact and tiny values mixed in"""
    g = torch.Generator().manual_seed(seed)
    rows = torch.full((B, cap, P), float("nan"))
    for b, n in enumerate(counts):
        r = torch.rand(n, P, generator=g)
        r[::3, 0] = 0.5
        r[1::4, 2] *= 1e-5
        rows[b, :n] = r
    return rows.cuda(), torch.tensor(counts, dtype=torch.int32).cuda()


def _host_text(sink):
    """drain() + split_records + prediction_rows_to_text, in drain_text's form"""
    return _reference(*sink.drain())


def _sinks(C):
    from yogo_amd.pred_sink import PredictionSink

    return PredictionSink(torch.device("cuda"), C, "rows"), PredictionSink(torch.device("cuda"), C, "rows")


def _same_drain(dev_sink, host_sink, images):
    text, offs = dev_sink.drain_text()
    want_text, want_offs = _host_text(host_sink)
    assert text.dtype == np.uint8 and offs.dtype == np.int64 and offs.shape == (images + 1,)
    assert np.array_equal(offs, want_offs) and text.tobytes() == want_text
    return want_text


def test_drain_text_over_appends_and_drains():
    a, b = _sinks(7)
    batches = [_batch(3, 40, 12, c, seed=20 + k) for k, c in enumerate(([40, 0, 17], [0, 0, 1], [5, 40, 39], [0, 0, 0]))]
    for s in (a, b):
        s.append(*batches[0], 0)
        s.append(*batches[1], 3)
    assert len(_same_drain(a, b, 6)) > 1000
    for s in (a, b):
        s.append(*batches[2], 6)
        s.append(*batches[3], 9)
    _same_drain(a, b, 6)
    for s in (a, b):                                                  # only empty images
        s.append(*batches[3], 12)
    text, offs = a.drain_text()
    assert text.shape == (0,) and offs.tolist() == [0, 0, 0, 0]
    text, offs = a.drain_text()                                       # nothing appended
    assert text.shape == (0,) and text.dtype == np.uint8 and offs.tolist() == [0] and offs.dtype == np.int64
    b.drain()
    for s in (a, b):                                                  # usable again
        s.append(*batches[0], 15)
    _same_drain(a, b, 3)


def test_drain_text_after_growth():
    a, b = _sinks(7)
    seq = [_batch(1, 4, 12, [3], seed=40), _batch(3, 40, 12, [40, 40, 40], seed=41), _batch(3, 40, 12, [39, 0, 40], seed=42),
           _batch(600, 4, 12, [k % 5 for k in range(600)], seed=43), _batch(600, 4, 12, [(k + 2) % 5 for k in range(600)], seed=44)]
    first = None
    for k, (rows, counts) in enumerate(seq):
        for s in (a, b):
            s.append(rows, counts, 100 * k)
        if first is None:
            first = (a.arena.shape[0], a.img_counts.shape[0])
    assert first == (8, 1024) and a.arena.shape[0] > 8 and a.img_counts.shape[0] > 1024
    _same_drain(a, b, 1 + 3 + 3 + 600 + 600)


def test_drain_text_needs_a_rows_sink():
    from yogo_amd.pred_sink import PredictionSink

    with pytest.raises(ValueError, match="rows"):
        PredictionSink(torch.device("cuda"), 4, "npy", img_hw=(64, 96)).drain_text()


# -----------------------------------------------------------------------------------------------------------------------------------
# end to end (the checkpoint and the inputs of tests/test_gpu_pred_sink.py, same sizes)
# -----------------------------------------------------------------------------------------------------------------------------------
def _make_checkpoint(tmp_path, seed=3):
    from yogo_amd.model import YOGO

    torch.manual_seed(seed)
    net = YOGO((64, 96), 0.0425, 0.0555, 4).cuda()
    net.eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 50.0)
                m.running_var.uniform_(2000.0, 9000.0)
        net.model[7].bias[4] += 2.0
    p = tmp_path / "m.pth"
    torch.save({"epoch": 0, "step": 7, "normalize_images": False, "classes": CLASSES, "model_name": "fake_model",
                "model_state_dict": {k: v.cpu() for k, v in net.state_dict().items()}, "model_version": "base_model"}, p)
    return p


@pytest.fixture(scope="module")
def e2e_inputs(tmp_path_factory):
    """10 random 64 x 96 frames as a PNG directory and as a zarr zip, and a checkpoint"""
    import _zarr_write as ZW
    from PIL import Image

    d = tmp_path_factory.mktemp("text_e2e")
    frames = np.random.default_rng(6).integers(0, 256, size=(64, 96, 10), dtype=np.uint8)
    (d / "png").mkdir()
    for i in range(10):
        Image.fromarray(frames[:, :, i]).save(d / "png" / f"img_{i:02d}.png")
    z = ZW.write_stack(d / "stack.zip", frames, (64, 96, 1), as_zip=True)
    return d / "png", z, _make_checkpoint(d)


@pytest.mark.parametrize("source", ["png", "zarr"])
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "bf16"])
def test_predict_writes_the_same_files_without_the_host_formatter(e2e_inputs, tmp_path, monkeypatch, half, source):
    import yogo_amd.infer
    from yogo_amd.infer import predict

    pngs, z, pth = e2e_inputs
    src = dict(path_to_images=pngs) if source == "png" else dict(path_to_zarr=z)
    base = dict(save_preds=True, batch_size=4, half=half, class_names=CLASSES, **src)   # 10 frames: the last batch is partial
    predict(str(pth), output_dir=str(tmp_path / "host"), device_outputs=False, **base)

    def forbidden(rows):
        raise AssertionError("prediction_rows_to_text was called on the device-outputs route")

    with monkeypatch.context() as m:   # the device route formats on the device: the host formatter is not reachable from it
        m.setattr(yogo_amd.infer, "prediction_rows_to_text", forbidden)
        m.setattr("yogo_amd.utils.prediction_formatting.prediction_rows_to_text", forbidden)
        predict(str(pth), output_dir=str(tmp_path / "dev"), device_outputs=True, **base)
    names = [f"img_{i:02d}.txt" for i in range(10)]
    a, b = tmp_path / "host", tmp_path / "dev"
    assert sorted(f.name for f in a.iterdir()) == names and sorted(f.name for f in b.iterdir()) == names
    texts = [(a / n).read_bytes() for n in names]
    lines = sum(len(t.splitlines()) for t in texts)
    print(f"txt: {lines} lines, per image {[len(t.splitlines()) for t in texts]}")
    assert lines >= 10 and sum(1 for t in texts if t) >= 2            # not vacuous (the checkpoint's objectness bias)
    for n, t in zip(names, texts):
        assert (b / n).read_bytes() == t, n
