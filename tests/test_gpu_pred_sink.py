"""The device half of `yogo infer --device-outputs` (yogo_amd/csrc/pred_sink.hip, yogo_amd/pred_sink.py, `predict(device_outputs=True)`):
* the kernel driven directly with hand-made rows / counts against the host code of the default path applied to rows.cpu() /
  counts.cpu() (`_rows_xyxy_to_numpy`, `count_cells_for_formatted_preds`, slicing) -- exact equality, no tolerance anywhere;
* the state carried over several appends, the capacity limits (through the ABI, with a guard region) and the growth path;
* argument errors without a launch;
* end to end: `predict` with and without `device_outputs=True` writes the same files and prints the same counts."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
CLASSES = ["you", "only", "glance", "once"]
IMG_H, IMG_W = 772, 1032


# -----------------------------------------------------------------------------------------------------------------------------------
# inputs and the host reference
# -----------------------------------------------------------------------------------------------------------------------------------
def _make_rows(B, cap, P, counts, seed):
    """rows [B, cap, P] with NaN beyond counts[b] (any read of that area shows), boxes in [0, 1], class scores all distinct within a
    row (a permutation of a grid plus jitter), some rows with every score <= 0 so that the > 0 rule is exercised"""
    g = torch.Generator().manual_seed(seed)
    C = P - 5
    rows = torch.full((B, cap, P), float("nan"))
    for b, n in enumerate(counts):
        if n == 0:
            continue
        r = torch.rand(n, P, generator=g)
        base = (torch.arange(C, dtype=torch.float32) + 1) / (C + 1)                  # distinct levels, spacing 1 / (C + 1)
        perm = torch.stack([base[torch.randperm(C, generator=g)] for _ in range(n)])
        r[:, 5:] = perm + (torch.rand(n, C, generator=g) - 0.5) * 0.5 / (C + 1)        # jitter below half the spacing: no ties
        neg = torch.rand(n, generator=g) < 0.2
        r[neg, 5:] -= 2.0                                                              # every score <= 0: not counted
        rows[b, :n] = r
    return rows, torch.tensor(counts, dtype=torch.int32)


def _ref_npy(rows, counts, first_img_id):
    """what the default path's format_to_numpy_batched computes from the host copy: [N, 8 + C] (its columns are the records)"""
    from yogo_amd.utils.prediction_formatting import _rows_xyxy_to_numpy

    C = rows.shape[2] - 5
    parts = [_rows_xyxy_to_numpy(first_img_id + b, rows[b, :n], IMG_H, IMG_W, np.float32) for b, n in enumerate(counts.tolist())]
    out = np.hstack(parts).T if parts else np.zeros((0, 8 + C), np.float32)
    assert out.dtype == np.float32
    return out


def _ref_rows(rows, counts):
    return torch.cat([rows[b, :n] for b, n in enumerate(counts.tolist())]).numpy() if len(counts) else np.zeros((0, rows.shape[2]), np.float32)


def _ref_class_counts(rows, counts):
    """get_prediction_class_counts' loop over the host copy"""
    from yogo_amd.utils.prediction_formatting import count_cells_for_formatted_preds

    tot = torch.zeros(rows.shape[2] - 5, dtype=torch.long)
    for b, n in enumerate(counts.tolist()):
        if n:
            tot += count_cells_for_formatted_preds(rows[b, :n, 5:])
    return tot


def _same(a, b):
    """exact equality that also holds a NaN equal to a NaN: the bits"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


_CASES = {
    "1x4x6-empty": (1, 4, 6, [0]),
    "3x5x12": (3, 5, 12, [0, 5, 1]),
    "5x7x21-mixed": (5, 7, 21, [3, 0, 7, 1, 6]),
    "515x4x12-cycling": (515, 4, 12, [b % 5 for b in range(515)]),     # more images than a single-workgroup scan is wide
    "2x300x12-full": (2, 300, 12, [300, 17]),                          # more rows than one workgroup has lanes
}


@pytest.fixture(scope="module")
def cases():
    """per case: host rows / counts, their device copies and the three references, computed once"""
    out = {}
    for k, (name, (B, cap, P, counts)) in enumerate(_CASES.items()):
        rows, cnt = _make_rows(B, cap, P, counts, seed=100 + k)
        out[name] = dict(rows=rows, counts=cnt, drows=rows.cuda(), dcounts=cnt.cuda(), npy=_ref_npy(rows, cnt, 1000), flat=_ref_rows(rows, cnt),
                         cls=_ref_class_counts(rows, cnt))
    return out


def _sink(mode, C):
    from yogo_amd.pred_sink import PredictionSink

    return PredictionSink(torch.device("cuda"), C, mode, img_hw=(IMG_H, IMG_W) if mode == "npy" else None)


@pytest.mark.parametrize("name", list(_CASES))
def test_npy_records(cases, name):
    c = cases[name]
    s = _sink("npy", c["rows"].shape[2] - 5)
    s.append(c["drows"], c["dcounts"], 1000, count_classes=True)
    rec, per = s.drain()
    assert _same(rec, c["npy"])
    assert per.dtype == np.int32 and np.array_equal(per, c["counts"].numpy())
    assert torch.equal(s.class_counts(), c["cls"]) and s.class_counts().dtype == torch.int64
    n = rec.shape[0]
    if n:   # ids are first_img_id + b, in image order
        want_ids = np.repeat(np.arange(len(per)) + 1000, per).astype(np.float32)
        assert np.array_equal(rec[:, 0], want_ids)


@pytest.mark.parametrize("name", list(_CASES))
def test_row_records(cases, name):
    c = cases[name]
    s = _sink("rows", c["rows"].shape[2] - 5)
    s.append(c["drows"], c["dcounts"], 0)
    rec, per = s.drain()
    assert _same(rec, c["flat"]) and np.array_equal(per, c["counts"].numpy())
    assert not np.isnan(rec).any()                                  # nothing past counts[b] was read into a result
    assert int(s.class_counts().sum()) == 0                          # counting was not requested


@pytest.mark.parametrize("name", list(_CASES))
def test_counts_only(cases, name):
    c = cases[name]
    s = _sink("rows", c["rows"].shape[2] - 5)
    s.add_counts(c["drows"], c["dcounts"])
    assert torch.equal(s.class_counts(), c["cls"])
    rec, per = s.drain()
    assert rec.shape == (0, c["rows"].shape[2]) and per.shape == (0,)   # nothing was compacted
    s.add_counts(c["drows"], c["dcounts"])                             # drain() resets the totals, not the class counts
    assert torch.equal(s.class_counts(), 2 * c["cls"])


def test_tie_nonpositive_and_nan_rows():
    """the first maximum wins a tie; a row whose scores are all <= 0 is not counted; a NaN score is the maximum (np.argmax,
    torch.max) and is not > 0.  The host reference on CPU tensors decides, bit for bit."""
    P, cap = 9, 6
    rows = torch.full((1, cap, P), float("nan"))
    rows[0, :5, :5] = torch.tensor([[0.1, 0.2, 0.3, 0.4, 0.9]]).repeat(5, 1) + torch.arange(5)[:, None] * 0.01
    rows[0, 0, 5:] = torch.tensor([0.2, 0.7, 0.7, 0.1])              # tie: class 1
    rows[0, 1, 5:] = torch.tensor([0.0, -0.5, 0.0, -1.0])            # all <= 0 (and tied at 0): class 0 in the record, not counted
    rows[0, 2, 5:] = torch.tensor([0.3, float("nan"), 0.9, 0.1])     # NaN: class 1 in the record, not counted
    rows[0, 3, 5:] = torch.tensor([0.3, 0.1, 0.2, 0.9])              # plain: class 3
    rows[0, 4, 5:] = torch.tensor([float("nan"), 0.5, float("nan"), 0.9])   # two NaNs: the first
    counts = torch.tensor([5], dtype=torch.int32)
    want, want_cls = _ref_npy(rows, counts, 3), _ref_class_counts(rows, counts)
    assert want[:, 6].tolist() == [1.0, 0.0, 1.0, 3.0, 0.0] and want_cls.tolist() == [0, 1, 0, 1]   # what the reference is expected to say
    s = _sink("npy", P - 5)
    s.append(rows.cuda(), counts.cuda(), 3, count_classes=True)
    rec, per = s.drain()
    assert _same(rec, want) and per.tolist() == [5]
    assert torch.equal(s.class_counts(), want_cls)
    s2 = _sink("rows", P - 5)
    s2.add_counts(rows.cuda(), counts.cuda())
    assert torch.equal(s2.class_counts(), want_cls)


def test_out_of_range_counts_are_clamped():
    rows, _ = _make_rows(3, 4, 8, [4, 4, 4], seed=7)
    bad = torch.tensor([-3, 9, 2], dtype=torch.int32)                # -> 0, cap, 2
    s = _sink("rows", 3)
    s.append(rows.cuda(), bad.cuda(), 0)
    rec, per = s.drain()
    assert per.tolist() == [0, 4, 2] and _same(rec, _ref_rows(rows, torch.tensor([0, 4, 2])))


@pytest.mark.parametrize("mode", ["npy", "rows"])
def test_state_is_carried_over_appends(cases, mode):
    """three appends with different B and first_img_id, one drain: the concatenation, and the totals start again afterwards"""
    seq = [("3x5x12", 40), ("515x4x12-cycling", 43), ("2x300x12-full", 7000)]
    s = _sink(mode, 7)
    want_rec, want_per, want_cls = [], [], torch.zeros(7, dtype=torch.long)
    for name, first in seq:
        c = cases[name]
        s.append(c["drows"], c["dcounts"], first, count_classes=True)
        want_rec.append(_ref_npy(c["rows"], c["counts"], first) if mode == "npy" else c["flat"])
        want_per.append(c["counts"].numpy())
        want_cls += c["cls"]
    rec, per = s.drain()
    assert _same(rec, np.concatenate(want_rec)) and np.array_equal(per, np.concatenate(want_per))
    assert torch.equal(s.class_counts(), want_cls)
    if mode == "npy":
        ids = np.concatenate([np.repeat(np.arange(len(p)) + first, p) for (_, first), p in zip(seq, want_per)]).astype(np.float32)
        assert np.array_equal(rec[:, 0], ids)
    rec2, per2 = s.drain()
    assert rec2.shape == (0, rec.shape[1]) and per2.shape == (0,)
    c = cases["3x5x12"]
    s.append(c["drows"], c["dcounts"], 40)
    rec3, per3 = s.drain()
    assert _same(rec3, want_rec[0]) and np.array_equal(per3, want_per[0])
    assert torch.equal(s.class_counts(), want_cls)


def test_capacity_through_the_abi(cases):
    """a deliberately small arena / image buffer: what does not fit is counted, nothing is written past either capacity (guard
    regions behind both stay as the test filled them), and drain() refuses"""
    from yogo_amd import _hip

    c = cases["5x7x21-mixed"]                                        # counts 3 0 7 1 6: 17 records
    B, cap, P = c["rows"].shape
    arena_cap, img_cap, guard = 8, 3, 64
    s = _sink("rows", P - 5)
    sentinel = 12345.0
    arena = torch.full((arena_cap + guard, P), sentinel, device="cuda")
    img_counts = torch.full((img_cap + guard,), -77, dtype=torch.int32, device="cuda")
    ws = torch.empty(_hip.query_size("yogo_pred_sink_workspace_bytes", B), dtype=torch.uint8, device="cuda")
    _hip.call("yogo_pred_sink_append", c["drows"], c["dcounts"], B, cap, P, 1, 1, 0, 0, 0, s.state, arena, arena_cap, img_counts, img_cap, ws,
              _hip.stream_ptr())
    st = s.state.cpu()
    assert int(st[s.off_rows]) == 8 and int(st[s.off_dropped]) == 17 - 8
    assert int(st[s.off_images]) == 3 and int(st[s.off_dropped_images]) == 5 - 3
    assert _same(arena[:arena_cap].cpu().numpy(), c["flat"][:arena_cap])
    assert bool((arena[arena_cap:] == sentinel).all()) and bool((img_counts[img_cap:] == -77).all())
    assert img_counts[:img_cap].tolist() == [3, 0, 7]
    assert torch.equal(st[s.off_counts:], c["cls"])                  # counting does not depend on room
    # a second append into the full arena: everything is dropped, nothing moves
    _hip.call("yogo_pred_sink_append", c["drows"], c["dcounts"], B, cap, P, 1, 0, 0, 0, 0, s.state, arena, arena_cap, img_counts, img_cap, ws,
              _hip.stream_ptr())
    st = s.state.cpu()
    assert int(st[s.off_rows]) == 8 and int(st[s.off_dropped]) == 9 + 17 and int(st[s.off_dropped_images]) == 2 + 5
    assert bool((arena[arena_cap:] == sentinel).all()) and bool((img_counts[img_cap:] == -77).all())
    with pytest.raises(RuntimeError, match="dropped"):
        s.drain()
    rec, per = s.drain()                                             # usable again afterwards
    assert rec.shape == (0, P) and per.shape == (0,)


def test_growth_keeps_every_record(cases):
    """a small first buffer (one tiny image: 2 * 1 * 4 records, 1024 image entries), then appends whose bounds and whose exact counts
    both exceed it: the arena and the image buffer grow and keep what they held"""
    tiny_rows, tiny_counts = _make_rows(1, 4, 12, [3], seed=5)
    s = _sink("npy", 7)
    s.append(tiny_rows.cuda(), tiny_counts.cuda(), 0, count_classes=True)
    first_cap = s.arena.shape[0]
    assert first_cap == 8 and s.img_counts.shape[0] == 1024
    want_rec, want_per = [_ref_npy(tiny_rows, tiny_counts, 0)], [tiny_counts.numpy()]
    want_cls = _ref_class_counts(tiny_rows, tiny_counts)
    for name, first in (("2x300x12-full", 1), ("515x4x12-cycling", 3), ("515x4x12-cycling", 518), ("2x300x12-full", 1033)):
        c = cases[name]
        s.append(c["drows"], c["dcounts"], first, count_classes=True)
        want_rec.append(_ref_npy(c["rows"], c["counts"], first))
        want_per.append(c["counts"].numpy())
        want_cls += c["cls"]
    assert s.arena.shape[0] > first_cap and s.img_counts.shape[0] > 1024
    rec, per = s.drain()
    assert _same(rec, np.concatenate(want_rec)) and np.array_equal(per, np.concatenate(want_per))
    assert torch.equal(s.class_counts(), want_cls)


def test_argument_errors_do_not_launch():
    from yogo_amd import _hip
    from yogo_amd.pred_sink import PredictionSink

    B, cap = 2, 3
    dev = torch.device("cuda")
    counts = torch.zeros(B, dtype=torch.int32, device=dev)
    state = torch.zeros(4 + 300, dtype=torch.int64, device=dev)
    img_counts = torch.zeros(8, dtype=torch.int32, device=dev)
    ws = torch.empty(64, dtype=torch.uint8, device=dev)

    def call(rows, counts_, P, mode, state_, arena, img_counts_, ws_, count=0):
        _hip.call("yogo_pred_sink_append", rows, counts_, B, cap, P, mode, count, 0, 64, 96, state_, arena, 16, img_counts_, 8, ws_,
                  _hip.stream_ptr())

    P = 9
    rows = torch.zeros(B, cap, P, device=dev)
    arena = torch.zeros(16, 8 + 300, device=dev)
    _hip.launch_log(True)
    try:
        for args in ((None, counts, P, 1, state, arena, img_counts, ws), (rows, None, P, 1, state, arena, img_counts, ws),
                     (rows, counts, P, 1, None, arena, img_counts, ws), (rows, counts, P, 1, state, arena, None, ws),
                     (rows, counts, P, 1, state, arena, img_counts, None),
                     (rows, counts, P, 1, state, None, None, None),              # no arena and no counting: nothing to do
                     (rows, counts, 5, 1, state, arena, img_counts, ws),         # P < 6
                     (rows, counts, 3, 0, state, arena, img_counts, ws),
                     (rows, counts, P, 2, state, arena, img_counts, ws)):        # no such mode
            with pytest.raises(RuntimeError, match="code 1"):
                call(*args)
        big = torch.zeros(B, cap, 5 + 256, device=dev)
        with pytest.raises(RuntimeError, match="code 1"):                        # C > 255 in mode 0 ...
            call(big, counts, 5 + 256, 0, state, arena, img_counts, ws)
        assert _hip.read_launch_log() == []
        call(big, counts, 5 + 256, 1, state, arena, img_counts, ws)              # ... but not in mode 1
        assert len(_hip.read_launch_log()) == 1
    finally:
        _hip.launch_log(False)
    with pytest.raises(ValueError, match="255"):
        PredictionSink(dev, 256, "npy", img_hw=(64, 96))
    with pytest.raises(ValueError):
        PredictionSink(dev, 4, "npy")                                            # no image size
    s = PredictionSink(dev, 4, "rows")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.append(torch.zeros(1, 2, 9), torch.zeros(1, dtype=torch.int32), 0)
    with pytest.raises(ValueError):
        s.append(torch.zeros(1, 2, 8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev), 0)   # 3 class scores, not 4


# -----------------------------------------------------------------------------------------------------------------------------------
# end to end
# -----------------------------------------------------------------------------------------------------------------------------------
def _make_checkpoint(tmp_path, seed=3):
    """as tests/test_gpu_zarr_feed.py::_make_checkpoint, with the objectness bias raised further: the comparison below needs at
    least 10 kept rows over at least two images at threshold 0.5 (asserted on the default path's output)"""
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

    d = tmp_path_factory.mktemp("sink_e2e")
    frames = np.random.default_rng(6).integers(0, 256, size=(64, 96, 10), dtype=np.uint8)
    (d / "png").mkdir()
    for i in range(10):
        Image.fromarray(frames[:, :, i]).save(d / "png" / f"img_{i:02d}.png")
    z = ZW.write_stack(d / "stack.zip", frames, (64, 96, 1), as_zip=True)
    return d / "png", z, _make_checkpoint(d)


@pytest.mark.parametrize("output", ["npy", "txt"])
@pytest.mark.parametrize("source", ["png", "zarr"])
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "bf16"])
def test_predict_with_device_outputs_writes_the_same_files(e2e_inputs, tmp_path, capsys, half, source, output):
    from yogo_amd.infer import predict

    pngs, z, pth = e2e_inputs
    src = dict(path_to_images=pngs) if source == "png" else dict(path_to_zarr=z)
    base = dict(count_predictions=True, batch_size=4, half=half, class_names=CLASSES, **src)   # 10 frames: the last batch is partial

    def run(tag, device_outputs, **kw):
        capsys.readouterr()
        out = tmp_path / tag
        predict(str(pth), output_dir=str(out), device_outputs=device_outputs, **base, **kw)
        return out, capsys.readouterr().out.strip().splitlines()[-1]

    if output == "npy":   # --save-npy + --count
        a, counts_a = run("host", False, save_npy=True)
        b, counts_b = run("dev", True, save_npy=True)
        fa, fb = sorted(a.glob("*.npy")), sorted(b.glob("*.npy"))
        assert len(fa) == 1 and [f.name for f in fa] == [f.name for f in fb]
        na, nb = np.load(fa[0]), np.load(fb[0])
        print(f"npy: {na.shape[1]} records, per image {np.bincount(na[0].astype(np.int64), minlength=10).tolist()}; counts {counts_a}")
        # the comparison is not vacuous (a condition on the input: the checkpoint's objectness bias)
        assert na.shape[0] == 8 + 4 and na.shape[1] >= 10 and len(set(na[0].tolist())) >= 2
        assert na.dtype == nb.dtype == np.float32 and np.array_equal(na, nb)
        assert fa[0].read_bytes() == fb[0].read_bytes()
        ja, jb = json.loads(fa[0].with_suffix(".json").read_text()), json.loads(fb[0].with_suffix(".json").read_text())
        ja.pop("write_date"), jb.pop("write_date")
        assert ja == jb and ja["model_name"] == "fake_model"
    else:                 # --save-preds + --count
        a, counts_a = run("host", False, save_preds=True)
        b, counts_b = run("dev", True, save_preds=True)
        names = [f"img_{i:02d}.txt" for i in range(10)]
        assert sorted(f.name for f in a.iterdir()) == names and sorted(f.name for f in b.iterdir()) == names
        texts = [(a / n).read_bytes() for n in names]
        lines = sum(len(t.splitlines()) for t in texts)
        print(f"txt: {lines} lines, per image {[len(t.splitlines()) for t in texts]}; counts {counts_a}")
        assert lines >= 10 and sum(1 for t in texts if t) >= 2      # not vacuous, as above
        for n, t in zip(names, texts):
            assert (b / n).read_bytes() == t, n
    assert counts_a == counts_b and counts_a.startswith("[('you',")
