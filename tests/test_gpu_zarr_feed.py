"""The device half of zarr input (yogo_amd/csrc/zarr_feed.hip, yogo_amd/zarr_feed.py, `predict(path_to_zarr=...)`):
* the unpack kernel's three paths against numpy slicing + CenterCrop + torch's CPU `/ 255`, bit for bit, in both output dtypes;
* the feed: batches in index order, names, a corrupt chunk costs exactly its batch;
* end to end: `predict` from a zarr zip == `predict` from the same frames as a PNG directory."""
import numpy as np
import pytest
import torch

import _zarr_write as ZW
from yogo_amd.image_path_dataset import CenterCrop, ZarrDataset
from yogo_amd.zarr_store import open_zarr

pytestmark = pytest.mark.gpu
CLASSES = ["you", "only", "glance", "once"]
FILL = 7


def _unpack_case(tmp_path, shape, chunks, order, idxs, crop=None, skip=()):
    """write the stack, stage what frames `idxs` (consecutive) need as the feed does, unpack in both dtypes ->
    ({dtype: device result}, {dtype: expectation}, launch log lines)"""
    from yogo_amd import _hip
    from yogo_amd.device_decode import center_crop_origin
    from yogo_amd.zarr_feed import ChunkStager, FrameSource, plan_batch, unpack

    H, W, N = shape
    stack = np.random.default_rng(sum(shape) + sum(chunks)).integers(0, 256, size=shape, dtype=np.uint8)
    p = ZW.write_stack(tmp_path / "s.zarr", stack, chunks, order=order, fill_value=FILL, skip=skip)
    want_stack = stack.copy()
    for ty, tx, tk in skip:
        want_stack[ty * chunks[0]:(ty + 1) * chunks[0], tx * chunks[1]:(tx + 1) * chunks[1], tk * chunks[2]:(tk + 1) * chunks[2]] = FILL
    src = FrameSource(open_zarr(p))
    plan = plan_batch(src, idxs[0], idxs[-1] + 1)
    if skip:
        assert (plan.tile_off < 0).any()
    stager = ChunkStager(src, threads=2)
    buf = np.zeros(plan.nbytes, np.uint8)
    try:
        stager.stage(plan, buf)
    finally:
        stager.close()
    staged = torch.from_numpy(buf).cuda()
    OH, OW = crop or (H, W)
    top, left = center_crop_origin(H, W, OH, OW)
    want_u8 = CenterCrop((OH, OW))(torch.from_numpy(want_stack[:, :, list(idxs)]).permute(2, 0, 1)[:, None].contiguous())
    want = {torch.uint8: want_u8, torch.float32: want_u8 / 255}
    got = {}
    _hip.launch_log(True)
    try:
        for dt in (torch.uint8, torch.float32):
            out = torch.full((len(idxs), 1, OH, OW), 3, dtype=dt, device="cuda")
            unpack(staged, plan.tile_off, plan.tile_k, chunks=chunks, order_f=order == "F", fill=FILL, frame_shape=(H, W), out=out,
                   top=top, left=left)
            got[dt] = out.cpu()
        log = _hip.read_launch_log()
    finally:
        _hip.launch_log(False)
    return got, want, log


def _check(got, want, log, path):
    assert [ln.split(" | ")[0] for ln in log] == [f"zarr_unpack_{path}_kernel<u8>", f"zarr_unpack_{path}_kernel<f32>"], log
    for dt in (torch.uint8, torch.float32):
        assert got[dt].dtype == dt and torch.equal(got[dt], want[dt]), (path, dt)


@pytest.mark.parametrize("shape,crop,path", [
    ((24, 48, 3), None, "rows_vec"),
    ((24, 48, 3), (10, 48), "rows_vec"),      # top 7: 7 * 48 bytes, the row starts stay 16-byte aligned
    ((24, 48, 3), (10, 40), "rows_byte"),     # left 4: unaligned
    ((13, 17, 3), None, "rows_byte"),
], ids=["vec", "vec-crop-rows", "byte-crop-cols", "byte-odd"])
def test_unpack_rows(tmp_path, shape, crop, path):
    got, want, log = _unpack_case(tmp_path, shape, (shape[0], shape[1], 1), "C", range(3), crop=crop)
    _check(got, want, log, path)


def test_unpack_rows_tiled_vector_and_absent_tile(tmp_path):
    # two tiles down the frame, one tile across: row-by-row 16-byte segments; one chunk is absent and reads as fill
    got, want, log = _unpack_case(tmp_path, (24, 48, 3), (16, 48, 1), "C", range(3), crop=(20, 48), skip=[(1, 0, 1)])
    _check(got, want, log, "rows_vec")


@pytest.mark.parametrize("chunks,skip", [
    ((24, 48, 2), [(0, 0, 3)]),     # frames 6 and 7 are filled
    ((24, 48, 3), ()),
    ((24, 48, 8), ()),
    ((5, 7, 2), [(2, 3, 2)]),       # tiles that divide neither H nor W; one tile of frames 4 and 5 is filled
], ids=["cn2-absent", "cn3", "cn8", "tiles-5x7x2"])
@pytest.mark.parametrize("crop", [None, (10, 40)], ids=["full", "crop"])
def test_unpack_deinterleave(tmp_path, chunks, skip, crop):
    # B = 5 from frames 4 .. 8 of 9: the batch starts inside a chunk (cn 3, 8), crosses a chunk boundary and ends in a
    # padded edge chunk (cn 2, 8)
    got, want, log = _unpack_case(tmp_path, (24, 48, 9), chunks, "C", range(4, 9), crop=crop, skip=skip)
    _check(got, want, log, "deinterleave")


@pytest.mark.parametrize("chunks", [(24, 48, 1), (24, 48, 3), (5, 7, 2)], ids=lambda c: "x".join(map(str, c)))
def test_unpack_gather_f_order(tmp_path, chunks):
    got, want, log = _unpack_case(tmp_path, (24, 48, 9), chunks, "F", range(4, 9), crop=(10, 40) if chunks[0] == 5 else None)
    _check(got, want, log, "gather")


def test_unpack_refuses_bad_arguments():
    """argument checks return before any launch"""
    from yogo_amd import _hip
    from yogo_amd.zarr_feed import unpack

    staged = torch.zeros(24 * 48, dtype=torch.uint8, device="cuda")
    toff = torch.zeros(1, dtype=torch.int64, device="cuda")
    tk = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.zeros(24 * 48, dtype=torch.float32, device="cuda")

    def call(top=0, OH=24, out_fp32=0):
        _hip.call("yogo_zarr_unpack", staged, staged.numel(), toff, tk, 1, 1, 1, 24, 48, 1, 0, 0, 24, 48, top, 0, OH, 48, out, out_fp32,
                  _hip.stream_ptr())

    call()
    with pytest.raises(RuntimeError, match="crop"):
        call(top=7, OH=18)          # OH > H - top
    with pytest.raises(RuntimeError, match="out_fp32"):
        call(out_fp32=2)
    # the wrapper holds the tables on the host and checks them before the launch
    o = torch.zeros((1, 1, 24, 48), dtype=torch.uint8, device="cuda")
    with pytest.raises(IndexError, match="tile_k"):
        unpack(staged, np.zeros((1, 1, 1), np.int64), np.array([1], np.int32), chunks=(24, 48, 1), order_f=False, fill=0,
               frame_shape=(24, 48), out=o)
    with pytest.raises(IndexError, match="tile offset"):
        unpack(staged, np.full((1, 1, 1), 16, np.int64), np.zeros(1, np.int32), chunks=(24, 48, 1), order_f=False, fill=0,
               frame_shape=(24, 48), out=o)


def _feed_frames():
    return np.random.default_rng(5).integers(0, 256, size=(24, 48, 10), dtype=np.uint8)


@pytest.mark.parametrize("normalize", [False, True], ids=["u8", "f32"])
def test_feed_batches_equal_the_stack(tmp_path, normalize):
    from yogo_amd.zarr_feed import ZarrDeviceFeed

    frames = _feed_frames()
    p = ZW.write_stack(tmp_path / "s.zip", frames, (24, 48, 1), as_zip=True, compressor="zlib")
    feed = ZarrDeviceFeed(ZarrDataset(p), 4, "cuda", normalize=normalize)
    batches = list(feed)
    assert [tuple(b.shape) for b, _ in batches] == [(4, 1, 24, 48), (4, 1, 24, 48), (2, 1, 24, 48)]
    assert all(b.is_cuda for b, _ in batches)
    assert [n for _, names in batches for n in names] == [f"img_{i:02d}.png" for i in range(10)]
    want = torch.from_numpy(frames).permute(2, 0, 1)[:, None].contiguous()
    assert torch.equal(torch.cat([b.cpu() for b, _ in batches]), want / 255 if normalize else want)


@pytest.fixture(scope="module")
def production_stack(tmp_path_factory):
    """five 772 x 1032 frames, one raw chunk each: the stacks the scopes write"""
    frames = np.random.default_rng(8).integers(0, 256, size=(772, 1032, 5), dtype=np.uint8)
    return frames, ZW.write_stack(tmp_path_factory.mktemp("zarr_prod") / "s.zarr", frames, (772, 1032, 1))


@pytest.mark.parametrize("normalize", [False, True], ids=["u8", "f32"])
def test_feed_at_the_production_frame_shape(production_stack, normalize):
    """772 x 1032: no multiple of 16 in a row, one in the frame -- every batch is one rows_vec launch of 49 workgroups per frame,
    the last of them partial (tests/test_gpu_zarr_unpack_edges.py holds the kernel alone to it)"""
    from yogo_amd import _hip
    from yogo_amd.zarr_feed import ZarrDeviceFeed

    frames, p = production_stack
    _hip.launch_log(True)
    try:
        feed = ZarrDeviceFeed(ZarrDataset(p), 2, "cuda", normalize=normalize)
        batches = [b.cpu() for b, _ in feed]
        log = [ln.split(" | ")[0] for ln in _hip.read_launch_log() if ln.startswith("zarr_unpack")]
    finally:
        _hip.launch_log(False)
    assert [tuple(b.shape) for b in batches] == [(2, 1, 772, 1032), (2, 1, 772, 1032), (1, 1, 772, 1032)]
    assert log == [f"zarr_unpack_rows_vec_kernel<{'f32' if normalize else 'u8'}>"] * 3, log
    want = torch.from_numpy(frames).permute(2, 0, 1)[:, None].contiguous()
    assert torch.equal(torch.cat(batches), want / 255 if normalize else want)


def test_feed_shares_chunks_between_batches_and_crops(tmp_path):
    from yogo_amd.zarr_feed import ZarrDeviceFeed

    frames = _feed_frames()
    p = ZW.write_stack(tmp_path / "s.zarr", frames, (24, 48, 3))
    feed = ZarrDeviceFeed(ZarrDataset(p), 4, "cuda", crop=(12, 48), num_frames=10)
    got = torch.cat([b.cpu() for b, _ in feed])
    want = CenterCrop((12, 48))(torch.from_numpy(frames).permute(2, 0, 1)[:, None].contiguous())
    assert torch.equal(got, want)
    assert dict(feed.stager.reads) == {f"0.0.{k}": 1 for k in range(4)}


def test_feed_corrupt_chunk_costs_exactly_its_batch(tmp_path):
    from yogo_amd.zarr_feed import ZarrDeviceFeed

    frames = _feed_frames()
    members = ZW.array_members(frames, (24, 48, 1), compressor="zlib")
    members["0.0.5"] = members["0.0.5"][:20] + b"\x00\xff\x00\xff" + members["0.0.5"][24:]
    p = ZW.write_members(tmp_path / "s.zip", members, as_zip=True)
    feed = ZarrDeviceFeed(ZarrDataset(p), 4, "cuda")
    want = torch.from_numpy(frames).permute(2, 0, 1)[:, None].contiguous()
    b0, n0 = next(feed)
    assert torch.equal(b0.cpu(), want[:4]) and n0[0] == "img_00.png"
    with pytest.raises(RuntimeError, match=r"0\.0\.5"):
        next(feed)
    b2, n2 = next(feed)
    assert torch.equal(b2.cpu(), want[8:]) and n2 == ("img_08.png", "img_09.png")
    with pytest.raises(StopIteration):
        next(feed)


def _make_checkpoint(tmp_path, seed=3):
    """as tests/test_gpu_cli.py::_make_checkpoint: random-init base_model whose statistics let a handful of cells fire"""
    from yogo_amd.model import YOGO

    torch.manual_seed(seed)
    net = YOGO((64, 96), 0.0425, 0.0555, 4).cuda()
    net.eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 50.0)
                m.running_var.uniform_(2000.0, 9000.0)
        net.model[7].bias[4] += 1.5
    p = tmp_path / "m.pth"
    torch.save({"epoch": 0, "step": 7, "normalize_images": False, "classes": CLASSES, "model_name": "fake_model",
                "model_state_dict": {k: v.cpu() for k, v in net.state_dict().items()}, "model_version": "base_model"}, p)
    return p


@pytest.fixture(scope="module")
def e2e_inputs(tmp_path_factory):
    """the same 10 random 64 x 96 frames as a PNG directory and as a zarr zip, and a checkpoint"""
    from PIL import Image

    d = tmp_path_factory.mktemp("zarr_e2e")
    frames = np.random.default_rng(6).integers(0, 256, size=(64, 96, 10), dtype=np.uint8)
    (d / "png").mkdir()
    for i in range(10):
        Image.fromarray(frames[:, :, i]).save(d / "png" / f"img_{i:02d}.png")
    z = ZW.write_stack(d / "stack.zip", frames, (64, 96, 1), as_zip=True)
    return d, d / "png", z, _make_checkpoint(d)


@pytest.mark.parametrize("half,crop", [(False, None), (True, None), (False, 0.5)], ids=["fp32", "bf16", "fp32-crop"])
def test_predict_from_zarr_equals_predict_from_pngs(e2e_inputs, tmp_path, capsys, half, crop):
    from yogo_amd.infer import predict

    d, pngs, z, pth = e2e_inputs
    kw = dict(save_preds=True, count_predictions=True, batch_size=4, obj_thresh=0.4, iou_thresh=0.5, half=half,
              return_full_predictions=True, class_names=CLASSES, vertical_crop_height=crop)
    capsys.readouterr()
    a = predict(str(pth), path_to_images=pngs, output_dir=str(tmp_path / "a"), **kw)
    counts_a = capsys.readouterr().out.strip().splitlines()[-1]
    b = predict(str(pth), path_to_zarr=z, output_dir=str(tmp_path / "b"), **kw)
    counts_b = capsys.readouterr().out.strip().splitlines()[-1]
    assert a.shape == (10, 9, 4 if crop else 8, 12) and torch.equal(a, b)
    assert counts_a == counts_b and counts_a.startswith("[('you',")
    for i in range(10):
        ta, tb = (tmp_path / "a" / f"img_{i:02d}.txt"), (tmp_path / "b" / f"img_{i:02d}.txt")
        assert ta.exists() and tb.exists() and ta.read_text() == tb.read_text()
