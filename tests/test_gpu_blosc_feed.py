"""Blosc-compressed zarr stacks through the feed (yogo_amd/zarr_feed.py with yogo_amd/csrc/blosc_lz4.hip in front of the unpack
launch): the batches equal the stack, the same stack stored raw and the host route; a chunk the device cannot decode travels
the mixed route; a corrupt chunk costs exactly its batch; `predict` writes the same .npy from a Blosc store as from a raw one."""
import numpy as np
import pytest
import torch

import _blosc_write as BW
import _zarr_write as ZW
from yogo_amd.image_path_dataset import ZarrDataset

pytestmark = pytest.mark.gpu
CLASSES = ["you", "only", "glance", "once"]
FILL = 9
N = 7


def _stack():
    """frames LZ4 shrinks, one it does not (2) and one whose lower half it does not (5: chunks of three frames then hold both kinds)"""
    rng = np.random.default_rng(21)
    s = rng.integers(0, 4, size=(24, 48, N), dtype=np.uint8) * 60
    s[:, :, 2] = rng.integers(0, 256, size=(24, 48), dtype=np.uint8)
    s[12:, :, 3:6] = rng.integers(0, 256, size=(12, 48, 3), dtype=np.uint8)
    return s


def _decode_launches(run):
    """run() with the launch log on -> (its result, how many decode launches it made)"""
    from yogo_amd import _hip

    _hip.launch_log(True)
    try:
        res = run()
        log = _hip.read_launch_log()
    finally:
        _hip.launch_log(False)
    return res, sum(ln.startswith("blosc_lz4_decode_kernel") for ln in log)


def _batches(path, batch, **kw):
    from yogo_amd.zarr_feed import ZarrDeviceFeed

    feed = ZarrDeviceFeed(ZarrDataset(path), batch, "cuda", num_frames=N, **kw)
    out = [b.cpu() for b, _ in feed]
    return torch.cat(out), feed


@pytest.mark.parametrize("blocksize,as_zip,batch", [(100, False, 2), (4096, True, 5), (100, True, 5), (4096, False, 2)],
                         ids=["bs100-dir-b2", "bs4096-zip-b5", "bs100-zip-b5", "bs4096-dir-b2"])
@pytest.mark.parametrize("chunks", [(24, 48, 1), (24, 48, 3), (12, 16, 2)], ids=lambda c: "x".join(map(str, c)))
def test_feed_batches_equal_the_stack(tmp_path, chunks, blocksize, as_zip, batch):
    stack = _stack()
    grid_n = -(-N // chunks[2])
    absent = (0, 0, grid_n - 1) if chunks[2] > 1 else (0, 0, 4)
    memcpyed_key = "0.0.0"
    members = BW.blosc_members(stack, chunks, blocksize=blocksize, fill_value=FILL, skip=[absent],
                               frame=lambda key, raw: BW.blosc_frame(raw, blocksize, memcpyed=key == memcpyed_key))
    kinds = [BW.blosc_raw_share(v) for k, v in members.items() if not k.endswith(".zarray") and k != memcpyed_key]
    if (chunks, blocksize) != ((24, 48, 3), 4096):     # (there the one chunk left is a single block, which LZ4 shrinks)
        assert sum(r for r, _ in kinds) > 0 and sum(c for _, c in kinds) > 0    # raw and LZ4 blocks both occur
    assert members[memcpyed_key][2] & 0x02
    ext = ".zip" if as_zip else ".zarr"
    p = ZW.write_members(tmp_path / ("blosc" + ext), members, as_zip=as_zip)
    p_raw = ZW.write_stack(tmp_path / ("raw" + ext), stack, chunks, as_zip=as_zip, fill_value=FILL, skip=[absent])
    want = stack.copy()
    want[absent[0] * chunks[0]:(absent[0] + 1) * chunks[0], absent[1] * chunks[1]:(absent[1] + 1) * chunks[1],
         absent[2] * chunks[2]:(absent[2] + 1) * chunks[2]] = FILL
    want = torch.from_numpy(want).permute(2, 0, 1)[:, None].contiguous()

    (got, feed), launches = _decode_launches(lambda: _batches(p, batch))
    # one decode launch per batch (none for a batch whose only chunk is the absent one)
    empty = sum(1 for lo in range(0, N, batch) if chunks[:2] == (24, 48) and
                all(k // chunks[2] == absent[2] for k in range(lo, min(lo + batch, N))))
    assert feed.device_decode and len(feed) == -(-N // batch) and launches == len(feed) - empty
    assert got.dtype == torch.uint8 and torch.equal(got, want)
    assert max(feed.stager.reads.values()) == 1          # a chunk two batches share is read once
    got_f32, _ = _batches(p, batch, normalize=True)
    assert got_f32.dtype == torch.float32 and torch.equal(got_f32, want / 255)
    (got_host, feed_host), launches = _decode_launches(lambda: _batches(p, batch, device_decode=False))
    assert not feed_host.device_decode and launches == 0 and torch.equal(got_host, got)
    (got_raw, feed_raw), launches = _decode_launches(lambda: _batches(p_raw, batch))
    assert not feed_raw.device_decode and launches == 0 and torch.equal(got_raw, got)


def test_feed_mixed_route(tmp_path):
    """a chunk with zlib inside among LZ4 ones is decoded on the host and enters the table as one raw entry"""
    import zlib

    stack = _stack()
    zl = lambda raw: BW.blosc_frame(raw, 500, flags=0x01 | (3 << 5), compress=lambda b: zlib.compress(b, 1))   # noqa: E731
    members = BW.blosc_members(stack, (24, 48, 1), blocksize=500, frame=lambda key, raw: zl(raw) if key == "0.0.3" else BW.blosc_frame(raw, 500))
    assert members["0.0.3"][2] >> 5 == 3 and BW.blosc_raw_share(members["0.0.3"])[1] > 0
    p = ZW.write_members(tmp_path / "s.zarr", members)
    (got, feed), launches = _decode_launches(lambda: _batches(p, 4))
    assert feed.device_decode and launches == 2
    assert torch.equal(got, torch.from_numpy(stack).permute(2, 0, 1)[:, None].contiguous())


@pytest.mark.parametrize("defect", ["lz4-offset-too-far", "header-truncated"])
@pytest.mark.parametrize("device_decode", [True, False], ids=["device", "host"])
def test_feed_corrupt_chunk_costs_exactly_its_batch(tmp_path, defect, device_decode):
    from yogo_amd import blosc
    from yogo_amd.zarr_feed import ZarrDeviceFeed

    stack = _stack()

    def frame(key, raw):
        if key != "0.0.3":
            return BW.blosc_frame(raw, 4096)
        if defect == "header-truncated":
            return BW.blosc_frame(raw, 4096)[:-7]
        # a well-framed chunk whose one LZ4 block has a match 30 bytes back after 20 bytes: the header parses, the block does not
        # decode (liblz4, which the host route uses where it is installed, refuses this one too; an offset of 0 it lets pass)
        bad = BW.lz4_sequence(raw[:20], 30, len(raw) - 25) + BW.lz4_sequence(raw[-5:])
        assert blosc.lz4_block_status(bad, len(raw))[0] == blosc.LZ4_BAD_OFFSET
        return BW.blosc_frame(raw, 4096, compress=lambda b: bad)

    p = ZW.write_members(tmp_path / "s.zip", BW.blosc_members(stack, (24, 48, 1), blocksize=4096, frame=frame), as_zip=True)
    feed = ZarrDeviceFeed(ZarrDataset(p), 2, "cuda", num_frames=N, device_decode=device_decode)
    assert feed.device_decode is device_decode
    want = torch.from_numpy(stack).permute(2, 0, 1)[:, None].contiguous()
    b0, _ = next(feed)
    assert torch.equal(b0.cpu(), want[:2])
    with pytest.raises(RuntimeError, match=r"0\.0\.3"):
        next(feed)
    b2, _ = next(feed)
    assert torch.equal(b2.cpu(), want[4:6])
    b3, _ = next(feed)
    assert torch.equal(b3.cpu(), want[6:])
    with pytest.raises(StopIteration):
        next(feed)


def _make_checkpoint(path, seed=3):
    """a random-init quarter_filters model whose statistics let a handful of cells fire (as tests/test_gpu_zarr_feed.py's)"""
    from yogo_amd.model import YOGO
    from yogo_amd.model_defns import get_model_func

    torch.manual_seed(seed)
    net = YOGO((64, 96), 0.0425, 0.0555, 4, model_func=get_model_func("quarter_filters")).cuda()
    net.eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 50.0)
                m.running_var.uniform_(2000.0, 9000.0)
        [m for m in net.modules() if isinstance(m, torch.nn.Conv2d)][-1].bias[4] += 1.5
    torch.save({"epoch": 0, "step": 7, "normalize_images": False, "classes": CLASSES, "model_name": "fake_model",
                "model_state_dict": {k: v.cpu() for k, v in net.state_dict().items()}, "model_version": "quarter_filters"}, path)
    return path


def test_predict_from_a_blosc_store_equals_predict_from_a_raw_store(tmp_path):
    from yogo_amd.infer import predict

    rng = np.random.default_rng(6)
    frames = rng.integers(0, 256, size=(64, 96, 10), dtype=np.uint8)
    frames[:, :, ::2] = frames[:, :, ::2] // 64 * 64          # every other frame is one LZ4 shrinks
    for d in ("a", "b", "out_a", "out_b"):
        (tmp_path / d).mkdir()
    members = BW.blosc_members(frames, (64, 96, 1), blocksize=2048)
    kinds = [BW.blosc_raw_share(v) for k, v in members.items() if not k.endswith(".zarray")]
    assert sum(r for r, _ in kinds) > 0 and sum(c for _, c in kinds) > 0
    z_blosc = ZW.write_members(tmp_path / "a" / "stack.zip", members, as_zip=True)
    z_raw = ZW.write_stack(tmp_path / "b" / "stack.zip", frames, (64, 96, 1), as_zip=True)
    pth = _make_checkpoint(tmp_path / "m.pth")
    kw = dict(save_npy=True, batch_size=4, obj_thresh=0.4, iou_thresh=0.5, class_names=CLASSES)
    _, launches = _decode_launches(lambda: predict(str(pth), path_to_zarr=z_blosc, output_dir=str(tmp_path / "out_a"), **kw))
    assert launches == 3
    predict(str(pth), path_to_zarr=z_raw, output_dir=str(tmp_path / "out_b"), **kw)
    a, b = (tmp_path / "out_a" / "stack.npy").read_bytes(), (tmp_path / "out_b" / "stack.npy").read_bytes()
    assert a == b and np.load(tmp_path / "out_a" / "stack.npy").shape[1] > 0
