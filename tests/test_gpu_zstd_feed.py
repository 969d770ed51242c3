"""Zstandard-compressed zarr stacks through the feed (yogo_amd/zarr_feed.py with yogo_amd/csrc/zstd.hip in front of the unpack
launch): Blosc-zstd stacks and stacks under the zstd codec, built from frames libzstd wrote (tests/golden/zstd_frames.npz) and from
the tests' writer -- the batches equal those of the same stack stored raw, on both routes; a corrupt chunk costs exactly its batch;
`predict` gives the same outputs from a Blosc-zstd store as from a raw one."""
import numpy as np
import pytest
import torch

import _zarr_write as ZW
import _zstd_write as W
from yogo_amd.image_path_dataset import ZarrDataset

pytestmark = pytest.mark.gpu
CLASSES = ["you", "only", "glance", "once"]
N = 8


@pytest.fixture(autouse=True)
def zstd_codec_on_the_device(monkeypatch):
    """the zstd codec's device route is switched off by default (it measured slower); these tests are about it"""
    from yogo_amd import zarr_feed

    monkeypatch.setattr(zarr_feed, "DEVICE_DECODE_ZSTD", True)


@pytest.fixture(scope="module")
def stack():
    return W.store_stack()


@pytest.fixture(scope="module")
def encode():
    return W.library_encoder()


def _launches(run):
    """run() with the launch log on -> (its result, how many zstd decode launches it made)"""
    from yogo_amd import _hip

    _hip.launch_log(True)
    try:
        res = run()
        log = _hip.read_launch_log()
    finally:
        _hip.launch_log(False)
    return res, sum(ln.startswith("zstd_decode_kernel") for ln in log)


def _batches(path, batch, **kw):
    from yogo_amd.zarr_feed import ZarrDeviceFeed

    feed = ZarrDeviceFeed(ZarrDataset(path), batch, "cuda", num_frames=N, **kw)
    out = [b.cpu() for b, _ in feed]
    return torch.cat(out), feed


@pytest.mark.parametrize("batch", [1, 4, 5])
@pytest.mark.parametrize("kind,chunks,as_zip", [("blosc-zstd", (48, 64, 1), False), ("blosc-zstd", (32, 40, 3), True), ("zstd", (48, 64, 1), True),
                                                ("zstd", (48, 64, 2), False)], ids=["blosc-cn1-dir", "blosc-cn3-zip", "codec-cn1-zip", "codec-cn2-dir"])
def test_feed_batches_equal_the_raw_stack(tmp_path, monkeypatch, stack, encode, kind, chunks, as_zip, batch):
    from yogo_amd import zarr_feed

    absent = (0, 0, 1)
    members = W.zstd_members(stack, chunks, kind, encode=encode, memcpyed={"0.0.0"}, fill_value=9, skip=[absent])
    ext = ".zip" if as_zip else ".zarr"
    p = ZW.write_members(tmp_path / ("z" + ext), members, as_zip=as_zip)
    p_raw = ZW.write_stack(tmp_path / ("raw" + ext), stack, chunks, as_zip=as_zip, fill_value=9, skip=[absent])
    want, feed_raw = _batches(p_raw, batch)
    assert not feed_raw.device_decode
    assert torch.equal(want[0, 0], torch.from_numpy(stack[:, :, 0]))

    (got, feed), launches = _launches(lambda: _batches(p, batch))
    assert feed.device_decode and feed.codec == kind and launches >= 1
    assert got.dtype == torch.uint8 and torch.equal(got, want)
    assert max(feed.stager.reads.values()) == 1          # a chunk two batches share is read once
    (got_host, feed_host), launches = _launches(lambda: _batches(p, batch, device_decode=False))
    assert not feed_host.device_decode and launches == 0 and torch.equal(got_host, want)
    # a crop and / 255 in the unpack launch behind the decode
    crop_raw, _ = _batches(p_raw, batch, crop=(30, 50), normalize=True)
    crop_got, _ = _batches(p, batch, crop=(30, 50), normalize=True)
    assert crop_got.dtype == torch.float32 and crop_got.shape[2:] == (30, 50) and torch.equal(crop_got, crop_raw)
    # the module switch of the zstd codec's route
    monkeypatch.setattr(zarr_feed, "DEVICE_DECODE_ZSTD", False)
    (got_off, feed_off), launches = _launches(lambda: _batches(p, batch))
    assert torch.equal(got_off, want)
    assert feed_off.device_decode is (kind == "blosc-zstd") and (launches == 0) is (kind == "zstd")
    monkeypatch.setattr(zarr_feed, "DEVICE_DECODE_ZSTD", True)
    (got_on, feed_on), launches = _launches(lambda: _batches(p, batch))
    assert feed_on.device_decode and launches >= 1 and torch.equal(got_on, want)


def _lz4_launches(run):
    """run() with the launch log on -> (its result, zstd decode launches, launches of the raw rows' copy kernel)"""
    from yogo_amd import _hip

    _hip.launch_log(True)
    try:
        res = run()
        log = _hip.read_launch_log()
    finally:
        _hip.launch_log(False)
    return res, sum(ln.startswith("zstd_decode_kernel") for ln in log), sum(ln.startswith("blosc_lz4_decode_kernel") for ln in log)


@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("kind", ["blosc-zstd", "zstd"])
def test_feed_group_of_2d_members_equals_the_raw_group(tmp_path, stack, encode, kind, batch):
    """a group whose members "0" .. "7" are 2-D arrays (keys such as 3/0.0): the same batches as the same group stored raw; member 5
    lies under another compressor (zlib) than member 0 -- it is decoded on the host and enters the table as raw rows"""
    import json

    frames = [stack[:, :, i] for i in range(N)]
    members = W.zstd_group_members(frames, (48, 64), kind, encode=encode)
    other = ZW.array_members(frames[5], (48, 64), compressor="zlib", prefix="5/")
    members = {k: v for k, v in members.items() if not k.startswith("5/")}
    members.update(other)
    assert json.loads(members["5/.zarray"])["compressor"]["id"] == "zlib" and "3/0.0" in members
    p = ZW.write_members(tmp_path / "g.zarr", members)
    p_raw = ZW.write_group(tmp_path / "raw.zarr", frames, (48, 64))
    want, feed_raw = _batches(p_raw, batch)
    assert not feed_raw.device_decode and torch.equal(want, torch.from_numpy(stack).permute(2, 0, 1)[:, None].contiguous())
    (got, feed), zstd_launches, raw_launches = _lz4_launches(lambda: _batches(p, batch))
    assert feed.device_decode and feed.codec == kind
    assert zstd_launches >= 1 and raw_launches >= 1       # frames on the device; the noise frame's raw blocks / the zlib member as raw rows
    assert torch.equal(got, want)
    got_host, feed_host = _batches(p, batch, device_decode=False)
    assert not feed_host.device_decode and torch.equal(got_host, want)


@pytest.mark.parametrize("kind", ["blosc-zstd", "zstd"])
def test_feed_chunk_longer_than_its_slot_is_decoded_on_the_host(tmp_path, stack, encode, kind):
    """a well-formed chunk whose stored size is above the room a stored chunk has (all blocks raw at a tiny block size): the host
    decodes it and it enters the decoder's table as raw rows (fifth field 1) beside the other chunks' frames"""
    import _blosc_write as BW
    from yogo_amd.zarr_feed import ChunkStager, FrameSource, plan_batch
    from yogo_amd.zarr_store import open_zarr

    raw3 = stack[:, :, 3].tobytes()
    if kind == "blosc-zstd":
        long_chunk = BW.blosc_frame(raw3, 4, flags=W.FLAGS_ZSTD, compress=lambda b: b)          # 768 raw blocks of 4 bytes
    else:
        long_chunk = W.frame([W.raw_block(raw3[at:at + 4]) for at in range(0, len(raw3), 4)], size=len(raw3))
    members = W.zstd_members(stack, (48, 64, 1), kind, encode=encode, replace={"0.0.3": lambda _stored: long_chunk})
    p = ZW.write_members(tmp_path / "s.zarr", members)
    src = FrameSource(open_zarr(p))
    assert len(long_chunk) > src.stored_stride
    stager = ChunkStager(src, threads=2)
    try:
        plan = plan_batch(src, 2, 5)
        table = stager.stage_stored(plan, np.zeros(len(plan.keys) * src.stored_stride, np.uint8))
    finally:
        stager.close()
    rows_of_3 = [r for r, owner in zip(table.tolist(), plan.row_chunk) if plan.keys[owner] == "0.0.3"]
    assert rows_of_3 == [[src.stored_stride, 3072, plan.offsets["0.0.3"], 3072, 1]]          # the decoded bytes, one raw row
    assert 0 in table[:, 4].tolist()                                                         # frames of the other chunks
    (got, feed), zstd_launches, raw_launches = _lz4_launches(lambda: _batches(p, 3))
    assert feed.device_decode and zstd_launches >= 1 and raw_launches >= 1
    assert torch.equal(got, torch.from_numpy(stack).permute(2, 0, 1)[:, None].contiguous())


def test_feed_host_decodes_what_the_device_cannot_take(tmp_path, stack, encode):
    """a bit-shuffled chunk (flag 0x04) among the others: refused by the host decoder too -- its batch raises, naming it; a chunk
    with typesize 4 stored memcpyed travels as raw rows"""
    import _blosc_write as BW
    from yogo_amd.zarr_feed import ZarrDeviceFeed

    def reframe(key, flags=W.FLAGS_ZSTD, **kw):
        raw = stack[:, :, int(key.split(".")[2])].tobytes()
        return lambda _stored: BW.blosc_frame(raw, 1000, flags=flags, compress=encode, **kw)

    members = W.zstd_members(stack, (48, 64, 1), "blosc-zstd", encode=encode,
                             replace={"0.0.2": reframe("0.0.2", flags=W.FLAGS_ZSTD | 0x04), "0.0.5": reframe("0.0.5", typesize=4, memcpyed=True)})
    p = ZW.write_members(tmp_path / "s.zarr", members)
    feed = ZarrDeviceFeed(ZarrDataset(p), 2, "cuda", num_frames=N)
    want = torch.from_numpy(stack).permute(2, 0, 1)[:, None].contiguous()
    assert torch.equal(next(feed)[0].cpu(), want[:2])
    with pytest.raises(RuntimeError, match=r"0\.0\.2"):
        next(feed)
    assert torch.equal(next(feed)[0].cpu(), want[4:6]) and torch.equal(next(feed)[0].cpu(), want[6:])


@pytest.mark.parametrize("kind", ["blosc-zstd", "zstd"])
@pytest.mark.parametrize("device_decode", [True, False], ids=["device", "host"])
def test_feed_corrupt_chunk_costs_exactly_its_batch(tmp_path, stack, encode, kind, device_decode):
    from yogo_amd import zstd as Z
    from yogo_amd.zarr_feed import ZarrDeviceFeed

    def spoil(stored):
        """the chunk's last Huffman stream (in front of the byte that says "no sequences") loses its marker bit: the headers parse, the
        bitstream does not (libzstd refuses it too)"""
        b = bytearray(stored)
        assert b[-1] == 0
        b[-2] = 0
        return bytes(b)

    members = W.zstd_members(stack, (48, 64, 1), kind, encode=encode, blocksize=4096, replace={"0.0.3": spoil})
    if kind == "zstd":
        assert Z.zstd_frame_status(members["0.0.3"], 3072)[0] == Z.ZSTD_BAD_BITSTREAM
    p = ZW.write_members(tmp_path / "s.zip", members, as_zip=True)
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


@pytest.mark.parametrize("device_outputs", [False, True], ids=["host-outputs", "device-outputs"])
def test_predict_from_a_blosc_zstd_store_equals_predict_from_a_raw_store(tmp_path, capsys, device_outputs):
    from yogo_amd.infer import predict

    rng = np.random.default_rng(6)
    frames = rng.integers(0, 256, size=(64, 96, 10), dtype=np.uint8)
    frames[:, :, ::2] = frames[:, :, ::2] // 64 * 30          # every other frame is one the compressor shrinks (Huffman-coded literals)
    for d in ("a", "b", "out_a", "out_b"):
        (tmp_path / d).mkdir()
    members = W.zstd_members(frames, (64, 96, 1), "blosc-zstd", encode=W.compress, blocksize=2048)
    z_zstd = ZW.write_members(tmp_path / "a" / "stack.zip", members, as_zip=True)
    z_raw = ZW.write_stack(tmp_path / "b" / "stack.zip", frames, (64, 96, 1), as_zip=True)
    pth = _make_checkpoint(tmp_path / "m.pth")
    kw = dict(save_npy=True, batch_size=4, obj_thresh=0.4, iou_thresh=0.5, class_names=CLASSES, count_predictions=True, device_outputs=device_outputs)
    capsys.readouterr()
    _, launches = _launches(lambda: predict(str(pth), path_to_zarr=z_zstd, output_dir=str(tmp_path / "out_a"), **kw))
    counts_a = capsys.readouterr().out
    assert launches == 3
    predict(str(pth), path_to_zarr=z_raw, output_dir=str(tmp_path / "out_b"), **kw)
    counts_b = capsys.readouterr().out
    a, b = (tmp_path / "out_a" / "stack.npy").read_bytes(), (tmp_path / "out_b" / "stack.npy").read_bytes()
    assert a == b and np.load(tmp_path / "out_a" / "stack.npy").shape[1] > 0
    assert counts_a == counts_b and counts_a.strip()
