"""zarr stacks under the `zlib` codec through the feed (yogo_amd/zarr_feed.py with yogo_amd/csrc/inflate.hip in front of the unpack
launch): the batches equal the stack and the host route, one inflate launch per non-empty batch, a chunk two batches share is read
once; a chunk whose wrapper is no plain zlib one goes the host way; a chunk longer than the stored-bytes room is inflated on the
host and copied as a raw row; a corrupt chunk costs exactly its batch."""
import zlib

import numpy as np
import pytest
import torch

import _zarr_write as ZW
from yogo_amd.image_path_dataset import ZarrDataset

pytestmark = pytest.mark.gpu
FILL = 9
N = 7


def _stack():
    """frames zlib shrinks (dynamic blocks with matches), one it stores (2) and three whose lower half it does not shrink"""
    rng = np.random.default_rng(21)
    s = rng.integers(0, 4, size=(24, 48, N), dtype=np.uint8) * 60
    s[:, :, 2] = rng.integers(0, 256, size=(24, 48), dtype=np.uint8)
    s[12:, :, 3:6] = rng.integers(0, 256, size=(12, 48, 3), dtype=np.uint8)
    return s


def _launches(run):
    """run() with the launch log on -> (its result, inflate launches, raw-row launches of the Blosc decoder)"""
    from yogo_amd import _hip

    _hip.launch_log(True)
    try:
        res = run()
        log = _hip.read_launch_log()
    finally:
        _hip.launch_log(False)
    return res, sum(ln.startswith("inflate_zlib_kernel") for ln in log), sum(ln.startswith("blosc_lz4_decode_kernel") for ln in log)


def _batches(path, batch, **kw):
    from yogo_amd.zarr_feed import ZarrDeviceFeed

    feed = ZarrDeviceFeed(ZarrDataset(path), batch, "cuda", num_frames=N, **kw)
    out = [b.cpu() for b, _ in feed]
    return torch.cat(out), feed


@pytest.fixture(autouse=True)
def _device_route(monkeypatch):
    """these tests are about the device route, whatever the module's default for the codec is"""
    from yogo_amd import zarr_feed

    monkeypatch.setattr(zarr_feed, "DEVICE_DECODE_ZLIB", True)


@pytest.mark.parametrize("as_zip,batch", [(False, 2), (True, 5)], ids=["dir-b2", "zip-b5"])
@pytest.mark.parametrize("chunks", [(24, 48, 1), (24, 48, 3), (12, 16, 2)], ids=lambda c: "x".join(map(str, c)))
def test_feed_batches_equal_the_stack(tmp_path, chunks, as_zip, batch):
    stack = _stack()
    grid_n = -(-N // chunks[2])
    absent = (0, 0, grid_n - 1) if chunks[2] > 1 else (0, 0, 4)
    members = ZW.array_members(stack, chunks, compressor="zlib", fill_value=FILL, skip=[absent])
    first_blocks = {(v[2] >> 1) & 3 for k, v in members.items() if not k.endswith(".zarray")}
    assert {0, 2} <= first_blocks or chunks == (24, 48, 3)        # stored and dynamic blocks both occur
    p = ZW.write_members(tmp_path / ("s.zip" if as_zip else "s.zarr"), members, as_zip=as_zip)
    want = stack.copy()
    want[absent[0] * chunks[0]:(absent[0] + 1) * chunks[0], absent[1] * chunks[1]:(absent[1] + 1) * chunks[1],
         absent[2] * chunks[2]:(absent[2] + 1) * chunks[2]] = FILL
    want = torch.from_numpy(want).permute(2, 0, 1)[:, None].contiguous()

    (got, feed), inflates, raws = _launches(lambda: _batches(p, batch))
    empty = sum(1 for lo in range(0, N, batch) if chunks[:2] == (24, 48) and
                all(k // chunks[2] == absent[2] for k in range(lo, min(lo + batch, N))))
    assert feed.device_decode and len(feed) == -(-N // batch) and inflates == len(feed) - empty and raws == 0
    assert got.dtype == torch.uint8 and torch.equal(got, want)
    assert max(feed.stager.reads.values()) == 1          # a chunk two batches share is read once
    got_f32, _ = _batches(p, batch, normalize=True)
    assert got_f32.dtype == torch.float32 and torch.equal(got_f32, want / 255)
    (got_host, feed_host), inflates, raws = _launches(lambda: _batches(p, batch, device_decode=False))
    assert not feed_host.device_decode and inflates == 0 and raws == 0 and torch.equal(got_host, got)


def test_module_constant_switches_the_route(tmp_path, monkeypatch):
    from yogo_amd import zarr_feed

    p = ZW.write_stack(tmp_path / "s.zarr", _stack(), (24, 48, 1), compressor="zlib")
    monkeypatch.setattr(zarr_feed, "DEVICE_DECODE_ZLIB", False)
    (got, feed), inflates, _ = _launches(lambda: _batches(p, 4))
    assert not feed.device_decode and inflates == 0
    assert torch.equal(got, torch.from_numpy(_stack()).permute(2, 0, 1)[:, None].contiguous())


def test_chunk_longer_than_the_room_is_inflated_on_the_host(tmp_path):
    """600 sync flushes (an empty stored block each) make chunk 0.0.3 longer than the room a stored chunk has: the host inflates
    it and it is copied as a raw row"""
    stack = _stack()
    members = ZW.array_members(stack, (24, 48, 1), compressor="zlib")
    raw3 = zlib.decompress(members["0.0.3"])
    c = zlib.compressobj(1)
    members["0.0.3"] = b"".join(c.compress(raw3[i:i + 2]) + c.flush(zlib.Z_SYNC_FLUSH) for i in range(0, len(raw3), 2)) + c.flush()
    assert len(members["0.0.3"]) > 2 * len(raw3) and zlib.decompress(members["0.0.3"]) == raw3
    p = ZW.write_members(tmp_path / "s.zarr", members)
    (got, feed), inflates, raws = _launches(lambda: _batches(p, 4))
    assert feed.device_decode and len(members["0.0.3"]) > feed.src.stored_stride and inflates == 2 and raws == 1
    assert torch.equal(got, torch.from_numpy(stack).permute(2, 0, 1)[:, None].contiguous())


@pytest.mark.parametrize("defect", ["bad-fcheck", "too-short", "flipped-bytes", "truncated"])
def test_bad_chunk_costs_exactly_its_batch(tmp_path, defect):
    """a wrapper that is no plain zlib one sends the chunk the host way, where zlib refuses it as well; damage inside the stream is
    the device's to find (the Adler-32, or a check before it)"""
    from yogo_amd import inflate
    from yogo_amd.zarr_feed import ZarrDeviceFeed

    stack = _stack()
    members = ZW.array_members(stack, (24, 48, 1), compressor="zlib")
    z = members["0.0.3"]
    host_way = defect in ("bad-fcheck", "too-short")
    if defect == "bad-fcheck":
        z = z[:1] + bytes([z[1] ^ 1]) + z[2:]
    elif defect == "too-short":
        z = z[:5]
    elif defect == "flipped-bytes":
        z = z[:300] + bytes(b ^ 0xFF for b in z[300:304]) + z[304:]
    else:
        z = z[:len(z) // 2] + z[-4:]
    if host_way:
        with pytest.raises(ValueError):
            inflate.split_zlib(z)
    else:
        off, ln, adler = inflate.split_zlib(z)
        assert inflate.inflate_status(z[off:off + ln], 24 * 48, adler)[0] != inflate.INF_OK
    with pytest.raises(zlib.error):
        zlib.decompress(z)
    members["0.0.3"] = z
    p = ZW.write_members(tmp_path / "s.zip", members, as_zip=True)
    feed = ZarrDeviceFeed(ZarrDataset(p), 2, "cuda", num_frames=N)
    assert feed.device_decode
    want = torch.from_numpy(stack).permute(2, 0, 1)[:, None].contiguous()
    b0, _ = next(feed)
    assert torch.equal(b0.cpu(), want[:2])
    with pytest.raises(RuntimeError, match=r"0\.0\.3.*could not be read" if host_way else r"0\.0\.3.*on the device.*status \d+"):
        next(feed)
    b2, _ = next(feed)
    assert torch.equal(b2.cpu(), want[4:6])
    b3, _ = next(feed)
    assert torch.equal(b3.cpu(), want[6:])
    with pytest.raises(StopIteration):
        next(feed)


@pytest.mark.parametrize("first", ["zlib", "blosc"])
def test_group_with_mixed_compressors(tmp_path, first):
    """a group whose members do not share member 0's compressor: a member under another one is decoded on the host and enters as a
    raw row, whatever the device route of the store is"""
    import json

    import _blosc_write as BW

    stack = _stack()
    other = "blosc" if first == "zlib" else "zlib"
    kinds = [first, other, None, "gzip", first, other, None]
    assert len(kinds) == N and len(set(kinds)) == 4
    members = {".zgroup": json.dumps({"zarr_format": 2}).encode()}
    for i, kind in enumerate(kinds):
        f = stack[:, :, i]
        if kind == "blosc":
            members.update(BW.blosc_members(f, (24, 48), blocksize=500, prefix=f"{i}/"))
        else:
            members.update(ZW.array_members(f, (24, 48), compressor=kind, prefix=f"{i}/"))
    p = ZW.write_members(tmp_path / "g.zarr", members)
    (got, feed), inflates, blosc_launches = _launches(lambda: _batches(p, 3))
    assert feed.device_decode and feed.codec == first
    assert torch.equal(got, torch.from_numpy(stack).permute(2, 0, 1)[:, None].contiguous())
    assert (inflates > 0) == (first == "zlib") and blosc_launches > 0
    (got_host, feed_host), inflates, blosc_launches = _launches(lambda: _batches(p, 3, device_decode=False))
    assert not feed_host.device_decode and inflates == 0 and blosc_launches == 0 and torch.equal(got_host, got)
