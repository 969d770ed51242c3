"""The Zarr v2 reader (yogo_amd/zarr_store.py), ZarrDataset / get_dataset and the planning half of the zarr feed, on the host.
Stores come from tests/_zarr_write.py; every frame is read back and compared byte for byte with the array it was written from."""
import itertools
import json
import os
import zipfile

import numpy as np
import pytest
import torch

import _zarr_write as ZW
from yogo_amd.zarr_store import ZarrArray, ZarrGroup, open_zarr

H, W, N = 13, 17, 7
CHUNKS = [(13, 17, 1), (13, 17, 3), (5, 7, 2)]


@pytest.fixture(scope="module")
def stack():
    return np.random.default_rng(0).integers(0, 256, size=(H, W, N), dtype=np.uint8)


def _path(tmp_path, as_zip):
    return tmp_path / ("s.zip" if as_zip else "s.zarr")


@pytest.mark.parametrize("chunks", CHUNKS, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("as_zip,compressor,order,separator",
                         [c for c in itertools.product([False, True], [None, "zlib", "gzip"], ["C", "F"], [".", "/"])],
                         ids=lambda v: {None: "raw", True: "zip", False: "dir", ".": "dot", "/": "slash"}.get(v, str(v)))
def test_every_frame_reads_back(tmp_path, stack, chunks, as_zip, compressor, order, separator):
    p = ZW.write_stack(_path(tmp_path, as_zip), stack, chunks, as_zip=as_zip, compressor=compressor, order=order, separator=separator)
    a = open_zarr(p)
    assert isinstance(a, ZarrArray) and a.shape == (H, W, N) and a.chunks == chunks
    for idx in range(N):
        got = a[:, :, idx]
        assert got.dtype == np.uint8 and got.shape == (H, W)
        assert np.array_equal(got, stack[:, :, idx]), idx
    with pytest.raises(IndexError):
        a[:, :, N]
    with pytest.raises(IndexError):
        a[:, :, N + 5]


def test_default_separator_and_deflated_zip_members(tmp_path, stack):
    p = ZW.write_stack(tmp_path / "s.zip", stack, (13, 17, 3), as_zip=True, deflate=True, write_separator=False)
    a = open_zarr(p)
    assert a.separator == "."
    assert all(np.array_equal(a[:, :, i], stack[:, :, i]) for i in range(N))


def test_last_zip_member_of_a_name_wins(tmp_path, stack):
    members = ZW.array_members(stack, (13, 17, 1))
    p = tmp_path / "s.zip"
    with pytest.warns(UserWarning):   # zipfile says "Duplicate name"
        with zipfile.ZipFile(p, "w") as zf:
            zf.writestr("0.0.2", bytes(H * W))
            for k, v in members.items():
                zf.writestr(k, v)
            zf.writestr("0.0.4", stack[:, :, 1].tobytes())
    a = open_zarr(p)
    assert np.array_equal(a[:, :, 2], stack[:, :, 2])
    assert np.array_equal(a[:, :, 4], stack[:, :, 1])
    assert len(a) == N


@pytest.mark.parametrize("as_zip", [False, True], ids=["dir", "zip"])
def test_group_of_2d_arrays(tmp_path, stack, as_zip):
    frames = [stack[:, :, i] for i in range(N)]
    p = ZW.write_group(_path(tmp_path, as_zip), frames, (5, 7), as_zip=as_zip, compressor="zlib")
    g = open_zarr(p)
    assert isinstance(g, ZarrGroup) and len(g) == N
    for idx in range(N):
        assert np.array_equal(g[idx][:], frames[idx])
    with pytest.raises(IndexError):
        g[N]


@pytest.mark.parametrize("chunks,skip", [((13, 17, 1), [(0, 0, 2)]), ((5, 7, 2), [(1, 2, 0)])], ids=["frame", "tile"])
def test_missing_chunk_reads_as_fill_value(tmp_path, stack, chunks, skip):
    p = ZW.write_stack(tmp_path / "s.zarr", stack, chunks, fill_value=9, skip=skip)
    a = open_zarr(p)
    want = stack.copy()
    (ty, tx, tk), (ch, cw, cn) = skip[0], chunks
    want[ty * ch:(ty + 1) * ch, tx * cw:(tx + 1) * cw, tk * cn:(tk + 1) * cn] = 9
    for idx in range(N):
        assert np.array_equal(a[:, :, idx], want[:, :, idx])


@pytest.mark.parametrize("as_zip", [False, True], ids=["dir", "zip"])
def test_len_is_the_number_of_keys_present(tmp_path, stack, as_zip):
    p = ZW.write_stack(_path(tmp_path, as_zip), stack, (13, 17, 1), as_zip=as_zip, shape=(H, W, 100), separator="/")
    a = open_zarr(p)
    assert a.shape[2] == 100 and len(a) == N == a.initialized
    assert np.array_equal(a[:, :, 50], np.zeros((H, W), np.uint8))   # declared, never written: fill
    # three frames per chunk: the reference's len counts chunks, not frames
    assert len(open_zarr(ZW.write_stack(tmp_path / "c3.zarr", stack, (13, 17, 3)))) == 3


def test_unknown_compressor_without_numcodecs(tmp_path, stack, monkeypatch):
    import sys

    monkeypatch.setitem(sys.modules, "numcodecs", None)   # `import numcodecs` raises ImportError
    p = ZW.write_stack(tmp_path / "s.zarr", stack, (13, 17, 1), compressor={"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1})
    with pytest.raises(NotImplementedError, match="blosc") as e:
        open_zarr(p)
    assert str(p) in str(e.value)


def test_other_dtype_and_filters_are_refused(tmp_path, stack):
    with pytest.raises(ValueError, match="<u2"):
        open_zarr(ZW.write_stack(tmp_path / "a.zarr", stack, (13, 17, 1), dtype="<u2"))
    with pytest.raises(NotImplementedError, match="delta"):
        open_zarr(ZW.write_stack(tmp_path / "b.zarr", stack, (13, 17, 1), filters=[{"id": "delta", "dtype": "|u1"}]))


def test_empty_and_missing_stores(tmp_path):
    (tmp_path / "empty.zarr").mkdir()
    with pytest.raises(ValueError):
        open_zarr(tmp_path / "empty.zarr")
    with pytest.raises(FileNotFoundError):
        open_zarr(tmp_path / "nothing.zarr")


def test_corrupt_chunks_raise_runtime_error_naming_the_key(tmp_path, stack):
    # a corrupt zlib stream in a directory store
    p = ZW.write_stack(tmp_path / "z.zarr", stack, (13, 17, 1), compressor="zlib")
    with open(os.path.join(p, "0.0.3"), "r+b") as f:
        f.seek(4)
        f.write(b"\xff\xff\xff\xff")
    a = open_zarr(p)
    with pytest.raises(RuntimeError, match=r"0\.0\.3"):
        a[:, :, 3]
    assert np.array_equal(a[:, :, 2], stack[:, :, 2])
    # a raw chunk that is too short
    p = ZW.write_stack(tmp_path / "r.zarr", stack, (13, 17, 1))
    with open(os.path.join(p, "0.0.5"), "r+b") as f:
        f.truncate(100)
    with pytest.raises(RuntimeError, match=r"0\.0\.5"):
        open_zarr(p)[:, :, 5]
    # a zip whose stored member was damaged after writing (CRC), and one cut off inside its last member
    p = ZW.write_stack(tmp_path / "s.zip", stack, (13, 17, 1), as_zip=True)
    with zipfile.ZipFile(p) as zf:
        info = zf.getinfo("0.0.1")
    raw = bytearray(open(p, "rb").read())
    at = info.header_offset + 30 + len("0.0.1") + 20
    raw[at] ^= 0xFF
    open(p, "wb").write(raw)
    with pytest.raises(RuntimeError, match=r"0\.0\.1"):
        open_zarr(p)[:, :, 1]
    members = ZW.array_members(stack, (13, 17, 1), compressor="zlib")
    members["0.0.6"] = members["0.0.6"][:-7]   # a truncated zlib stream as a zip member
    p = ZW.write_members(tmp_path / "t.zip", members, as_zip=True)
    with pytest.raises(RuntimeError, match=r"0\.0\.6"):
        open_zarr(p)[:, :, 6]


def test_zarr_dataset_and_get_dataset(tmp_path):
    from yogo_amd.image_path_dataset import CenterCrop, ZarrDataset, get_dataset

    frames = np.random.default_rng(1).integers(0, 256, size=(H, W, 12), dtype=np.uint8)
    p = ZW.write_stack(tmp_path / "s.zip", frames, (13, 17, 1), as_zip=True, compressor="zlib")
    ds = ZarrDataset(p)
    assert len(ds) == 12
    img, name = ds[3]
    assert img.dtype == torch.uint8 and tuple(img.shape) == (1, H, W) and name == "img_03.png"
    assert torch.equal(img, torch.from_numpy(frames[:, :, 3])[None])
    got = get_dataset(path_to_zarr=p, image_transforms=[CenterCrop((5, W))], normalize_images=True)
    assert isinstance(got, ZarrDataset)
    img, name = got[11]
    assert name == "img_11.png" and img.dtype == torch.float32
    assert torch.equal(img, torch.from_numpy(frames[4:9, :, 11])[None] / 255)
    assert ZarrDataset(p, image_name_from_idx=lambda i: f"f{i}")[2][1] == "f2"
    with pytest.raises(FileNotFoundError):
        ZarrDataset(tmp_path / "nothing.zip")
    with pytest.raises(ValueError):
        get_dataset(path_to_images=tmp_path, path_to_zarr=p)
    with pytest.raises(ValueError):
        get_dataset()
    # a store with no chunk written: the reference fails on math.log(0)
    empty = ZW.write_stack(tmp_path / "e.zarr", frames, (13, 17, 1), skip=[(0, 0, k) for k in range(12)])
    with pytest.raises(ValueError):
        ZarrDataset(empty)


def test_feed_plan_of_a_batch_inside_shared_chunks(tmp_path):
    from yogo_amd.zarr_feed import FrameSource, plan_batch

    frames = np.random.default_rng(2).integers(0, 256, size=(H, W, 10), dtype=np.uint8)
    src = FrameSource(open_zarr(ZW.write_stack(tmp_path / "s.zarr", frames, (13, 17, 3))))
    plan = plan_batch(src, 4, 9)
    # frames 4 5 | 6 7 8 : chunks 1 and 2 on the frame axis, positions 1 2 | 0 1 2
    assert plan.keys == ["0.0.1", "0.0.2"]
    assert plan.tile_k.tolist() == [1, 2, 0, 1, 2]
    o1, o2 = plan.offsets["0.0.1"], plan.offsets["0.0.2"]
    assert o1 == 0 and o2 >= H * W * 3 and o2 % 16 == 0
    assert plan.tile_off.reshape(-1).tolist() == [o1, o1, o2, o2, o2]
    # tiles that divide neither H nor W, one chunk absent: 3 x 3 tiles per frame
    p = ZW.write_stack(tmp_path / "t.zarr", frames, (5, 7, 2), skip=[(1, 2, 1)])
    plan = plan_batch(FrameSource(open_zarr(p)), 1, 4)   # frames 1 | 2 3 -> chunks 0 | 1 1
    assert plan.tile_k.tolist() == [1, 0, 1] and plan.tile_off.shape == (3, 3, 3)
    assert plan.keys[:3] == ["0.0.0", "0.1.0", "0.2.0"] and "1.2.1" not in plan.keys and len(plan.keys) == 17
    assert plan.tile_off[0, 1, 2] == plan.offsets["1.2.0"] and plan.tile_off[1, 1, 2] == -1 and plan.tile_off[2, 1, 2] == -1
    assert plan.tile_off[1, 2, 1] == plan.tile_off[2, 2, 1] == plan.offsets["2.1.1"]


@pytest.mark.parametrize("as_zip,compressor", [(False, None), (True, None), (True, "zlib")], ids=["dir-raw", "zip-raw", "zip-zlib"])
def test_feed_stager_reads_a_shared_chunk_once(tmp_path, as_zip, compressor):
    from yogo_amd.zarr_feed import ChunkStager, FrameSource, plan_batch

    frames = np.random.default_rng(3).integers(0, 256, size=(H, W, 10), dtype=np.uint8)
    p = ZW.write_stack(_path(tmp_path, as_zip), frames, (13, 17, 3), as_zip=as_zip, compressor=compressor)
    src = FrameSource(open_zarr(p))
    stager = ChunkStager(src, threads=4)
    bufs = [np.zeros(src.max_chunks(5) * src.chunk_stride, np.uint8) for _ in range(2)]
    prev = None
    try:
        for n, (lo, hi) in enumerate([(0, 5), (5, 10)]):
            plan = plan_batch(src, lo, hi)
            stager.stage(plan, bufs[n], prev)
            prev = (plan, bufs[n])
            for b, idx in enumerate(range(lo, hi)):   # what the kernel would read
                off = int(plan.tile_off[b, 0, 0])
                chunk = bufs[n][off:off + src.chunk_nbytes].reshape(13, 17, 3)
                assert np.array_equal(chunk[:, :, plan.tile_k[b]], frames[:, :, idx])
    finally:
        stager.close()
    # frames 0-4 need chunks 0 1, frames 5-9 chunks 1 2 3: chunk 1 is shared and read once
    assert dict(stager.reads) == {"0.0.0": 1, "0.0.1": 1, "0.0.2": 1, "0.0.3": 1}


def test_reads_a_store_written_by_the_zarr_package(tmp_path):
    """interoperability with real files: runs wherever the zarr package is installed"""
    zarr = pytest.importorskip("zarr")
    frames = np.random.default_rng(4).integers(0, 256, size=(H, W, N), dtype=np.uint8)
    p = str(tmp_path / "real.zip")
    store = zarr.ZipStore(p, mode="w")
    z = zarr.zeros((H, W, N), chunks=(H, W, 1), dtype="u1", store=store, compressor=None)
    for i in range(N):
        z[:, :, i] = frames[:, :, i]
    store.close()
    a = open_zarr(p)
    assert len(a) == N
    for i in range(N):
        assert np.array_equal(a[:, :, i], frames[:, :, i])
