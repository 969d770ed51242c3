"""tests/_zarr_unpack_ref.py -- the numpy statement tests/test_gpu_zarr_unpack_edges.py holds the unpack kernel to -- against the
code it restates, without a GPU: `stage` against the real `FrameSource` / `plan_batch` / `ChunkStager.stage` on stores written by
tests/_zarr_write.py, `expect` against the host route (`ZarrDataset` + `CenterCrop`).  And, as plain integers, the arithmetic of
yogo_amd/csrc/zarr_feed.hip that the GPU cases are chosen by."""
import numpy as np
import pytest
import torch

import _zarr_unpack_ref as R
import _zarr_write as ZW
from yogo_amd.device_decode import center_crop_origin
from yogo_amd.image_path_dataset import CenterCrop, ZarrDataset
from yogo_amd.zarr_feed import ChunkStager, FrameSource, plan_batch
from yogo_amd.zarr_store import open_zarr

SHAPE = (24, 48, 9)
FILL = 7
LO, HI = 4, 9      # the batch starts inside a chunk (cn 2, 3), crosses chunk boundaries and ends in a padded edge chunk (cn 2)
# chunks -> a chunk of the batch to leave out of the store
GEOMETRIES = {(24, 48, 1): (0, 0, 5), (24, 48, 3): (0, 0, 2), (16, 48, 1): (1, 0, 6), (5, 7, 2): (2, 3, 2), (32, 64, 1): (0, 0, 8)}


@pytest.fixture(scope="module")
def stack():
    return np.random.default_rng(11).integers(0, 256, size=SHAPE, dtype=np.uint8)


@pytest.mark.parametrize("with_skip", [False, True], ids=["whole", "skip"])
@pytest.mark.parametrize("chunks", list(GEOMETRIES), ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("order", ["C", "F"])
def test_stage_and_expect_equal_the_feed_and_the_host_route(tmp_path, stack, order, chunks, with_skip):
    skip = [GEOMETRIES[chunks]] if with_skip else []
    p = ZW.write_stack(tmp_path / "s.zarr", stack, chunks, order=order, fill_value=FILL, skip=skip)
    src = FrameSource(open_zarr(p))
    plan = plan_batch(src, LO, HI)
    buf = np.full(plan.nbytes, 0x55, np.uint8)
    stager = ChunkStager(src, threads=2)
    try:
        stager.stage(plan, buf)
    finally:
        stager.close()

    staged, tile_off, tile_k = R.stage(stack, chunks, order, range(LO, HI), skip=skip)
    assert tile_off.dtype == np.int64 and tile_k.dtype == np.int32 and staged.dtype == np.uint8
    assert np.array_equal(tile_off, plan.tile_off) and np.array_equal(tile_k, plan.tile_k)
    assert (tile_off < 0).any() == with_skip
    assert staged.shape == buf.shape
    # the positions that hold a pixel of the array are those a second poison does not change
    other, _, _ = R.stage(stack, chunks, order, range(LO, HI), skip=skip, poison=0x11)
    inside = staged == other
    assert np.array_equal(staged[inside], buf[inside])
    ch, cw, cn = chunks
    n_chunks = len(plan.keys)
    pixels = sum(min(ch, SHAPE[0] - ty * ch) * min(cw, SHAPE[1] - tx * cw) * min(cn, SHAPE[2] - tk * cn)
                 for ty, tx, tk in (tuple(int(v) for v in k.split(".")) for k in plan.keys))
    assert int(inside.sum()) == pixels and n_chunks == len(np.unique(tile_off[tile_off >= 0]))
    assert bool((staged[~inside] == 0xEE).all())
    # without the padding the buffer ends with the last chunk
    short, toff2, _ = R.stage(stack, chunks, order, range(LO, HI), skip=skip, pad_end=False)
    assert len(short) == (n_chunks - 1) * src.chunk_stride + src.chunk_nbytes and np.array_equal(short, staged[:len(short)])
    assert np.array_equal(toff2, tile_off)

    for crop in (None, (10, 40)):
        OH, OW = crop or SHAPE[:2]
        top, left = center_crop_origin(SHAPE[0], SHAPE[1], OH, OW)
        ds = ZarrDataset(p, image_transforms=[CenterCrop((OH, OW))])
        host = torch.stack([ds[i][0] for i in range(LO, HI)])
        got = R.expect(stack, range(LO, HI), top, left, OH, OW, skip, chunks, FILL)
        assert got.dtype == np.uint8 and got.shape == (HI - LO, 1, OH, OW)
        assert torch.equal(torch.from_numpy(got), host), (crop,)


def test_stage_takes_frames_in_any_order(stack):
    """what plan_batch cannot be asked for: repeated frames, frames out of order -- first-use order of the chunks, by hand"""
    from yogo_amd import device_decode

    assert R.ALIGN == device_decode.ALIGN
    n = 24 * 48 * 3
    for align, stride in ((R.ALIGN, 3584), (16, 3456)):
        staged, tile_off, tile_k = R.stage(stack, (24, 48, 3), "C", [7, 0, 8, 1, 7], align=align)
        assert tile_off.reshape(-1).tolist() == [0, stride, 0, stride, 0] and tile_k.tolist() == [1, 0, 2, 1, 1]
        assert len(staged) == 2 * stride
        assert np.array_equal(staged[:n].reshape(24, 48, 3), stack[:, :, 6:9])
        assert np.array_equal(staged[stride:stride + n].reshape(24, 48, 3), stack[:, :, 0:3])
        assert bool((staged[n:stride] == 0xEE).all())
    want = R.expect(stack, [7, 0, 8, 1, 7], 2, 3, 5, 6, (), (24, 48, 3), FILL)
    assert np.array_equal(want[2, 0], stack[2:7, 3:9, 8]) and np.array_equal(want[0], want[4])


# ---- the kernel's arithmetic, restated (yogo_amd/csrc/zarr_feed.hip) -------------------------------------------------------------
BLOCK, UNROLL, SLAB = 256, 4, 4096
SLAB_DW = 1028 + 1028 // 32 + 4


def _slab(chunks, ly, sl, left=0, OW=None, raw=0):
    """(head, pieces, pixels) of slab sl of chunk row ly of tile 0 -- the deinterleave kernel's `start`, `head`, `npieces`"""
    ch, cw, cn = chunks
    XS = (SLAB // cn) & ~3
    xa = left + sl * XS
    nx = min(left + (OW or cw), cw, xa + XS) - xa
    start = raw + (ly * cw + xa) * cn
    head = start % 16
    return head, (head + nx * cn + 15) >> 4, nx


def _lds_dword_of_piece(l):
    return 4 * l + (l >> 3)


def _lds_byte_of(p):
    return p + ((p >> 7) << 2)


def test_the_257_piece_slab_and_the_top_of_the_lds_array():
    assert SLAB_DW == 1064
    chunks = (3, 4099, 2)
    assert _slab(chunks, 1, 0) == (6, 257, 2048)
    assert _slab(chunks, 2, 0) == (12, 257, 2048)
    assert _slab(chunks, 0, 0) == (0, 256, 2048) and _slab(chunks, 1, 2) == (6, 1, 3)
    head, pieces, nx = _slab(chunks, 1, 0)
    assert pieces > BLOCK                                   # the piece loop goes round a second time
    assert _lds_dword_of_piece(pieces - 1) + 3 == 1059      # the top dword the staging writes
    top_read = _lds_byte_of(12 + nx * 2 - 1)                # the last byte any lane reads (head 12)
    assert top_read // 4 == 1058 and top_read // 4 < SLAB_DW
    # piece l's four dwords and the bytes read back through the other formula are the same place
    for l in (0, 7, 8, 255, 256):
        assert _lds_byte_of(16 * l) == 4 * _lds_dword_of_piece(l) and _lds_byte_of(16 * l + 15) == 4 * _lds_dword_of_piece(l) + 15
    # no slab of any cn has more pieces: nx * cn <= SLAB and head <= 15
    assert max((15 + ((SLAB // cn) & ~3) * cn + 15) >> 4 for cn in range(2, 1025)) == 257


def test_the_geometries_the_gpu_cases_are_chosen_by():
    # the production frame as one span: 49 794 pieces in 49 workgroups, the last with 642
    seg16, per_block = 772 * 1032 // 16, BLOCK * UNROLL
    assert 772 * 1032 % 16 == 0 and 1032 % 16 != 0
    assert (seg16, -(-seg16 // per_block), seg16 - 48 * per_block) == (49794, 49, 642)
    assert (30 * 1000 // 16, 16 * 1024 // 16, 16 * 1040 // 16 - per_block, 20480 // 16) == (1875, 1024, 16, 1280)
    assert (2 * 1000) % 16 == 0 and (1 * 1000) % 16 != 0 and -(-65535 // per_block) == 64 and -(-30 * 1000 // per_block) == 30
    # slabs per tile and pixels per slab
    assert [_slab((6, 1032, 8), 0, s)[2] for s in range(3)] == [512, 512, 8]
    assert [_slab((4, 200, 64), 0, s)[2] for s in range(4)] == [64, 64, 64, 8]
    assert [_slab((2, 10, 1024), 0, s)[2] for s in range(3)] == [4, 4, 2]
    assert [-(-85 // ((SLAB // cn) & ~3)) for cn in (5, 100, 1000)] == [1, 3, 22]   # (23 slabs uncropped: 90 px)
    assert 5 * 128 > BLOCK and 6 * 128 > BLOCK                                        # nmem * nq of the cn = 8 runs
    # the reduced last piece of an unpadded buffer needs the last chunk's last row INSIDE the frame: 24 x 48 frames in (5, 7, 2)
    # chunks end in a chunk whose last row and column lie outside, 25 x 49 frames do not
    def last_piece_end(H, W):
        ly, lx = (H - 1) % 5, (W - 1) % 7
        return -(-((ly * 7 + lx) * 2 + 2) // 16) * 16
    assert last_piece_end(24, 48) == 64 <= 70 and last_piece_end(25, 49) == 80 > 70
