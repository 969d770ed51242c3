"""`yogo_zarr_unpack` (yogo_amd/csrc/zarr_feed.hip) at the sizes where its five kernels take another turn: more than one workgroup
and a partial last one, the unrolled steps past the first, several slabs per tile, the 257-piece slab and the top of the LDS array,
runs of rows longer than a workgroup, an output that is not 16-byte aligned, an unpadded staging buffer, C-order gather -- and the
production frame, 772 x 1032.  Inputs come from tests/_zarr_unpack_ref.py (`stage`: the feed's layout, with every byte that is no
pixel poisoned), the expectation from its `expect` (numpy slicing; fp32 = torch's CPU `uint8 / 255`).  Every case: both output
dtypes, `out` pre-filled with poison inside a larger buffer whose guard elements must survive, the path read from the launch log
and compared with a literal, `torch.equal` -- nothing here has a tolerance.  What the table's geometry does to the kernel's
indices is pinned as integers in tests/test_zarr_unpack_ref_host.py."""
import numpy as np
import pytest
import torch

import _zarr_unpack_ref as R

pytestmark = pytest.mark.gpu
FILL = 7
GUARD = 64                                             # elements either side of `out` (a multiple of 16 bytes in both dtypes)
OUT_POISON = {torch.uint8: 0xA5, torch.float32: -3.0}   # no pixel / 255 is negative; 0xA5 is neither FILL nor the staging poison


def _stack(shape):
    return np.random.default_rng(sum(shape)).integers(0, 256, size=shape, dtype=np.uint8)


def _guarded_out(dt, B, OH, OW, out_off):
    """-> (the whole buffer, `out` as a view of it that starts `out_off` elements after a 16-byte boundary)"""
    n = B * OH * OW
    big = torch.full((GUARD + out_off + n + GUARD,), OUT_POISON[dt], dtype=dt, device="cuda")
    out = big[GUARD + out_off:GUARD + out_off + n].view(B, 1, OH, OW)
    assert big.data_ptr() % 16 == 0 and out.data_ptr() % 16 == (out_off * big.element_size()) % 16 and out.is_contiguous()
    return big, out


def _guards_intact(big, out_off, n):
    host = big.cpu()
    poison = OUT_POISON[big.dtype]
    return bool((host[:GUARD + out_off] == poison).all()) and bool((host[GUARD + out_off + n:] == poison).all())


def _launch(staged, tile_off, tile_k, *, chunks, order, frame_shape, crop, B, out_off=0, staged_bytes=None, raw_call=False):
    """both dtypes through `unpack` (or, raw_call, straight through the C ABI: the wrapper refuses tables it calls wrong)
    -> ({dtype: host result}, log lines); asserts the guards"""
    from yogo_amd import _hip
    from yogo_amd.zarr_feed import unpack

    top, left, OH, OW = crop
    H, W = frame_shape
    ch, cw, cn = chunks
    got = {}
    if raw_call:
        toff_d, tk_d = torch.from_numpy(np.ascontiguousarray(tile_off)).cuda(), torch.from_numpy(np.ascontiguousarray(tile_k)).cuda()
    _hip.launch_log(True)
    try:
        for dt in (torch.uint8, torch.float32):
            big, out = _guarded_out(dt, B, OH, OW, out_off)
            if raw_call:
                _hip.call("yogo_zarr_unpack", staged, staged.numel() if staged_bytes is None else staged_bytes, toff_d, tk_d, B,
                          -(-H // ch), -(-W // cw), ch, cw, cn, 1 if order == "F" else 0, FILL, H, W, top, left, OH, OW, out,
                          1 if dt == torch.float32 else 0, _hip.stream_ptr())
            else:
                unpack(staged, tile_off, tile_k, chunks=chunks, order_f=order == "F", fill=FILL, frame_shape=frame_shape, out=out,
                       top=top, left=left)
            torch.cuda.synchronize()
            assert _guards_intact(big, out_off, B * OH * OW), ("a guard element was written", dt)
            got[dt] = out.cpu()
        log = _hip.read_launch_log()
    finally:
        _hip.launch_log(False)
    return got, log


def _check(got, want_u8, log, path):
    assert [ln.split(" | ")[0] for ln in log] == [f"zarr_unpack_{path}_kernel<u8>", f"zarr_unpack_{path}_kernel<f32>"], log
    want_u8 = torch.from_numpy(want_u8)
    want = {torch.uint8: want_u8, torch.float32: want_u8 / 255}
    for dt in (torch.uint8, torch.float32):
        assert got[dt].dtype == dt and got[dt].shape == want[dt].shape
        if not torch.equal(got[dt], want[dt]):
            bad = (got[dt] != want[dt]).nonzero()
            raise AssertionError(f"{path} {dt}: {len(bad)} of {want[dt].numel()} elements differ, the first at {bad[0].tolist()}: "
                                 f"{got[dt][tuple(bad[0])].item()} for {want[dt][tuple(bad[0])].item()}")


def _case(shape, chunks, idxs, crop, path, order="C", skip=(), pad_end=True, align=R.ALIGN, out_off=0):
    stack = _stack(shape)
    idxs = list(idxs)
    crop = crop or (0, 0, shape[0], shape[1])
    staged, tile_off, tile_k = R.stage(stack, chunks, order, idxs, skip=skip, pad_end=pad_end, align=align)
    if skip:
        assert (tile_off < 0).any()
    want = R.expect(stack, idxs, *crop, skip, chunks, FILL)
    got, log = _launch(torch.from_numpy(staged).cuda(), tile_off, tile_k, chunks=chunks, order=order, frame_shape=shape[:2], crop=crop,
                       B=len(idxs), out_off=out_off)
    _check(got, want, log, path)


# id: (frame H x W x N, chunks, frames, crop (top, left, OH, OW) or None, the path the launch log must name, further arguments)
ROWS = {
    # rows_vec as ONE span per batch row (whole rows of a single tile)
    "prod": ((772, 1032, 3), (772, 1032, 1), range(3), None, "rows_vec", {}),                            # 49 workgroups, the last with 642 pieces
    "span-crop-rows": ((34, 1000, 2), (34, 1000, 1), range(2), (2, 0, 30, 1000), "rows_vec", {}),        # 1 875 pieces, top != 0
    "span-exact-block": ((16, 1024, 2), (16, 1024, 1), range(2), None, "rows_vec", {}),                  # exactly 1 024 pieces
    "span-16-past": ((16, 1040, 2), (16, 1040, 1), range(2), None, "rows_vec", {}),                      # 16 lanes of a second workgroup
    "span-refused": ((34, 1000, 2), (34, 1000, 1), range(2), (1, 0, 30, 1000), "rows_byte", {}),         # top * cw no multiple of 16
    # rows_vec as one segment per image row, and rows_byte
    "seg-tiles-down": ((40, 64, 2), (16, 64, 1), range(2), (3, 16, 33, 32), "rows_vec", {"skip": [(1, 0, 1)]}),
    "seg-wide": ((3, 20480, 1), (2, 20480, 1), range(1), None, "rows_vec", {}),                          # 1 280 pieces per row: blockIdx.x = 1, u >= 1
    "chunk-over-frame": ((24, 48, 2), (32, 64, 1), range(2), None, "rows_vec", {}),
    "widest": ((1, 65535, 1), (1, 65535, 1), range(1), None, "rows_byte", {}),                           # the W limit, 64 workgroups
    "byte-tiles": ((40, 56, 3), (16, 24, 1), range(3), (3, 5, 33, 47), "rows_byte", {"skip": [(1, 1, 2)]}),
    "out-off-by-one": ((34, 1000, 2), (34, 1000, 1), range(2), (2, 0, 30, 1000), "rows_byte", {"out_off": 1}),
}

DEINTERLEAVE = {
    "cn8-slabs": ((6, 1032, 16), (6, 1032, 8), range(3, 14), None, {}),             # slabs of 512, 512, 8 px; runs of 5 and 6 rows
    "cn2-257-pieces": ((3, 4099, 4), (3, 4099, 2), range(1, 4), None, {}),          # heads 6 and 12: 257 pieces, the top of the LDS array
    "cn64": ((4, 200, 70), (4, 200, 64), range(70), None, {}),                      # 4 slabs; runs of 64 and 6; edge chunk on the frame axis
    "cn1024": ((2, 10, 1030), (2, 10, 1024), range(1020, 1028), None, {}),          # XS = 4; a run across the chunk boundary
    "cn-odd-5": ((5, 90, 8), (5, 90, 5), range(4, 7), (1, 3, 3, 85), {}),           # strides that are no power of two: 1 slab,
    "cn-odd-100": ((5, 90, 103), (5, 90, 100), range(99, 102), (1, 3, 3, 85), {}),  # 3 slabs,
    "cn-odd-1000": ((5, 90, 1003), (5, 90, 1000), range(999, 1002), (1, 3, 3, 85), {}),   # 22 slabs
    "tiles-odd-crop": ((24, 48, 9), (5, 7, 3), range(4, 8), (6, 10, 11, 29), {}),   # the crop starts inside a tile; OH * OW odd
    "tiles-odd-crop-16": ((24, 48, 9), (5, 7, 3), range(4, 8), (6, 10, 11, 29), {"align": 16}),   # chunks 112 bytes apart
    "shared-not-adjacent": ((24, 48, 9), (24, 48, 3), [0, 3, 1, 0, 2], None, {}),
    "unpadded-end": ((24, 48, 4), (5, 7, 2), range(2, 4), None, {"pad_end": False, "align": 16}),
    # ... whose last chunk's last row and column lie outside the frame, so no piece reaches the buffer's end (pinned in
    # test_zarr_unpack_ref_host.py).  25 x 49 frames fill the last chunk: its last piece has 6 of 16 bytes
    "unpadded-end-reduced-piece": ((25, 49, 4), (5, 7, 2), range(2, 4), None, {"pad_end": False, "align": 16}),
    "deint-out-off": ((6, 1032, 16), (6, 1032, 8), range(3, 6), None, {"out_off": 1}),   # scalar stores throughout
}

GATHER = {
    "c-order-cn1030": ((30, 40, 1033), (16, 24, 1030), range(1028, 1032), (2, 3, 27, 35), "C", {}),
    "f-order-large": ((40, 56, 5), (16, 24, 3), range(1, 5), (3, 5, 33, 47), "F", {"skip": [(1, 1, 0)]}),
}


@pytest.mark.parametrize("name", list(ROWS))
def test_rows(name):
    shape, chunks, idxs, crop, path, kw = ROWS[name]
    _case(shape, chunks, idxs, crop, path, **kw)


@pytest.mark.parametrize("name", list(DEINTERLEAVE))
def test_deinterleave(name):
    shape, chunks, idxs, crop, kw = DEINTERLEAVE[name]
    _case(shape, chunks, idxs, crop, "deinterleave", **kw)


@pytest.mark.parametrize("name", list(GATHER))
def test_gather(name):
    shape, chunks, idxs, crop, order, kw = GATHER[name]
    _case(shape, chunks, idxs, crop, "gather", order=order, **kw)


# ---- the C ABI's own rules (include/yogo_hip.h), past the wrapper's checks -----------------------------------------------------
# id: (frame, chunks, order, frames, crop, path)
ABI_PATHS = {
    "rows_vec-span": ((16, 64, 3), (16, 64, 1), "C", range(3), None, "rows_vec"),
    "rows_vec-segments": ((40, 64, 3), (16, 64, 1), "C", range(3), (3, 16, 33, 32), "rows_vec"),
    "rows_byte": ((13, 17, 3), (13, 17, 1), "C", range(3), None, "rows_byte"),
    "deinterleave": ((24, 48, 3), (24, 48, 3), "C", range(3), None, "deinterleave"),       # the three rows are one run
    "gather-f": ((24, 48, 3), (24, 48, 3), "F", range(3), None, "gather"),
    "gather-c": ((6, 10, 1033), (6, 10, 1030), "C", range(3), None, "gather"),
}


@pytest.mark.parametrize("bad", ["cn", "minus-one"])
@pytest.mark.parametrize("name", list(ABI_PATHS))
def test_tile_k_outside_the_chunk_reads_as_fill_for_that_row(name, bad):
    """`a value outside reads as fill` (include/yogo_hip.h), one row of three and that row only, on every path.  The guard is
    `k_ok = (unsigned)tile_k[b] < (unsigned)cn` in zarr_feed.hip: in zarr_unpack_rows_vec_kernel (once per workgroup) and in
    unpack_bytes (rows_byte, gather) it turns the row's offset into -1 before anything is read, in the deinterleave kernel's output
    loop it replaces the LDS index by that of k = 0 -- so nothing is read outside `staged`."""
    shape, chunks, order, idxs, crop, path = ABI_PATHS[name]
    stack = _stack(shape)
    crop = crop or (0, 0, shape[0], shape[1])
    staged, tile_off, tile_k = R.stage(stack, chunks, order, idxs)
    tile_k[1] = chunks[2] if bad == "cn" else -1
    want = R.expect(stack, idxs, *crop, (), chunks, FILL)
    want[1] = FILL
    got, log = _launch(torch.from_numpy(staged).cuda(), tile_off, tile_k, chunks=chunks, order=order, frame_shape=shape[:2], crop=crop,
                       B=3, raw_call=True)
    _check(got, want, log, path)


@pytest.mark.parametrize("name", ["rows_vec-span", "rows_vec-segments", "deinterleave", "gather-f", "gather-c"])
def test_tile_offset_whose_chunk_ends_past_the_staged_bytes_reads_as_fill(name):
    """Four rows, two and two on either side of a chunk boundary on the frame axis; the kernel is told of one byte less than the
    first chunk of the second pair needs, and row 1's offsets are replaced by one far beyond the buffer: rows 1, 2 and 3 are fill,
    row 0 is read.  The guard is `off + chunk_bytes > staged_bytes` in
    tile_base (rows_vec, unpack_bytes) and `valid` in the deinterleave kernel, both evaluated before the first read of `staged`;
    the tensor itself holds both chunks whole, so even a kernel without the guard would stay inside the allocation."""
    shape, chunks, order, _, crop, path = ABI_PATHS[name]
    cn = chunks[2]
    shape = shape[:2] + (2 * cn,)
    idxs = [0, cn - 1, cn, 2 * cn - 1] if cn > 1 else [0, 0, 1, 1]
    stack = _stack(shape)
    crop = crop or (0, 0, shape[0], shape[1])
    staged, tile_off, tile_k = R.stage(stack, chunks, order, idxs)
    second = int(tile_off[2].min())   # the first chunk of the second frame-axis chunk: every tile of rows 2 and 3 lies at or behind it
    assert second > int(tile_off[0].max()) >= 0 and np.array_equal(tile_off[2], tile_off[3])
    tile_off[1] = 1 << 40
    want = R.expect(stack, idxs, *crop, (), chunks, FILL)
    want[1:] = FILL
    got, log = _launch(torch.from_numpy(staged).cuda(), tile_off, tile_k, chunks=chunks, order=order, frame_shape=shape[:2], crop=crop,
                       B=4, staged_bytes=second + chunks[0] * chunks[1] * cn - 1, raw_call=True)
    _check(got, want, log, path)


def test_refusals_come_back_as_errors_without_a_launch():
    from yogo_amd import _hip

    H, W, ch, cw = 24, 48, 16, 48
    staged = torch.zeros(2 * ch * cw + 16, dtype=torch.uint8, device="cuda")
    toff = torch.zeros(2, dtype=torch.int64, device="cuda")
    tk = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.zeros(H * W, dtype=torch.uint8, device="cuda")

    def call(staged=staged, B=1, gh=2, gw=1, fill=FILL, H=H, W=W):
        _hip.call("yogo_zarr_unpack", staged, 2 * ch * cw, toff, tk, B, gh, gw, ch, cw, 1, 0, fill, H, W, 0, 0, 24, 48, out, 0, _hip.stream_ptr())

    _hip.launch_log(True)
    try:
        call()
        assert len(_hip.read_launch_log()) == 1
        _hip.launch_log(True)
        for kw, text in [(dict(gh=1), "tile grid"), (dict(gh=3), "tile grid"), (dict(gw=2), "tile grid"),
                         (dict(staged=staged[1:]), "16-byte aligned"), (dict(fill=256), "no uint8"), (dict(B=65536), "at most 65535"),
                         (dict(H=65536, gh=4096), "bad frame shape"), (dict(W=65536, gw=1366), "bad frame shape")]:
            with pytest.raises(RuntimeError, match=text):
                call(**kw)
        assert _hip.read_launch_log() == []
    finally:
        _hip.launch_log(False)
    torch.cuda.synchronize()
    assert not bool(out.any())   # (the one launch read the zeros)
