"""What `yogo_zarr_unpack` (yogo_amd/csrc/zarr_feed.hip) computes, stated in numpy: the staging buffer and the tables the feed
hands the kernel (`stage`, after yogo_amd/zarr_feed.py's `plan_batch` + `ChunkStager.stage`), and the batch it has to give back
(`expect`, by slicing).  No store is opened on disk, so a geometry with a thousand frames per chunk costs a few megabytes of
memory and nothing else.  tests/test_zarr_unpack_ref_host.py holds both functions to the real planner, stager and host dataset."""
import numpy as np

ALIGN = 256   # yogo_amd/device_decode.py's: where the feed starts a chunk (the kernel itself asks for 16)


def _grid(shape, chunks):
    return tuple(-(-s // c) for s, c in zip(shape, chunks))


def stage(stack, chunks, order, idxs, skip=(), pad_end=True, poison=0xEE, align=ALIGN):
    """-> (staged uint8 [bytes], tile_off int64 [B, gh, gw], tile_k int32 [B]) for the frames `idxs` (any order, repeats allowed)
    of the [H, W, N] uint8 `stack` in chunks (ch, cw, cn) written in `order` ("C" / "F").  The distinct chunks lie in first-use
    order (batch row, then ty, then tx) at multiples of chunk_nbytes rounded up to `align` (the feed's 256; 16 is the least the
    kernel takes); a chunk in `skip` (coordinates (ty, tx, tk)) is absent: -1 in tile_off and no room in the buffer.  Every byte
    that belongs to no pixel of the array -- the part of an edge chunk beyond the array, the gap between two chunks -- holds
    `poison`.  pad_end=False ends the buffer with the last chunk's last byte instead of at the next multiple of `align`."""
    stack = np.asarray(stack)
    assert stack.dtype == np.uint8 and stack.ndim == 3 and order in ("C", "F") and align % 16 == 0
    ch, cw, cn = (int(c) for c in chunks)
    gh, gw, _ = _grid(stack.shape, (ch, cw, cn))
    nbytes = ch * cw * cn
    stride = -(-nbytes // align) * align
    absent = {tuple(int(v) for v in s) for s in skip}
    idxs = [int(i) for i in idxs]
    tile_off = np.full((len(idxs), gh, gw), -1, dtype=np.int64)
    tile_k = np.zeros(len(idxs), dtype=np.int32)
    placed = {}
    for b, idx in enumerate(idxs):
        assert 0 <= idx < stack.shape[2]
        tk, tile_k[b] = idx // cn, idx % cn
        for ty in range(gh):
            for tx in range(gw):
                if (ty, tx, tk) in absent:
                    continue
                tile_off[b, ty, tx] = placed.setdefault((ty, tx, tk), len(placed) * stride)
    total = len(placed) * stride if pad_end else (len(placed) - 1) * stride + nbytes
    staged = np.full(max(total, align if pad_end else 1), poison, dtype=np.uint8)
    for (ty, tx, tk), off in placed.items():
        block = np.full((ch, cw, cn), poison, dtype=np.uint8)
        part = stack[ty * ch:(ty + 1) * ch, tx * cw:(tx + 1) * cw, tk * cn:(tk + 1) * cn]
        block[:part.shape[0], :part.shape[1], :part.shape[2]] = part
        staged[off:off + nbytes] = np.frombuffer(block.tobytes(order=order), dtype=np.uint8)
    return staged, tile_off, tile_k


def expect(stack, idxs, top, left, OH, OW, skip, chunks, fill):
    """-> uint8 [B, 1, OH, OW]: out[b, 0] = stack[top:top + OH, left:left + OW, idxs[b]], the chunks in `skip` reading as `fill`"""
    stack = np.asarray(stack)
    ch, cw, cn = (int(c) for c in chunks)
    want = stack.copy() if len(skip) else stack
    for ty, tx, tk in skip:
        want[ty * ch:(ty + 1) * ch, tx * cw:(tx + 1) * cw, tk * cn:(tk + 1) * cn] = fill
    rows = want[top:top + OH, left:left + OW, [int(i) for i in idxs]]
    assert rows.shape == (OH, OW, len(idxs)), "the crop does not lie inside the frame"
    return np.ascontiguousarray(rows.transpose(2, 0, 1)[:, None])
