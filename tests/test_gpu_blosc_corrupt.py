"""Malformed LZ4 blocks through the device decoder (yogo_amd/csrc/blosc_lz4.hip): each is a valid block with exactly one defect and
must end in the status code the Python decoder names for it, with every byte outside the destination ranges untouched and the
other entries of the launch decoded.  These are inputs a store can hold, and every one goes through the Python decoder first,
where an access out of range would be an exception.  A file of its own, so that it can run as a step after
tests/test_gpu_blosc_lz4.py."""
import numpy as np
import pytest

import _blosc_write as BW
from yogo_amd import blosc

pytestmark = pytest.mark.gpu
GOOD = [(b"0123456789abcdef", 16, 40), (b"XYZ", 5, 12), (b"the end..", None, None)]


@pytest.mark.parametrize("defect,code", [
    ("offset0", blosc.LZ4_BAD_OFFSET), ("offset_far", blosc.LZ4_BAD_OFFSET), ("literals", blosc.LZ4_LITERALS_PAST_SOURCE),
    ("extension", blosc.LZ4_SOURCE_ENDS_IN_SEQUENCE), ("match_past_dst", blosc.LZ4_PAST_DESTINATION), ("early", blosc.LZ4_ENDS_EARLY)])
def test_one_defect_ends_in_its_status(defect, code):
    block, dst_len = BW.corrupt_block(defect)
    want_status, produced = blosc.lz4_block_status(block, dst_len)     # the host first: every access of it is checked
    assert want_status == code and len(produced) <= dst_len
    good = BW.lz4_build(GOOD)
    good_data = BW.lz4_expand(GOOD)
    raw = np.random.default_rng(3).integers(0, 256, 300, dtype=np.uint8).tobytes()
    status, got, canaries = BW.decode_on_device([(good, len(good_data), False), (block, dst_len, False), (raw, len(raw), True),
                                                 (good, len(good_data), False)])
    assert canaries, "a byte outside the destination ranges was written"
    assert status == [0, code, 0, 0]
    assert got[0] == good_data and got[2] == raw and got[3] == good_data
    # the bad entry: what the checks let through before the failing one, and nothing behind it
    assert got[1] == bytes(produced) + bytes([BW.CANARY]) * (dst_len - len(produced))


def test_rows_outside_the_buffers_are_refused_before_any_access():
    import torch

    from yogo_amd.device_decode import decode_blocks

    src = torch.full((64,), 7, dtype=torch.uint8, device="cuda")
    dst = torch.full((96,), BW.CANARY, dtype=torch.uint8, device="cuda")
    rows = [[0, 16, 16, 16, 1],          # fine
            [60, 16, 32, 16, 1],         # the source ends after the buffer
            [0, 16, 90, 16, 1],          # the destination ends after the buffer
            [-4, 16, 48, 16, 1], [0, 16, -16, 16, 1], [0, -1, 48, 16, 0], [0, 8, 48, 16, 1],   # negative, or raw with two lengths
            [0, 16, 64, 16, 1]]          # fine
    status = torch.full((len(rows),), -1, dtype=torch.int32, device="cuda")
    decode_blocks(src, torch.tensor(rows, dtype=torch.int64, device="cuda"), dst, status)
    assert status.cpu().tolist() == [0, 6, 6, 6, 6, 6, 6, 0]
    want = np.full(96, BW.CANARY, np.uint8)
    want[16:32] = 7
    want[64:80] = 7
    assert np.array_equal(dst.cpu().numpy(), want)
