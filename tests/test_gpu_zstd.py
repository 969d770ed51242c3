"""yogo_zstd_decode (csrc/zstd.hip) against the frames libzstd wrote (tests/golden/zstd_frames.npz), the hand-written frames of
tests/_zstd_write.py and the pure-Python twin (yogo_amd/zstd.py): bytes, statuses and every byte outside the rows' ranges."""
import numpy as np
import pytest
import torch

import _zstd_write as W
from yogo_amd import zstd as Z

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def frames():
    out = dict(W.golden_frames())
    out.update(W.hand_written())
    return out


def test_every_frame_decodes_bit_for_bit_and_nothing_else_is_touched(frames):
    rng = np.random.default_rng(3)
    names = list(frames)
    entries = [(frames[n][0], len(frames[n][1]), False) for n in names]
    raws = [rng.integers(0, 256, size, dtype=np.uint8).tobytes() for size in (1, 15, 255, 256, 4097, 70001)]
    entries += [(r, len(r), True) for r in raws]
    status, got, clean, work_clean = W.decode_on_device(entries)
    assert status == [0] * len(entries), dict(zip(names + ["raw"] * len(raws), status))
    for name, g in zip(names, got):
        assert g == frames[name][1], name
    assert got[len(names):] == raws
    assert clean and work_clean


def test_no_rows_is_no_launch():
    from yogo_amd.device_decode import zstd_frames

    dst = torch.zeros(64, dtype=torch.uint8, device="cuda")
    zstd_frames(torch.zeros(64, dtype=torch.uint8, device="cuda"), torch.zeros((0, 5), dtype=torch.int64, device="cuda"), dst,
                torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(64, dtype=torch.uint8, device="cuda"))
    assert not bool(dst.any())


def test_a_thousand_rows_in_one_launch(frames):
    small = ["sentence", "text", "rle_literals", "repeat_ll0", "huffman_11_bits"]
    entries = [(frames[small[i % 5]][0], len(frames[small[i % 5]][1]), False) for i in range(1000)]
    status, got, clean, work_clean = W.decode_on_device(entries)
    assert status == [0] * 1000 and clean and work_clean
    assert all(g == frames[small[i % 5]][1] for i, g in enumerate(got))


def test_each_defect_gets_the_status_of_the_python_decoder():
    """the enumerated defects only, each answered with a status by the pure-Python decoder first; plus rows outside the buffers"""
    cases = [W.corrupt_frame(d) for d in W.DEFECTS]
    want = []
    for f, n, code, _ in cases:
        st, _ = Z.zstd_frame_status(f, n)
        assert st == code != 0
        want.append(st)
    entries = [(f, n, False) for f, n, _, _ in cases]
    good = W.corrupt_frame("trailing")[0][:-1]
    extra = [(-1, 10, 0, 10, 0), ("src", 1, 0, 10, 0), (0, 10, "dst", 1, 0), (0, 10, -16, 10, 1), (0, 1 << 40, 0, 10, 0), (0, 10, 0, 1 << 40, 0),
             (0, 10, 0, 11, 1)]
    entries.append((good, 80, False))
    status, got, clean, work_clean = W.decode_on_device(entries, extra)
    assert status[:len(cases)] == want, list(zip(W.DEFECTS, status, want))
    assert status[len(cases)] == 0 and got[len(cases)] == W.corrupt_frame("trailing")[3]
    assert status[len(cases) + 1:] == [Z.ZSTD_BAD_ROW] * len(extra)
    for d, (f, n, _, truth), g in zip(W.DEFECTS, cases, got):   # a refused row wrote what the twin produced, a prefix of the truth, and no more
        out = Z.zstd_frame_status(f, n)[1]
        assert truth.startswith(out) or not truth, d
        assert g[:len(out)] == out and g[len(out):] == bytes([W.CANARY]) * (len(g) - len(out)), d
    assert clean and work_clean
