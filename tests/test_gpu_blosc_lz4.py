"""The device decoder of Blosc blocks (yogo_amd/csrc/blosc_lz4.hip) against the pure-Python decoder of the same format
(yogo_amd.blosc.lz4_block_decode), byte for byte, with canary bytes around every destination range: the liblz4 fixtures, built
sequences at every edge of the encoding, and the launch geometry.  Every case first proves on the host that its bytes hold the
sequences it is named after."""
import os

import numpy as np
import pytest

import _blosc_write as BW
from yogo_amd import blosc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lz4_blocks.npz")
SEED = b"The quick brown fox!"      # 20 literals of history in front of a built sequence


def _rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _check(blocks):
    """blocks: [(name, stored bytes, dst_len, raw)] -> one launch; every entry equals the Python decoder's bytes"""
    want = [bytes(b) if raw else blosc.lz4_block_decode(b, n) for _, b, n, raw in blocks]
    status, got, canaries = BW.decode_on_device([(b, n, raw) for _, b, n, raw in blocks])
    assert canaries, "a byte outside the destination ranges was written"
    for (name, _, _, _), s, g, w in zip(blocks, status, got, want):
        assert s == 0, (name, s)
        assert g == w, name


def _built(name, seqs, expect):
    """a block of exactly `seqs`; `expect` (literal length, offset, match length) must be one of its sequences as parsed back"""
    block = BW.lz4_build(seqs)
    assert expect in BW.lz4_sequences(block), (name, expect)
    data = BW.lz4_expand(seqs)
    assert blosc.lz4_block_decode(block, len(data)) == data, name
    return (name, block, len(data), False)


def test_golden_blocks():
    z = np.load(GOLDEN)
    blocks = []
    for n in ("zeros", "period3", "low_entropy", "incompressible", "far_match"):
        blocks.append((n, z[n + "_c"].tobytes(), int(z[n + "_d"].size), False))
        assert blosc.lz4_block_decode(blocks[-1][1], blocks[-1][2]) == z[n + "_d"].tobytes()
    assert max(o or 0 for _, o, _ in BW.lz4_sequences(blocks[-1][1])) > 65000
    _check(blocks)


def test_length_encodings():
    blocks = []
    for L in (0, 14, 15, 15 + 254, 15 + 255, 15 + 255 + 255 + 3):
        lits = _rand(L, L)
        b = _built(f"literals-{L}", [(SEED, 7, 9), (lits, 5, 6), (b"end", None, None)], (L, 5, 6))
        if L >= 15:   # the extension bytes themselves: 255s, then the remainder (15 + 255 is 255 followed by 0)
            ext = bytes([255] * ((L - 15) // 255) + [(L - 15) % 255])
            assert BW.lz4_sequence(lits, 5, 6)[1:1 + len(ext)] == ext and BW.lz4_sequence(lits, 5, 6)[0] >> 4 == 15
        blocks.append(b)
    for M in (4, 18, 19, 19 + 255, 19 + 510):
        b = _built(f"match-{M}", [(SEED, 7, M), (b"end", None, None)], (20, 7, M))
        if M >= 19:
            ext = bytes([255] * ((M - 19) // 255) + [(M - 19) % 255])
            assert b[1].startswith(bytes([0xFF, 5]) + SEED + b"\x07\x00" + ext)
        blocks.append(b)
    blocks.append(_built("one-literal-run", [(_rand(1000, 1), None, None)], (1000, None, None)))
    blocks.append(_built("last-sequence-without-literals", [(SEED, 7, 9), (b"", None, None)], (0, None, None)))
    assert blocks[-1][1][-1] == 0
    _check(blocks)


@pytest.mark.parametrize("offset", [1, 2, 3, 63, 64, 65, 4096, 65535])
def test_match_offsets(offset):
    """a match shorter than, as long as, and several times longer than its offset (a match cannot be shorter than 4); more than
    64 bytes at an offset under 64 make the wave wrap around the period"""
    blocks = []
    history = _rand(max(offset, 4), offset)
    for kind, M in (("shorter", offset // 2), ("equal", offset), ("longer", 3 * offset + 5), ("wraps", 3 * offset + 200)):
        if M < 4 or (kind == "wraps" and offset > 65):
            continue
        blocks.append(_built(f"offset-{offset}-{kind}", [(history, offset, M), (b"xy", offset, 4), (b"end", None, None)],
                             (len(history), offset, M)))
    assert len(blocks) >= 2
    _check(blocks)


def test_geometry():
    """dst_len 1 .. 131 072 as LZ4 and as raw entries, at destinations of every alignment (decode_on_device packs them so)"""
    blocks = []
    for n in (1, 63, 64, 65, 100, 131072):
        data = (np.random.default_rng(n).integers(0, 3, n, dtype=np.uint8) * 90).tobytes()
        comp = BW.lz4_compress(data)
        if n >= 63:
            assert len(comp) < n and any(o is not None for _, o, _ in BW.lz4_sequences(comp)), n
        blocks.append((f"lz4-{n}", comp, n, False))
        blocks.append((f"raw-{n}", _rand(n, n + 1), n, True))
        blocks.append((f"raw-again-{n}", _rand(n, n + 2), n, True))    # (a second alignment of the same length)
    _check(blocks)


def test_300_entries_in_one_launch():
    blocks = []
    for i in range(300):
        data = (bytes([i % 256, i >> 8, (7 * i) % 256, 255 - i % 256, 3]) * 30)[:50 + i % 40]
        if i % 3 == 0:
            blocks.append((f"raw-{i}", data, len(data), True))
        else:
            comp = BW.lz4_compress(data)
            assert any(o == 5 for _, o, _ in BW.lz4_sequences(comp)), i
            blocks.append((f"lz4-{i}", comp, len(data), False))
    _check(blocks)


def test_entry_point_refuses_bad_arguments():
    import torch

    from yogo_amd.device_decode import decode_blocks

    src = torch.zeros(64, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(80, dtype=torch.uint8, device="cuda")
    table = torch.tensor([[0, 4, 0, 4, 1]], dtype=torch.int64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    decode_blocks(src, table, dst, status)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        decode_blocks(src, table, dst[8:], status)
    with pytest.raises(RuntimeError, match="overlap"):
        decode_blocks(dst[:48], table, dst, status)
    with pytest.raises(ValueError, match="table"):
        decode_blocks(src, table.to(torch.int32), dst, status)
    with pytest.raises(RuntimeError, match="host tensor|MI355X"):
        decode_blocks(src.cpu(), table, dst, status)
