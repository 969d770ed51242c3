"""Writes tests/golden/zstd_frames.npz: Zstandard frames compressed by the system's libzstd (ZSTD_compress through ctypes) with
what they decode to, as pairs `<name>_c` / `<name>_d` of uint8 arrays, plus the library's version.  They pin the decoders
(yogo_amd/zstd.py, csrc/zstd.hip) to the real format on machines without the library.  Also the libzstd frames of a small stack of
6 frames of 48 x 64 (`stack_d`, [48, 64, 6]), once per frame (`stack_chunks_c`, back to back, their lengths in `stack_chunks_n`) and
once per 1 000-byte Blosc block of every frame (`stack_blocks_c` / `stack_blocks_n`, 4 blocks per frame): the feed tests build
stores out of them.  The script parses every frame it wrote and fails when a feature a case is there for is missing from what the
library produced.  Run it where libzstd is installed; it does nothing where it is not.

  python tests/golden/make_zstd_frames.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from yogo_amd import zstd as Z  # noqa: E402

SENTENCE = (b"It was the best of times, it was the worst of times, it was the age of wisdom, it was the age of foolishness, "
            b"it was the epoch of belief, it was the epoch of incredulity, it was.")


def noisy_frame(rng, H=48, W=64):
    y, x = np.mgrid[0:H, 0:W]
    return (120 + 60 * np.sin(x / 9.0) * np.cos(y / 7.0) + rng.normal(0, 6, (H, W))).clip(0, 255).astype(np.uint8)


def cases():
    """name -> (bytes, level, the features the library's frame must show)"""
    rng = np.random.default_rng(2024)
    return {
        "random": (rng.integers(0, 256, 6000, dtype=np.uint8).tobytes(), 1, {"raw_block"}),
        "zeros": (bytes(300000), 1, {"rle_block", "several_blocks"}),
        "text": (b"the quick brown fox jumps over the lazy dog; " * 12, 3,
                 {"raw_literals", "ll_table_predefined", "of_table_predefined", "ml_table_predefined"}),
        "four_values": (rng.integers(0, 4, 20000, dtype=np.uint8).tobytes(), 1, {"huffman_4_streams", "huffman_direct_weights"}),
        "noisy_frame": (noisy_frame(rng).tobytes(), 1, {"huffman_4_streams", "huffman_fse_weights", "zero_sequences"}),
        "sentence": (SENTENCE, 3, {"huffman_1_stream"}),
        "two_values": ((rng.random(300000) < 0.1).astype(np.uint8).tobytes(), 9,
                       {"several_blocks", "treeless_literals", "ll_table_fse", "of_table_fse", "ml_table_fse", "a_table_repeat",
                        "match_into_earlier_block"}),
    }


def stack():
    rng = np.random.default_rng(7)
    return np.stack([noisy_frame(rng) for _ in range(6)], axis=2)


def main() -> int:
    L = Z.libzstd()
    if L is None:
        print("libzstd is not installed here: nothing written")
        return 0
    version = L.ZSTD_versionString()
    out = {}
    for key, (data, level, must) in cases().items():
        comp = Z.lib_compress(data, level)
        assert Z.lib_decode(comp, len(data)) == data, key
        seen = set()
        status, back = Z.zstd_frame_status(comp, len(data), seen)
        assert status == 0 and back == data, (key, status)
        if any(f.endswith("_table_repeat") for f in seen):
            seen.add("a_table_repeat")
        assert must <= seen, f"{key}: libzstd {version.decode()} did not produce {sorted(must - seen)}"
        out[key + "_c"] = np.frombuffer(comp, dtype=np.uint8)
        out[key + "_d"] = np.frombuffer(data, dtype=np.uint8)
        print(f"{key}: {len(data)} -> {len(comp)} bytes at level {level}: {', '.join(sorted(seen))}")
    s = stack()
    chunks, blocks = [], []
    for i in range(s.shape[2]):
        raw = s[:, :, i].tobytes()
        chunks.append(Z.lib_compress(raw, 1))
        blocks += [Z.lib_compress(raw[at:at + 1000], 1) for at in range(0, len(raw), 1000)]
    out["stack_d"] = s
    for name, frames in (("stack_chunks", chunks), ("stack_blocks", blocks)):
        out[name + "_c"] = np.frombuffer(b"".join(frames), dtype=np.uint8)
        out[name + "_n"] = np.asarray([len(f) for f in frames], dtype=np.int64)
    out["libzstd_version"] = np.frombuffer(version, dtype=np.uint8)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "zstd_frames.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes) with libzstd {version.decode()}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
