"""Writes tests/golden/lz4_blocks.npz: LZ4 blocks compressed by the system's liblz4 (LZ4_compress_default through ctypes) with
what they decode to, as pairs `<name>_c` / `<name>_d` of uint8 arrays.  They pin the decoders (yogo_amd/blosc.py,
csrc/blosc_lz4.hip) to the real format on machines without the library.  Run it where liblz4 is installed; it does nothing
where it is not.

  python tests/golden/make_lz4_blocks.py
"""
import ctypes
import ctypes.util
import os
import sys

import numpy as np


def cases():
    rng = np.random.default_rng(2017)
    head = rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
    return {
        "zeros": bytes(4096),
        "period3": (b"abc" * 400)[:1000],
        "low_entropy": rng.integers(0, 4, 4096, dtype=np.uint8).tobytes(),
        "incompressible": rng.integers(0, 256, 2048, dtype=np.uint8).tobytes(),
        # the second `head` is a match at distance 300 + 64 900 = 65 200 (the format's limit is 65 535)
        "far_match": head + bytes(64900) + head + bytes(range(40)),
    }


def main() -> int:
    name = ctypes.util.find_library("lz4")
    if not name:
        print("liblz4 is not installed here: nothing written")
        return 0
    L = ctypes.CDLL(name)
    L.LZ4_versionString.restype = ctypes.c_char_p
    out = {}
    for key, data in cases().items():
        cap = L.LZ4_compressBound(len(data))
        buf = ctypes.create_string_buffer(cap)
        n = L.LZ4_compress_default(data, buf, len(data), cap)
        assert n > 0, key
        back = ctypes.create_string_buffer(len(data))
        assert L.LZ4_decompress_safe(buf.raw[:n], back, n, len(data)) == len(data) and back.raw == data, key
        out[key + "_c"] = np.frombuffer(buf.raw[:n], dtype=np.uint8)
        out[key + "_d"] = np.frombuffer(data, dtype=np.uint8)
        print(f"{key}: {len(data)} -> {n} bytes")
    out["liblz4_version"] = np.frombuffer(L.LZ4_versionString(), dtype=np.uint8)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lz4_blocks.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes) with liblz4 {L.LZ4_versionString().decode()}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
