"""The float32 bit patterns that tests/test_float_text_host.py (host build of float_text.h) and tests/test_gpu_pred_text.py (the device
kernels) both print, and the reference: Python's own ``repr`` of the widened value."""
import numpy as np

# the mantissa fields at which something changes: the asymmetric interval (0), its neighbours, the middle, the top
MANTISSAS = (0, 1, 2, 0x3FFFFF, 0x400000, 0x400001, 0x7FFFFE, 0x7FFFFF)


def structured_bits() -> np.ndarray:
    """every exponent field x MANTISSAS x both signs; the float32 nearest to 10^k (k = -45 .. 38) and its two neighbours; zeros,
    infinities, NaNs of both signs with several payloads, the smallest and the largest subnormal"""
    grid = [(s << 31) | (e << 23) | m for e in range(256) for m in MANTISSAS for s in (0, 1)]
    with np.errstate(over="ignore", under="ignore"):   # 10^-45 rounds to the smallest subnormal, nothing overflows below 3.4e38
        near = np.array([float(f"1e{k}") for k in range(-45, 39)], dtype=np.float64).astype(np.float32).view(np.uint32).astype(np.int64)
    pow10 = np.concatenate([near - 1, near, near + 1])
    pow10 = pow10[(pow10 >= 0) & (pow10 < 0x7F800000)]
    special = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF,
               0x7FA5A5A5, 0xFFD00001, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF]
    return np.concatenate([np.array(grid, dtype=np.uint32), pow10.astype(np.uint32), (pow10 | 0x80000000).astype(np.uint32),
                           np.array(special, dtype=np.uint32)])


def python_reprs(bits: np.ndarray):
    with np.errstate(invalid="ignore"):   # (widening a signalling NaN)
        return [repr(v) for v in bits.view(np.float32).astype(np.float64).tolist()]
