"""``yogo_resize_aa_u8`` (csrc/resize_aa.hip) through ``device_decode.resize_aa`` on the MI355X, against the fp64 oracle of
tests/_resize_ref.py under its rules D and E, and bit for bit against the kernel's numpy twin (yogo_amd/resize.py: the same taps, the
same order of the same fp32 operations).  Every case: C = 1 and C = 3, three images (noise, smooth plus noise, noise) scattered to
slots 5, 0 and 3 of a destination of 7 whose other slots hold 0x5A and must keep it.

The shapes, source -> destination: an exact 2 x (rule E), an identity axis beside a 2 x one, non-dyadic down-scales (2.4 x and 3.9 x:
5 and 8 taps), up-scales, up in y and down in x; 33 x 47 -> 97 x 131 has an odd width and no whole number of tiles in either axis
(tiles are 32 x 64); 68 x 300 -> 33 x 151 walks several column tiles from a word-aligned source whose tiles start between words, into
an odd width; 40 x 272 -> 20 x 136 does so with word stores and a last tile of 8 columns."""
import numpy as np
import pytest
import torch

import _resize_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SLOTS, N_DST, FILL = [5, 0, 3], 7, 0x5A
SHAPES = [((64, 96), (32, 48)), ((40, 56), (40, 28)), ((97, 131), (40, 56)), ((97, 131), (25, 33)), ((50, 70), (64, 96)),
          ((33, 47), (97, 131)), ((61, 131), (64, 56)), ((68, 300), (33, 151)), ((40, 272), (20, 136))]
IDS = [f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in SHAPES]


def _resize(img: np.ndarray, dst_hw, slots=SLOTS, n_dst=N_DST):
    from yogo_amd.device_decode import resize_aa
    from yogo_amd.resize import aa_taps

    src = torch.from_numpy(img).to(DEV)
    dst = torch.full((n_dst, img.shape[1], *dst_hw), FILL, dtype=torch.uint8, device=DEV)
    resize_aa(src, dst, slots, aa_taps(img.shape[2], dst_hw[0]), aa_taps(img.shape[3], dst_hw[1]))
    torch.cuda.synchronize()
    return dst.cpu().numpy()


@pytest.mark.parametrize("src,dst", SHAPES, ids=IDS)
@pytest.mark.parametrize("C", [1, 3])
def test_kernel_under_rules_d_and_e(src, dst, C):
    from yogo_amd.resize import resize_aa_host

    img = R.images(3, C, *src, seed=src[0] * 1000 + dst[1])
    v = R.exact(img, dst)
    R.assert_cap(v)
    out = _resize(img, dst)
    rest = [s for s in range(N_DST) if s not in SLOTS]
    assert (out[rest] == FILL).all()
    got = out[SLOTS]
    R.assert_rule(got, v, R.TOL_FP32, "kernel")
    if (src, dst) == SHAPES[0]:
        R.assert_exact_interior(got[0], v[0], 10, what="kernel, noise image")
        R.assert_exact_interior(got, v, 10, what="kernel, all images")
    if (src, dst) == SHAPES[1]:   # the identity axis is exact: only the first and last column are not
        R.assert_exact_interior(got, v, 10, rows=False, what="kernel, identity rows")
    twin = resize_aa_host(img, dst)
    print(f"kernel against its numpy twin: {int((got != twin).sum())} of {got.size} pixels differ")
    assert np.array_equal(got, twin)


def test_destination_view_with_an_odd_offset():
    """the destination a view that starts at an odd byte (a slice of the cache): byte stores, the bytes around it untouched"""
    from yogo_amd.device_decode import resize_aa
    from yogo_amd.resize import aa_taps, resize_aa_host

    img = R.images(2, 1, 30, 44, seed=9)
    flat = torch.full((1 + 3 * 15 * 20 + 5,), FILL, dtype=torch.uint8, device=DEV)
    dst = flat[1:1 + 3 * 15 * 20].view(3, 1, 15, 20)
    resize_aa(torch.from_numpy(img).to(DEV), dst, [2, 0], aa_taps(30, 15), aa_taps(44, 20))
    torch.cuda.synchronize()
    got = flat.cpu().numpy()
    want = np.full_like(got, FILL)
    twin = resize_aa_host(img, (15, 20))
    want[1 + 2 * 300:1 + 3 * 300], want[1:1 + 300] = twin[0].reshape(-1), twin[1].reshape(-1)
    assert np.array_equal(got, want)


def test_refusals_come_back_as_errors_without_a_launch():
    from yogo_amd import _hip
    from yogo_amd.device_decode import resize_aa
    from yogo_amd.resize import aa_taps

    src = torch.zeros((2, 1, 90, 40), dtype=torch.uint8, device=DEV)
    dst = torch.full((3, 1, 10, 20), FILL, dtype=torch.uint8, device=DEV)
    ok_y, ok_x = aa_taps(40, 10), aa_taps(40, 20)
    half = src[:, :, :40].contiguous()
    _hip.launch_log(True)
    try:
        with pytest.raises(RuntimeError, match="scales down by more than 8"):
            resize_aa(src, dst, [0, 1], aa_taps(90, 10), ok_x)
        with pytest.raises(RuntimeError, match="outside the 3 destination images"):
            resize_aa(half, dst, [0, 3], ok_y, ok_x)
        with pytest.raises(RuntimeError, match="outside the 3 destination images"):
            resize_aa(half, dst, [-1, 2], ok_y, ok_x)
        with pytest.raises(RuntimeError, match="same destination"):
            resize_aa(half, dst, [1, 1], ok_y, ok_x)
        with pytest.raises(ValueError, match="the y taps"):
            resize_aa(half, dst, [0, 1], aa_taps(40, 11), ok_x)                 # a table of the wrong length
        with pytest.raises(ValueError, match="destination slots"):
            resize_aa(half, dst, [0], ok_y, ok_x)
        with pytest.raises(RuntimeError, match="the vertical table: "):
            resize_aa(half, dst, [0, 1], aa_taps(48, 10), ok_x)                 # a table made for a taller source
        start, weights = (a.copy() for a in ok_x)
        start[7] = 40
        with pytest.raises(RuntimeError, match="horizontal table: a start index"):
            resize_aa(half, dst, [0, 1], ok_y, (start, weights))
        start, weights = (a.copy() for a in ok_x)
        weights[3, 0] = np.float32("nan")
        with pytest.raises(RuntimeError, match="horizontal table: a weight is outside"):
            resize_aa(half, dst, [0, 1], ok_y, (start, weights))
        torch.cuda.synchronize()
        assert _hip.read_launch_log() == []
    finally:
        _hip.launch_log(False)
    assert (dst.cpu().numpy() == FILL).all()
