"""tests/_png_write.py against PIL at 1 and 3 bytes per pixel: every file the helper writes -- grey and RGB, each filter type, mixed filters, several
IDAT chunks -- is read back by ``read_image`` to the source pixels.  This validates the helper, not the decoder."""
import numpy as np
import pytest
import torch

from _png_write import filter_rows, png_bytes, unfilter_rows
from yogo_amd.yogo_dataset import read_image


@pytest.mark.parametrize("hw", [(1, 1), (3, 2), (17, 23), (65, 5)])
@pytest.mark.parametrize("rgb", [False, True])
def test_files_read_back_to_the_source_pixels(tmp_path, hw, rgb):
    rng = np.random.default_rng(hw[0] * 100 + hw[1] + rgb)
    H, W = hw
    img = rng.integers(0, 256, size=(H, W, 3) if rgb else (H, W), dtype=np.uint8)
    cases = [[t] * H for t in range(5)] + [list(rng.integers(0, 5, size=H))]
    for k, types in enumerate(cases):
        p = tmp_path / f"f{k}.png"
        p.write_bytes(png_bytes(img, types, idat_sizes=[7, 11] if k == 5 else None))
        got = read_image(p, rgb=rgb)
        want = torch.from_numpy(img).permute(2, 0, 1) if rgb else torch.from_numpy(img)[None]
        assert torch.equal(got, want), (hw, rgb, types[:4])


def test_one_byte_per_pixel_is_what_unfilter_rows_reverses_and_a_channel_of_three():
    """one writer now serves both pixel sizes: at one byte per pixel it is held to `unfilter_rows` (the filters' reverse, written
    pixel by pixel), and a channel of a 3-byte pixel is filtered as the grey image of that channel is"""
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, size=(9, 13), dtype=np.uint8)
    types = list(rng.integers(0, 5, size=9))
    scan = filter_rows(img, types)
    assert scan.shape == (9, 14) and list(scan[:, 0]) == types
    assert np.array_equal(unfilter_rows(scan), img)
    rgb = rng.integers(0, 256, size=(9, 13, 3), dtype=np.uint8)
    scan3 = filter_rows(rgb, types)
    for c in range(3):
        assert np.array_equal(scan3[:, 1 + c::3], filter_rows(rgb[..., c], types)[:, 1:])
