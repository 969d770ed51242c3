"""Host side of the device resize (`yogo train ... --device-image-resize`; yogo_amd/resize.py): the tap tables against the fp64
oracle's matrices, the numpy twin of the kernel and ``resize_image`` itself under the rules of tests/_resize_ref.py, and the flag's
plumbing.  No GPU."""
import numpy as np
import pytest
import torch

import _resize_ref as R

# source -> destination: an exact 2 x, an identity axis beside a 2 x one, non-dyadic down-scales (2.4 x: 5 taps; 3.9 x: 8 taps),
# up-scales, up in y and down in x
SHAPES = [((64, 96), (32, 48)), ((40, 56), (40, 28)), ((97, 131), (40, 56)), ((97, 131), (25, 33)), ((50, 70), (64, 96)),
          ((33, 47), (97, 131)), ((61, 131), (64, 56))]
IDS = [f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in SHAPES]


def _dense(start, weights, n_in):
    W = np.zeros((len(start), n_in), dtype=np.float64)
    for i, s in enumerate(start):
        for j, w in enumerate(weights[i]):
            if w != 0:
                assert s + j < n_in
                W[i, s + j] += float(w)
    return W


@pytest.mark.parametrize("n_in,n_out,K", [(64, 32, 4), (96, 48, 4), (56, 56, 2), (97, 40, 5), (131, 56, 5), (97, 25, 8), (131, 33, 8),
                                          (50, 64, 2), (47, 131, 2), (772, 386, 4), (1032, 129, 16), (1031, 129, 16), (7, 1, 7), (1, 5, 1)])
def test_taps_against_the_oracle_matrix(n_in, n_out, K):
    """K: the longest run hi - lo of the axis, between 2 * support - 1 and 2 * support + 1"""
    from yogo_amd.resize import aa_taps

    start, weights = aa_taps(n_in, n_out)
    assert start.dtype == np.int32 and start.shape == (n_out,) and weights.dtype == np.float32 and weights.shape == (n_out, K)
    assert K <= min(n_in, int(2 * max(n_in / n_out, 1.0)) + 1)
    assert (start >= 0).all() and (start < n_in).all() and (np.diff(start) >= 0).all() and (weights >= 0).all()
    want = R.aa_matrix(n_in, n_out)
    # fp64 taps rounded to fp32: half an ulp of a weight <= 1
    assert np.abs(_dense(start, weights, n_in) - want).max() <= 2.0 ** -25
    assert aa_taps(n_in, n_out)[0] is start   # cached per size pair


def test_what_the_device_serves():
    from yogo_amd.resize import MAX_TAPS, aa_taps, device_serves

    assert device_serves(772, 386) and device_serves(800, 100) and device_serves(3, 1000) and not device_serves(801, 100)
    assert all(aa_taps(n_in, n_out)[1].shape[1] <= MAX_TAPS for n_in, n_out in ((800, 100), (1032, 129), (65535, 8192), (799, 100), (17, 3)))


@pytest.mark.parametrize("src,dst", SHAPES, ids=IDS)
@pytest.mark.parametrize("C", [1, 3])
def test_numpy_twin_under_rules_d_and_e(src, dst, C):
    from yogo_amd.resize import resize_aa_host

    img = R.images(3, C, *src, seed=src[0] * 1000 + dst[1])
    v = R.exact(img, dst)
    R.assert_cap(v)
    got = resize_aa_host(img, dst)
    assert got.dtype == np.uint8 and got.shape == v.shape
    R.assert_rule(got, v, R.TOL_FP32, "twin")
    if (src, dst) == SHAPES[0]:
        R.assert_exact_interior(got[0], v[0], 10, what="twin, noise image")
        R.assert_exact_interior(got, v, 10, what="twin, all images")
    if (src, dst) == SHAPES[1]:   # the identity axis is exact: only the first and last column are not
        assert np.array_equal(R.aa_matrix(40, 40), np.eye(40))
        R.assert_exact_interior(got, v, 10, rows=False, what="twin, identity rows")


@pytest.mark.parametrize("src,dst", SHAPES, ids=IDS)
def test_resize_image_under_rule_h(src, dst):
    """``resize_image`` (torch's CPU kernel) against the oracle: its weights are fp32 and its code depends on the CPU's feature level.
    Measured on the development machine: over these shapes and images it deviates from the fp64 definition by up to 1.18e-3 before
    rounding (1.24e-3 over a wider set) and flips 0 .. 6 pixels per image by one level, all at rounding edges; rule H's 2e-3 is the
    wider figure with a margin of 1.6."""
    from yogo_amd.yogo_dataset import resize_image

    img = R.images(2, 3, *src, seed=src[1] * 1000 + dst[0])
    v = R.exact(img, dst)
    got = np.stack([resize_image(torch.from_numpy(im), dst).numpy() for im in img])
    R.assert_rule(got, v, R.TOL_TORCH, "resize_image")


def test_the_flag_needs_device_decode(capsys, tmp_path):
    from yogo_amd.image_cache import ImageCache
    from yogo_amd.trainer import build_config
    from yogo_amd.utils.argparsers import global_parser, train_parser
    from yogo_amd.yogo_dataloader import get_dataloader

    on = ["--device-image-cache", "2", "--device-image-decode", "--device-image-resize"]
    args = global_parser().parse_args(["train", "defn.yml"] + on)
    assert args.device_image_resize is True and build_config(args)["device_image_resize"] is True
    args = global_parser().parse_args(["train", "defn.yml"] + on[:3])
    assert args.device_image_resize is False and build_config(args)["device_image_resize"] is False
    assert train_parser().parse_args(["defn.yml"] + on).device_image_resize is True
    for parse in (lambda a: global_parser().parse_args(["train"] + a), lambda a: train_parser().parse_args(a)):
        with pytest.raises(SystemExit) as e:
            parse(["defn.yml", "--device-image-cache", "2", "--device-image-resize"])
        assert e.value.code == 2
        assert "error: --device-image-resize resizes what the device decoded: it needs --device-image-decode" in capsys.readouterr().err
    with pytest.raises(ValueError, match="--device-image-resize .* needs --device-image-decode"):
        get_dataloader(None, 4, 12, 8, device_image_cache_gib=1.0, device_image_resize=True)
    with pytest.raises(ValueError, match="--device-image-resize .* needs --device-image-decode"):
        ImageCache([0, 1], 2, (1, 8, 8), False, device_resize=True)
