"""The exact-integer instrument of the bf16 convolution engine on the host (tests/_conv_bf16_exact.py): for every case of the GPU file the
preconditions hold, the reference agrees with F.conv2d and autograd in float64, and the comparison has teeth -- each planted defect, applied to
a copy of the reference output, is reported as a mismatch."""
import pytest
import torch
import torch.nn.functional as F

import _conv_bf16_exact as X
from test_gpu_conv_bf16_exact import CASES, PAIR_CASES, _id

f64 = torch.float64
_REFS = {}


def _ref(case):
    if case not in _REFS:
        _REFS[case] = X.Ref(case) if len(case) == 7 else X.PairRef(case)
    return _REFS[case]


@pytest.mark.parametrize("case", CASES + PAIR_CASES, ids=_id)
def test_preconditions_hold_and_reference_agrees_with_autograd(case):
    ref = _ref(case)
    ref.check_preconditions()
    if len(case) == 5:
        B, C1, C2, IH, IW = case
        y1 = F.leaky_relu(F.conv2d(ref.x, ref.w1, ref.b1, padding=1), 0.01) * ref.s1[:, :, None, None]
        # one bf16 rounding and the float32 slope: 2^-8 relative (+ the slope's own 2^-24)
        assert bool(((ref.y1.double() - y1).abs() <= 2.0 ** -8 * y1.abs() * (1 + 1e-6)).all())
        y2 = F.leaky_relu(F.conv2d(ref.y1.double(), ref.w2, ref.b2, stride=2, padding=1), 0.01) * ref.s2[:, :, None, None]
        assert bool(((ref.y2.double() - y2).abs() <= 2.0 ** -8 * y2.abs() * (1 + 1e-6)).all())
        assert tuple(ref.y2.shape) == (B, C2, ref.OH, ref.OW)
        return
    B, Cin, Cout, IH, IW, k, s = case
    x = ref.x.clone().requires_grad_(True)
    w = ref.w.clone().requires_grad_(True)
    b = ref.bias.clone().requires_grad_(True)
    y = F.conv2d(x, w, b, stride=s, padding=1 if k == 3 else 0)
    assert torch.equal(y.detach(), ref.y)
    y.backward(ref.dy)
    assert torch.equal(x.grad, ref.g) and torch.equal(w.grad, ref.dw) and torch.equal(b.grad, ref.db)
    # the stored values: integers (and -0.01 n within the float32 slope's and one bf16 rounding) of the float64 activation
    want = F.leaky_relu(ref.y, 0.01) * ref.so[:, :, None, None]
    got = ref.stored().double()
    assert torch.equal(got[want >= 0], want[want >= 0])
    assert bool(((got - want).abs() <= 2.0 ** -8 * want.abs() * (1 + 1e-6)).all())
    wantd = ref.g * torch.where(ref.refy > 0, 1.0, 0.01) * ref.si[:, :, None, None]
    assert bool(((ref.dx(True, True).double() - wantd).abs() <= 2.0 ** -8 * wantd.abs() * (1 + 1e-6)).all())
    # the sign map: every bit of an existing channel is (stored > 0), decoded bit by bit
    st = ref.stored()
    sg = X.sign_map(st).reshape(B, 2, ref.OH, ref.OW, -1).long()
    for ch in range(0, Cout, 3):
        q, e, h, i = ch // 16, (ch % 16) // 8, (ch % 8) // 4, ch % 4
        assert torch.equal(((sg[:, h, :, :, q] >> (i + 4 * e)) & 1).bool(), st[:, ch] > 0), ch
    assert sg.numel() == B * ref.OH * ref.OW * (X.cpad_of(Cout) // 8)


def test_densities_keep_the_sums_small():
    """the figures the issue states for this density: outputs of a few tens, ~5 % zeros, about half negative"""
    for case in ((2, 16, 32, 20, 37, 3, 1), (1, 128, 128, 25, 33, 3, 1), (1, 128, 128, 25, 33, 3, 2), (1, 256, 128, 31, 29, 3, 2), (1, 128, 12, 7, 11, 1, 1)):
        r = _ref(case)
        ymax, zero, neg = float(r.y.abs().max()), float((r.y == 0).double().mean()), float((r.y < 0).double().mean())
        print(case, "max|y|", ymax, "zeros", zero, "negative", neg, "max|dx|", float(r.g.abs().max()), "max|dw|", float(r.dw.abs().max()), "max sum y^2", float(r.stats[:, 1].max()))
        assert 8 <= ymax <= 64 and 0.01 < zero < 0.15 and 0.35 < neg < 0.6
        assert float(r.g.abs().max()) <= 128 and float(r.dw.abs().max()) <= 256 and float(r.stats[:, 1].max()) < 1e6


# ---- the comparison has teeth ----------------------------------------------------------------------------------------------------
TEETH = (2, 32, 64, 13, 67, 3, 1)     # bands of TW = 32: column 31 is the last of the first band
TEETH_PLAN = "conv_bf16_kernel<2, 2, 4, false, 16, false, 0, true, true> | K=32 M=64 in=13x67 out=13x67 a=1 s2d=0 T=9 ncb=3 TW=32 tiles_per_band=4 CKb=2"


def _first(mask):
    return tuple(int(v) for v in mask.nonzero()[0])


def test_clean_copy_passes():
    ref = _ref(TEETH)
    X.compare_8c("clean", X.to8c(ref.stored()), ref.stored(), TEETH_PLAN)
    X.compare_signs("clean", X.sign_map(ref.stored()), ref.stored(), TEETH_PLAN)
    X.compare("clean -0.0", torch.tensor([-0.0, 1.0]), torch.tensor([0.0, 1.0]))
    with pytest.raises(AssertionError, match="1 of 2 elements differ"):
        X.compare("unwritten", torch.tensor([float("nan"), 1.0]), torch.tensor([0.0, 1.0]))


def test_one_tap_dropped_at_the_last_column_of_a_band_is_reported():
    ref = _ref(TEETH)
    B, Cin, Cout, IH, IW, k, s = TEETH
    b, h, wcol = 1, 5, 31
    # the first (channel, tap) whose product at this pixel is not zero, for an output channel with a non-zero scale
    co = int((ref.so[b] != 0).nonzero()[0])
    patch = ref.x[b, :, h - 1:h + 2, wcol - 1:wcol + 2] * ref.w[co]
    ci, i, j = _first(patch != 0)
    y = ref.y.clone()
    y[b, co, h, wcol] -= patch[ci, i, j]
    bad = X.epilogue(y, X.ACT_LEAKY, ref.so)
    with pytest.raises(AssertionError, match=r"1 of \d+ elements differ; 1 of them on a band \(TW = 32\) or image border; first at \(1, %d, 5, 31\)" % co):
        X.compare_8c("tap dropped", X.to8c(bad), ref.stored(), TEETH_PLAN)


def test_two_channels_of_a_block_swapped_at_one_pixel_is_reported():
    ref = _ref(TEETH)
    st = ref.stored()
    bad = st.clone()
    b, c, h, w = _first(st[:, 8:9] != st[:, 11:12])
    bad[b, 8, h, w], bad[b, 11, h, w] = st[b, 11, h, w], st[b, 8, h, w]
    with pytest.raises(AssertionError, match=r"2 of \d+ elements differ.*first at \(%d, 8, %d, %d\)" % (b, h, w)):
        X.compare_8c("channels swapped", X.to8c(bad), st, TEETH_PLAN)


def test_last_row_of_an_odd_height_stride2_gradient_shifted_is_reported():
    ref = _ref((1, 128, 128, 7, 7, 3, 2))
    dx = ref.dx(True, True)
    bad = dx.clone()
    bad[:, :, -1, :] = torch.roll(dx[:, :, -1, :], 1, dims=-1)
    with pytest.raises(AssertionError, match=r"elements differ; \d+ of them on a band \(TW = None\) or image border; first at \(0, \d+, 6, \d\)"):
        X.compare_8c("row shifted", X.to8c(bad), dx)


def test_nonzero_padding_channel_is_reported():
    ref = _ref((1, 24, 40, 11, 9, 3, 1))     # 40 channels in 6 blocks of 8: channels 40 .. 47 are padding
    got = X.to8c(ref.stored())
    got[0, 5, 3, 4, 2] = 1.0
    with pytest.raises(AssertionError, match=r"\[padding channels\]: 1 of \d+ elements differ.*first at \(0, 2, 3, 4\)"):
        X.compare_8c("padding", got, ref.stored())


def test_sign_bit_of_an_exact_zero_is_reported():
    ref = _ref(TEETH)
    st = ref.stored()
    Cout = st.shape[1]
    b, c, h, w = _first(st == 0)
    sg = X.sign_map(st).clone()
    q, e, hh, i = c // 16, (c % 16) // 8, (c % 8) // 4, c % 4
    sg[b, hh, h, w, q] |= 1 << (i + 4 * e)
    with pytest.raises(AssertionError, match=r"sign bytes.*: 1 of \d+ elements differ"):
        X.compare_signs("sign of zero", sg, st, TEETH_PLAN)
    # ... and -0.0 (a negative value times the scale 0) reads "not positive"
    neg0 = torch.where(st == 0, torch.tensor(-0.0), st)
    X.compare_signs("sign of -0.0", X.sign_map(neg0), st, TEETH_PLAN)


def test_one_weight_gradient_element_off_by_one_is_reported():
    ref = _ref(TEETH)
    dw, db = ref.wgrad(X.CLIP)
    bad = dw.clone().float()
    bad[63, 31, 2, 2] += 1.0
    with pytest.raises(AssertionError, match=r"1 of \d+ elements differ.*first at \(63, 31, 2, 2\)"):
        X.compare("dw", bad, dw.float())
    assert float(dw.abs().max()) == X.CLIP and float(ref.dw.abs().max()) > X.CLIP    # (the clamp is active on this case)
