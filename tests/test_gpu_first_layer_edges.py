"""Every route of yogo_amd/csrc/conv_first.hip against the fp64 restatement of tests/_first_layer_ref.py, at the shapes where its indexing can
go wrong (`pix = pbase + k * 256 + tid`, the `pix < npix` tail, the partial row at `b * gridDim.x + blockIdx.x`, channels picked out of
8-channel units, the sign word's bit permutation).

EXACT cases (the method of check_exact_case in test_gpu_first_fused_bwd.py): integer pixels, g in {-1, 0, 1}, integer z and mean, invstd a
power of two -- every term of every sum is a multiple of 0.5, and where every column's sum of magnitudes is below 2^24 such quanta
(asserted on the reference before the GPU is touched) every partial sum of every summation order is an fp32 value: each partial row, the
rows summed on the host and the output of yogo_partials_reduce must equal fp64 BIT FOR BIT.  Modes "none" (no activation) and "allpos"
(LeakyReLU, every value on the positive side) are exact; "mixed" (both sides) rounds in the float32(0.01) products and is held to

    |d| <= D * 2^-24 * sum |terms|   per column,                                                      D = D_SWEEP = 45

D is the depth of the summation tree, read off the kernels (conv_first.hip), every level contributing one rounding of at most 2^-24 of
the sum of magnitudes below it:
    32  a lane's CFW_PPT = 32 pixels (pk2: 16 steps of 2 pixels), one fma or add each
     6  the DPP levels of wave_sum (quads x 2, half rows, rows, rows 0 -> 1 / 2 -> 3, rows 0..1 -> 3)
     3  the four wavefronts' sums added in LDS order
     1  the rows: yogo_partials_reduce adds them in double and rounds once (the host sum in fp64 rounds not at all)
     2  xh = (z - mean) * invstd: a subtraction and a product (A2 and S2 terms)
     1  gb = g * act' (the float32(0.01) product)
The random cases (real batch statistics, bf16 data) are held to the same bound.  SiLU's derivative s * (1 + y * (1 - s)) is not one
rounding: the fast exponential (counted as 3: its argument scaling and a 2-ulp result), 1 + e, the reciprocal (counted as 2), 1 - s,
y * (1 - s), 1 + ..., s * ... = 10 more, D_SILU = 55, against |g| * max|silu'| as the magnitude of a term.

The measured ratios |d| / (2^-24 sum|terms|) are printed per case (`pytest -s`); DESIGN.md section 4 and profiles/first_layer_edges.log
hold the largest per route.

ROUTES.  The dispatch rules of conv_first_bn_wgrad_impl, restated in instantiation() below; every case names the instantiation it is there
to reach and the test asserts that its arguments select it:
    z == NULL (the _xs launcher; its shape gate: uint8, Cin 1, stride 2, even IH / IW >= 4, Cout 8 | 16, no activation | LeakyReLU)
        OW even and >= 4, image 4-byte aligned, the pairs plan on  -> conv_first_bn_wgrad_pk2_kernel
        else (OW odd, OW = 2, pairs plan off, image at 4k + 2)     -> conv_first_bn_wgrad_pk_kernel<true>
    FAST = uint8, Cin 1, stride 2, IH and IW even; needs a 2-byte aligned image
        FAST, caller's Gram matrix (_xg), Cout % 8 == 0, no SiLU   -> conv_first_bn_wgrad_pk_kernel<false>
        FAST otherwise (Cout 4 / 12, SiLU, or the _bf16 launcher)  -> conv_first_bn_wgrad_kernel<uint8_t, 1, 8, true, true>
    uint8 Cin 1 (odd size, stride 1, odd address)                  -> conv_first_bn_wgrad_kernel<uint8_t, 1, 8, true>
    uint8 Cin 3 -> <uint8_t, 3, 2, false>;  float Cin 1 -> <float, 1, 8, true>;  float Cin 3 -> <float, 3, 2, false>
conv_first_wgrad_impl and conv_first_fwd_impl pick by (in_dtype, Cin) and by which gradient / output pointer is given."""
import numpy as np
import pytest
import torch

import _first_layer_ref as R
from _util import Guarded, assert_bf16_tensor_matches, hooks_library

pytestmark = pytest.mark.gpu

D_SWEEP = 45
D_SILU = 55
NAN = float("nan")


def H():
    from yogo_amd import _hip

    return _hip


# ---- the dispatch rules, restated ---------------------------------------------------------------------------------------------------
def instantiation(launcher, c, pairs=True, align=4):
    fast = c["in_dtype"] == 0 and c["Cin"] == 1 and c["stride"] == 2 and c["IH"] % 2 == 0 and c["IW"] % 2 == 0
    if launcher == "xs":
        assert fast and c["Cout"] in (8, 16) and c["act"] != R.ACT_SILU and c["IH"] >= 4 and c["IW"] >= 4 and align % 2 == 0
        return "pk2" if (c["OW"] % 2 == 0 and c["OW"] >= 4 and pairs and align % 4 == 0) else "pk<true>"
    ext = launcher == "xg"
    if fast and align % 2 == 0:
        return "pk<false>" if (ext and c["Cout"] % 8 == 0 and c["act"] != R.ACT_SILU) else "generic<u8,1,8,true,true>"
    t = "u8" if c["in_dtype"] == 0 else "float"
    return f"generic<{t},1,8,true>" if c["Cin"] == 1 else f"generic<{t},3,2,false>"


def columns_of(launcher, c):
    """(unwritten, zero) column sets of a route: the Gram kernels (Cin = 1) leave the A2 columns unwritten; with a caller-held Gram matrix
    (_xg, _xs) the P / G columns are zero-filled; the sign-map sweeps write S2 = 0 (the finalize kernel derives it)"""
    Cin, Cout = c["Cin"], c["Cout"]
    unwritten = R.sweep_columns(Cin, Cout, "A2") if Cin == 1 else []
    zero = []
    if launcher in ("xg", "xs"):
        zero += R.sweep_columns(Cin, Cout, "P") + R.sweep_columns(Cin, Cout, "G")
    if launcher == "xs":
        zero += R.sweep_columns(Cin, Cout, "S2")
    return unwritten, zero


LAUNCHER = {"xs": "yogo_conv_first_bn_wgrad_bf16_xs", "xg": "yogo_conv_first_bn_wgrad_bf16_xg", "plain": "yogo_conv_first_bn_wgrad_bf16"}


def run_sweep(h, launcher, c, x_dev=None):
    """-> (partial rows [rows][cols] as written into an exact-size NaN-poisoned buffer between sentinels, the sums of yogo_partials_reduce)"""
    st = h.stream_ptr()
    B, Cin, Cout, IH, IW, s = c["B"], c["Cin"], c["Cout"], c["IH"], c["IW"], c["stride"]
    rows = h.query_ints("yogo_conv_first_wgrad_rows", 1, B, IH, IW, s)[0]
    cols = h.query_ints("yogo_conv_first_bn_wgrad_cols", 1, Cin, Cout)[0]
    assert rows == B * -(-c["OH"] * c["OW"] // R.TILE_SWEEP) and cols == R.sweep_layout(Cin, Cout)[2]
    part = Guarded(rows * cols)
    x = c["x"].cuda() if x_dev is None else x_dev
    g8 = c["g8"].cuda()
    dev = [c[k].cuda() for k in ("mean", "invstd", "gamma", "beta")]
    if launcher == "xs":
        second = c["signs"].cuda() if c["signs"] is not None else None
    else:
        second = c["z8"].cuda()
    h.call(LAUNCHER[launcher], x, c["in_dtype"], g8, second, *dev, part.view, B, Cin, Cout, IH, IW, s, c["act"], st)
    part.check(f"{launcher} partial rows")
    rows_cpu = part.view.cpu().reshape(rows, cols)
    scratch, sums = part.view.clone(), Guarded(cols)     # (yogo_partials_reduce folds its input in place)
    h.call("yogo_partials_reduce", scratch, rows, cols, 0.0, sums.view, st)
    sums.check("partials_reduce")
    return rows_cpu, sums.view.cpu()


# ---- cases --------------------------------------------------------------------------------------------------------------------------
# route -> (launcher, Cin, float image, pixel range of the exact cases).  Pixel ranges: 255 wherever only A1 and S1 are summed from pixels
# (255 * 3 * 8316 * 0.5 < 2^23); 15 for the in-kernel Gram pass (G sums pixel^2); 63 for A2 = sum xh * pixel on the rgb route (|xh| <= 8).
ROUTES = {
    "xs": ("xs", 1, False, 255), "xg": ("xg", 1, False, 255), "xg_f": ("xg", 1, True, 63),
    "plain": ("plain", 1, False, 15), "plain_f": ("plain", 1, True, 15), "rgb": ("plain", 3, False, 63), "rgb_f": ("plain", 3, True, 63),
}
# (route, instantiation the case is there for, B, Cout, IH, IW, stride)
SWEEP_CASES = [
    # _xs: OW even and >= 4 -> pk2; OW = 2 and OW odd -> pk<true>.  128x256 = one full tile (rows = B), 132x252 = 8192 + 124 pixels (62
    # pairs: less than one wavefront), 132x250 = 66 x 125: 8192 + 58 pixels
    ("xs", "pk<true>", 3, 16, 4, 4, 2), ("xs", "pk2", 1, 8, 4, 8, 2), ("xs", "pk2", 3, 16, 128, 256, 2), ("xs", "pk2", 3, 16, 132, 252, 2),
    ("xs", "pk2", 1, 8, 132, 252, 2), ("xs", "pk<true>", 3, 8, 132, 250, 2), ("xs", "pk<true>", 1, 16, 132, 250, 2),
    # _xg on a FAST shape with Cout % 8 == 0 -> pk<false> (2x2: OW = 1, the one shape whose pixel / OW is a division, not a multiply-high)
    ("xg", "pk<false>", 3, 8, 2, 2, 2), ("xg", "pk<false>", 3, 8, 4, 4, 2), ("xg", "pk<false>", 1, 16, 128, 256, 2), ("xg", "pk<false>", 3, 16, 132, 252, 2), ("xg", "pk<false>", 1, 8, 132, 250, 2),
    # _xg on a FAST shape with Cout % 8 != 0 -> the generic FAST kernel with the caller's Gram matrix (quarter_filters on grey images)
    ("xg", "generic<u8,1,8,true,true>", 3, 4, 2, 2, 2), ("xg", "generic<u8,1,8,true,true>", 1, 12, 128, 256, 2), ("xg", "generic<u8,1,8,true,true>", 3, 12, 132, 252, 2),
    ("xg", "generic<u8,1,8,true,true>", 1, 4, 132, 250, 2),
    # _xg off the FAST shapes (odd size; stride 1) -> <u8,1,8,true>; 91x91 = 8192 + 89, 181x183 -> 91 x 92 = 8192 + 180
    ("xg", "generic<u8,1,8,true>", 3, 7, 1, 1, 1), ("xg", "generic<u8,1,8,true>", 1, 9, 7, 1, 2), ("xg", "generic<u8,1,8,true>", 3, 20, 91, 91, 1),
    ("xg", "generic<u8,1,8,true>", 1, 16, 181, 183, 2), ("xg", "generic<u8,1,8,true>", 3, 8, 33, 31, 1),
    # _xg with a float image -> <float,1,8,true>
    ("xg_f", "generic<float,1,8,true>", 3, 9, 1, 7, 1), ("xg_f", "generic<float,1,8,true>", 1, 20, 181, 183, 2), ("xg_f", "generic<float,1,8,true>", 3, 7, 128, 256, 2),
    # _bf16 on a FAST shape -> the generic FAST kernel with the in-kernel Gram pass
    ("plain", "generic<u8,1,8,true,true>", 3, 1, 2, 2, 2), ("plain", "generic<u8,1,8,true,true>", 1, 9, 4, 8, 2), ("plain", "generic<u8,1,8,true,true>", 3, 16, 128, 256, 2),
    ("plain", "generic<u8,1,8,true,true>", 3, 20, 132, 252, 2), ("plain", "generic<u8,1,8,true,true>", 1, 7, 132, 250, 2),
    # _bf16 off the FAST shapes -> <u8,1,8,true>
    ("plain", "generic<u8,1,8,true>", 3, 1, 1, 1, 2), ("plain", "generic<u8,1,8,true>", 1, 8, 1, 7, 2), ("plain", "generic<u8,1,8,true>", 3, 9, 7, 1, 1),
    ("plain", "generic<u8,1,8,true>", 3, 7, 91, 91, 1), ("plain", "generic<u8,1,8,true>", 1, 20, 181, 183, 2), ("plain", "generic<u8,1,8,true>", 1, 16, 33, 31, 1),
    # _bf16 with an rgb image (passes of two channels) -> <u8,3,2,false>
    ("rgb", "generic<u8,3,2,false>", 3, 1, 1, 1, 1), ("rgb", "generic<u8,3,2,false>", 1, 5, 1, 7, 2), ("rgb", "generic<u8,3,2,false>", 3, 9, 7, 1, 2),
    ("rgb", "generic<u8,3,2,false>", 3, 5, 91, 91, 1), ("rgb", "generic<u8,3,2,false>", 1, 8, 181, 183, 2), ("rgb", "generic<u8,3,2,false>", 1, 9, 128, 256, 2),
    # _bf16 with float images
    ("plain_f", "generic<float,1,8,true>", 3, 7, 1, 1, 1), ("plain_f", "generic<float,1,8,true>", 1, 16, 91, 91, 1), ("plain_f", "generic<float,1,8,true>", 3, 9, 181, 183, 2),
    ("rgb_f", "generic<float,3,2,false>", 3, 5, 7, 1, 1), ("rgb_f", "generic<float,3,2,false>", 1, 9, 91, 91, 1), ("rgb_f", "generic<float,3,2,false>", 3, 8, 181, 183, 2),
]
# one random case per instantiation, at its two-tile shape
RANDOM_CASES = [
    ("xs", "pk2", 3, 16, 132, 252, 2), ("xs", "pk<true>", 3, 16, 132, 250, 2), ("xg", "pk<false>", 3, 16, 132, 252, 2),
    ("xg", "generic<u8,1,8,true,true>", 3, 12, 132, 252, 2), ("xg", "generic<u8,1,8,true>", 3, 20, 91, 91, 1), ("xg_f", "generic<float,1,8,true>", 1, 20, 181, 183, 2),
    ("plain", "generic<u8,1,8,true,true>", 3, 20, 132, 252, 2), ("plain", "generic<u8,1,8,true>", 3, 7, 91, 91, 1), ("rgb", "generic<u8,3,2,false>", 3, 5, 91, 91, 1),
    ("plain_f", "generic<float,1,8,true>", 3, 9, 181, 183, 2), ("rgb_f", "generic<float,3,2,false>", 3, 8, 181, 183, 2),
]
# SiLU on generic routes (the FAST kernel: SiLU keeps a Cout % 8 == 0 shape off pk<false>; and the rgb kernel)
SILU_CASES = [("xg", "generic<u8,1,8,true,true>", 3, 16, 132, 252, 2), ("rgb", "generic<u8,3,2,false>", 3, 5, 91, 91, 1)]

_CACHE = {}


def get_case(route, B, Cout, IH, IW, stride, mode):
    """the inputs and their fp64 reference, computed once and shared (never modified)"""
    key = (route, B, Cout, IH, IW, stride, mode)
    if key not in _CACHE:
        launcher, Cin, in_float, pmax = ROUTES[route]
        c = R.make_case(B, Cin, Cout, IH, IW, stride, mode, in_float=in_float, pmax=pmax, signs=launcher == "xs")
        _CACHE[key] = (c,) + R.case_reference(c)
    return _CACHE[key]


def check_sweep(route, kernel, B, Cout, IH, IW, stride, mode, pairs=True):
    h = H()
    launcher = ROUTES[route][0]
    c, rows, mags = get_case(route, B, Cout, IH, IW, stride, mode)
    assert instantiation(launcher, c, pairs=pairs) == kernel, "the case's arguments do not select the instantiation it is there for"
    what = f"{LAUNCHER[launcher][5:]} {kernel} B={B} Cout={Cout} {IH}x{IW}/{stride} {mode}"
    unwritten, zero = columns_of(launcher, c)
    m = mags.clone()
    m[:, unwritten + zero] = 0
    frac = R.exact_precondition(m, c["Cin"], Cout, 0.5, what) if c["exact"] else float(m.sum(0).max()) / 2.0 ** 23
    part, sums = run_sweep(h, launcher, c)
    D = D_SILU if mode == "silu" else D_SWEEP
    ratio = R.compare_sweep(part, rows, mags, c["Cin"], Cout, exact=c["exact"], D=D, what=what, unwritten=unwritten, zero=zero, sums=sums, quantum=0.5)
    print(f"   {what}: {c['OH'] * c['OW']} pixels, {rows.shape[0]} rows; largest sum|terms| {frac * 2.0 ** 23:.4g} = {frac:.3f} of 2^24 quanta; "
          f"measured |d| / (2^-24 sum|terms|) {ratio:.3f} (D = {0 if c['exact'] else D})")
    return part, sums


@pytest.mark.parametrize("mode", ["none", "allpos", "mixed"])
@pytest.mark.parametrize("route,kernel,B,Cout,IH,IW,stride", SWEEP_CASES)
def test_fused_sweep_exact_cases(route, kernel, B, Cout, IH, IW, stride, mode):
    check_sweep(route, kernel, B, Cout, IH, IW, stride, mode)


@pytest.mark.parametrize("route,kernel,B,Cout,IH,IW,stride", RANDOM_CASES)
def test_fused_sweep_random_cases(route, kernel, B, Cout, IH, IW, stride):
    check_sweep(route, kernel, B, Cout, IH, IW, stride, "random")


@pytest.mark.parametrize("route,kernel,B,Cout,IH,IW,stride", SILU_CASES)
def test_fused_sweep_silu(route, kernel, B, Cout, IH, IW, stride):
    check_sweep(route, kernel, B, Cout, IH, IW, stride, "silu")


@pytest.mark.parametrize("mode", ["none", "allpos", "mixed"])
@pytest.mark.parametrize("B,Cout,IH,IW", [(1, 8, 4, 8), (3, 16, 128, 256), (3, 16, 132, 252)])
def test_one_pixel_sweep_on_the_pair_shapes_gives_the_same_sums(B, Cout, IH, IW, mode):
    """pk<true> on the pk2 shapes (the hooks library with the pairs plan off): held to fp64 like every route; in the exact modes the two
    kernels' partial rows are the same bits (both equal fp64)"""
    part2, sums2 = check_sweep("xs", "pk2", B, Cout, IH, IW, 2, mode)
    with hooks_library() as L:
        L.yogo_hook_conv_first_bn_wgrad_pairs(0)
        part1, sums1 = check_sweep("xs", "pk<true>", B, Cout, IH, IW, 2, mode, pairs=False)
    if mode != "mixed":
        c = get_case("xs", B, Cout, IH, IW, 2, mode)[0]
        keep = torch.ones(part1.shape[1], dtype=torch.bool)
        keep[columns_of("xs", c)[0]] = False
        assert torch.equal(part1[:, keep], part2[:, keep]) and torch.equal(sums1[keep], sums2[keep])


# ---- image alignment ----------------------------------------------------------------------------------------------------------------
def _offset_view(x, off):
    buf = torch.zeros(x.numel() + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 4 == off % 4
    return v


@pytest.mark.parametrize("off", [1, 2])
@pytest.mark.parametrize("route,B,Cout,IH,IW", [("xs", 3, 16, 132, 252), ("xg", 3, 16, 132, 252), ("xg", 1, 12, 4, 8), ("plain", 3, 9, 132, 252)])
def test_image_at_a_byte_offset(route, B, Cout, IH, IW, off):
    """no load wider than the pointer's alignment: an image at 4k + 2 takes the 16-bit routes, at an odd address the byte-wise kernel --
    the same sums (exact case: the same bits) -- and the sign-map sweep, which has no byte-wise route, refuses an odd address"""
    h = H()
    launcher = ROUTES[route][0]
    c, rows, mags = get_case(route, B, Cout, IH, IW, 2, "allpos")
    kernel = None if (launcher == "xs" and off == 1) else instantiation(launcher, c, align=off)
    xv = _offset_view(c["x"].cuda(), off)
    if kernel is None:
        with pytest.raises(RuntimeError, match="aligned to 2 bytes"):
            run_sweep(h, launcher, c, x_dev=xv)
        return
    assert kernel == {("xs", 2): "pk<true>", ("xg", 2): instantiation("xg", c), ("plain", 2): "generic<u8,1,8,true,true>",
                      ("xg", 1): "generic<u8,1,8,true>", ("plain", 1): "generic<u8,1,8,true>"}[(launcher, off)]
    unwritten, zero = columns_of(launcher, c)
    part, sums = run_sweep(h, launcher, c, x_dev=xv)
    R.compare_sweep(part, rows, mags, c["Cin"], Cout, exact=True, D=0, what=f"{route} image at byte offset {off} ({kernel})", unwritten=unwritten,
                    zero=zero, sums=sums, quantum=0.5)


# ---- rows queries -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
def test_rows_queries_at_exact_tiles(B):
    h = H()
    for IH, IW, s, tiles in ((128, 256, 2, 1), (64, 128, 1, 1), (132, 252, 2, 2), (91, 91, 1, 2), (1, 1, 2, 1), (8193, 1, 1, 2), (1, 16384, 1, 2), (1, 16385, 1, 3)):
        assert h.query_ints("yogo_conv_first_wgrad_rows", 1, B, IH, IW, s)[0] == B * tiles, (IH, IW, s)
    for IH, IW, s, tiles in ((32, 32, 1, 1), (64, 64, 2, 1), (33, 31, 1, 1), (25, 41, 1, 2), (1, 1, 1, 1), (181, 183, 2, 9), (1, 2048, 1, 2), (1, 2049, 1, 3)):
        assert h.query_ints("yogo_conv_first_stats_rows", 1, B, IH, IW, s)[0] == B * tiles, (IH, IW, s)


# ---- the plain weight gradient --------------------------------------------------------------------------------------------------------
# conv_first_wgrad_impl: (in_dtype, Cin) picks <TIn, CIN>, a bf16 gradient (the _bf16g launcher) picks BF16G = true.  Cin = 1: passes of 16
# channels (two units; the second unit of the last pass clamped to Mb - 1); Cin = 3: passes of 4 inside one unit.
WGRAD_CASES = [
    (1, 1, 1, 1, 1, 1), (1, 3, 7, 7, 1, 2), (1, 1, 16, 128, 256, 2), (1, 3, 20, 91, 91, 1), (1, 1, 48, 181, 183, 2), (1, 3, 7, 33, 31, 1),
    (3, 3, 3, 1, 1, 2), (3, 1, 4, 1, 7, 1), (3, 3, 5, 91, 91, 1), (3, 1, 9, 181, 183, 2), (3, 3, 4, 128, 256, 2),
]


@pytest.mark.parametrize("bf16g", [False, True])
@pytest.mark.parametrize("in_float", [False, True])
@pytest.mark.parametrize("Cin,B,Cout,IH,IW,stride", WGRAD_CASES)
def test_plain_weight_gradient_exact(Cin, B, Cout, IH, IW, stride, in_float, bf16g):
    """conv_first_wgrad_kernel<{uint8_t, float}, {1, 3}, {false, true}>: integer pixels and g in {-1, 0, 1} -- no step rounds, so every
    partial row and the reduced sums equal fp64 bit for bit; the padding channels of the bf16 gradient hold 3.0 and must be ignored"""
    h = H()
    st = h.stream_ptr()
    key = ("wgrad", Cin, B, Cout, IH, IW, stride, in_float)
    if key not in _CACHE:
        c = R.make_case(B, Cin, Cout, IH, IW, stride, "none", in_float=in_float, pmax=63 if in_float else 255)
        _CACHE[key] = (c,) + R.wgrad_rows(c["x"], c["g"], stride)
    c, rows, mags = _CACHE[key]
    NJ = 9 * Cin + 1
    what = f"conv_first_wgrad<{'float' if in_float else 'u8'},{Cin},{'bf16' if bf16g else 'fp32'} g> B={B} Cout={Cout} {IH}x{IW}/{stride}"
    names = lambda i: f"row {i[0]} dW[c={i[-2]}][j={i[-1]}]" if i[-1] < NJ - 1 else f"row {i[0]} db[c={i[-2]}]"
    assert float(mags.sum(0).max()) < 2.0 ** 24, what
    nrows = h.query_ints("yogo_conv_first_wgrad_rows", 1, B, IH, IW, stride)[0]
    assert nrows == rows.shape[0]
    part = Guarded(nrows * Cout * NJ)
    if bf16g:
        h.call("yogo_conv_first_wgrad_bf16g", c["x"].cuda(), c["in_dtype"], c["g8"].cuda(), part.view, B, Cin, Cout, IH, IW, stride, st)
    else:
        h.call("yogo_conv_first_wgrad", c["x"].cuda(), c["in_dtype"], c["g"].cuda(), part.view, B, Cin, Cout, IH, IW, stride, st)
    part.check(what)
    got = part.view.cpu().reshape(nrows, Cout, NJ)
    R.compare_exact(got, rows, mags, what, names)
    sums = Guarded(Cout * NJ)
    h.call("yogo_partials_reduce", part.view.clone(), nrows, Cout * NJ, 0.0, sums.view, st)
    sums.check("partials_reduce")
    R.compare_exact(sums.view.cpu().reshape(1, Cout, NJ), rows.sum(0, keepdim=True), mags.sum(0, keepdim=True), what + " reduced", names)
    print(f"   {what}: {nrows} rows, largest sum|terms| {float(mags.sum(0).max()):.4g} of 2^24 = {2.0 ** 24:.4g}: exact")


# ---- the forward kernels --------------------------------------------------------------------------------------------------------------
# conv_first_fwd_impl: (in_dtype, Cin) picks <TIn, CIN>; a bf16 output pointer (the _fwd_train_bf16 launcher) picks conv_first_train_bf16_kernel,
# else conv_first_kernel.  Tiles of 1024 pixels: 32x32 = one tile exactly, 33x31 = 1023, 25x41 = 1025, 181x183 / 2 = 8372 (nine tiles).
FWD_CASES = [(1, 3, 16, 32, 32, 1), (1, 1, 7, 33, 31, 1), (1, 3, 20, 25, 41, 1), (1, 3, 1, 1, 1, 1), (1, 1, 33, 181, 183, 2),
             (3, 1, 16, 32, 32, 1), (3, 3, 7, 33, 31, 1), (3, 1, 33, 25, 41, 1), (3, 3, 20, 1, 1, 2), (3, 3, 1, 181, 183, 2)]


def _fwd_case(Cin, B, Cout, IH, IW, stride, in_float):
    """pixels in [0, 3] (float: [-3, 3]), weights in {-1, 0, 1}, integer bias: pre is an integer with |pre| <= 27 Cin + 2 and sum pre^2 over
    every statistics row and over all rows stays below 2^24 (asserted); chan_scale is any fp32 value (one multiplication)"""
    key = ("fwd", Cin, B, Cout, IH, IW, stride, in_float)
    if key not in _CACHE:
        gen = torch.Generator().manual_seed(100 * IH + IW + Cout)
        x = torch.randint(-3 if in_float else 0, 4, (B, Cin, IH, IW), generator=gen)
        x = x.float() if in_float else x.to(torch.uint8)
        w = torch.randint(-1, 2, (Cout, Cin, 3, 3), generator=gen).float()
        bias = torch.randint(-2, 3, (Cout,), generator=gen).float()
        cs = (0.5 + torch.rand(B, Cout, generator=gen)).float()
        pre = R.forward(x, w, bias, cs, stride, R.ACT_NONE)[0] + 0.0
        rows, mags = R.forward_stat_rows(pre)
        assert float(mags.sum(0).max()) < 2.0 ** 24 and float(pre.abs().max()) <= 27 * Cin + 2
        _CACHE[key] = dict(x=x, w=w, bias=bias, cs=cs, pre=pre, rows=rows, mags=mags)
    return _CACHE[key]


def _act32(pre32, cs, act):
    """what the kernels form in fp32: act(pre) with ONE multiplication on the negative side of LeakyReLU, times chan_scale (one more)"""
    if act == R.ACT_LEAKY:
        v = torch.where(pre32 > 0, pre32, pre32 * np.float32(0.01))
    elif act == R.ACT_SILU:
        v = torch.nn.functional.silu(pre32)
    else:
        v = pre32
    return v * cs[:, :, None, None]


@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_LEAKY, R.ACT_SILU])
@pytest.mark.parametrize("in_float", [False, True])
@pytest.mark.parametrize("Cin,B,Cout,IH,IW,stride", FWD_CASES)
def test_forward_kernels(Cin, B, Cout, IH, IW, stride, in_float, act):
    """conv_first_kernel and conv_first_train_bf16_kernel, <{uint8_t, float}, {1, 3}>: pre is an exact integer, so the fp32 pre-activation,
    the per-tile statistics rows, and (no activation, LeakyReLU) the fp32 output and every bit of the bf16 output -- padding channels +0 --
    equal what torch forms with the same single multiplications.  SiLU: one bf16 ulp, and in fp32 four times torch's own fp32 error."""
    h = H()
    st = h.stream_ptr()
    c = _fwd_case(Cin, B, Cout, IH, IW, stride, in_float)
    OH, OW = R.out_size(IH, IW, stride)
    npix = OH * OW
    what = f"conv_first_fwd<{'float' if in_float else 'u8'},{Cin}> B={B} Cout={Cout} {IH}x{IW}/{stride} act={act}"
    pre32 = c["pre"].float()
    assert torch.equal(pre32.double(), c["pre"])
    want32 = _act32(pre32, c["cs"], act)
    y64 = R.forward(c["x"], c["w"], c["bias"], c["cs"], stride, act, slope=R.LEAKY32)[1]
    nrows = h.query_ints("yogo_conv_first_stats_rows", 1, B, IH, IW, stride)[0]
    assert nrows == c["rows"].shape[0] == B * -(-npix // R.TILE_FWD)
    xd, wd, bd, csd = c["x"].cuda(), c["w"].cuda(), c["bias"].cuda(), c["cs"].cuda()
    names = lambda i: f"statistics row {i[0]} channel {i[1]} {'sum pre^2' if i[2] else 'sum pre'}"
    # ---- fp32 output
    out, outp, stats = Guarded(B * Cout * npix), Guarded(B * Cout * npix), Guarded(nrows * Cout * 2)
    h.call("yogo_conv_first_fwd", xd, int(in_float), wd, bd, out.view, outp.view, csd, stats.view, B, Cin, Cout, IH, IW, stride, act, st)
    out.check(what), outp.check(what), stats.check(what)
    R.compare_exact(stats.view.cpu().reshape(nrows, Cout, 2), c["rows"], c["mags"], what + " fp32", names)
    got_pre = outp.view.cpu().reshape(B, Cout, OH, OW)
    assert torch.equal(got_pre, pre32), (what, "pre-activation", float((got_pre - pre32).abs().max()))
    got = out.view.cpu().reshape(B, Cout, OH, OW)
    # ---- bf16 output (NCHW8c, padding channels included)
    Mb = ((Cout + 15) // 16) * 2
    o8 = Guarded(B * Mb * npix * 4)
    o8.view.view(torch.int32).fill_(0x7FC07FC0)   # bf16 NaN
    stats2 = Guarded(nrows * Cout * 2)
    h.call("yogo_conv_first_fwd_train_bf16", xd, int(in_float), wd, bd, o8.view, csd, stats2.view, B, Cin, Cout, IH, IW, stride, act, st)
    o8.check(what), stats2.check(what)
    R.compare_exact(stats2.view.cpu().reshape(nrows, Cout, 2), c["rows"], c["mags"], what + " bf16", names)
    got8 = o8.view.cpu().view(torch.bfloat16).reshape(B, Mb, OH, OW, 8)
    if act != R.ACT_SILU:
        assert torch.equal(got, want32), (what, "fp32 output", float((got - want32).abs().max()))
        want8 = R.to8c(want32 + 0.0, pad=0.0)
        assert torch.equal(got8.view(torch.int16), want8.view(torch.int16)), (what, "bf16 output bits", float((got8.float() - want8.float()).abs().max()))
    else:
        full = R.from8c(got8)
        assert torch.equal(full[:, Cout:].contiguous().view(torch.int32), torch.zeros_like(full[:, Cout:]).view(torch.int32)), (what, "padding channels must be +0")
        assert_bf16_tensor_matches(full[:, :Cout], y64.float().to(torch.bfloat16).float(), what + " bf16 SiLU")
        e_torch = float((want32.double() - y64).abs().max())
        d = float((got.double() - y64).abs().max())
        ratio = d / e_torch if e_torch > 0 else 0.0
        print(f"   {what}: fp32 SiLU max|d| {d:.3e}, torch's own fp32 SiLU against fp64 {e_torch:.3e}: ratio {ratio:.2f} (bound 4)")
        assert d <= 4 * e_torch, (what, d, e_torch)


def test_forward_without_the_optional_pointers():
    """bias, chan_scale, the pre-activation copy and the statistics rows are optional: the same bits without them (33x31: a tile's tail)"""
    h = H()
    st = h.stream_ptr()
    for Cin, B, Cout, in_float in ((1, 3, 7, False), (3, 1, 20, True)):
        gen = torch.Generator().manual_seed(Cin)
        x = torch.randint(0, 4, (B, Cin, 33, 31), generator=gen)
        x = x.float() if in_float else x.to(torch.uint8)
        w = torch.randint(-1, 2, (Cout, Cin, 3, 3), generator=gen).float()
        pre32 = (R.forward(x, w, None, None, 1, R.ACT_NONE)[0] + 0.0).float()
        want32 = _act32(pre32, torch.ones(B, Cout), R.ACT_LEAKY)
        out = Guarded(B * Cout * 1023)
        h.call("yogo_conv_first_fwd", x.cuda(), int(in_float), w.cuda(), None, out.view, None, None, None, B, Cin, Cout, 33, 31, 1, R.ACT_LEAKY, st)
        out.check("fp32 output")
        assert torch.equal(out.view.cpu().reshape(B, Cout, 33, 31), want32)
        Mb = ((Cout + 15) // 16) * 2
        o8 = Guarded(B * Mb * 1023 * 4)
        o8.view.view(torch.int32).fill_(0x7FC07FC0)
        h.call("yogo_conv_first_fwd_train_bf16", x.cuda(), int(in_float), w.cuda(), None, o8.view, None, None, B, Cin, Cout, 33, 31, 1, R.ACT_LEAKY, st)
        o8.check("bf16 output")
        got8 = o8.view.cpu().view(torch.bfloat16).reshape(B, Mb, 33, 31, 8)
        assert torch.equal(got8.view(torch.int16), R.to8c(want32 + 0.0).view(torch.int16))


# ---- the finalize kernel, alone -------------------------------------------------------------------------------------------------------
# |d| <= K_FINALIZE * 2^-24 * M, M = the same expression with every term replaced by its magnitude.  K_FINALIZE = the fp32 operations on the
# longest path of conv_first_bn_wgrad_finalize_kernel (the Gram form of dW under batch statistics):
#   9  t = fma(w, G, t) over the nine taps          1  mean * P          1  t - ...          1  invstd * (...)              -> a2: 12
#   1  S2 * inv_count    1  ... * a2     2  the two subtractions from A1     1  c1 = gamma * invstd     1  c1 * (...)          ->  6
#   1  inv_count = 1 / (B OH OW) formed in fp32 by the launcher     1  the derived S2's final rounding (its sum is formed in double) ->  2
K_FINALIZE = 20
# (Cin, Cout, form): 16 x 27 -> 464 and 48 x 9 -> 528 outputs, two and three blocks of 256; a caller-held Gram matrix exists for one input channel only
FIN_CASES = [(3, 1, "plain"), (3, 16, "plain")] + [(1, co, f) for co in (1, 48) for f in ("plain", "xg", "xs", "xs_cancel")]


@pytest.mark.parametrize("clip_half", [False, True])
@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("Cin,Cout,form", FIN_CASES)
def test_finalize_kernel_alone(Cin, Cout, form, training, clip_half):
    """synthetic sums.  plain: the row's own P / G (Cin = 1, the Gram form) or A2 columns (Cin = 3); xg: the caller's Gram matrix; xs: the
    same with S2 derived; xs_cancel: W . A1 and mean * S1 agree to 1 part in 1000 -- the cancellation the kernel's double is there for (the
    derived S2 enters M with its VALUE's magnitude: it may contribute its final rounding only)"""
    h = H()
    st = h.stream_ptr()
    NJ, PER, ncol = R.sweep_layout(Cin, Cout)
    gen = torch.Generator().manual_seed(1000 * Cin + Cout + 7 * training)
    B, IH, IW, stride = 3, 20, 14, 2
    count = B * 10 * 7
    sums = (torch.randn(ncol, generator=gen) * 50).float()
    sums[Cout * PER:] = sums[Cout * PER:].abs() * 20          # P, G: sums of non-negative pixels and products
    w = (torch.randn(Cout, Cin, 3, 3, generator=gen) * 0.2).float()
    mean, invstd = torch.randn(Cout, generator=gen).float() * 3, (0.2 + torch.rand(Cout, generator=gen)).float()
    gamma = torch.randn(Cout, generator=gen).float()
    gram = (torch.randn(NJ + NJ * NJ, generator=gen).abs() * 900).float() if form != "plain" else None
    derive = form.startswith("xs")
    if form == "xs_cancel":
        A1 = sums[: Cout * PER].reshape(Cout, PER)[:, :NJ].abs() + 1
        sums[: Cout * PER].reshape(Cout, PER)[:, :NJ] = A1
        w = w.abs() + 0.05
        S1 = sums[: Cout * PER].reshape(Cout, PER)[:, 2 * NJ].abs() + 10
        sums[: Cout * PER].reshape(Cout, PER)[:, 2 * NJ] = S1
        dot = (w.reshape(Cout, NJ).double() * A1.double()).sum(1)
        mean = (dot / S1.double() * (1 - 1e-3)).float()
        resid = (dot - mean.double() * S1.double()).abs() / dot
        assert float(resid.max()) < 1.1e-3 and float(resid.min()) > 0.9e-3
    if derive:
        sums[R.sweep_columns(Cin, Cout, "S2")] = 0.0          # what the sign-map sweeps write
    if Cin == 1:
        sums[R.sweep_columns(Cin, Cout, "A2")] = NAN          # unwritten by the Gram kernels: the finalize kernel must not read them
    if gram is not None:
        sums[Cout * PER:] = NAN                               # the caller's matrix replaces the row's
    ref = R.finalize(sums, Cin, Cout, mean, invstd, gamma, w, count, training=bool(training), gram=gram, derive_s2=derive)
    M = R.finalize(sums, Cin, Cout, mean, invstd, gamma, w, count, training=bool(training), gram=gram, derive_s2=derive, mag=True)
    clip = 0.0
    if clip_half:
        clip = float(np.float32(torch.cat([t.reshape(-1) for t in ref]).abs().median()))
        ref = tuple(t.clamp(-clip, clip) for t in ref)
    dw, dg, db = Guarded(Cout * NJ), Guarded(Cout), Guarded(Cout)
    name = {"plain": "yogo_conv_first_bn_wgrad_finalize", "xg": "yogo_conv_first_bn_wgrad_finalize_xg"}.get(form, "yogo_conv_first_bn_wgrad_finalize_xs")
    extra = (gram.cuda(),) if gram is not None else ()
    h.call(name, sums.cuda(), *extra, mean.cuda(), invstd.cuda(), gamma.cuda(), w.cuda(), dw.view, dg.view, db.view, B, Cin, Cout, IH, IW, stride,
           training, clip, st)
    dw.check("dw"), dg.check("dgamma"), db.check("dbeta")
    worst = 0.0
    nclamped = 0
    for label, got, r, m in (("dW", dw.view.cpu().reshape(Cout, NJ), ref[0], M[0]), ("dgamma", dg.view.cpu(), ref[1], M[1]), ("dbeta", db.view.cpu(), ref[2], M[2])):
        assert bool(torch.isfinite(got).all()), (form, label, "not finite: an unwritten column was read")
        d = (got.double() - r).abs()
        tol = K_FINALIZE * R.U24 * m
        ratio = float((d / (R.U24 * m)).max())
        worst = max(worst, ratio)
        nclamped += int((r.abs() == clip).sum()) if clip_half else 0
        assert bool((d <= tol).all()), (form, Cin, Cout, training, label, "index", int((d - tol).argmax()), "|d| / (2^-24 M)", ratio, "bound", K_FINALIZE)
    n = Cout * (NJ + 2)
    if clip_half and n > 4:
        assert 0.25 * n <= nclamped <= 0.75 * n, (nclamped, n)
    print(f"   finalize {form} Cin={Cin} Cout={Cout} training={training} clip={clip:.3g}: measured |d| / (2^-24 M) {worst:.2f} (k = {K_FINALIZE}); {nclamped} of {n} clamped")
