"""tests/_first_layer_ref.py without a GPU: (a) the restatement is the mathematics (torch autograd, fp64); (b) a CPU stand-in for a correct
fused sweep -- fp64, written the way the kernels index (pixel = tile base + offset, taps by address arithmetic, channels picked out of
8-channel units, the sign word decoded bit by bit, one partial row per 8192-pixel tile) -- passes the comparison helper the GPU tests use;
(c) the helper fails on each seeded indexing defect of that stand-in and names a column."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _first_layer_ref as R

f64 = torch.float64
EPS = 1e-5


# ---- (a) the restatement is the mathematics --------------------------------------------------------------------------------------
def _real_case(Cin, Cout, B, IH, IW, stride, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(B, Cin, IH, IW, generator=gen, dtype=f64) * 3 + 0.5
    w = torch.randn(Cout, Cin, 3, 3, generator=gen, dtype=f64) * 0.3
    g = torch.randn(B, Cout, *R.out_size(IH, IW, stride), generator=gen, dtype=f64)
    gamma = torch.randn(Cout, generator=gen, dtype=f64)
    beta = torch.randn(Cout, generator=gen, dtype=f64) * 0.3
    return x, w, g, gamma, beta


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("Cin,Cout,B,IH,IW,stride", [(1, 5, 3, 9, 11, 2), (3, 4, 2, 7, 6, 1), (1, 16, 2, 8, 12, 2), (3, 9, 2, 1, 7, 2)])
@pytest.mark.parametrize("training", [True, False])
def test_finalized_sums_are_autograd(Cin, Cout, B, IH, IW, stride, training):
    """conv2d -> batch_norm -> leaky_relu under torch autograd (fp64) against sweep_rows + finalize: dW, dgamma, dbeta to 1e-10"""
    x, w, g, gamma, beta = _real_case(Cin, Cout, B, IH, IW, stride, 11 * IH + IW)
    wp, gp, bp = w.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    z = F.conv2d(x, wp, None, stride=stride, padding=1)
    if training:
        mean, var = z.detach().mean((0, 2, 3)), z.detach().var((0, 2, 3), unbiased=False)
        yb = F.batch_norm(z, None, None, gp, bp, training=True, eps=EPS)
    else:
        gen = torch.Generator().manual_seed(5)
        mean, var = torch.randn(Cout, generator=gen, dtype=f64), torch.rand(Cout, generator=gen, dtype=f64) + 0.5
        yb = F.batch_norm(z, mean, var, gp, bp, training=False, eps=EPS)
    F.leaky_relu(yb, 0.01).backward(g)
    invstd = 1.0 / torch.sqrt(var + EPS)
    rows, _ = R.sweep_rows(x, g, z.detach(), mean, invstd, gamma, beta, stride, R.ACT_LEAKY, tile=16)   # (several rows per image)
    assert rows.shape[0] == B * -(-z.shape[2] * z.shape[3] // 16)
    sums = rows.sum(0)
    count = z.numel() // Cout
    for derive in ((False, True) if Cin == 1 else (False,)):   # (derive_s2 reads no S2 column; z is the unrounded bias-free convolution)
        s = sums.clone()
        if derive:
            s[R.sweep_columns(Cin, Cout, "S2")] = float("nan")
        if Cin == 1:
            s[R.sweep_columns(Cin, Cout, "A2")] = float("nan")   # the Gram form reads no A2 column
        dW, dgamma, dbeta = R.finalize(s, Cin, Cout, mean, invstd, gamma, w, count, training=training, derive_s2=derive)
        assert _rel(dW.reshape(wp.shape), wp.grad) < 1e-10
        assert _rel(dgamma, gp.grad) < 1e-10 and _rel(dbeta, bp.grad) < 1e-10


def test_gram_and_derived_sums_are_the_direct_ones():
    """A2 from the Gram matrix and S2 from W . A1, against the directly summed columns, where z is the unrounded bias-free convolution"""
    Cin, Cout, B, IH, IW, stride = 1, 12, 2, 10, 14, 2
    x, w, g, gamma, beta = _real_case(Cin, Cout, B, IH, IW, stride, 3)
    z = F.conv2d(x, w, None, stride=stride, padding=1)
    mean, invstd = z.mean((0, 2, 3)), 1.0 / torch.sqrt(z.var((0, 2, 3), unbiased=False) + EPS)
    rows, _ = R.sweep_rows(x, g, z, mean, invstd, gamma, beta, stride, R.ACT_LEAKY)
    sums = rows.sum(0)
    NJ, PER, ncol = R.sweep_layout(Cin, Cout)
    sc = sums[: Cout * PER].reshape(Cout, PER)
    P, G = sums[Cout * PER: Cout * PER + NJ], sums[Cout * PER + NJ:].reshape(NJ, NJ)
    W = w.reshape(Cout, NJ)
    A2 = invstd[:, None] * (W @ G - mean[:, None] * P[None])
    S2 = invstd * ((W * sc[:, :NJ]).sum(1) - mean * sc[:, 2 * NJ])
    assert _rel(A2, sc[:, NJ:2 * NJ]) < 1e-10
    assert _rel(S2, sc[:, 2 * NJ + 1]) < 1e-10
    # ... and a caller-held Gram matrix is the row's own
    a = R.finalize(sums, Cin, Cout, mean, invstd, gamma, w, z.numel() // Cout)
    b = R.finalize(sums, Cin, Cout, mean, invstd, gamma, w, z.numel() // Cout, gram=sums[Cout * PER:].clone())
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_forward_and_plain_weight_gradient_are_autograd():
    for Cin, Cout, stride, act in ((1, 7, 2, R.ACT_LEAKY), (3, 5, 1, R.ACT_SILU), (3, 4, 2, R.ACT_NONE)):
        x, w, g, gamma, beta = _real_case(Cin, Cout, 2, 9, 8, stride, 17 + Cin)
        cs = torch.rand(2, Cout, dtype=f64) + 0.5
        wp, bp = w.clone().requires_grad_(), beta.clone().requires_grad_()
        pre_t = F.conv2d(x, wp, bp, stride=stride, padding=1)
        y_t = {R.ACT_LEAKY: lambda v: F.leaky_relu(v, 0.01), R.ACT_SILU: F.silu, R.ACT_NONE: lambda v: v}[act](pre_t) * cs[:, :, None, None]
        pre, y = R.forward(x, w, beta, cs, stride, act)
        assert _rel(pre, pre_t.detach()) < 1e-12 and _rel(y, y_t.detach()) < 1e-12
        rows, mags = R.forward_stat_rows(pre, tile=7)
        assert _rel(rows.sum(0)[:, 0], pre.sum((0, 2, 3))) < 1e-12 and _rel(rows.sum(0)[:, 1], (pre * pre).sum((0, 2, 3))) < 1e-12
        pre_t.backward(g)
        wr, _ = R.wgrad_rows(x, g, stride, tile=5)
        dw = wr.sum(0)
        assert _rel(dw[:, :-1].reshape(wp.shape), wp.grad) < 1e-12 and _rel(dw[:, -1], bp.grad) < 1e-12
        # the activation derivative the sweep multiplies with is the derivative of the forward's activation
        v = torch.randn(50, dtype=f64).requires_grad_()
        R.act_apply(v, act).sum().backward()
        assert _rel(R.act_deriv(v.detach(), act), v.grad) < 1e-12


def test_sign_map_layout_round_trip():
    pos = torch.rand(2, 16, 3, 5) < 0.5
    s = R.pack_sign_bits(pos)
    assert torch.equal(R.sign_bits(s, 3, 5), pos)
    one = torch.zeros(1, 16, 1, 1, dtype=torch.bool)
    one[0, 9] = True    # channel 9 = 8 + 4 * 0 + 1: byte 0, bit 5
    assert R.pack_sign_bits(one).tolist() == [[1 << 5, 0]]


# ---- (b) / (c) the stand-in ------------------------------------------------------------------------------------------------------
DEFECTS = ["tail_pixel_twice", "first_pixel_of_tile_2_dropped", "right_column_without_kw2", "bottom_row_reads_kh2", "lane_c_plus_1",
           "unit_1_from_unit_0", "sign_bits_4_7_and_8_11_swapped", "row_of_image_1_at_b_times_1"]


def standin_rows(case, defect=None):
    """A correct sweep, indexed as the kernels index (conv_first.hip), in fp64; ``defect`` seeds one off-by-one."""
    B, Cin, Cout, IH, IW, OH, OW, s, act = (case[k] for k in ("B", "Cin", "Cout", "IH", "IW", "OH", "OW", "stride", "act"))
    NJ, PER, ncol = R.sweep_layout(Cin, Cout)
    npix = OH * OW
    tiles = -(-npix // R.TILE_SWEEP)
    flat = np.concatenate((case["x"].double().numpy().reshape(-1), np.zeros(IW + 2)))   # the images as they lie in memory
    Mb = case["g8"].shape[1]
    g8 = case["g8"].double().numpy().reshape(B, Mb, npix, 8)
    z8 = None if case["z8"] is None else case["z8"].double().numpy().reshape(B, Mb, npix, 8)
    sg = None if case["signs"] is None else case["signs"].numpy().reshape(B, npix, 2).astype(np.int64)
    mean, invstd, gamma, beta = (case[k].double().numpy() for k in ("mean", "invstd", "gamma", "beta"))
    part = np.full((B * tiles, ncol), np.nan)
    for b in range(B):
        for t in range(tiles):
            pix = np.arange(t * R.TILE_SWEEP, min((t + 1) * R.TILE_SWEEP, npix))
            if defect == "tail_pixel_twice" and t == tiles - 1:
                pix = np.append(pix, pix[-1])
            if defect == "first_pixel_of_tile_2_dropped" and t == 1:
                pix = pix[1:]
            oy, ox = pix // OW, pix % OW
            X = np.zeros((NJ, len(pix)))
            for ci in range(Cin):
                for kh in range(3):
                    for kw in range(3):
                        iy, ix = oy * s + kh - 1, ox * s + kw - 1
                        ok = (iy >= 0) & (iy < IH) & (ix >= 0) & (ix < IW)
                        if defect == "right_column_without_kw2" and kw == 2:
                            ok &= ox != OW - 1
                        if defect == "bottom_row_reads_kh2" and kh == 2:
                            ok = (iy >= 0) & (iy <= IH) & (ix >= 0) & (ix < IW)
                        addr = ((b * Cin + ci) * IH + iy) * IW + ix
                        X[(ci * 3 + kh) * 3 + kw] = np.where(ok, flat[np.clip(addr, 0, len(flat) - 1)], 0.0)
            row = np.full(ncol, np.nan)
            for c in range(Cout):
                unit, lane = c >> 3, c & 7
                if defect == "lane_c_plus_1":
                    lane = (lane + 1) & 7
                if defect == "unit_1_from_unit_0" and unit == 1:
                    unit = 0
                gv = g8[b, unit, pix, lane]
                xh = np.zeros(len(pix)) if z8 is None else (z8[b, unit, pix, lane] - mean[c]) * invstd[c]
                if sg is not None and act == R.ACT_LEAKY:
                    bit = c if (c < 4 or c >= 12) else (c + 4 if c < 8 else c - 4)   # of the pixel's 16-bit word (little endian)
                    if defect == "sign_bits_4_7_and_8_11_swapped":
                        bit = c
                    word = sg[b, pix, 0] | (sg[b, pix, 1] << 8)
                    f = np.where((word >> bit) & 1, 1.0, R.LEAKY32)
                else:
                    f = R.act_deriv(torch.from_numpy(gamma[c] * xh + beta[c]), act, R.LEAKY32).numpy()
                gb = gv * f
                o = c * PER
                row[o:o + NJ] = X @ gb
                row[o + NJ:o + 2 * NJ] = X @ xh
                row[o + 2 * NJ], row[o + 2 * NJ + 1] = gb.sum(), (gb * xh).sum()
            row[Cout * PER:Cout * PER + NJ] = X.sum(1)
            if Cin == 1:
                row[Cout * PER + NJ:] = (X @ X.T).reshape(-1)
            r = b * tiles + t
            if defect == "row_of_image_1_at_b_times_1":
                r = b * 1 + t
            part[r] = row
    return part


def _case_for(defect):
    """the smallest shape at which the defect changes a sum; g without zeros and pixels >= 1 so that every pixel counts"""
    kw = dict(density=1.0, pmin=1, pmax=9, seed=1)
    if defect in (None, "tail_pixel_twice", "first_pixel_of_tile_2_dropped", "row_of_image_1_at_b_times_1"):
        return R.make_case(2, 1, 16, 132, 252, 2, "mixed", signs=True, **kw)       # two tiles: 8192 + 124 pixels
    if defect == "right_column_without_kw2":
        # stride 2, even image width 250, ODD output width 125: the last output column's kw = 2 tap is image column 249, inside the image
        return R.make_case(1, 1, 8, 6, 250, 2, "mixed", signs=True, **kw)
    if defect == "bottom_row_reads_kh2":
        # stride 1, even height: the bottom row's kh = 2 tap is row IH -- in memory the next image's first row
        return R.make_case(2, 3, 5, 4, 6, 1, "mixed", **kw)
    if defect == "unit_1_from_unit_0":
        return R.make_case(1, 1, 20, 5, 7, 1, "mixed", **kw)
    if defect == "lane_c_plus_1":
        return R.make_case(1, 3, 8, 5, 7, 2, "none", **kw)     # (a full unit: lane 7 wraps to lane 0)
    assert defect == "sign_bits_4_7_and_8_11_swapped"
    return R.make_case(1, 1, 16, 4, 8, 2, "mixed", signs=True, **kw)


_CASES = {}


def _shared(defect):
    key = id(_case_for) if defect in (None, "tail_pixel_twice", "first_pixel_of_tile_2_dropped", "row_of_image_1_at_b_times_1") else defect
    if key not in _CASES:
        case = _case_for(defect)
        _CASES[key] = (case,) + R.case_reference(case)
    return _CASES[key]


@pytest.mark.parametrize("like", [None] + DEFECTS[2:7])
def test_standin_passes_the_helper(like):
    """every case of the defect tests, without the defect.  fp64 on these inputs: every order of summation gives the same bits only
    where no float32(0.01) product enters ("none"); elsewhere fp64's own rounding is held to the helper's bound with D = 1 (2^-24 of the
    sum of magnitudes: nine orders of magnitude above an fp64 sum's error, nine below a dropped term)"""
    case, rows, mags = _shared(like)
    exact = case["mode"] == "none"
    ratio = R.compare_sweep(standin_rows(case), rows, mags, case["Cin"], case["Cout"], exact=exact, D=1, what=f"stand-in for {like}", quantum=0.5)
    assert ratio < 1e-6


@pytest.mark.parametrize("defect", DEFECTS)
def test_helper_names_the_column_of_a_seeded_defect(defect):
    case, rows, mags = _shared(defect)
    exact = case["mode"] == "none"
    with pytest.raises(AssertionError) as ei:
        R.compare_sweep(standin_rows(case, defect), rows, mags, case["Cin"], case["Cout"], exact=exact, D=45, what=defect, quantum=0.5)
    msg = str(ei.value)
    print(defect, "->", msg[:220])
    assert msg.startswith(defect) and "column " in msg
    col = msg.split("column ")[1].split(":")[0].split(" ")[0]
    assert col.split("[")[0] in ("A1", "A2", "S1", "S2", "P", "G"), msg
    if defect == "sign_bits_4_7_and_8_11_swapped":
        c = int(col.split("c=")[1].split("]")[0])
        assert 4 <= c < 12, msg          # only the channels whose bits moved
    if defect == "unit_1_from_unit_0":
        assert 8 <= int(col.split("c=")[1].split("]")[0]) < 16, msg
    if defect == "row_of_image_1_at_b_times_1":
        assert "never written" in msg    # the last row stays poisoned


def test_helper_checks_zero_and_unwritten_columns():
    case, rows, mags = _shared(None)
    Cin, Cout = case["Cin"], case["Cout"]
    a2, pg = R.sweep_columns(Cin, Cout, "A2"), R.sweep_columns(Cin, Cout, "P") + R.sweep_columns(Cin, Cout, "G")
    part = standin_rows(case)
    part[:, a2] = np.nan
    with pytest.raises(AssertionError, match=r"column A2\[c=0\]\[j=0\] of partial row 0 was never written"):
        R.compare_sweep(part, rows, mags, Cin, Cout, exact=False, D=45, what="x")
    with pytest.raises(AssertionError, match=r"column P\[j=0\] of partial row 0 must be exactly zero"):
        R.compare_sweep(part, rows, mags, Cin, Cout, exact=False, D=45, what="x", unwritten=a2, zero=pg)
    part[:, pg] = 0.0
    R.compare_sweep(part, rows, mags, Cin, Cout, exact=False, D=45, what="x", unwritten=a2, zero=pg)
    with pytest.raises(AssertionError, match="precondition"):
        R.compare_sweep(part, rows, mags * 1e4, Cin, Cout, exact=True, D=45, what="x", unwritten=a2, zero=pg)
