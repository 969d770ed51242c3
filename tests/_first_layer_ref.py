"""The first layer (yogo_amd/csrc/conv_first.hip) restated in plain fp64 on the CPU, from the formulas of that file's comment blocks and
not from its loops; the comparison helper the GPU tests hold the kernels with (tests/test_gpu_first_layer_edges.py); and the input
generator both they and the host tests (tests/test_first_layer_ref_host.py) use.

  patches      patch_j = F.unfold(x, 3, padding=1, stride=s), j = (ci * 3 + kh) * 3 + kw
  forward      pre = W . patch + bias,  y = act(pre) * chan_scale[b][c],  per channel sum pre and sum pre^2
  plain wgrad  dW[c][j] = sum g[c] patch_j, the bias gradient sum g[c] as the last column: [Cout][9 Cin + 1]
  fused sweep  xh = (z - mean) * invstd,  gb = g * act'(gamma * xh + beta)   (the sign of gamma * xh + beta from a sign map when one is given)
               A1[c][j] = sum gb patch_j   A2[c][j] = sum xh patch_j   S1[c] = sum gb   S2[c] = sum gb xh   P[j] = sum patch_j
               G[j][j'] = sum patch_j patch_j'  (Cin = 1 only); columns [Cout * (2 NJ + 2) + NJ (+ NJ * NJ)], per channel A1, A2, S1, S2
  finalize     N = B OH OW, c1 = gamma * invstd:  dW[c][j] = c1 (A1 - S1 / N P[j] - S2 / N A2)  [batch statistics],  c1 A1  [eval];
               dgamma = S2, dbeta = S1; Gram form A2[c][j] = invstd (sum_j' W[c][j'] G[j'][j] - mean P[j]);
               derived S2 = invstd (W[c] . A1[c] - mean S1)  (z = W . patch, no conv bias); every output clamped to +-clip when clip > 0
Next to every sum stands the same sum over magnitudes: the scale of every rounding bound, and the precondition of the exact cases."""
import numpy as np
import torch
import torch.nn.functional as F

ACT_NONE, ACT_LEAKY, ACT_SILU = 0, 1, 2
LEAKY32 = float(np.float32(0.01))   # the slope the kernels multiply with
TILE_SWEEP = 8192                   # output pixels per partial row of the weight-gradient and fused sweeps (CF_THREADS * CFW_PPT)
TILE_FWD = 1024                     # ... of the forward kernels' statistics rows (CF_THREADS * CF_PPT)
U24 = 2.0 ** -24
SILU_DMAX = 1.0998                  # max |d silu / dv| (at v = 2.3994): the magnitude of a SiLU term is |g| times this


# ---- layouts --------------------------------------------------------------------------------------------------------------------
def sign_bits(signs_u8, H, W):
    """[B][H*W][2] bytes -> bool [B][16][H][W]: byte h of a pixel: bit i = channel 4h + i, bit 4 + i = channel 8 + 4h + i (include/yogo_hip.h)"""
    s = signs_u8.reshape(-1, H, W, 2).to(torch.int32)
    out = torch.zeros(s.shape[0], 16, H, W, dtype=torch.bool)
    for h in range(2):
        for i in range(4):
            out[:, 4 * h + i] = ((s[..., h] >> i) & 1).bool()
            out[:, 8 + 4 * h + i] = ((s[..., h] >> (4 + i)) & 1).bool()
    return out


def pack_sign_bits(pos):
    """the inverse of sign_bits: bool [B][C <= 16][H][W] -> uint8 [B][H*W*2] (bits of absent channels zero)"""
    B, C, H, W = pos.shape
    s = torch.zeros(B, H, W, 2, dtype=torch.int32)
    for c in range(C):
        h, i = (c >> 2) & 1, (c & 3) + (4 if c >= 8 else 0)
        s[..., h] |= pos[:, c].to(torch.int32) << i
    return s.to(torch.uint8).reshape(B, H * W * 2)


def out_size(IH, IW, stride):
    return (IH - 1) // stride + 1, (IW - 1) // stride + 1


def to8c(t, pad=0.0):
    """fp32 NCHW [B][C][H][W] -> bf16 NCHW8c [B][Mb][H][W][8], Mb = 2 * ceil(C / 16); the padding channels hold ``pad``"""
    B, C, H, W = t.shape
    Mb = ((C + 15) // 16) * 2
    full = torch.full((B, Mb * 8, H, W), float(pad), dtype=torch.float32)
    full[:, :C] = t
    return full.reshape(B, Mb, 8, H, W).permute(0, 1, 3, 4, 2).contiguous().to(torch.bfloat16)


def from8c(t8, C=None):
    """bf16 NCHW8c [B][Mb][H][W][8] -> fp32 NCHW [B][Mb * 8 or C][H][W]"""
    B, Mb, H, W, _ = t8.shape
    full = t8.float().permute(0, 1, 4, 2, 3).reshape(B, Mb * 8, H, W)
    return full if C is None else full[:, :C].contiguous()


def sweep_layout(Cin, Cout):
    NJ = 9 * Cin
    PER = 2 * NJ + 2
    return NJ, PER, Cout * PER + NJ + (NJ * NJ if Cin == 1 else 0)


def column_name(col, Cin, Cout):
    NJ, PER, ncol = sweep_layout(Cin, Cout)
    assert 0 <= col < ncol, col
    if col < Cout * PER:
        c, k = divmod(col, PER)
        if k < NJ:
            return f"A1[c={c}][j={k}]"
        if k < 2 * NJ:
            return f"A2[c={c}][j={k - NJ}]"
        return f"S1[c={c}]" if k == 2 * NJ else f"S2[c={c}]"
    k = col - Cout * PER
    return f"P[j={k}]" if k < NJ else f"G[{(k - NJ) // NJ}][{(k - NJ) % NJ}]"


def sweep_columns(Cin, Cout, which):
    """the column indices of one family: "A1", "A2", "S1", "S2", "P", "G" """
    NJ, PER, ncol = sweep_layout(Cin, Cout)
    return [c for c in range(ncol) if column_name(c, Cin, Cout).startswith(which)]


# ---- the mathematics ------------------------------------------------------------------------------------------------------------
def patches(x, stride):
    """[B][Cin][IH][IW] -> fp64 [B][9 Cin][OH * OW]"""
    return F.unfold(x.double(), 3, padding=1, stride=stride)


def act_apply(v, act, slope=0.01):
    if act == ACT_LEAKY:
        return torch.where(v > 0, v, slope * v)
    if act == ACT_SILU:
        return v * torch.sigmoid(v)
    return v


def act_deriv(v, act, slope=0.01):
    if act == ACT_LEAKY:
        return torch.where(v > 0, torch.ones_like(v), torch.full_like(v, slope))
    if act == ACT_SILU:
        s = torch.sigmoid(v)
        return s * (1 + v * (1 - s))
    return torch.ones_like(v)


def forward(x, w, bias, chan_scale, stride, act, slope=0.01):
    """pre, y fp64 [B][Cout][OH][OW]"""
    B, Cin, IH, IW = x.shape
    OH, OW = out_size(IH, IW, stride)
    Cout = w.shape[0]
    pre = torch.einsum("cj,bjl->bcl", w.double().reshape(Cout, -1), patches(x, stride))
    if bias is not None:
        pre = pre + bias.double()[None, :, None]
    y = act_apply(pre, act, slope)
    if chan_scale is not None:
        y = y * chan_scale.double().reshape(B, Cout, 1)
    return pre.reshape(B, Cout, OH, OW), y.reshape(B, Cout, OH, OW)


def _tiles(npix, tile):
    return [(p0, min(p0 + tile, npix)) for p0 in range(0, npix, tile)]


def forward_stat_rows(pre, tile=TILE_FWD):
    """fp64 [B * tiles][Cout][2] = (sum pre, sum pre^2) per tile of ``tile`` pixels, and the same over magnitudes"""
    B, Cout = pre.shape[:2]
    f = pre.reshape(B, Cout, -1)
    rows, mags = [], []
    for b in range(B):
        for p0, p1 in _tiles(f.shape[2], tile):
            t = f[b, :, p0:p1]
            rows.append(torch.stack((t.sum(1), (t * t).sum(1)), 1))
            mags.append(torch.stack((t.abs().sum(1), (t * t).sum(1)), 1))
    return torch.stack(rows), torch.stack(mags)


def wgrad_rows(x, g, stride, tile=TILE_SWEEP):
    """fp64 [B * tiles][Cout][9 Cin + 1] (the bias gradient as the last column) and the same over magnitudes"""
    B, Cout = g.shape[:2]
    pt = patches(x, stride)
    gf = g.double().reshape(B, Cout, -1)
    rows, mags = [], []
    for b in range(B):
        for p0, p1 in _tiles(gf.shape[2], tile):
            gt, ptt = gf[b, :, p0:p1], pt[b, :, p0:p1]
            rows.append(torch.cat((gt @ ptt.t(), gt.sum(1, keepdim=True)), 1))
            mags.append(torch.cat((gt.abs() @ ptt.abs().t(), gt.abs().sum(1, keepdim=True)), 1))
    return torch.stack(rows), torch.stack(mags)


def sweep_terms(g, z, mean, invstd, gamma, beta, act, signs=None, slope=0.01):
    """xh, gb and |gb| (fp64 [B][Cout][OH][OW]).  z = None: the sweep sees no z (xh = 0; the sign map decides the LeakyReLU side)."""
    B, Cout, OH, OW = g.shape
    bc = lambda t: t.double().reshape(1, Cout, 1, 1)
    xh = torch.zeros(B, Cout, OH, OW, dtype=torch.float64) if z is None else (z.double() - bc(mean)) * bc(invstd)
    if signs is not None and act == ACT_LEAKY:
        f = torch.where(sign_bits(signs, OH, OW)[:, :Cout], 1.0, slope).double()
    else:
        assert z is not None or act == ACT_NONE, "no z: the activation side must come from a sign map"
        f = act_deriv(bc(gamma) * xh + bc(beta), act, slope)
    gb = g.double() * f
    gmag = g.double().abs() * SILU_DMAX if act == ACT_SILU else gb.abs()
    return xh, gb, gmag


def sweep_rows(x, g, z, mean, invstd, gamma, beta, stride, act, signs=None, slope=0.01, tile=TILE_SWEEP):
    """the fused sweep's sums per partial row (row b * tiles + t = pixels [t * tile, (t + 1) * tile) of image b), fp64 [rows][ncol] in the
    kernels' column layout, and the same sums over magnitudes"""
    B, Cin = x.shape[:2]
    Cout = g.shape[1]
    NJ, PER, ncol = sweep_layout(Cin, Cout)
    xh, gb, gmag = sweep_terms(g, z, mean, invstd, gamma, beta, act, signs, slope)
    pt = patches(x, stride)
    flat = lambda t: t.reshape(B, Cout, -1)
    xh, gb, gmag = flat(xh), flat(gb), flat(gmag)
    rows, mags = [], []
    for b in range(B):
        for p0, p1 in _tiles(pt.shape[2], tile):
            for out, (gt, xt, ptt) in ((rows, (gb[b, :, p0:p1], xh[b, :, p0:p1], pt[b, :, p0:p1])),
                                       (mags, (gmag[b, :, p0:p1], xh[b, :, p0:p1].abs(), pt[b, :, p0:p1].abs()))):
                per = torch.cat((gt @ ptt.t(), xt @ ptt.t(), gt.sum(1, keepdim=True), (gt * xt).sum(1, keepdim=True)), 1)   # [Cout][PER]
                tail = [ptt.sum(1)] + ([(ptt @ ptt.t()).reshape(-1)] if Cin == 1 else [])
                out.append(torch.cat([per.reshape(-1)] + tail))
    rows, mags = torch.stack(rows), torch.stack(mags)
    assert rows.shape[1] == ncol
    return rows, mags


def finalize(sums, Cin, Cout, mean, invstd, gamma, w, count, training=True, gram=None, derive_s2=False, clip=0.0, mag=False):
    """sums [ncol] -> dW [Cout][9 Cin], dgamma, dbeta in fp64.  gram: the caller's P[9] + G[81] (else the row's own P / G columns);
    Cin = 1 takes A2 from the Gram matrix, Cin = 3 from its columns.  mag = True: the same expression with every term replaced by its
    magnitude (M of the rounding bound; no clamp)."""
    NJ, PER, ncol = sweep_layout(Cin, Cout)
    f = (lambda t: t.double().abs()) if mag else (lambda t: t.double())
    sub = (lambda a, b: a + b) if mag else (lambda a, b: a - b)
    if derive_s2 and mag:   # the kernel forms the derived S2 in double: it contributes its final rounding only, so its magnitude is its value's
        s2_value = finalize(sums, Cin, Cout, mean, invstd, gamma, w, count, training, gram, True)[1].abs()
    sums = f(sums)
    sc = sums[: Cout * PER].reshape(Cout, PER)
    A1, A2, S1, S2 = sc[:, :NJ], sc[:, NJ:2 * NJ], sc[:, 2 * NJ], sc[:, 2 * NJ + 1]
    pg = f(gram) if gram is not None else sums[Cout * PER:]
    P = pg[:NJ]
    W, mu, isd, ga = f(w).reshape(Cout, NJ), f(mean), f(invstd), f(gamma)
    if derive_s2:
        S2 = s2_value if mag else isd * sub((W * A1).sum(1), mu * S1)
    c1 = ga * isd
    if training:
        if Cin == 1:
            G = pg[NJ:NJ + NJ * NJ].reshape(NJ, NJ)
            A2 = isd[:, None] * sub(W @ G, mu[:, None] * P[None])
        dW = c1[:, None] * sub(sub(A1, S1[:, None] / count * P[None]), S2[:, None] / count * A2)
    else:
        dW = c1[:, None] * A1
    dgamma, dbeta = S2, S1
    if clip > 0 and not mag:
        dW, dgamma, dbeta = dW.clamp(-clip, clip), dgamma.clamp(-clip, clip), dbeta.clamp(-clip, clip)
    return dW, dgamma, dbeta


# ---- the comparison helper ------------------------------------------------------------------------------------------------------
def compare_sweep(part, ref_rows, ref_mags, Cin, Cout, exact, D, what, unwritten=(), zero=(), sums=None, quantum=1.0):
    """``part``: the partial rows a sweep wrote into a NaN-poisoned buffer, [rows][ncol]; ``ref_rows`` / ``ref_mags``: sweep_rows().
      every column of every row is written (no NaN), except the columns ``unwritten`` (the A2 columns of the Gram kernels: not compared);
      the columns ``zero`` are exactly zero in every row (P / G of the routes with a caller-held Gram matrix, the sign-map sweeps' S2);
      exact: every row, and the rows summed in fp64, equal the reference bit for bit -- precondition, asserted here: every column's sum
        of magnitudes, per row and over all rows, is below 2^24 quanta (``quantum``: the largest power of two every term is a multiple of);
      else: the rows summed in fp64 are within D * 2^-24 * sum |terms| of the reference, per column;
      ``sums`` (the output of yogo_partials_reduce, [ncol]) is held the same way.
    Every failure names the column.  Returns the largest measured |d| / (2^-24 sum |terms|)."""
    part = torch.as_tensor(part).double()
    R, ncol = ref_rows.shape
    assert tuple(part.shape) == (R, ncol), (what, "partial rows", tuple(part.shape), "expected", (R, ncol))
    name = lambda c: column_name(c, Cin, Cout)
    skip = torch.zeros(ncol, dtype=torch.bool)
    skip[list(unwritten)] = True
    zero = list(zero)
    want, mags = ref_rows.clone(), ref_mags.clone()
    want[:, zero] = 0.0
    mags[:, zero] = 0.0
    mags[:, skip] = 0.0    # (never summed by the kernel)
    nan = torch.isnan(part) & ~skip[None]
    if bool(nan.any()):
        r, c = [int(v) for v in nan.nonzero()[0]]
        raise AssertionError(f"{what}: column {name(c)} of partial row {r} was never written, or was formed from a padding channel's NaN ({int(nan.sum())} NaN values)")
    keep = ~skip
    if zero:
        bad = part[:, zero] != 0
        if bool(bad.any()):
            r, k = [int(v) for v in bad.nonzero()[0]]
            raise AssertionError(f"{what}: column {name(zero[k])} of partial row {r} must be exactly zero, is {float(part[r, zero[k]])}")
    tot_want, tot_mag = want.sum(0), mags.sum(0)
    tot_got = part.sum(0)
    if exact:
        lim = 2.0 ** 24 * quantum
        worst = int(tot_mag.argmax())
        assert float(tot_mag.max()) < lim, (f"{what}: precondition: column {name(worst)} sums magnitudes {float(tot_mag[worst]):.4g} >= 2^24 quanta "
                                            f"({lim:.4g}) over all rows: lower the pixel range")
        d = (part - want).abs() * keep[None]
        if bool((d > 0).any()):
            r, c = [int(v) for v in (d == d.max()).nonzero()[0]]
            raise AssertionError(f"{what}: column {name(c)} of partial row {r}: got {float(part[r, c])!r}, fp64 says {float(want[r, c])!r} "
                                 f"(exact case: every summation order gives this)")
    checks = [("rows summed in fp64", tot_got)] + ([("yogo_partials_reduce", torch.as_tensor(sums).double())] if sums is not None else [])
    ratio = 0.0
    for label, got in checks:
        assert got.shape == (ncol,), (what, label, tuple(got.shape))
        nn = torch.isnan(got) & keep
        if bool(nn.any()):
            raise AssertionError(f"{what}: {label}: column {name(int(nn.nonzero()[0]))} is NaN")
        d = torch.where(keep, (got - tot_want).abs(), torch.zeros(ncol, dtype=torch.float64))
        if exact:
            tol = torch.zeros(ncol, dtype=torch.float64)
        else:
            tol = D * U24 * tot_mag
        bad = d > tol
        if bool(bad.any()):
            c = int(((d - tol) * bad).argmax())
            raise AssertionError(f"{what}: {label}: column {name(c)}: got {float(got[c])!r}, fp64 says {float(tot_want[c])!r}, |d| = {float(d[c]):.4g} "
                                 f"> {'0 (exact case)' if exact else f'{D} * 2^-24 * sum|terms| = {float(tol[c]):.4g}'} (sum|terms| {float(tot_mag[c]):.4g})")
        nz = tot_mag > 0
        if bool(nz.any()):
            ratio = max(ratio, float((d[nz] / (U24 * tot_mag[nz])).max()))
    return ratio


def exact_precondition(mags, Cin, Cout, quantum, what):
    """before the GPU is touched: every column's sum of magnitudes over all rows (so over each row as well) is below 2^24 quanta, so every
    partial sum of every summation order is exactly representable in fp32.  Returns the largest sum as a fraction of the limit."""
    tot = mags.sum(0)
    c = int(tot.argmax())
    lim = 2.0 ** 24 * quantum
    assert float(tot[c]) < lim, f"{what}: precondition: column {column_name(c, Cin, Cout)} sums magnitudes {float(tot[c]):.4g} >= {lim:.4g}: lower the pixel range"
    return float(tot[c]) / lim


def compare_exact(got, want, mags, what, names, quantum=1.0):
    """plain tensors of the same shape (the plain weight gradient's rows, the forward's statistics rows): precondition sum of magnitudes
    below 2^24 quanta over everything that is ever added together (``mags`` summed over dim 0), no NaN, then bit for bit.  ``names(idx)``
    names an element."""
    got = torch.as_tensor(got).double()
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    tot = mags.sum(0)
    assert float(tot.max()) < 2.0 ** 24 * quantum, f"{what}: precondition: sum of magnitudes {float(tot.max()):.4g} >= 2^24 quanta: lower the pixel range"
    nan = torch.isnan(got)
    if bool(nan.any()):
        raise AssertionError(f"{what}: {names(tuple(int(v) for v in nan.nonzero()[0]))} was never written, or was formed from a padding channel's NaN")
    d = (got - want).abs()
    if bool((d > 0).any()):
        idx = tuple(int(v) for v in (d == d.max()).nonzero()[0])
        raise AssertionError(f"{what}: {names(idx)}: got {float(got[idx])!r}, fp64 says {float(want[idx])!r} (exact case)")


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def make_case(B, Cin, Cout, IH, IW, stride, mode, in_float=False, pmax=255, pmin=0, signs=False, density=0.5, seed=0):
    """One sweep's inputs (CPU tensors).  mode:
      "none" / "allpos" / "mixed": the EXACT inputs -- pixels integers in [pmin, pmax] (float images: integer-valued, either sign), g in
        {-1, 0, 1} (a fraction ``density`` non-zero), z integers in [-3, 3], mean integers in [-1, 1], invstd in {0.5, 1, 2}, gamma in
        +-{1, 2} with every fourth channel negative, beta an odd multiple of 0.25: gamma * xh + beta is an odd multiple of 0.25, never 0.
        Every term of every sum is a multiple of 0.5 (the quantum).  "none": no activation; "allpos": LeakyReLU, beta = 1000.25 (and a
        sign map of ones) so every value is on the positive side; "mixed": LeakyReLU, both sides -- the float32(0.01) products round;
      "silu": the "mixed" inputs with SiLU;
      "random": g bf16-valued normal data, z the bf16-rounded convolution of the image with random weights, real batch statistics, gamma
        +-U(0.5, 1.5) with every fourth channel negative, beta ~ N(0, 0.5), LeakyReLU; the image is uint8 noise over a flat region.  Where
        gamma * xh + beta is within 1e-4 of zero g is set to 0: there an fp32 kernel may take the other side of the kink.
    signs = True: a sign map stands in for z (z8 is None) -- of gamma * xh + beta where that decides anything, so the z and the sign-map
    routes see the same gb.  g8 / z8: bf16 NCHW8c with the padding channels of g filled with 3.0 and those of z with NaN."""
    gen = torch.Generator().manual_seed(seed * 7919 + 31 * IH + IW + 1000 * Cout + B)
    OH, OW = out_size(IH, IW, stride)
    exact = mode != "random"
    if exact:
        lo = -pmax if in_float else pmin
        x = torch.randint(lo, pmax + 1, (B, Cin, IH, IW), generator=gen)
        g = torch.randint(0, 2, (B, Cout, OH, OW), generator=gen).float() * 2 - 1
        g = g * (torch.rand(B, Cout, OH, OW, generator=gen) < density).float()
        z = torch.randint(-3, 4, (B, Cout, OH, OW), generator=gen).float()
        mean = torch.randint(-1, 2, (Cout,), generator=gen).float()
        invstd = 2.0 ** torch.randint(-1, 2, (Cout,), generator=gen).float()
        gamma = torch.randint(1, 3, (Cout,), generator=gen).float()
        gamma[3::4] = -gamma[3::4]
        beta = (2 * torch.randint(-2, 2, (Cout,), generator=gen).float() + 1) * 0.25
        if mode == "allpos":
            beta = torch.full((Cout,), 1000.25)
        w = None
    else:
        x = torch.randint(0, 256, (B, Cin, IH, IW), generator=gen)
        x[0, :, : IH // 2] = 200
        w = (torch.randn(Cout, Cin, 3, 3, generator=gen) * 0.1).to(torch.bfloat16).float()
        g = (torch.randn(B, Cout, OH, OW, generator=gen) * 0.5).to(torch.bfloat16).float()
        z64 = F.conv2d(x.double(), w.double(), None, stride=stride, padding=1)
        z = z64.float().to(torch.bfloat16).float()
        mean = z64.mean((0, 2, 3)).float()
        invstd = (1.0 / torch.sqrt(z64.var((0, 2, 3), unbiased=False) + 1e-5)).float()
        gamma = 0.5 + torch.rand(Cout, generator=gen)
        gamma[3::4] = -gamma[3::4]
        beta = 0.5 * torch.randn(Cout, generator=gen)
    x = x.float() if in_float else x.to(torch.uint8)
    act = {"none": ACT_NONE, "silu": ACT_SILU}.get(mode, ACT_LEAKY)
    bc = lambda t: t.double().reshape(1, Cout, 1, 1)
    yb = bc(gamma) * (z.double() - bc(mean)) * bc(invstd) + bc(beta)
    if not exact:
        g = torch.where(yb.abs() < 1e-4, torch.zeros_like(g), g)
    else:
        assert float(yb.abs().min()) >= 0.25
    case = dict(B=B, Cin=Cin, Cout=Cout, IH=IH, IW=IW, OH=OH, OW=OW, stride=stride, act=act, mode=mode, in_dtype=1 if in_float else 0, x=x, g=g,
                z=z, w=w, mean=mean, invstd=invstd, gamma=gamma, beta=beta, g8=to8c(g, pad=3.0), z8=to8c(z, pad=float("nan")), signs=None,
                exact=mode in ("none", "allpos"), quantum=0.5 if exact else None)
    if signs:
        assert Cout <= 16
        case["signs"] = pack_sign_bits(yb > 0) if act == ACT_LEAKY else None
        case["z"], case["z8"] = None, None
    return case


def case_reference(case, tile=TILE_SWEEP):
    """sweep_rows() of a case, with the slope the kernels multiply with"""
    return sweep_rows(case["x"], case["g"], case["z"], case["mean"], case["invstd"], case["gamma"], case["beta"], case["stride"], case["act"],
                      signs=case["signs"], slope=LEAKY32, tile=tile)
