"""The BatchNorm, reduction, layout-conversion kernels of yogo_amd/csrc/bn.hip against the float64 reference tests/_bn_ref.py, at the
shapes where their tiling acts: one pixel, the last pixel before / first pixel after a workgroup's span (2048 pixels fp32, 1024 bf16
NCHW8c), the 64-workgroup cap, batch and channel counts that make the partial-row index b * nb + blockIdx.x a product of two factors
above 1, channel blocks that are half or all padding.

Every output and workspace is a Guarded buffer of exactly the size the `*_rows` queries report (NaN payload between sentinels): after a
call the sentinels are intact and everything that should have been written is finite.  Elementwise outputs are held per element; sums
to 4 e_ref, e_ref = the error against float64 of a plain fp32 restatement on the CPU summed in several orders (never a figure of the
kernel under test), plus derived rounding counts.  u = 2^-24 (fp32 unit roundoff), 2^-8 for bf16.  Every case prints
`[bn_edges] entry | case | d e_ref bound ratio`; one full run is kept as profiles/bn_edges.log."""
import math

import pytest
import torch

import _bn_ref as R
from _util import Guarded

pytestmark = pytest.mark.gpu

U, U16 = R.U32, R.U16
F64 = torch.float64
NONE, LEAKY, SILU = R.NONE, R.LEAKY, R.SILU
ACTS = (NONE, LEAKY, SILU)
INF = float("inf")


def H():
    from yogo_amd import _hip

    return _hip


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


EPS = f32(1e-5)
MOM = f32(0.1)


def dev(t):
    return t.contiguous().cuda()


def _c(v):
    return v.to(F64).reshape(1, -1, 1)


def gbf16(shape):
    """a Guarded bf16 tensor (through fp32 words, as the sentinels are), every bf16 element NaN"""
    n = math.prod(shape)
    assert n % 2 == 0
    G = Guarded(n // 2)
    t = G.view.view(torch.bfloat16).view(shape)
    t.fill_(float("nan"))
    return G, t


def ratio(d, bound):
    d, bound = torch.as_tensor(d, dtype=F64), torch.as_tensor(bound, dtype=F64)
    r = torch.where(bound > 0, d / bound.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, INF), torch.zeros_like(d)))
    return float(r.max())


def log(entry, case, d, e_ref, bound):
    d, e_ref, bound = float(torch.as_tensor(d).max()), float(torch.as_tensor(e_ref).max()), float(torch.as_tensor(bound).max())
    print(f"[bn_edges] {entry} | {case} | d {d:.3e} e_ref {e_ref:.3e} bound {bound:.3e}")


def log_ratio(entry, case, r):
    print(f"[bn_edges] {entry} | {case} | worst d / bound {r:.4f}")


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def sums32_orders(t2d, pieces=1):
    """fp32 sums of the rows of t2d [R][n] in four orders (torch's pairwise sum, first to last, last to first, 256 interleaved running
    sums), over ``pieces`` contiguous pieces whose totals are then added in float64.  Returns a list of [R] float64."""
    out = [0.0, 0.0, 0.0, 0.0]
    for p in torch.tensor_split(t2d, pieces, dim=1):
        n = p.shape[1]
        if n == 0:
            continue
        pad = torch.zeros(p.shape[0], (-n) % 256, dtype=torch.float32)
        inter = torch.cat([p, pad], 1).reshape(p.shape[0], -1, 256).cumsum(1)[:, -1, :].sum(1)
        for i, v in enumerate((p.sum(1), p.cumsum(1)[:, -1], p.flip(1).cumsum(1)[:, -1], inter)):
            out[i] = out[i] + v.to(F64)
    return out


# ============================================================================================================================
# apply
# ============================================================================================================================
# fp32 kernel: y = act(fmaf(fl(z - mu), sc, beta)), sc = fl(invstd * gamma).  Three roundings: the subtraction (u |z - mu|, times |sc|),
# sc (u |sc|, times |z - mu|) and the fma (u |y|, |y| <= |z - mu| |sc| + |beta|): 3 u M, M = |z - mu| |sc| + |beta|.  LeakyReLU's multiply
# by 0.01 is one more (and LeakyReLU is 1-Lipschitz, so a pre-activation next to zero cannot jump): K_INV = 4.  With stat_is_var the kernel
# forms invstd = 1 / sqrtf(var + eps): the add, the square root (which halves the add's error) and the division, correctly rounded each
# (-fhip-fp32-correctly-rounded-divide-sqrt), are 2.5 u more on sc: K_VAR = 7.
# SiLU = v / (1 + __expf(-v)): |silu'| <= 1.1 carries the pre-activation's error, and the __expf form costs 2^-22 (2 + |v|) |ref| (derived in
# tests/test_gpu_infer_teacher_forced.py above test_conv_first_fwd_bf16_against_float64; no new number).
# bf16 kernel: y = bf16(act(fmaf(z, sc, sh2))), sh2 = fmaf(-mu, sc, beta): the same three roundings (sc, sh2, the fma), but of the magnitudes
# THIS form adds up, M = |z sc| + |mu sc| + |beta|; then one bf16 rounding of the result, 2^-8 |ref| (and of the fp32 error: a factor 1 + 2^-7).
K_INV, K_VAR = 4, 7


def apply_bound(k, stat_is_var, act, bf16, ref):
    z = k["z"].to(F64)
    istd = 1.0 / torch.sqrt(_c(k["var"]) + EPS) if stat_is_var else _c(k["invstd"])
    sc = istd * _c(k["gamma"])
    if bf16:
        M = (z * sc).abs() + (_c(k["mean"]) * sc).abs() + _c(k["beta"]).abs()
    else:
        M = (z - _c(k["mean"])).abs() * sc.abs() + _c(k["beta"]).abs()
    b = (K_VAR if stat_is_var else K_INV) * U * M
    if act == SILU:
        y = (z - _c(k["mean"])) * sc + _c(k["beta"])
        b = 1.1 * b + 2.0 ** -22 * (2 + y.abs()) * ref.abs()
    if bf16:
        b = b * (1 + 2 * U16) + U16 * ref.abs()
    return b


@pytest.mark.parametrize("B,C,HW", R.f32_shapes())
def test_apply_f32(B, C, HW):
    h = H()
    st = h.stream_ptr()
    k = R.bn_case(B, C, HW, False)
    d = {n: dev(k[n]) for n in ("z", "mean", "invstd", "var", "gamma", "beta")}
    multi = HW == 2049 or (B, C) == (3, 5)
    worst = 0.0
    for act in ACTS if multi else (LEAKY,):
        for siv in (0, 1):
            y = Guarded(B * C * HW)
            h.call("yogo_bn_apply_act", d["z"], y.view, d["mean"], d["var"] if siv else d["invstd"], siv, EPS, d["gamma"], d["beta"], B, C, HW, act, st)
            y.check("bn_apply_act y")
            got = y.view.cpu().view(B, C, HW)
            assert bool(torch.isfinite(got).all()), "an output element was left unwritten"
            ref = R.apply(k["z"], k["mean"], k["var"] if siv else k["invstd"], siv, EPS, k["gamma"], k["beta"], act)
            r = ratio((got.to(F64) - ref).abs(), apply_bound(k, siv, act, False, ref))
            worst = max(worst, r)
            assert r <= 1.0, (act, siv, r)
    log_ratio("yogo_bn_apply_act", f"B={B} C={C} HW={HW}", worst)
    # yogo_bn_invstd beside it: fl(1 / fl(sqrt(fl(var + eps)))), 0.5 u + u + u <= 3 u relative
    inv = Guarded(C)
    h.call("yogo_bn_invstd", d["var"], EPS, inv.view, C, st)
    inv.check("bn_invstd")
    ref = 1.0 / torch.sqrt(k["var"].to(F64) + EPS)
    r = ratio((inv.view.cpu().to(F64) - ref).abs(), 3 * U * ref)
    log_ratio("yogo_bn_invstd", f"C={C}", r)
    assert r <= 1.0


def run_apply_bf16(h, k, z8d, siv, act):
    B, C, HW = k["z"].shape
    Cb = R.cb_of(C)
    G, y8 = gbf16((B, Cb, HW, 8))
    h.call("yogo_bn_apply_act_bf16", z8d, y8, dev(k["mean"]), dev(k["var"] if siv else k["invstd"]), siv, EPS, dev(k["gamma"]), dev(k["beta"]),
           B, C, HW, act, h.stream_ptr())
    G.check("bn_apply_act_bf16 y")
    y8 = y8.cpu()
    assert bool(torch.isfinite(y8.float()).all()), "an output unit was left unwritten"
    assert bool((R.pad_lanes(y8, C) == 0).all()), "output padding lanes not zero"
    return y8


@pytest.mark.parametrize("B,C,HW", R.bf16_shapes())
def test_apply_bf16(B, C, HW):
    h = H()
    k = R.bn_case(B, C, HW, True)
    z8d = dev(R.to8c(k["z"]))
    multi = HW == 1025 or (B, C) == (3, 5)
    worst = 0.0
    for act in ACTS if multi else (LEAKY,):
        for siv in (0, 1):
            got = R.from8c(run_apply_bf16(h, k, z8d, siv, act), C)
            ref = R.apply(k["z"], k["mean"], k["var"] if siv else k["invstd"], siv, EPS, k["gamma"], k["beta"], act)
            r = ratio((got.to(F64) - ref).abs(), apply_bound(k, siv, act, True, ref))
            worst = max(worst, r)
            assert r <= 1.0, (act, siv, r)
    log_ratio("yogo_bn_apply_act_bf16", f"B={B} C={C} HW={HW}", worst)


# ============================================================================================================================
# backward
# ============================================================================================================================
def run_bwd(h, bf16, k, gd, zd, act, training, clip, inplace=False, head=None):
    """gd / zd: device inputs (fp32 [B][C][HW] or bf16 8c).  Returns dz (CPU; fp32 [B][C][HW] or bf16 8c), dgamma, dbeta, sums, part.
    head = (gh 8c, w, P) on the device: yogo_bn_bwd_bf16_head forms g from them (gd is not read; dz must not alias gh: never in place)."""
    B, C, HW = k["z"].shape
    st = h.stream_ptr()
    rows = h.query_ints("yogo_bn_bwd_bf16_rows" if bf16 else "yogo_bn_bwd_rows", 1, B, HW)[0]
    assert rows == B * max(1, min(64, -(-HW // (1024 if bf16 else 2048))))
    part, sums, dg, db = Guarded(rows * C * 2), Guarded(2 * C), Guarded(C), Guarded(C)
    if bf16:
        G, dz = gbf16(tuple(zd.shape))
    else:
        G = Guarded(B * C * HW)
        dz = G.view.view(B, C, HW)
    if inplace:
        dz.copy_(gd)
    if head is not None:
        assert bf16 and not inplace
        h.call("yogo_bn_bwd_bf16_head", head[0], head[1], head[2], zd, dz, dev(k["mean"]), dev(k["invstd"]), dev(k["gamma"]), dev(k["beta"]), act,
               dg.view, db.view, part.view, sums.view, B, C, HW, training, clip, st)
    else:
        h.call("yogo_bn_bwd_bf16" if bf16 else "yogo_bn_bwd", dz if inplace else gd, zd, dz, dev(k["mean"]), dev(k["invstd"]), dev(k["gamma"]),
               dev(k["beta"]), act, dg.view, db.view, part.view, sums.view, B, C, HW, training, clip, st)
    for b_, w in ((G, "dz"), (part, "part"), (sums, "sums"), (dg, "dgamma"), (db, "dbeta")):
        b_.check("bn_bwd " + w)
    out = dict(dz=dz.cpu(), dgamma=dg.view.cpu(), dbeta=db.view.cpu(), sums=sums.view.cpu(), part=part.view.cpu())
    for n, v in out.items():
        assert bool(torch.isfinite(v.float()).all()), f"{n}: an element that the call must write was left unwritten (or is not finite)"
    return out


def bwd_reference(k, act):
    """everything of the reference that does not depend on training / clip: float64 terms, the edge elements, e_ref and the bounds of
    the two sums"""
    z, g = k["z"].to(F64), k["g"].to(F64)
    mu, istd, ga, be = _c(k["mean"]), _c(k["invstd"]), _c(k["gamma"]), _c(k["beta"])
    xh = (z - mu) * istd
    y = xh * ga + be
    f = R.act_factor(y, act)
    ge = g * f
    S1, S2 = ge.sum((0, 2)), (ge * xh).sum((0, 2))
    C = z.shape[1]
    edge = R.leaky_edge_mask(k["z"], k["mean"], k["invstd"], k["gamma"], k["beta"]) if act == LEAKY else torch.zeros_like(z, dtype=torch.bool)
    assert int(edge.sum()) <= R.EDGE_CAP * edge.numel()
    # the activation factor's own error (SiLU only; the LeakyReLU branch is handled through `edge`): s = 1 / (1 + __expf(-y)) is within
    # E s, E = 2^-22 (2 + |y|) (the bound quoted above); f = s t, t = 1 + y (1 - s): dt <= |y| E s + 3 u (1 + |y|), so
    # df <= E s t + s dt + u |f| <= E (1 + 2 |y|) + 4 u (1 + |y|); and |f'| <= 0.5 carries the pre-activation's own error dy <= 4 u (|xh ga| + |be|)
    if act == SILU:
        E = 2.0 ** -22 * (2 + y.abs())
        df = E * (1 + 2 * y.abs()) + 4 * U * (1 + y.abs()) + 0.5 * 4 * U * ((xh * ga).abs() + be.abs())
    else:
        df = torch.zeros_like(y)
    # e_ref: the plain fp32 restatement (the branch of the float64 reference, so that e_ref is the error of the fp32 arithmetic alone)
    z32, g32 = k["z"], k["g"]
    m32, i32, ga32, be32 = (k[n].reshape(1, -1, 1) for n in ("mean", "invstd", "gamma", "beta"))
    xh32 = (z32 - m32) * i32
    y32 = xh32 * ga32 + be32
    if act == SILU:
        s32 = torch.sigmoid(y32)
        f32_ = s32 * (1 + y32 * (1 - s32))
    else:
        f32_ = f.float()
    ge32 = g32 * f32_
    t2d = lambda t: t.permute(1, 0, 2).reshape(C, -1)
    # (the largest over the orders AND the channels, as tests/test_gpu_head_bn_fused.py takes it: one channel's four orders can all be lucky)
    e1 = torch.stack([(s - S1).abs() for s in sums32_orders(t2d(ge32))]).max()
    e2 = torch.stack([(s - S2).abs() for s in sums32_orders(t2d(ge32 * xh32))]).max()
    # bound of a sum: 4 e_ref (the spread between orders) + the elements whose LeakyReLU branch may go either way (0.99 |g|, 0.99 |g xhat|)
    # + the final rounding to fp32 of the fp64 total and the sum's own last rounding (2 u |S|) + the four roundings of ONE element's
    # chain (a restatement of a handful of elements can reproduce the kernel exactly by luck: e_ref = 0) + SiLU's factor error, summed
    gabs, gxabs = (g.abs() * edge).sum((0, 2)), ((g * xh).abs() * edge).sum((0, 2))
    b1 = 4 * e1 + 0.99 * gabs + 2 * U * S1.abs() + 4 * U * ge.abs().amax((0, 2)) + (g.abs() * df).sum((0, 2))
    b2 = 4 * e2 + 0.99 * gxabs + 2 * U * S2.abs() + 4 * U * (ge * xh).abs().amax((0, 2)) + ((g * xh).abs() * df).sum((0, 2))
    return dict(xh=xh, y=y, f=f, ge=ge, S1=S1, S2=S2, e1=e1, e2=e2, b1=b1, b2=b2, edge=edge, df=df, g=g)


def dz_candidates(k, rf, training, bf16):
    """[(dz64, bound)]: the reference, and for LeakyReLU the same with the OTHER factor on the elements within tau of the branch.
    fp32 kernel: dz = gi * (gv - mg - xh * mgx), gi = fl(ga * is), gv = fl(g * f), mg = fl(sum_g * inv_count), xh = fl(fl(z - mu) * is):
      gv: |g| (df + u |f|);  mg, mgx: the kernel's OWN fp32 sums, within b1, b2 of the reference's, over n, plus 2 u;  xh: 2 u |xh| (times |S2 / n|);
      the product, the two subtractions, gi and the last multiply: 8 u of |ge| + |S1 / n| + |xh S2 / n| covers them with room.
    bf16 kernel: one bf16 rounding of that (2^-8 |dz|, and of the fp32 error: a factor 1 + 2^-7)."""
    xh, g, S1, S2 = rf["xh"], rf["g"], rf["S1"], rf["S2"]
    n = g.shape[0] * g.shape[2]
    gi = _c(k["gamma"]) * _c(k["invstd"])
    out = []
    for alt in (False, True):
        f = rf["f"]
        if alt:
            if not bool(rf["edge"].any()):
                break
            f = torch.where(rf["edge"], 1.0 + R.LEAKY_SLOPE - f, f)
        ge = g * f
        mag = ge.abs()
        b = g.abs() * (rf["df"] + U * f.abs())
        if training:
            dz = gi * (ge - _c(S1 / n) - xh * _c(S2 / n))
            b = b + _c(rf["b1"]) / n + xh.abs() * _c(rf["b2"]) / n
            mag = mag + _c(S1 / n).abs() + (xh * _c(S2 / n)).abs()
        else:
            dz = gi * ge
        b = gi.abs() * (b + 8 * U * mag)
        if bf16:
            b = b * (1 + 2 * U16) + U16 * dz.abs()
        out.append((dz, b))
    return out


def branch_disagreements(k, bf16):
    """elements whose LeakyReLU branch the forward kernel and the backward kernel choose differently, from an exact emulation of the two fp32
    expressions (a product of two fp32 values is exact in float64 and the sign of the sum survives its rounding):
    forward fmaf(fl(z - mu), sc, beta) [fp32] / fmaf(z, sc, fmaf(-mu, sc, beta)) [bf16]; backward fmaf(fl(fl(z - mu) * is), gamma, beta)"""
    z = k["z"]
    mu, istd, ga, be = (k[n].reshape(1, -1, 1) for n in ("mean", "invstd", "gamma", "beta"))
    sc = istd * ga
    zmu = z - mu
    if bf16:
        sh2 = (-mu.double() * sc.double() + be.double()).float()
        fwd = z.double() * sc.double() + sh2.double() > 0
    else:
        fwd = zmu.double() * sc.double() + be.double() > 0
    bwd = (zmu * istd).double() * ga.double() + be.double() > 0
    return int((fwd != bwd).sum())


def check_bwd(entry, case, k, rf, out, act, training, clip, bf16):
    C = k["z"].shape[1]
    S1, S2, b1, b2 = rf["S1"], rf["S2"], rf["b1"], rf["b2"]
    sums = out["sums"].to(F64)
    d1, d2 = (sums[:C] - S1).abs(), (sums[C:] - S2).abs()
    log(entry + " dbeta", case, d1, rf["e1"], b1)
    log(entry + " dgamma", case, d2, rf["e2"], b2)
    assert bool((d1 <= b1).all()) and bool((d2 <= b2).all()), ("the unclamped sums", d1, b1, d2, b2)
    for got, S, b, what in ((out["dbeta"].to(F64), S1, b1, "dbeta"), (out["dgamma"].to(F64), S2, b2, "dgamma")):
        want = S.clamp(-clip, clip) if clip > 0 else S
        assert bool(((got - want).abs() <= b).all()), (what, got, want, b)
        if clip > 0:
            hi, lo = S > clip + b, S < -clip - b
            assert bool((got[hi] == clip).all()) and bool((got[lo] == -clip).all()), (what, "a binding clip must give exactly +-clip")
            assert float(got.abs().max()) <= clip
    dz = out["dz"]
    if bf16:
        assert bool((R.pad_lanes(dz, C) == 0).all()), "dz padding lanes not zero"
        dz = R.from8c(dz, C)
    dz = dz.to(F64)
    cands = dz_candidates(k, rf, training, bf16)
    ok = torch.zeros_like(dz, dtype=torch.bool)
    r_main = None
    for i, (ref, b) in enumerate(cands):
        within = (dz - ref).abs() <= b
        ok |= within if i == 0 else (within & rf["edge"])
        if i == 0:
            r_main = torch.where(rf["edge"], torch.zeros_like(dz), (dz - ref).abs() / b.clamp_min(1e-300))
    nbad = int((~ok).sum())
    r = float(r_main.max())
    assert nbad == 0, (entry, case, "dz elements outside their bound", nbad, r)
    return r


BWD_COMBOS = [(a, t, c) for a in ACTS for t in (1, 0) for c in (False, True)]


def _bwd_case(bf16, B, C, HW):
    h = H()
    entry = "yogo_bn_bwd_bf16" if bf16 else "yogo_bn_bwd"
    k = R.bn_case(B, C, HW, bf16)
    if bf16:
        gd, zd = dev(R.to8c(k["g"])), dev(R.to8c(k["z"]))
    else:
        gd, zd = dev(k["g"]), dev(k["z"])
    multi = HW == (1025 if bf16 else 2049)
    combos = BWD_COMBOS if multi else [(LEAKY, 1, False)]
    ndis = branch_disagreements(k, bf16)
    print(f"[bn_edges] {entry} | B={B} C={C} HW={HW} | forward / backward LeakyReLU branch disagreements: {ndis} of {k['z'].numel()}")
    worst = 0.0
    refs = {}
    for act, training, clipped in combos:
        if act not in refs:
            refs[act] = bwd_reference(k, act)
        rf = refs[act]
        clip = 0.0
        if clipped:
            if C < 5:
                continue
            clip = R.clip_both_signs(torch.cat([rf["S2"], rf["S1"]]))
        case = f"B={B} C={C} HW={HW} act={act} training={training} clip={clip:.4g}"
        out = run_bwd(h, bf16, k, gd, zd, act, training, clip)
        worst = max(worst, check_bwd(entry, case, k, rf, out, act, training, clip, bf16))
        if multi or (B, C) == (3, 5):
            again = run_bwd(h, bf16, k, gd, zd, act, training, clip)
            inpl = run_bwd(h, bf16, k, gd, zd, act, training, clip, inplace=True)
            for n in ("dz", "dgamma", "dbeta", "sums", "part"):
                assert torch.equal(bits(out[n]), bits(again[n])), (case, n, "a second identical call gave other bits")
                assert torch.equal(bits(out[n]), bits(inpl[n])), (case, n, "in place (dz == g) differs from out of place")
    log_ratio(entry + " dz", f"B={B} C={C} HW={HW}", worst)


@pytest.mark.parametrize("B,C,HW", R.f32_shapes())
def test_bwd_f32(B, C, HW):
    _bwd_case(False, B, C, HW)


@pytest.mark.parametrize("B,C,HW", R.bf16_shapes())
def test_bwd_bf16(B, C, HW):
    _bwd_case(True, B, C, HW)


@pytest.mark.parametrize("B,C,P,HW", R.head_shapes())
def test_bwd_bf16_head(B, C, P, HW):
    """yogo_bn_bwd_bf16_head through the checker of yogo_bn_bwd_bf16: gh and w are small integers (R.head_case), so the g the kernel forms
    with its MFMA and rounds to bf16 is exactly k["g"] and every bound of check_bwd holds unchanged.  The shapes walk the 16-pixel stripes
    and their `px < HW` guards, one operand half and both (P <= 8, P > 8), one and several channel pairs, the 64-workgroup cap."""
    h = H()
    entry = "yogo_bn_bwd_bf16_head"
    k = R.head_case(B, C, P, HW)
    zd = dev(R.to8c(k["z"]))
    gh8 = R.to8c(k["gh"])
    assert gh8.shape == (B, 2, HW, 8)
    head = (dev(gh8), dev(k["w"]), P)
    multi = HW == 1025
    combos = BWD_COMBOS if multi else [(LEAKY, 1, False)]
    worst = 0.0
    refs = {}
    g8d = None
    for act, training, clipped in combos:
        if act not in refs:
            refs[act] = bwd_reference(k, act)
        rf = refs[act]
        clip = R.clip_both_signs(torch.cat([rf["S2"], rf["S1"]])) if clipped else 0.0
        case = f"B={B} C={C} P={P} HW={HW} act={act} training={training} clip={clip:.4g}"
        out = run_bwd(h, True, k, None, zd, act, training, clip, head=head)
        worst = max(worst, check_bwd(entry, case, k, rf, out, act, training, clip, True))
        again = run_bwd(h, True, k, None, zd, act, training, clip, head=head)
        for n in ("dz", "dgamma", "dbeta", "sums", "part"):
            assert torch.equal(bits(out[n]), bits(again[n])), (case, n, "a second identical call gave other bits")
        if training == 0 and act in (NONE, LEAKY):
            # both kernels compute sc * (ge - 0 - xh * 0) = sc * ge from the same g, under either contraction
            if g8d is None:
                g8d = dev(R.to8c(k["g"]))
            unfused = run_bwd(h, True, k, g8d, zd, act, training, clip)
            assert torch.equal(bits(out["dz"]), bits(unfused["dz"])), (case, "dz differs from yogo_bn_bwd_bf16 fed the same g")
    log_ratio(entry + " dz", f"B={B} C={C} P={P} HW={HW}", worst)


@pytest.mark.parametrize("bf16", [False, True])
def test_bwd_leaky_factor_at_exactly_zero(bf16):
    """beta = 0 and mean[c] a value that occurs in z: z - mean is exactly 0 there, so is the recomputed pre-activation, `ref > 0` is false and
    the factor is 0.01 (as torch's).  With frozen statistics dz = fl(gi * fl(g * 0.01f)) (then bf16): asserted exactly."""
    h = H()
    B, C, HW = 3, 5, 1025 if bf16 else 2049
    k = R.bn_case(B, C, HW, bf16)
    k["beta"] = torch.zeros(C)
    k["mean"] = k["z"][0, :, 0].clone()
    k["z"][:, :, ::7] = k["mean"].reshape(1, C, 1)
    at0 = (k["z"] == k["mean"].reshape(1, C, 1))
    assert int(at0.sum()) >= B * C * (HW // 7)
    if bf16:
        gd, zd = dev(R.to8c(k["g"])), dev(R.to8c(k["z"]))
    else:
        gd, zd = dev(k["g"]), dev(k["z"])
    out = run_bwd(h, bf16, k, gd, zd, LEAKY, 0, 0.0)
    dz = R.from8c(out["dz"], C) if bf16 else out["dz"]
    gi = (k["gamma"] * k["invstd"]).reshape(1, C, 1)
    want = gi * (k["g"] * torch.tensor(0.01, dtype=torch.float32))
    if bf16:
        want = want.to(torch.bfloat16).float()
    assert torch.equal(bits(dz[at0]), bits(want[at0])), "the factor at a pre-activation of exactly 0 is not 0.01"
    one = gi * k["g"]
    assert not torch.equal(dz[at0], (one.to(torch.bfloat16).float() if bf16 else one)[at0])


@pytest.mark.parametrize("bf16", [False, True])
def test_bwd_branch_within_tau(bf16):
    """a few elements (the last pixel of the second image, in the second workgroup of its plane, of some channels) whose recomputed pre-activation is
    the rounding residue of xhat * gamma: the fp32 branch is the residue's sign, the float64 reference's may be the other.  dz there may
    match either factor, the sums are allowed 0.99 |g| / 0.99 |g xhat| per such element -- and every other element is held as usual."""
    h = H()
    B, C, HW = 3, 5, 1025 if bf16 else 2049
    entry = "yogo_bn_bwd_bf16" if bf16 else "yogo_bn_bwd"
    k = R.branch_case(B, C, HW, bf16)
    if bf16:
        gd, zd = dev(R.to8c(k["g"])), dev(R.to8c(k["z"]))
    else:
        gd, zd = dev(k["g"]), dev(k["z"])
    rf = bwd_reference(k, LEAKY)
    nedge = int(rf["edge"].sum())
    assert nedge >= 2
    ndis = branch_disagreements(k, bf16)
    for training in (1, 0):
        out = run_bwd(h, bf16, k, gd, zd, LEAKY, training, 0.0)
        check_bwd(entry, f"branch within tau B={B} C={C} HW={HW} training={training}", k, rf, out, LEAKY, training, 0.0, bf16)
        dz = (R.from8c(out["dz"], C) if bf16 else out["dz"]).to(F64)
        cands = dz_candidates(k, rf, training, bf16)
        other = int((((dz - cands[0][0]).abs() > cands[0][1]) & rf["edge"]).sum())
        print(f"[bn_edges] {entry} | branch within tau training={training} | {nedge} elements within tau, {other} took the other branch than float64; "
              f"forward / backward disagreements {ndis}")


# ============================================================================================================================
# statistics
# ============================================================================================================================
# yogo_bn_finalize adds the rows in float64 (in another order than the reference: 2^-53 effects), so what separates the two is the one
# rounding of each result to fp32, half an ulp; the float64 orders can move a result across a rounding boundary, one ulp.  2 ulp = 2^-22 |ref|
# is allowed, plus 2^-50 of the magnitudes a running statistic is summed from (its two terms may cancel).
ULP2 = 2.0 ** -22


def finalize_call(h, part_g, rows, stride, C, count, rm, rv, nbt):
    mean, invstd = Guarded(C), Guarded(C)
    h.call("yogo_bn_finalize", part_g.view, rows, stride, C, count, EPS, MOM, mean.view, invstd.view, rm.view if rm else None, rv.view if rv else None,
           nbt, h.stream_ptr())
    for b_, w in ((mean, "mean"), (invstd, "invstd"), (part_g, "part"), (rm, "running_mean"), (rv, "running_var")):
        if b_:
            b_.check("bn_finalize " + w)
    return mean.view.cpu(), invstd.view.cpu()


@pytest.mark.parametrize("rows", [1, 31, 32, 33, 255, 256, 257, 289, 8192])
def test_finalize_synthetic_rows(rows):
    h = H()
    gen = torch.Generator().manual_seed(rows)
    nbt = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    calls = 0
    worst = 0.0
    for C in (1, 5, 8, 9, 20):
        for stride in (C, ((C + 15) // 16) * 16):
            part = torch.full((rows, stride, 2), 1000.0)
            part[:, :C, 0] = torch.randn(rows, C, generator=gen) * 5 + 2
            part[:, :C, 1] = torch.rand(rows, C, generator=gen) * 10 + 30
            for count in ((3 * rows, 1) if rows == 1 else (3 * rows,)):
                pg = Guarded(part.numel())
                pg.view.copy_(part.reshape(-1))
                rm0, rv0 = torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5
                rm, rv = Guarded(C), Guarded(C)
                rm.view.copy_(rm0)
                rv.view.copy_(rv0)
                mean, invstd = finalize_call(h, pg, rows, stride, C, count, rm, rv, nbt)
                calls += 1
                rmean, rinv, rrm, rrv, _ = R.finalize(part[:, :C], count, EPS, MOM, rm0, rv0)
                mag_rm = 2.0 ** -50 * (rm0.to(F64).abs() + rmean.abs())
                mag_rv = 2.0 ** -50 * (rv0.to(F64).abs() + 40.0)
                for got, ref, extra, what in ((mean, rmean, 0.0, "mean"), (invstd, rinv, 0.0, "invstd"), (rm.view.cpu(), rrm, mag_rm, "running_mean"),
                                              (rv.view.cpu(), rrv, mag_rv, "running_var")):
                    r = ratio((got.to(F64) - ref).abs(), ULP2 * ref.abs() + extra)
                    worst = max(worst, r)
                    assert r <= 1.0, (what, rows, C, stride, count, r)
                # running_mean = NULL: mean / invstd the same bits, nothing else touched
                pg2 = Guarded(part.numel())
                pg2.view.copy_(part.reshape(-1))
                m2, i2 = finalize_call(h, pg2, rows, stride, C, count, None, None, nbt)
                calls += 1
                assert torch.equal(bits(m2), bits(mean)) and torch.equal(bits(i2), bits(invstd))
    assert int(nbt.item()) == 5 + calls, "num_batches_tracked must rise by exactly 1 per call"
    log_ratio("yogo_bn_finalize", f"rows={rows}", worst)


def test_finalize_constant_channel_with_negative_variance():
    """a constant channel whose fp32 partial rows make q / count - mean^2 negative: var is clamped to 0, invstd == 1 / sqrt(eps) exactly"""
    h = H()
    rows, per_row = 33, 7
    found = None
    for j in range(1, 200):
        v = torch.tensor(1.0 + 0.013 * j, dtype=torch.float32)
        s, q = (v * per_row), ((v * v) * per_row)       # fp32 roundings, as a producer's
        mean = s.double() * rows / (rows * per_row)
        var = q.double() * rows / (rows * per_row) - mean * mean
        if float(var) < 0:
            found = (s, q)
            break
    assert found is not None, "no constant with a negative fp32 variance among the candidates"
    C = 5
    part = torch.zeros(rows, C, 2)
    gen = torch.Generator().manual_seed(1)
    part[:, :, 0] = torch.randn(rows, C, generator=gen)
    part[:, :, 1] = torch.rand(rows, C, generator=gen) * 10 + 30
    part[:, 2, 0], part[:, 2, 1] = found
    pg = Guarded(part.numel())
    pg.view.copy_(part.reshape(-1))
    rm, rv = Guarded(C), Guarded(C)
    rm.view.fill_(0.25)
    rv.view.fill_(1.5)
    nbt = torch.zeros(1, dtype=torch.int64, device="cuda")
    mean, invstd = finalize_call(h, pg, rows, C, C, rows * per_row, rm, rv, nbt)
    want = f32(1.0 / math.sqrt(EPS))
    assert float(invstd[2]) == want, (float(invstd[2]), want)
    rmean, rinv, rrm, rrv, _ = R.finalize(part, rows * per_row, EPS, MOM, torch.full((C,), 0.25), torch.full((C,), 1.5))
    assert float(rinv[2].float()) == want
    got_rv = rv.view.cpu()
    assert bool(torch.isfinite(rm.view.cpu()).all()) and bool(torch.isfinite(got_rv).all())
    assert ratio((got_rv.to(F64) - rrv).abs(), ULP2 * rrv.abs()) <= 1.0 and ratio((mean.to(F64) - rmean).abs(), ULP2 * rmean.abs()) <= 1.0
    assert int(nbt.item()) == 1


def run_stats(h, z8d, B, C, HW):
    rows = h.query_ints("yogo_bn_bwd_bf16_rows", 1, B, HW)[0]
    part = Guarded(rows * C * 2)
    h.call("yogo_bn_stats_bf16", z8d, part.view, B, C, HW, h.stream_ptr())
    part.check("bn_stats_bf16 part")
    assert bool(torch.isfinite(part.view).all()), "a partial row was left unwritten"
    return part, rows


@pytest.mark.parametrize("B,C,HW", R.bf16_shapes())
def test_stats_bf16_then_finalize(B, C, HW):
    """z = bf16(50 + randn): mean^2 / var ~ 2500.  e_ref: fp32 sums of z and z^2 over workgroup-sized pieces of each plane in four orders, the
    pieces added in float64 (what the two kernels do, in other orders), mean and invstd from them in float64.  Bound: 4 e_ref + the final
    rounding to fp32 (u |ref|)."""
    h = H()
    z = R.stats_case(B, C, HW)
    part, rows = run_stats(h, dev(R.to8c(z)), B, C, HW)
    count = B * HW
    nbt = torch.zeros(1, dtype=torch.int64, device="cuda")
    rm, rv = Guarded(C), Guarded(C)
    rm.view.fill_(0.0)
    rv.view.fill_(1.0)
    mean, invstd = finalize_call(h, part, rows, C, C, count, rm, rv, nbt)
    z64 = z.to(F64)
    p64 = torch.stack([z64.sum((0, 2)), (z64 * z64).sum((0, 2))], 1).reshape(1, C, 2)
    rmean, rinv, rrm, rrv, _ = R.finalize(p64, count, EPS, MOM, torch.zeros(C), torch.ones(C))
    nb = rows // B
    planes = z.reshape(B * C, HW)
    so, qo = sums32_orders(planes, nb), sums32_orders(planes * planes, nb)
    em = ei = erv = torch.zeros((), dtype=F64)   # the largest over the orders and the channels
    for s, q in zip(so, qo):
        pp = torch.stack([s.reshape(B, C).sum(0), q.reshape(B, C).sum(0)], 1).reshape(1, C, 2)
        m_o, i_o, _, rv_o, _ = R.finalize(pp, count, EPS, MOM, torch.zeros(C), torch.ones(C))
        em, ei, erv = torch.maximum(em, (m_o - rmean).abs().max()), torch.maximum(ei, (i_o - rinv).abs().max()), torch.maximum(erv, (rv_o - rrv).abs().max())
    case = f"B={B} C={C} HW={HW}"
    for got, ref, e, what in ((mean, rmean, em, "mean"), (invstd, rinv, ei, "invstd"), (rv.view.cpu(), rrv, erv, "running_var")):
        d, b = (got.to(F64) - ref).abs(), 4 * e + U * ref.abs()
        log("yogo_bn_stats_bf16+finalize " + what, case, d, e, b)
        assert bool((d <= b).all()), (what, case, d, b)
    assert int(nbt.item()) == 1


# ============================================================================================================================
# reductions
# ============================================================================================================================
# yogo_partials_reduce adds in float64 and rounds once: u |S|.  Above 64 rows it first folds rows s, s + 64, ... into row s in float64 and
# STORES that as fp32: one rounding per folded row, u |fold_s|, 64 of them, before the second sum.  (2^-50 sum |x| for the float64 orders.)
@pytest.mark.parametrize("rows", [1, 7, 8, 9, 64, 65, 128, 129, 513, 577])
def test_partials_reduce(rows):
    h = H()
    st = h.stream_ptr()
    gen = torch.Generator().manual_seed(rows)
    worst = 0.0
    for N in (1, 255, 256, 257):
        part = R.partials_case(rows, N, gen)
        p64 = part.to(F64)
        S = p64.sum(0)
        b = U * S.abs() + 2.0 ** -50 * p64.abs().sum(0)
        if rows > 64:
            for s in range(64):
                b = b + U * p64[s::64].sum(0).abs()
        clip_on = R.clip_both_signs(S) if N > 1 else 0.5 * f32(float(S.abs()))
        for clip in (0.0, clip_on):
            pg, out = Guarded(rows * N), Guarded(N)
            pg.view.copy_(part.reshape(-1))
            h.call("yogo_partials_reduce", pg.view, rows, N, clip, out.view, st)
            pg.check("partials_reduce part")
            out.check("partials_reduce out")
            got = out.view.cpu().to(F64)
            assert bool(torch.isfinite(got).all())
            want = S.clamp(-clip, clip) if clip > 0 else S
            r = ratio((got - want).abs(), b)
            worst = max(worst, r)
            assert r <= 1.0, (rows, N, clip, r)
            if clip > 0:
                assert bool((got[S > clip + b] == clip).all()) and bool((got[S < -clip - b] == -clip).all()) and float(got.abs().max()) <= clip
    log_ratio("yogo_partials_reduce", f"rows={rows}", worst)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("HW", [1, 255, 257, 2049])
def test_channel_sum(B, HW):
    """fp32 running sums per thread and image, the rest in float64.  e_ref: fp32 sums of each plane in four orders, planes added in float64;
    bound 4 e_ref + the final rounding u |S|."""
    h = H()
    st = h.stream_ptr()
    for C in (1, 5):
        g = R.channel_sum_case(B, C, HW)
        S = g.to(F64).sum((0, 2))
        e = torch.stack([(s.reshape(B, C).sum(0) - S).abs() for s in sums32_orders(g.reshape(B * C, HW))]).max()   # over orders and channels
        b = 4 * e + U * S.abs()
        clip_on = R.clip_both_signs(S) if C > 1 and HW > 1 else 0.5 * f32(float(S.abs().max()))
        gd = dev(g)
        for clip in (0.0, clip_on):
            out = Guarded(C)
            h.call("yogo_channel_sum", gd, B, C, HW, clip, out.view, st)
            out.check("channel_sum out")
            got = out.view.cpu().to(F64)
            assert bool(torch.isfinite(got).all())
            want = S.clamp(-clip, clip) if clip > 0 else S
            d = (got - want).abs()
            log("yogo_channel_sum", f"B={B} C={C} HW={HW} clip={clip:.4g}", d, e, b)
            assert bool((d <= b).all()), (B, C, HW, clip, d, b)
            if clip > 0:
                assert bool((got[S > clip + b] == clip).all()) and bool((got[S < -clip - b] == -clip).all()) and float(got.abs().max()) <= clip


# ============================================================================================================================
# layout conversions
# ============================================================================================================================
def run_to8c(h, x):
    B, C, HW = x.shape
    G, t = gbf16((B, R.cb_of(C), HW, 8))
    h.call("yogo_nchw_f32_to_bf16_8c", dev(x), t, B, C, HW, h.stream_ptr())
    G.check("nchw_f32_to_bf16_8c out")
    return t.cpu()


def run_from8c(h, t8, C):
    B, Cb, HW, _ = t8.shape
    out = Guarded(B * C * HW)     # exactly B * C * HW floats: a write for c >= C lands in the sentinels
    h.call("yogo_bf16_8c_to_nchw_f32", dev(t8), out.view, B, C, HW, h.stream_ptr())
    out.check("bf16_8c_to_nchw_f32 out")
    return out.view.cpu().view(B, C, HW)


def _special_values():
    """name -> fp32 values (through their bit patterns)"""
    gen = torch.Generator().manual_seed(11)

    def from_bits(v):
        return torch.tensor(v, dtype=torch.int64).to(torch.int32).view(torch.float32) if not isinstance(v, torch.Tensor) else v.to(torch.int32).view(torch.float32)

    rnd = torch.randint(0x00800000, 0x7F000000, (4096,), generator=gen, dtype=torch.int64)   # normal numbers, exponent below the top
    sign = torch.randint(0, 2, (4096,), generator=gen, dtype=torch.int64) << 31
    wrap = lambda b: torch.where(b >= 2 ** 31, b - 2 ** 32, b)
    ties = (rnd & 0xFFFF0000) | 0x8000          # exactly half way between two bf16 values; bit 16 takes both parities
    assert int(((ties >> 16) & 1).sum()) not in (0, ties.numel())
    return {
        "random": from_bits(wrap(rnd | sign)),
        "ties": from_bits(wrap(ties | sign)),
        "round up to inf": from_bits([0x7F7F8000, 0x7F7F8001, 0x7F7FFFFF, 0xFF7F8000 - 2 ** 32, 0xFF7FFFFF - 2 ** 32, 0x7F7F7FFF, 0xFF7F7FFF - 2 ** 32]),
        "zeros and infinities": from_bits([0x00000000, 0x80000000 - 2 ** 32, 0x7F800000, 0xFF800000 - 2 ** 32]),
        "nan": from_bits([0x7FC00000, 0x7F800001, 0x7F80FFFF, 0xFFC00001 - 2 ** 32, 0x7FFFFFFF, 0xFF800100 - 2 ** 32]),
        "subnormal": from_bits([0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x00400000, 0x007FFFFF, 0x007F8000,
                                0x80000001 - 2 ** 32, 0x80018000 - 2 ** 32, 0x807FFFFF - 2 ** 32, 0x80400000 - 2 ** 32]),
    }


def test_to8c_is_torchs_cast_bit_for_bit():
    h = H()
    C = 5
    for name, v in _special_values().items():
        HW = -(-v.numel() // C)
        x = torch.zeros(C * HW)
        x[:v.numel()] = v
        x = x.view(1, C, HW)
        got = run_to8c(h, x)
        want = R.to8c(x)
        assert bool((R.pad_lanes(got, C).view(torch.int16) == 0).all()), (name, "padding lanes must be +0")
        g, w = R.from8c(got, C), R.from8c(want, C)
        nan = torch.isnan(w)
        assert torch.equal(torch.isnan(g), nan), (name, "NaN must stay NaN (and nothing else become one)")
        gb, wb = bits(got.permute(0, 1, 3, 2).reshape(1, -1, HW)[:, :C].contiguous()), bits(want.permute(0, 1, 3, 2).reshape(1, -1, HW)[:, :C].contiguous())
        nbad = int(((gb != wb) & ~nan).sum())
        print(f"[bn_edges] yogo_nchw_f32_to_bf16_8c | {name} | {nbad} of {v.numel()} values differ from torch's cast")
        assert nbad == 0, (name, nbad)


@pytest.mark.parametrize("B,C,HW", R.bf16_shapes())
def test_8c_round_trip(B, C, HW):
    h = H()
    gen = torch.Generator().manual_seed(B * 100000 + C * 1000 + HW % 1000)
    x = torch.randn(B, C, HW, generator=gen) * 3
    t8 = run_to8c(h, x)
    want = R.to8c(x)
    assert torch.equal(bits(t8), bits(want)), "to 8c: not torch's cast, or padding lanes not zero"
    junk = R.to8c(x, pad=1000.0)                   # padding lanes of the INPUT must not reach the output
    back = run_from8c(h, junk, C)
    assert torch.equal(bits(back), bits(x.to(torch.bfloat16).float())), "from 8c is not exact"


# ============================================================================================================================
# padding isolation (bf16, C = 5: one block half padding, one all padding; C = 20: the third block half, the fourth all padding)
# ============================================================================================================================
@pytest.mark.parametrize("B,C", [(3, 5), (1, 20), (3, 20)])
def test_padding_lanes_do_not_leak(B, C):
    h = H()
    HW = 1025
    k = R.bn_case(B, C, HW, True)
    zs = R.stats_case(B, C, HW)
    res = []
    for pad in (0.0, 1000.0):
        z8, g8 = dev(R.to8c(k["z"], pad)), dev(R.to8c(k["g"], pad))
        assert bool((R.pad_lanes(z8.cpu(), C) == pad).all())
        o = {}
        o["y"] = run_apply_bf16(h, k, z8, 0, SILU)
        o["y_var"] = run_apply_bf16(h, k, z8, 1, LEAKY)
        clip = R.clip_both_signs(torch.cat([bwd_reference(k, LEAKY)[n] for n in ("S2", "S1")]))
        for tag, inplace in (("bwd", False), ("bwd_inplace", True)):
            out = run_bwd(h, True, k, g8, z8, LEAKY, 1, clip, inplace=inplace)
            assert bool((R.pad_lanes(out["dz"], C) == 0).all()), "dz padding lanes not zero"
            for n, v in out.items():
                o[tag + "." + n] = v
        part, rows = run_stats(h, dev(R.to8c(zs, pad)), B, C, HW)
        o["stats.part"] = part.view.cpu()
        res.append(o)
    for n in res[0]:
        assert torch.equal(bits(res[0][n]), bits(res[1][n])), (n, "junk in the input's padding lanes changed an output")


# ============================================================================================================================
# grid.y = B * C (fp32) / B * Cb (conversions) is held to 65535 like the bf16 entry points: both sides of the limit, HW = 1
# ============================================================================================================================
def test_plane_count_limit_f32():
    h = H()
    st = h.stream_ptr()
    B, C, HW = 4369, 15, 1
    assert B * C == 65535
    k = R.bn_case(B, C, HW, False)
    d = {n: dev(k[n]) for n in ("z", "g", "mean", "invstd", "gamma", "beta")}
    y = Guarded(B * C)
    h.call("yogo_bn_apply_act", d["z"], y.view, d["mean"], d["invstd"], 0, EPS, d["gamma"], d["beta"], B, C, HW, LEAKY, st)
    y.check("bn_apply_act at 65535 planes")
    got = y.view.cpu().view(B, C, HW)
    ref = R.apply(k["z"], k["mean"], k["invstd"], 0, EPS, k["gamma"], k["beta"], LEAKY)
    assert ratio((got.to(F64) - ref).abs(), apply_bound(k, 0, LEAKY, False, ref)) <= 1.0
    out = run_bwd(h, False, k, d["g"], d["z"], LEAKY, 1, 0.0)
    check_bwd("yogo_bn_bwd", "65535 planes", k, bwd_reference(k, LEAKY), out, LEAKY, 1, 0.0, False)
    # one batch element more: the library's argument error, before any launch
    B2 = B + 1
    big = torch.zeros(B2 * C, device="cuda")
    y2 = Guarded(B2 * C)
    with pytest.raises(RuntimeError, match="exceeds 65535"):
        h.call("yogo_bn_apply_act", big, y2.view, d["mean"], d["invstd"], 0, EPS, d["gamma"], d["beta"], B2, C, HW, LEAKY, st)
    y2.check("refused bn_apply_act")
    assert bool(torch.isnan(y2.view).all()), "a refused call must not have launched"
    dz, part, sums, dg, db = Guarded(B2 * C), Guarded(B2 * C * 2), Guarded(2 * C), Guarded(C), Guarded(C)
    with pytest.raises(RuntimeError, match="exceeds 65535"):
        h.call("yogo_bn_bwd", big, big, dz.view, d["mean"], d["invstd"], d["gamma"], d["beta"], LEAKY, dg.view, db.view, part.view, sums.view, B2, C, HW,
               1, 0.0, st)
    for b_ in (dz, part, sums, dg, db):
        b_.check("refused bn_bwd")
        assert bool(torch.isnan(b_.view).all()), "a refused call must not have launched"


def test_plane_count_limit_conversions():
    h = H()
    st = h.stream_ptr()
    B, C, HW = 32767, 16, 1
    assert B * R.cb_of(C) == 65534
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(B, C, HW, generator=gen)
    t8 = run_to8c(h, x)
    assert torch.equal(bits(t8), bits(R.to8c(x)))
    back = run_from8c(h, t8, C)
    assert torch.equal(bits(back), bits(x.to(torch.bfloat16).float()))
    B2 = B + 1                                    # 65536 planes
    xin = torch.zeros(B2 * C, device="cuda")
    G, t = gbf16((B2, 2, HW, 8))
    with pytest.raises(RuntimeError, match="exceeds 65535"):
        h.call("yogo_nchw_f32_to_bf16_8c", xin, t, B2, C, HW, st)
    G.check("refused nchw_f32_to_bf16_8c")
    assert bool(torch.isnan(t.float()).all()), "a refused call must not have launched"
    out = Guarded(B2 * C)
    tin = torch.zeros(B2 * 2 * 8, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="exceeds 65535"):
        h.call("yogo_bf16_8c_to_nchw_f32", tin, out.view, B2, C, HW, st)
    out.check("refused bf16_8c_to_nchw_f32")
    assert bool(torch.isnan(out.view).all()), "a refused call must not have launched"
