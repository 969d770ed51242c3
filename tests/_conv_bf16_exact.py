"""The exact-integer instrument of the bf16 convolution engine (host only: no GPU import).

With small-integer operands every product and every partial sum of a convolution is an exactly representable fp32 integer in ANY
summation order (chunking, split-K, tap order, 32x32x16 or 16x16x32 MFMAs), so the value a kernel stores is determined to the bit and is
compared with a plain float64 reference with NO tolerance.  A mismatch is never a legitimate reordering: it is a wrong element.

Inputs (``draw``): x, w, bias, dy from {-2, -1, 0, 1, 2}, mostly +-1 (one non-zero in ten is +-2), non-zero with probability
``density(Cin, k)`` = min(0.5, 1.5 sqrt(16 / (Cin k k))) (the bias: 0.75) -- outputs of a few tens at most, ~5 % exact zeros, half negative.
Channel scales (the Dropout2d masks of yogo/model_defns.py) come from {0, 0.5, 1, 2}: a power of two commutes with every rounding, so the
result does not depend on how a kernel associates value * slope * scale.  The PRODUCTION values 1 / (1 - p) are not powers of two; they stay
with the tolerance tests (test_gpu_bf16.py, test_gpu_ws.py, the teacher-forced checks of _util.py) -- this instrument does not cover them,
nor the rounding of non-integer data.

Reference (``Ref``): torch float64 on the CPU.  y = conv(x, w) + bias; the stored output is bf16(scale * (y > 0 ? y : float32(0.01) * y)) with
the one inexact step -- the float32 product with LEAKY_SLOPE -- evaluated in float32 as csrc/common.h states it (act_fwd); the sign map from
the STORED output in the byte layout of include/yogo_hip.h (yogo_bf16_signs_bytes); BatchNorm partials sum y, sum y^2 per channel; the data
gradient dx = bf16(conv_transpose(dy) * (ref > 0 ? 1 : float32(0.01)) * scale) (act_bwd_factor) with a reference holding +0.0, -0.0 and both
signs, given as a bf16 tensor and as a sign map; dw, db as integers, also clamped at the integer CLIP; the pair: y1 AS STORED feeds layer 2.

Preconditions (``Ref.check_preconditions``, on the reference alone): every sum has terms that are integer multiples of one quantum q (1; for
layer 2 of the pair 2^-15, its input being bf16(0.01 n) * 0.5) with sum |terms| < 2^24 q; every bf16-stored pre-activation is an integer
of magnitude <= 256; statistics, dw, db below 2^24; every output holds zeros, negatives and positives.

Comparison (``compare`` / ``compare_8c`` / ``compare_signs``): equal as values (-0.0 == 0.0 is the only latitude, NaN = unwritten), padding
channels exactly zero; a mismatch reports the first differing (b, c, h, w), both values, the count and how many lie on a band / image border."""
import math
import re

import torch
import torch.nn.functional as F

LEAKY32 = torch.tensor(0.01, dtype=torch.float32)   # LEAKY_SLOPE = 0.01f (csrc/common.h)
SCALES = (0.0, 0.5, 1.0, 2.0)
CLIP = 8.0
LIMIT = 2 ** 24
ACT_NONE, ACT_LEAKY, ACT_SILU = 0, 1, 2
f64 = torch.float64


def density(Cin, k):
    return min(0.5, 1.5 * math.sqrt(16.0 / (Cin * k * k)))


def out_hw(IH, IW, k, s):
    pad = 1 if k == 3 else 0
    return (IH + 2 * pad - k) // s + 1, (IW + 2 * pad - k) // s + 1


def blocks(C):
    """channel blocks of 8 of a bf16 NCHW8c tensor (C padded to a multiple of 16)"""
    return ((C + 15) // 16) * 2


def cpad_of(C):
    """channels a sign map covers: C rounded up to 32 / 64 / a multiple of 128 (csrc/conv_bf16_plan.h: bf_mpad_of)"""
    return 32 if C <= 32 else (64 if C <= 64 else (C + 127) // 128 * 128)


def draw_ints(shape, p, g):
    """float64 integers from {-2 .. 2}: non-zero with probability p, +-1 nine times in ten"""
    nz = torch.rand(shape, generator=g) < p
    mag = torch.where(torch.rand(shape, generator=g) < 0.1, 2.0, 1.0)
    sgn = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    return torch.where(nz, mag * sgn, torch.zeros(())).to(f64)


def draw_scales(B, C, g):
    """[B][C] from {0, 0.5, 1, 2}, every value on about a quarter of the channels of every image"""
    vals = torch.tensor(SCALES, dtype=f64)
    return torch.stack([vals[(torch.randperm(C, generator=g) + b) % 4] for b in range(B)])


def to8c(t):
    """NCHW [B][C][H][W] (bf16-valued) -> bf16 NCHW8c [B][blocks(C)][H][W][8], padding channels +0.0; keeps -0.0"""
    B, C, H, W = t.shape
    full = torch.zeros(B, blocks(C) * 8, H, W, dtype=torch.float32)
    full[:, :C] = t.float()
    return full.reshape(B, blocks(C), 8, H, W).permute(0, 1, 3, 4, 2).contiguous().to(torch.bfloat16)


def from8c(t8):
    """bf16 NCHW8c (CPU) -> float32 NCHW with ALL blocks(C) * 8 channels"""
    B, cb, H, W, _ = t8.shape
    return t8.float().permute(0, 1, 4, 2, 3).reshape(B, cb * 8, H, W)


def sign_map(stored, pad_bits=0):
    """the sign map of a stored NCHW tensor: uint8 [B][2][H][W][cpad / 16]; byte (h, pixel, q), bit i + 4 e = (channel 16 q + 8 e + 4 h + i > 0).
    pad_bits = 1 sets the bits of channels that do not exist (a data gradient must not depend on them: their bytes are unspecified)"""
    B, C, H, W = stored.shape
    cp = cpad_of(C)
    pos = torch.full((B, cp, H, W), int(pad_bits), dtype=torch.int64)
    pos[:, :C] = (stored > 0)
    pos = pos.view(B, cp // 16, 2, 2, 4, H, W).permute(0, 3, 5, 6, 1, 2, 4)   # [B][q][e][h][i][H][W] -> [B][h][H][W][q][e][i]
    wts = torch.tensor([[1, 2, 4, 8], [16, 32, 64, 128]])
    return (pos * wts).sum((-1, -2)).to(torch.uint8).contiguous()


def sign_bytes_used(sg, C):
    """the bytes of a sign map that belong to existing channel blocks: [B * 2 * H * W][ceil(C / 16)]"""
    return sg.reshape(-1, cpad_of(C) // 16)[:, : (C + 15) // 16]


def conv64(x, w, bias, k, s):
    return F.conv2d(x, w, bias, stride=s, padding=1 if k == 3 else 0)


def conv_t64(dy, w, IH, IW, k, s):
    pad = 1 if k == 3 else 0
    OH, OW = dy.shape[2:]
    return F.conv_transpose2d(dy, w, stride=s, padding=pad, output_padding=(IH - ((OH - 1) * s + k - 2 * pad), IW - ((OW - 1) * s + k - 2 * pad)))


def wgrad64(x, dy, k, s):
    """dw[o][c][i][j] = sum over images and output pixels of dy[b][o][p] * x[b][c][patch p, tap (i, j)], image by image"""
    B, Cin = x.shape[:2]
    Cout = dy.shape[1]
    dw = torch.zeros(Cout, Cin * k * k, dtype=f64)
    for b in range(B):
        dw += dy[b].reshape(Cout, -1) @ F.unfold(x[b:b + 1], k, padding=1 if k == 3 else 0, stride=s)[0].t()
    return dw.reshape(Cout, Cin, k, k)


def epilogue(y, act, scale):
    """float64 exact fp32 values y -> the stored bf16 values (as float32): scale * act(y), the LeakyReLU product in float32"""
    v = y.float()
    assert torch.equal(v.to(f64), y), "the pre-activation is not exact in float32: no test"
    if act == ACT_LEAKY:
        v = torch.where(v > 0, v, v * LEAKY32)
    if scale is not None:
        v = v * scale.float()[:, :, None, None]
    return v.to(torch.bfloat16).float()


class Ref:
    """operands and float64 reference of one case (B, Cin, Cout, IH, IW, k, s), computed once"""

    def __init__(self, case, seed=0):
        B, Cin, Cout, IH, IW, k, s = case
        self.case = case
        OH, OW = out_hw(IH, IW, k, s)
        self.OH, self.OW = OH, OW
        g = torch.Generator().manual_seed(1000 + seed + 31 * Cin + 17 * Cout + 7 * IH + 3 * IW + k + s)
        p, pd = density(Cin, k), density(Cout, k)
        self.p = p
        self.x = draw_ints((B, Cin, IH, IW), p, g)
        self.w = draw_ints((Cout, Cin, k, k), p, g)
        self.bias = draw_ints((Cout,), 0.75, g)
        self.dy = draw_ints((B, Cout, OH, OW), pd, g)
        self.dy[:, Cout // 2] = 0            # one dead gradient channel: its dw slice and db element are exact zeros
        self.so = draw_scales(B, Cout, g)    # scale of the forward output
        self.si = draw_scales(B, Cin, g)     # scale of the data gradient
        r = draw_ints((B, Cin, IH, IW), 0.6, g).float()
        self.refy = torch.where((r == 0) & (torch.rand(r.shape, generator=g) < 0.5), torch.tensor(-0.0), r)   # +0.0, -0.0, both signs
        self.y0 = conv64(self.x, self.w, None, k, s)
        self.y = self.y0 + self.bias[None, :, None, None]
        self.g = conv_t64(self.dy, self.w, IH, IW, k, s)
        self.dw = wgrad64(self.x, self.dy, k, s)
        self.db = self.dy.sum((0, 2, 3))
        self.stats = torch.stack([self.y.sum((0, 2, 3)), (self.y ** 2).sum((0, 2, 3))], 1)   # [Cout][2]

    # ---- forward
    def stored(self, act=ACT_LEAKY, bias=True, scale=True):
        return epilogue(self.y if bias else self.y0, act, self.so if scale else None)

    def silu(self, scale=True):
        """float64: y / (1 + exp(-y)) * scale, NOT rounded (held to TF_ULP)"""
        v = self.y * torch.sigmoid(self.y)
        return v * self.so[:, :, None, None] if scale else v

    # ---- data gradient
    def factor(self):
        return torch.where(self.refy > 0, torch.ones((), dtype=torch.float32), LEAKY32)

    def dx(self, ref=False, scale=False):
        v = self.g.float()
        if ref:
            v = v * self.factor()
        if scale:
            v = v * self.si.float()[:, :, None, None]
        return v.to(torch.bfloat16).float()

    def ref_signs(self):
        return sign_map(self.refy, pad_bits=1)

    # ---- weight gradient
    def wgrad(self, clip=0.0):
        if clip > 0:
            return self.dw.clamp(-clip, clip), self.db.clamp(-clip, clip)
        return self.dw, self.db

    def check_preconditions(self):
        B, Cin, Cout, IH, IW, k, s = self.case
        hint = f"case {self.case}: lower the density ({self.p:.3f}) of x / w / dy in _conv_bf16_exact.Ref"
        T = k * k
        # sum |terms| of every sum a kernel forms, q = 1: |operand| <= 2, so a sum of n products is bounded by 4 n
        assert 4 * Cin * T + 2 < LIMIT and 4 * Cout * T < LIMIT, ("convolution / data-gradient sums", hint)
        npix = B * self.OH * self.OW
        assert 4 * npix < LIMIT and float(self.dw.abs().max()) < LIMIT and float(self.db.abs().max()) < LIMIT, ("weight-gradient sums over pixels", hint)
        for name, t in (("x", self.x), ("w", self.w), ("bias", self.bias), ("dy", self.dy)):
            assert torch.equal(t, t.round()) and float(t.abs().max()) <= 2, (name, "not a small integer")
        for name, t in (("y", self.y), ("y0", self.y0), ("conv_transpose(dy)", self.g)):
            assert torch.equal(t, t.round()) and float(t.abs().max()) <= 256, (name, "a bf16-stored value is not an integer <= 256", float(t.abs().max()), hint)
        # BatchNorm partials: a partial never spans images, so the per-image sums bound every one of them (sum y^2 >= |sum y|)
        assert float((self.y ** 2).sum((2, 3)).max()) < LIMIT, ("BatchNorm partial sums", hint)
        outs = dict(y=self.stored(), y_plain=self.stored(ACT_NONE, True, False), y_nobias=self.stored(ACT_NONE, False, False), dx=self.dx(), dx_ref=self.dx(True, True),
                    dw=self.dw, db=self.db)
        if npix < 8:
            del outs["db"]     # (a handful of pixels: db is a sum of a few values)
        for name, t in outs.items():
            assert bool((t == 0).any()) and bool((t < 0).any()) and bool((t > 0).any()), (name, "lacks zeros, negatives or positives", hint)
        assert bool((self.refy == 0).any()) and bool(torch.signbit(self.refy[self.refy == 0]).any()) and not bool(torch.signbit(self.refy[self.refy == 0]).all()), "reference lacks +0.0 / -0.0"


class WgradRef(Ref):
    """the weight-gradient part of Ref alone (x, dy, dw, db; the same draws): for the long walks, whose planes are too large for a forward and
    a data-gradient reference they would not use"""

    def __init__(self, case, seed=0):
        B, Cin, Cout, IH, IW, k, s = case
        self.case = case
        self.OH, self.OW = out_hw(IH, IW, k, s)
        g = torch.Generator().manual_seed(2000 + seed + 31 * Cin + 17 * Cout + 7 * IH + 3 * IW + k + s)
        self.p = density(Cin, k)
        self.x = draw_ints((B, Cin, IH, IW), self.p, g)
        self.dy = draw_ints((B, Cout, self.OH, self.OW), density(Cout, k), g)
        self.dy[:, Cout // 2] = 0
        self.dw = wgrad64(self.x, self.dy, k, s)
        self.db = self.dy.sum((0, 2, 3))

    def check_preconditions(self):
        hint = f"case {self.case}: lower the density ({self.p:.3f}) of x / dy in _conv_bf16_exact.WgradRef"
        npix = self.case[0] * self.OH * self.OW
        assert 4 * npix < LIMIT and float(self.dw.abs().max()) < LIMIT and float(self.db.abs().max()) < LIMIT, ("weight-gradient sums over pixels", hint)
        for name, t in (("x", self.x), ("dy", self.dy)):
            assert torch.equal(t, t.round()) and float(t.abs().max()) <= 2, (name, "not a small integer")
        for name, t in (("dw", self.dw), ("db", self.db)):
            assert bool((t == 0).any()) and bool((t < 0).any()) and bool((t > 0).any()), (name, "lacks zeros, negatives or positives", hint)


class PairRef:
    """layers 1 + 2 of base_model (yogo/model_defns.py:39-46): 16 -> C1 (3x3, stride 1) -> C2 (3x3, stride 2), LeakyReLU, scale and sign map
    each; layer 2 reads y1 AS STORED in bf16.  Its terms are multiples of q = 2^-15: y1 = bf16(float32(0.01) n) * scale, scale >= 0.5."""
    Q = 2.0 ** -15

    def __init__(self, case, seed=0):
        B, C1, C2, IH, IW = case
        self.case = case
        self.OH, self.OW = out_hw(IH, IW, 3, 2)
        g = torch.Generator().manual_seed(2000 + seed + 7 * IH + 3 * IW + C2)
        self.p1, self.p2 = 0.25, 0.2     # (lower than density(): layer 2 sums |y1| of up to a few tens against 2^24 q = 512)
        self.x = draw_ints((B, 16, IH, IW), self.p1, g)
        self.w1 = draw_ints((C1, 16, 3, 3), self.p1, g)
        self.b1 = draw_ints((C1,), 0.75, g)
        self.w2 = draw_ints((C2, C1, 3, 3), self.p2, g)
        self.b2 = draw_ints((C2,), 0.75, g)
        self.s1 = draw_scales(B, C1, g)
        self.s2 = draw_scales(B, C2, g)
        self.y1_pre = conv64(self.x, self.w1, self.b1, 3, 1)
        self.y1 = epilogue(self.y1_pre, ACT_LEAKY, self.s1)
        self.y2_pre = conv64(self.y1.to(f64), self.w2, self.b2, 3, 2)
        self.y2 = epilogue(self.y2_pre, ACT_LEAKY, self.s2)

    def check_preconditions(self):
        hint = f"pair {self.case}: lower the densities ({self.p1}, {self.p2}) in _conv_bf16_exact.PairRef"
        assert torch.equal(self.y1_pre, self.y1_pre.round()) and float(self.y1_pre.abs().max()) <= 256, ("y1", hint)
        u = self.y1.to(f64) / self.Q
        assert torch.equal(u, u.round()), ("the stored y1 is not a multiple of 2^-15", hint)
        mag = conv64(self.y1.to(f64).abs(), self.w2.abs(), self.b2.abs(), 3, 2)
        assert float(mag.max()) < LIMIT * self.Q, ("layer 2: sum |terms| = %g, not below 2^24 q = 512" % float(mag.max()), hint)
        for name, t in (("y1", self.y1), ("y2", self.y2)):
            assert bool((t == 0).any()) and bool((t < 0).any()) and bool((t > 0).any()), (name, "lacks zeros, negatives or positives", hint)


# ---- comparison ------------------------------------------------------------------------------------------------------------------
def band_width(plan):
    """columns of one band of the launch-log line ``plan`` (None: unknown); the stride-2 data gradient tiles 2x2 quads"""
    m = re.search(r"\bTW=(\d+)", plan or "")
    if not m:
        return None
    return int(m.group(1)) * (2 if "s2d=1" in plan else 1)


def compare(what, got, want, plan=None):
    """``got`` == ``want`` as values, elementwise (CPU tensors of one shape; -0.0 == 0.0; NaN = never written = a mismatch).  On a mismatch:
    the first differing index ((b, c, h, w) for a 4-d tensor), both values, the count, and how many of the differing elements lie on a
    band border of the logged plan or on the image border."""
    assert tuple(got.shape) == tuple(want.shape), (what, tuple(got.shape), tuple(want.shape))
    bad = ~(got.to(f64) == want.to(f64))
    n = int(bad.sum())
    if n == 0:
        return
    idx = bad.nonzero()
    first = tuple(int(v) for v in idx[0])
    where = ""
    if got.dim() == 4:
        H, W = got.shape[2:]
        tw = band_width(plan)
        h, w = idx[:, 2], idx[:, 3]
        edge = (h == 0) | (h == H - 1) | (w == 0) | (w == W - 1)
        if tw:
            edge |= (w % tw == 0) | (w % tw == tw - 1)
        where = f"; {int(edge.sum())} of them on a band (TW = {tw}) or image border"
    raise AssertionError(f"{what}: {n} of {bad.numel()} elements differ{where}; first at {first}: got {float(got[first])!r}, want {float(want[first])!r}"
                         + (f" | plan: {plan}" if plan else ""))


def compare_8c(what, got8, want, plan=None):
    """a bf16 NCHW8c output (CPU) against the stored NCHW reference: existing channels equal, padding channels exactly zero"""
    C = want.shape[1]
    full = from8c(got8)
    assert full.shape[1] == blocks(C) * 8, (what, tuple(got8.shape))
    compare(what, full[:, :C], want, plan)
    compare(what + " [padding channels]", full[:, C:], torch.zeros_like(full[:, C:]), plan)


def compare_signs(what, got, stored, plan=None):
    """the sign-map bytes of existing channel blocks against the map of the STORED reference (padding channels read "not positive")"""
    C = stored.shape[1]
    B, _, H, W = stored.shape
    a = sign_bytes_used(got, C).reshape(B, 2, H, W, -1).permute(0, 1, 4, 2, 3).reshape(B, -1, H, W)   # [B][(half, block)][H][W]
    b = sign_bytes_used(sign_map(stored), C).reshape(B, 2, H, W, -1).permute(0, 1, 4, 2, 3).reshape(B, -1, H, W)
    compare(what + " [sign bytes, index (b, half * blocks + block, h, w)]", a, b, plan)
