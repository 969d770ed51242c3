"""float64 reference of the BatchNorm, reduction, layout and AdamW operations as yogo_amd/csrc/bn.hip and optim.hip define them, and the
input generators of tests/test_gpu_bn_edges.py.  Plain torch on the CPU: no project code.  tests/test_bn_ref_host.py holds the reference
to torch itself (F.batch_norm / autograd / torch.optim.AdamW in float64) and the generators to the caps the GPU tests rely on.

Layouts: fp32 tensors are [B][C][HW]; bf16 tensors are NCHW8c [B][Cb][HW][8] with Cb = 2 * ceil(C / 16) channel blocks (C padded to a
multiple of 16, padding lanes zero).  Every function widens what it is given to float64 first: fed the fp32 / bf16 values a kernel was
given, it returns what that kernel would return in exact arithmetic."""
import math

import torch

NONE, LEAKY, SILU = 0, 1, 2
LEAKY_SLOPE = 0.01
U32 = 2.0 ** -24      # unit roundoff of fp32 (half an ulp, relative)
U16 = 2.0 ** -8       # unit roundoff of bf16 (8 significand bits: half an ulp, relative)
F64 = torch.float64


def _c(v):
    """per-channel vector -> [1][C][1] float64"""
    return torch.as_tensor(v).to(F64).reshape(1, -1, 1)


def act_fwd(y, act):
    if act == LEAKY:
        return torch.where(y > 0, y, LEAKY_SLOPE * y)
    if act == SILU:
        return y * torch.sigmoid(y)
    return y


def act_factor(y, act):
    """derivative of the activation at the pre-activation y (LeakyReLU: y > 0 ? 1 : 0.01, so 0.01 AT zero, as torch)"""
    if act == LEAKY:
        return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, LEAKY_SLOPE))
    if act == SILU:
        s = torch.sigmoid(y)
        return s * (1 + y * (1 - s))
    return torch.ones_like(y)


def finalize(part, count, eps, momentum, rm=None, rv=None, nbt=0):
    """part [rows][>= C][2] partial (sum, sum of squares) rows -> mean, invstd, running_mean, running_var, num_batches_tracked.
    Biased variance (clamped at 0) to normalise, unbiased into running_var (the biased one when count == 1)."""
    p = part.to(F64)
    s, q = p[..., 0].sum(0), p[..., 1].sum(0)
    mean = s / count
    var = (q / count - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    rm2 = rv2 = None
    if rm is not None:
        unbiased = var * count / (count - 1.0) if count > 1 else var
        rm2 = (1.0 - momentum) * rm.to(F64) + momentum * mean
        rv2 = (1.0 - momentum) * rv.to(F64) + momentum * unbiased
    return mean, invstd, rm2, rv2, nbt + 1


def apply(z, mean, invstd_or_var, stat_is_var, eps, gamma, beta, act):
    """y = act((z - mean) * (invstd * gamma) + beta), z [B][C][HW]"""
    z = z.to(F64)
    sv = _c(invstd_or_var)
    istd = 1.0 / torch.sqrt(sv + eps) if stat_is_var else sv
    return act_fwd((z - _c(mean)) * (istd * _c(gamma)) + _c(beta), act)


def backward(g, z, mean, invstd, gamma, beta, act, training, clip):
    """g: gradient w.r.t. the block OUTPUT.  Returns dz, dgamma, dbeta (clamped to +-clip when clip > 0; dz uses the unclamped sums) and
    the recomputed pre-activation y64 = xhat * gamma + beta the activation derivative is taken from."""
    g, z = g.to(F64), z.to(F64)
    xh = (z - _c(mean)) * _c(invstd)
    y = xh * _c(gamma) + _c(beta)
    ge = g * act_factor(y, act)
    s1, s2 = ge.sum((0, 2)), (ge * xh).sum((0, 2))
    n = g.shape[0] * g.shape[2]
    if training:
        dz = _c(gamma) * _c(invstd) * (ge - _c(s1 / n) - xh * _c(s2 / n))
    else:
        dz = _c(gamma) * _c(invstd) * ge
    dgamma, dbeta = s2, s1
    if clip > 0:
        dgamma, dbeta = dgamma.clamp(-clip, clip), dbeta.clamp(-clip, clip)
    return dz, dgamma, dbeta, y


def cb_of(C):
    return ((C + 15) // 16) * 2


def to8c(x, pad=0.0):
    """fp32 [B][C][HW] -> bf16 [B][Cb][HW][8]; the rounding is torch's .to(torch.bfloat16); padding lanes hold ``pad``"""
    B, C, HW = x.shape
    Cb = cb_of(C)
    full = torch.full((B, Cb * 8, HW), float(pad), dtype=torch.float32)
    full[:, :C] = x
    return full.to(torch.bfloat16).reshape(B, Cb, 8, HW).permute(0, 1, 3, 2).contiguous()


def from8c(t, C):
    """bf16 [B][Cb][HW][8] -> fp32 [B][C][HW] (exact)"""
    B, Cb, HW, _ = t.shape
    return t.float().permute(0, 1, 3, 2).reshape(B, Cb * 8, HW)[:, :C].contiguous()


def pad_lanes(t, C):
    """the padding lanes of an 8c tensor, [B][Cb * 8 - C][HW]"""
    B, Cb, HW, _ = t.shape
    return t.permute(0, 1, 3, 2).reshape(B, Cb * 8, HW)[:, C:]


def adamw(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, wd=5e-2, grad_scale=1.0):
    """torch.optim.AdamW's single-tensor update in float64 on grad_scale * g; step is 1-based.  Returns p, m, v."""
    b1, b2 = betas
    p, g, m, v = p.to(F64), g.to(F64) * grad_scale, m.to(F64), v.to(F64)
    p = p * (1.0 - lr * wd)
    m = m + (1.0 - b1) * (g - m)
    v = v * b2 + (1.0 - b2) * g * g
    denom = v.sqrt() / math.sqrt(1.0 - b2 ** step) + eps
    return p - (lr / (1.0 - b1 ** step)) * (m / denom), m, v


# ---- the LeakyReLU branch next to zero ------------------------------------------------------------------------------------------------
# The kernels recompute the pre-activation in fp32 as fmaf(xhat, gamma, beta) with xhat = fl(fl(z - mean) * invstd): two roundings in
# xhat (relative 2 u, u = 2^-24, carried into xhat * gamma) and one of the fma (u |y|, |y| <= |xhat gamma| + |beta|), i.e. at most
# 3 u (|xhat gamma| + |beta|) to first order.  tau takes 8 u of the same magnitude (second-order terms and a reading of "a few roundings"
# that cannot be too tight): where |y64| <= tau the fp32 branch may legitimately differ from the float64 one.
def leaky_tau(z, mean, invstd, gamma, beta):
    xh = (z.to(F64) - _c(mean)) * _c(invstd)
    return 8.0 * U32 * ((xh * _c(gamma)).abs() + _c(beta).abs())


def leaky_edge_mask(z, mean, invstd, gamma, beta):
    xh = (z.to(F64) - _c(mean)) * _c(invstd)
    y = xh * _c(gamma) + _c(beta)
    return y.abs() <= leaky_tau(z, mean, invstd, gamma, beta)


EDGE_CAP = 1e-3   # at most 0.1 % of a case's elements may sit within tau of the branch (a condition on the INPUTS, asserted on the CPU)


# ---- input generators (shared by the host test, which asserts the caps, and the GPU tests) -----------------------------------------------
# (path, B, C, HW) lists: every HW at one (B, C), then every (B, C) at the first multi-block HW.  fp32: a workgroup covers 2048 pixels
# (256 threads x 8), bf16 NCHW8c: 1024 (256 x 4); 64 workgroups per plane at the most.
F32_HW = (1, 255, 257, 2048, 2049, 2052, 131076)
F32_C = (1, 5, 16)
BF16_HW = (1, 1023, 1024, 1025, 65540)
BF16_C = (5, 16, 20)
BS = (1, 3)


def f32_shapes():
    out = [(3, 5, hw) for hw in F32_HW if hw != 131076] + [(1, 2, 131076)]
    out += [(b, c, 2049) for b in BS for c in F32_C if (b, c) != (3, 5)]
    return out


def bf16_shapes():
    out = [(3, 5, hw) for hw in BF16_HW if hw != 65540] + [(1, 16, 65540)]
    out += [(b, c, 1025) for b in BS for c in BF16_C if (b, c) != (3, 5)]
    return out


def head_shapes():
    """(B, C, P, HW) of yogo_bn_bwd_bf16_head: every HW around its 16-pixel stripes, a wavefront's 64 pixels and a workgroup's 1024 at one
    (B, C, P); then, at the first multi-block HW, head outputs P of one operand half (<= 8), both (9..16), one and several channel pairs;
    the 64-workgroup cap."""
    out = [(3, 32, 9, hw) for hw in (1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025)]
    out += [(1, 16, 1, 1025), (1, 16, 8, 1025), (3, 16, 16, 1025), (1, 32, 12, 1025), (3, 128, 12, 1025)]
    return out + [(1, 16, 12, 65540)]


def _seed(*k):
    s = 17
    for v in k:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return s


def bn_case(B, C, HW, bf16, offset=0.0, seed=0):
    """inputs of one apply / backward case: z, g [B][C][HW] fp32 (bf16-valued when ``bf16``) and fp32 per-channel mean, invstd, var, gamma
    (both signs), beta.  mean / invstd are NEAR the batch statistics, not equal to them (the mean terms of the backward stay visible)."""
    gen = torch.Generator().manual_seed(_seed(B, C, HW, bf16, seed))
    z = torch.randn(B, C, HW, generator=gen) * (0.5 + torch.rand(1, C, 1, generator=gen)) + offset + torch.randn(1, C, 1, generator=gen)
    g = torch.randn(B, C, HW, generator=gen) * 0.3
    if bf16:
        z, g = z.to(torch.bfloat16).float(), g.to(torch.bfloat16).float()
    if B * HW > 1:
        mean = z.double().mean((0, 2)) + 0.05
        var = z.double().var((0, 2), unbiased=False) * 1.2 + 1e-3
    else:
        mean = z.double().reshape(C) - 0.3
        var = torch.full((C,), 0.35, dtype=F64)
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    gamma = 0.5 + torch.rand(C, generator=gen)
    gamma[::3] = -gamma[::3]
    beta = torch.randn(C, generator=gen) * 0.3
    return dict(z=z, g=g, mean=mean.float(), invstd=invstd.float(), var=var.float(), gamma=gamma, beta=beta)


def head_case(B, C, P, HW):
    """bn_case(B, C, HW, bf16=True) with g replaced by the head's data gradient g[b][c][i] = sum_k gh[b][k][i] * w[k][c], gh [B][P][HW] and
    w [P][C] integers in {-2..2}: with P <= 16 every g is an integer of magnitude <= 64, exact in bf16 and in fp32 in any order, so the
    kernel's MFMA sum and its bf16 rounding of g are the identity and the reference may take g as given."""
    k = bn_case(B, C, HW, True)
    gen = torch.Generator().manual_seed(_seed(B, C, P, HW, 5))
    k["gh"] = torch.randint(-2, 3, (B, P, HW), generator=gen).float()
    k["w"] = torch.randint(-2, 3, (P, C), generator=gen).float()
    while True:   # no channel without a weight (its g would be all zero): such columns are drawn again
        dead = (k["w"] == 0).all(0)
        if not bool(dead.any()):
            break
        k["w"][:, dead] = torch.randint(-2, 3, (P, int(dead.sum())), generator=gen).float()
    # (+ 0.0: a zero of g is +0 as the kernel's is -- its sum starts from a +0 accumulator -- where 0 * -2 alone would leave -0)
    k["g"] = (torch.einsum("bki,kc->bci", k["gh"].double(), k["w"].double()) + 0.0).float()
    return k


def branch_case(B, C, HW, bf16):
    """bn_case with beta[c] = -fl(fl(xhat) * gamma[c]) for the LAST pixel of image 1 of every channel, xhat as the kernels form it in fp32:
    that element's pre-activation is the rounding residue of one product, within tau of zero, and its fp32 sign is the residue's -- the
    element whose LeakyReLU branch may legitimately differ from the float64 reference's.  A handful of elements: inside the cap."""
    k = bn_case(B, C, HW, bf16, seed=1)
    b = min(1, B - 1)
    xh32 = (k["z"][b, :, HW - 1] - k["mean"]) * k["invstd"]
    ch = [0, 2] if bf16 else list(range(C))   # (a bf16 z repeats its values: every pixel that shares the chosen one's sits within tau too)
    k["beta"][ch] = -(xh32 * k["gamma"])[ch]
    edge = leaky_edge_mask(k["z"], k["mean"], k["invstd"], k["gamma"], k["beta"])
    assert bool(edge[b, ch, HW - 1].all()) and len(ch) <= int(edge.sum()) <= EDGE_CAP * edge.numel(), int(edge.sum())
    return k


def stats_case(B, C, HW, seed=0):
    """z = bf16(50 + randn): mean^2 / var ~ 2500, the cancellation the fp32 sums of squares must survive"""
    gen = torch.Generator().manual_seed(_seed(B, C, HW, 7, seed))
    return (50.0 + torch.randn(B, C, HW, generator=gen)).to(torch.bfloat16).float()


def clip_both_signs(values):
    """a clip that binds on both sides and not everywhere: 0.9 of the smaller of the largest positive and the largest negative magnitude.
    Asserts that the values allow it (some value above +clip, some below -clip, some strictly inside)."""
    v = values.to(F64).flatten()
    assert bool((v > 0).any()) and bool((v < 0).any()), "the values have one sign only"
    c = 0.9 * min(float(v.max()), float(-v.min()))
    assert bool((v > c).any()) and bool((v < -c).any()) and bool((v.abs() < c).any()), "no clip binds on both sides and not everywhere"
    return float(torch.tensor(c, dtype=torch.float32))   # (the fp32 value the kernel is given)


def partials_case(rows, N, gen):
    return torch.randn(rows, N, generator=gen) * 3 + torch.randn(1, N, generator=gen)


def channel_sum_case(B, C, HW):
    gen = torch.Generator().manual_seed(_seed(B, C, HW, 3))
    return torch.randn(B, C, HW, generator=gen) + 0.2 * torch.randn(1, C, 1, generator=gen)
