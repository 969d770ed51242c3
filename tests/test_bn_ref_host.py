"""tests/_bn_ref.py (the float64 reference the GPU tests of bn.hip / optim.hip compare against) held to torch itself on the CPU:
F.batch_norm + F.leaky_relu / F.silu under autograd in float64, torch.optim.AdamW in float64, torch's bfloat16 cast.  Agreement 1e-12
relative.  It also runs the input generators of tests/test_gpu_bn_edges.py and asserts the caps that file relies on: at most 0.1 % of a
case's elements within tau of the LeakyReLU branch, and a clip that binds on both sides but not everywhere."""
import pytest
import torch
import torch.nn.functional as F

import _bn_ref as R

F64 = torch.float64
RTOL = 1e-12


def _close(a, b, what):
    a, b = a.to(F64), b.to(F64)
    d = float((a - b).abs().max())
    assert d <= RTOL * (float(b.abs().max()) + 1e-300), (what, d)


def _torch_act(y, act):
    return F.leaky_relu(y, 0.01) if act == R.LEAKY else F.silu(y) if act == R.SILU else y


@pytest.mark.parametrize("act", [R.NONE, R.LEAKY, R.SILU])
@pytest.mark.parametrize("C", [1, 5, 20])
def test_apply_backward_finalize_match_torch(act, C):
    B, H, W = 3, 7, 9
    HW = H * W
    gen = torch.Generator().manual_seed(100 * C + act)
    z = (torch.randn(B, C, H, W, generator=gen, dtype=F64) * 3 + 5).requires_grad_(True)
    gamma = (1 + 0.3 * torch.randn(C, generator=gen, dtype=F64)).requires_grad_(True)
    beta = (0.3 * torch.randn(C, generator=gen, dtype=F64)).requires_grad_(True)
    rm, rv = torch.randn(C, generator=gen, dtype=F64), torch.rand(C, generator=gen, dtype=F64) + 0.5
    rm_t, rv_t = rm.clone(), rv.clone()
    eps, mom = 1e-5, 0.1
    y_t = _torch_act(F.batch_norm(z, rm_t, rv_t, gamma, beta, training=True, momentum=mom, eps=eps), act)
    gy = torch.randn(B, C, H, W, generator=gen, dtype=F64)
    y_t.backward(gy)
    # partial rows as a producer would write them: 4 uneven chunks of the (b, h, w) range, row stride C + 3 with junk behind C
    zc = z.detach().permute(1, 0, 2, 3).reshape(C, -1)
    cuts = [0, 5, 6, 100, B * HW]
    part = torch.full((4, C + 3, 2), 1000.0, dtype=F64)
    for r in range(4):
        c = zc[:, cuts[r]:cuts[r + 1]]
        part[r, :C, 0], part[r, :C, 1] = c.sum(1), (c * c).sum(1)
    mean, invstd, rm2, rv2, nbt = R.finalize(part[:, :C], B * HW, eps, mom, rm, rv, nbt=4)
    assert nbt == 5
    _close(mean, zc.mean(1), "mean")
    _close(invstd, 1.0 / torch.sqrt(zc.var(1, unbiased=False) + eps), "invstd")
    _close(rm2, rm_t, "running_mean")
    _close(rv2, rv_t, "running_var")
    z3, g3 = z.detach().reshape(B, C, HW), gy.reshape(B, C, HW)
    _close(R.apply(z3, mean, invstd, 0, eps, gamma.detach(), beta.detach(), act), y_t.detach().reshape(B, C, HW), "apply (training)")
    dz, dgamma, dbeta, y64 = R.backward(g3, z3, mean, invstd, gamma.detach(), beta.detach(), act, 1, 0.0)
    _close(dz, z.grad.reshape(B, C, HW), "dz")
    _close(dgamma, gamma.grad, "dgamma")
    _close(dbeta, beta.grad, "dbeta")
    _close(y64, F.batch_norm(z.detach(), None, None, gamma.detach(), beta.detach(), training=True, eps=eps).reshape(B, C, HW), "pre-activation")
    # eval mode: running statistics, stat_is_var = 1; the frozen backward (training = 0) is autograd through the same call
    z2 = z.detach().clone().requires_grad_(True)
    ga2, be2 = gamma.detach().clone().requires_grad_(True), beta.detach().clone().requires_grad_(True)
    y_e = _torch_act(F.batch_norm(z2, rm, rv, ga2, be2, training=False, eps=eps), act)
    y_e.backward(gy)
    _close(R.apply(z3, rm, rv, 1, eps, gamma.detach(), beta.detach(), act), y_e.detach().reshape(B, C, HW), "apply (eval)")
    dz0, dg0, db0, _ = R.backward(g3, z3, rm, 1.0 / torch.sqrt(rv + eps), gamma.detach(), beta.detach(), act, 0, 0.0)
    _close(dz0, z2.grad.reshape(B, C, HW), "dz (frozen)")
    _close(dg0, ga2.grad, "dgamma (frozen)")
    _close(db0, be2.grad, "dbeta (frozen)")
    # clip acts on dgamma / dbeta only
    clip = R.clip_both_signs(torch.cat([dgamma, dbeta])) if C > 1 else 0.5 * float(dgamma.abs().max())
    dzc, dgc, dbc, _ = R.backward(g3, z3, mean, invstd, gamma.detach(), beta.detach(), act, 1, clip)
    assert torch.equal(dzc, dz) and torch.equal(dgc, dgamma.clamp(-clip, clip)) and torch.equal(dbc, dbeta.clamp(-clip, clip))


def test_finalize_edges():
    # count == 1: the biased variance goes into running_var; a negative variance is clamped
    part = torch.tensor([[[3.0, 9.0], [2.0, 3.9]]], dtype=F64)   # channel 1: q - mean^2 = -0.1
    mean, invstd, rm, rv, nbt = R.finalize(part, 1, 1e-5, 0.1, torch.zeros(2, dtype=F64), torch.ones(2, dtype=F64))
    assert torch.equal(mean, torch.tensor([3.0, 2.0], dtype=F64))
    _close(invstd, torch.full((2,), 1e-5, dtype=F64).rsqrt(), "invstd of a zero variance")
    _close(rv, torch.tensor([0.9, 0.9], dtype=F64), "running_var, count 1")
    assert nbt == 1
    m2 = R.finalize(part, 1, 1e-5, 0.1)
    assert m2[2] is None and m2[3] is None


def test_leaky_factor_at_zero_is_the_slope():
    y = torch.tensor([0.0, -0.0, 1e-300, -1e-300], dtype=F64)
    assert R.act_factor(y, R.LEAKY).tolist() == [0.01, 0.01, 1.0, 0.01]
    x = y.clone().requires_grad_(True)
    F.leaky_relu(x, 0.01).sum().backward()
    assert x.grad.tolist() == [0.01, 0.01, 1.0, 0.01]


@pytest.mark.parametrize("grad_scale", [1.0, 0.25])
def test_adamw_matches_torch(grad_scale):
    gen = torch.Generator().manual_seed(3)
    n = 257
    p0 = torch.randn(n, generator=gen, dtype=F64)
    pt = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([pt], lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-2)
    p, m, v = p0.clone(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    for step in range(1, 6):
        g = torch.randn(n, generator=gen, dtype=F64) * 0.1
        lr = 3e-4 * (1 - 0.1 * step)
        for grp in opt.param_groups:
            grp["lr"] = lr
        pt.grad = g * grad_scale
        opt.step()
        p, m, v = R.adamw(p, g, m, v, step, lr, (0.9, 0.999), 1e-8, 5e-2, grad_scale)
        st = opt.state[pt]
        _close(p, pt.detach(), "p")
        _close(m, st["exp_avg"], "m")
        _close(v, st["exp_avg_sq"], "v")


@pytest.mark.parametrize("C", [1, 5, 16, 20])
def test_8c_layout_round_trip(C):
    gen = torch.Generator().manual_seed(C)
    B, HW = 3, 11
    x = torch.randn(B, C, HW, generator=gen)
    t = R.to8c(x)
    Cb = R.cb_of(C)
    assert t.shape == (B, Cb, HW, 8) and t.dtype == torch.bfloat16 and Cb * 8 == ((C + 15) // 16) * 16
    for b, c, i in ((0, 0, 0), (B - 1, C - 1, HW - 1), (1, C // 2, 5)):
        assert float(t[b, c // 8, i, c % 8]) == float(x[b, c, i].to(torch.bfloat16))
    assert bool((R.pad_lanes(t, C) == 0).all())
    assert torch.equal(R.from8c(t, C), x.to(torch.bfloat16).float())
    junk = R.to8c(x, pad=1000.0)
    assert bool((R.pad_lanes(junk, C) == 1000.0).all()) and torch.equal(R.from8c(junk, C), R.from8c(t, C))


# ---- the generators of the GPU tests: the caps those tests rely on ----------------------------------------------------------------------
def _cases():
    return [(False,) + s for s in R.f32_shapes()] + [(True,) + s for s in R.bf16_shapes()]


def test_shape_lists_are_what_the_tiling_needs():
    f, h = R.f32_shapes(), R.bf16_shapes()
    assert {s[2] for s in f} == set(R.F32_HW) and {s[2] for s in h} == set(R.BF16_HW)
    assert {(b, c) for b, c, hw in f if hw == 2049} == {(b, c) for b in R.BS for c in R.F32_C}
    assert {(b, c) for b, c, hw in h if hw == 1025} == {(b, c) for b in R.BS for c in R.BF16_C}
    assert [s for s in f if s[2] == 131076] == [(1, 2, 131076)] and [s for s in h if s[2] == 65540] == [(1, 16, 65540)]
    assert max(b * c * hw for b, c, hw in f) * 4 <= 2 ** 21 and max(b * R.cb_of(c) * 8 * hw for b, c, hw in h) * 2 <= 2 ** 22


@pytest.mark.parametrize("bf16,B,C,HW", _cases())
def test_generated_cases_stay_within_the_edge_cap(bf16, B, C, HW):
    """|y64| <= tau on at most 0.1 % of the elements (the only elements whose LeakyReLU branch the GPU tests accept either way), and the
    clip the backward tests use binds on both sides but not on every channel"""
    k = R.bn_case(B, C, HW, bool(bf16))
    edge = R.leaky_edge_mask(k["z"], k["mean"], k["invstd"], k["gamma"], k["beta"])
    n = edge.numel()
    assert int(edge.sum()) <= R.EDGE_CAP * n, (int(edge.sum()), n)
    assert bool(torch.isfinite(k["invstd"]).all()) and float(k["invstd"].min()) > 0
    if bf16:
        assert torch.equal(k["z"], k["z"].to(torch.bfloat16).float()) and torch.equal(k["g"], k["g"].to(torch.bfloat16).float())
    if C >= 5:
        for act in (R.NONE, R.LEAKY, R.SILU):
            _, dg, db, _ = R.backward(k["g"], k["z"], k["mean"], k["invstd"], k["gamma"], k["beta"], act, 1, 0.0)
            R.clip_both_signs(torch.cat([dg, db]))   # asserts


def test_head_shape_list_is_what_the_tiling_needs():
    s = R.head_shapes()
    assert {hw for b, c, p, hw in s if (b, c, p) == (3, 32, 9)} == {1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025}
    assert {(b, c, p) for b, c, p, hw in s if hw == 1025} == {(3, 32, 9), (1, 16, 1), (1, 16, 8), (3, 16, 16), (1, 32, 12), (3, 128, 12)}
    assert [x for x in s if x[3] == 65540] == [(1, 16, 12, 65540)] and len(s) == 16
    assert all(c % 16 == 0 and 1 <= p <= 16 for b, c, p, hw in s) and max(b * c * hw for b, c, p, hw in s) * 2 <= 2 ** 22


@pytest.mark.parametrize("B,C,P,HW", R.head_shapes())
def test_head_cases_have_an_exact_gradient_within_the_caps(B, C, P, HW):
    """g = sum_k gh w is an integer of magnitude <= 64: its own bf16 value, so the kernel's rounding of g is the identity; no channel of g is
    all zero; z stays within the edge cap; and at the multi-block HW the clip of the backward tests binds on both sides"""
    k = R.head_case(B, C, P, HW)
    g, gh, w = k["g"], k["gh"], k["w"]
    assert gh.shape == (B, P, HW) and w.shape == (P, C) and g.shape == (B, C, HW)
    for t in (gh, w):
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= 2
    assert torch.equal(g, g.to(torch.bfloat16).float()) and torch.equal(g, g.round()) and float(g.abs().max()) <= 4 * P <= 64
    assert torch.equal(g, torch.einsum("bki,kc->bci", gh, w))          # fp32, another order: the same integers
    assert not bool(torch.signbit(g[g == 0]).any()), "a zero of g is -0: the kernel's sum gives +0, the bit comparison would see it"
    assert bool((g != 0).any(2).any(0).all()), "a channel of g is all zero"
    assert torch.equal(k["z"], R.bn_case(B, C, HW, True)["z"])
    edge = R.leaky_edge_mask(k["z"], k["mean"], k["invstd"], k["gamma"], k["beta"])
    assert int(edge.sum()) <= R.EDGE_CAP * edge.numel(), (int(edge.sum()), edge.numel())
    if HW == 1025:
        for act in (R.NONE, R.LEAKY, R.SILU):
            _, dg, db, _ = R.backward(g, k["z"], k["mean"], k["invstd"], k["gamma"], k["beta"], act, 1, 0.0)
            R.clip_both_signs(torch.cat([dg, db]))   # asserts


@pytest.mark.parametrize("bf16,B,C,HW", [(False, 3, 5, 2049), (True, 3, 5, 1025)])
def test_branch_case_puts_a_few_elements_within_tau(bf16, B, C, HW):
    k = R.branch_case(B, C, HW, bf16)   # asserts: those elements are within tau, and the case stays within the cap
    _, _, _, y = R.backward(k["g"], k["z"], k["mean"], k["invstd"], k["gamma"], k["beta"], R.LEAKY, 1, 0.0)
    ch = [0, 2] if bf16 else list(range(C))
    assert float(y[1, ch, HW - 1].abs().max()) < 1e-6


def test_stats_case_has_the_cancellation():
    z = R.stats_case(3, 5, 1025).double()
    ratio = z.mean((0, 2)) ** 2 / z.var((0, 2), unbiased=False)
    assert float(ratio.min()) > 2000 and float(ratio.max()) < 3200, ratio


def test_reduction_cases_allow_a_clip_on_both_sides():
    for rows in (1, 7, 8, 9, 64, 65, 128, 129, 513, 577):
        gen = torch.Generator().manual_seed(rows)
        for N in (1, 255, 256, 257):
            S = R.partials_case(rows, N, gen).double().sum(0)
            if N > 1:
                R.clip_both_signs(S)
    for B in (1, 3):
        for HW in (255, 257, 2049):
            R.clip_both_signs(R.channel_sum_case(B, 5, HW).double().sum((0, 2)))
