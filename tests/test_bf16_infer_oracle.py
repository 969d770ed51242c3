"""The oracle's emulation of the bf16 INFERENCE forward (oracle/yogo_oracle.py: bf16_infer_block_forward / bf16_infer_forward) and the
teacher-forced checker built on it (tests/_util.py: teacher_forced_infer_trace_check), on the host:

1. the folding algebra: the folded form in float64 without any rounding IS the unfolded eval-mode BatchNorm forward (1e-12);
2. the emulation is sane: within the 3e-2 of the fp32 forward that the end-to-end inference tests use;
3. the checker catches seeded defects: a stand-in for a correct kernel (the same block, convolution accumulated in float64, then rounded)
   passes, and each of eight defects applied to ONE layer of a copy of the emulation fails.
"""
import pytest
import torch
import torch.nn.functional as F

import yogo_oracle as O
from _util import infer_bn_state, rel_err, teacher_forced_infer_trace_check, to8c_cpu

AW, AH = 0.0425, 0.0555
STATES = ("initial", "trained", "edges")


def _case(name, classes, hw, B, kind, seed=0):
    spec = O.arch(name, classes)
    x = torch.randint(0, 256, (B, 1, *hw), dtype=torch.uint8, generator=torch.Generator().manual_seed(40 + seed))
    sd = infer_bn_state(O, spec, O.init_state(spec, 1, seed=seed), x, kind, seed=seed)
    return spec, x, sd


_BASE = {}


def _base(kind):
    if kind not in _BASE:   # (computed once, shared, never modified)
        _BASE[kind] = _case("base_model", 7, (104, 136), 3, kind)
    return _BASE[kind]


@pytest.mark.parametrize("kind", STATES)
def test_folded_form_in_float64_is_the_unfolded_batchnorm_forward(kind):
    spec, x, sd = _base(kind)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    want_raw = O.backbone_forward(x.double(), sd64, spec)
    got_raw = O.bf16_infer_forward(x, sd, spec, exact=True)
    assert got_raw.dtype == torch.float64 and bool(torch.isfinite(want_raw).all())
    e = rel_err(got_raw, want_raw)
    print(f"{kind}: raw head, folded against unfolded in float64: {e:.2e}")
    assert e <= 1e-12, (kind, e)
    for inference in (False, True):
        want = O.yogo_forward(x.double(), sd64, spec, AW, AH, inference=inference)
        cxs, cys = O.make_grids(*O.grid_size(spec, *x.shape[-2:]))
        got = O.decode(got_raw, cxs.double(), cys.double(), AW, AH, inference=inference)
        fin = torch.isfinite(want)   # (exp of a clamped width at 80 is inf in both; the edges state reaches it)
        assert torch.equal(fin, torch.isfinite(got))
        e = float(((got - want)[fin]).abs().max() / want[fin].abs().max())
        assert e <= 1e-12, (kind, inference, e)


@pytest.mark.parametrize("kind", STATES)
def test_emulation_stays_within_the_fp32_bound_of_the_inference_tests(kind):
    spec, x, sd = _base(kind)
    want = O.backbone_forward(x.float(), sd, spec)
    taps = {}
    got = O.bf16_infer_forward(x, sd, spec, taps=taps)
    assert all(bool(torch.isfinite(t).all()) for t in taps.values())
    e = rel_err(got, want)
    print(f"{kind}: bf16 inference emulation against the fp32 forward: {e:.2e} of the output range")
    assert e <= 3e-2, (kind, e)
    # bf16-valued everywhere but at the fp32 head
    for i, t in taps.items():
        assert (i == len(spec) - 1) or torch.equal(t, t.to(torch.bfloat16).float()), i


# ---- the checker against seeded defects -------------------------------------------------------------------------------------------
DEFECTS = ("plus_running_mean", "no_eps", "no_beta", "no_conv_bias", "act_before_bias", "right_column_outer_taps", "scale_of_next_channel",
           "padding_not_zeroed")


def _block(i, x_in, sd, spec, l0_mfma, defect=None):
    """a COPY of O.bf16_infer_block_forward(conv64=True) with one switchable defect (test_the_copy_is_the_emulation pins defect=None)"""
    n = len(spec)
    co, k, s, hb, hbn, act, dp = spec[i]
    f64 = torch.float64
    pre = O.conv_prefix(spec, i)
    bias = sd[pre + "bias"].float() if hb else None
    scale = None
    if hbn:
        b = f"model.{i}.1."
        gamma, beta, rm, rv = (sd[b + q].float() for q in ("weight", "bias", "running_mean", "running_var"))
        scale = gamma / torch.sqrt(rv if defect == "no_eps" else rv + O.BN_EPS)
        base = bias if (bias is not None and defect != "no_conv_bias") else torch.zeros_like(scale)
        rm_t = base + rm if defect == "plus_running_mean" else base - rm
        bias = (torch.zeros_like(beta) if defect == "no_beta" else beta) + rm_t * scale
    w = sd[pre + "weight"].float()
    sc_w = scale
    if defect == "scale_of_next_channel":
        sc_w = torch.roll(scale, -1)   # channel c multiplied by the scale of channel c + 1
    wf = w * sc_w[:, None, None, None] if sc_w is not None else w
    wq = wf if (i == 0 and not l0_mfma) else O._rb(wf)
    a = F.conv2d(x_in.to(f64), wq.to(f64), None, stride=s, padding=1 if k == 3 else 0)
    if defect == "right_column_outer_taps":
        assert k == 3
        wc = wq.clone()
        wc[:, :, :, 0] = 0
        wc[:, :, :, 2] = 0
        a[..., -1] = F.conv2d(x_in.to(f64), wc.to(f64), None, stride=s, padding=1)[..., -1]
    if defect == "act_before_bias":
        v = O._act(a.float(), act) + (bias[None, :, None, None] if bias is not None else 0)
    else:
        if bias is not None:
            a = a + bias.to(f64)[None, :, None, None]
        v = O._act(a.float(), act)
    y = v if i == n - 1 else O._rb(v)
    return {"scale": scale, "bias": bias, "y": y}


def _fake_trace(spec, x, sd, at=None, defect=None):
    """what a traced forward would hold if every layer were the float64-accumulated stand-in (and layer ``at`` had ``defect``)"""
    l0_mfma = O.l0_infer_on_matrix_cores(spec, x)
    n = len(spec)
    tc = {}
    cur = x.float()
    for i in range(n):
        S = _block(i, cur, sd, spec, l0_mfma, defect if i == at else None)
        tc[("scale", i)], tc[("bias", i)] = S["scale"], S["bias"]
        if i == n - 1:
            tc[("y", i)] = S["y"]
        else:
            t8 = to8c_cpu(S["y"])
            if i == at and defect == "padding_not_zeroed":
                assert t8.shape[1] * 8 > spec[i][0], "the layer has no padding channel"
                t8[1, -1, 2, 3, 7] = 2.0 ** -20   # ONE element of the last padding channel
            tc[("y", i)] = t8
        cur = S["y"]
    return tc


_SMALL = {}


def _small(kind):
    """half_filters (8 channels after layer 0: padding channels 8..15; a conv bias in front of the BatchNorm of layer 5)"""
    if kind not in _SMALL:
        _SMALL[kind] = _case("half_filters", 7, (40, 56), 2, kind, seed=1)
    return _SMALL[kind]


def test_the_copy_is_the_emulation():
    spec, x, sd = _small("trained")
    l0 = O.l0_infer_on_matrix_cores(spec, x)
    assert l0
    cur = x.float()
    for i in range(len(spec)):
        a = O.bf16_infer_block_forward(i, cur, sd, spec, l0, conv64=True)
        b = _block(i, cur, sd, spec, l0)
        assert torch.equal(a["y"], b["y"]), i
        for q in ("scale", "bias"):
            assert (a[q] is None and b[q] is None) or torch.equal(a[q], b[q]), (i, q)
        cur = a["y"]
    # the direct layer-0 kernel's form (odd size): fp32 weights, unrounded
    xo = x[:, :, :39, :55]
    assert not O.l0_infer_on_matrix_cores(spec, xo)
    a, b = O.bf16_infer_block_forward(0, xo.float(), sd, spec, False, conv64=True), _block(0, xo.float(), sd, spec, False)
    assert torch.equal(a["y"], b["y"])
    assert not torch.equal(a["wq"], O._rb(a["wq"]))


@pytest.mark.parametrize("kind", STATES)
def test_float64_stand_in_passes_the_checker(kind):
    spec, x, sd = _small(kind)
    rec = teacher_forced_infer_trace_check(O, _fake_trace(spec, x, sd), x, spec, sd, f"stand-in {kind}")
    assert len(rec) == len(spec)


# the layer each defect is seeded at (half_filters: BatchNorm at 0, 4, 5; conv bias + BatchNorm at 5; 8 of 16 stored channels used at 0)
# and the state it is visible in: leaving eps out moves a trained scale by 1e-5 / (2 var) -- below an fp32 ulp -- and shows where
# running_var = 0 (the edges state)
_SEED_AT = {"plus_running_mean": (4, "trained"), "no_eps": (4, "edges"), "no_beta": (0, "trained"), "no_conv_bias": (5, "trained"),
            "act_before_bias": (2, "trained"), "right_column_outer_taps": (3, "trained"), "scale_of_next_channel": (5, "trained"),
            "padding_not_zeroed": (0, "trained")}


@pytest.mark.parametrize("defect", DEFECTS)
def test_checker_catches_seeded_defect(defect):
    at, kind = _SEED_AT[defect]
    spec, x, sd = _small(kind)
    tc = _fake_trace(spec, x, sd, at=at, defect=defect)
    with pytest.raises(AssertionError) as ei:
        teacher_forced_infer_trace_check(O, tc, x, spec, sd, f"{defect} at layer {at}")
    print(defect, "->", str(ei.value)[:200])
    # ... and it is the seeded layer that fails: the layers before it pass (the checker is teacher-forced, layer by layer)
    msg = str(ei.value)
    assert (f"L{at} " in msg) or (f", {at}, " in msg), (defect, msg)
