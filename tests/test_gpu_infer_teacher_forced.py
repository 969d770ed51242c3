"""The bf16 INFERENCE forward (`yogo infer`'s path: yogo_amd/engine.py InferEngineBF16, eval-mode BatchNorm folded on the host), layer by
layer against the oracle's folded bf16-storage emulation (oracle/yogo_oracle.py: bf16_infer_block_forward), with BatchNorm states a
trained network has -- where a wrong sign on running_mean, a dropped beta, eps on the wrong side or a conv bias lost in front of
BatchNorm are visible (they are not at running_mean 0, gamma 1, beta 0).

Per case (the smallest shapes that reach the inference kernels; tests/golden/launch_plans.json):
  * the launch log of a TRACED forward equals that of an untraced one line for line, and the two outputs are the same bits;
  * teacher-forced (tests/_util.py: teacher_forced_infer_check): every layer's stored output given the forward's own stored input to one
    bf16 ulp, the fp32 head to 3e-5, the folded scale / bias to 2 fp32 ulp, padding channels exactly zero, everything finite;
  * end to end: `model.model(x)` against O.bf16_infer_forward(x) on the raw head output within BF16_INFER_E2E_RTOL (measured, _util.py);
  * `model(x)`: heads of 6 .. 16 channels run head + decode as ONE launch (conv_bf16_1x1_f32_kernel<., true>), the 17-channel head shows
    the fallback (conv_bf16_1x1_f32_kernel<., false> + decode_fwd_kernel); either way the bits of forward_raw(x).decoded().
Kernel coverage: the union of the cases' convolution launches holds every conv_bf16* / conv_first* entry of the newest committed
profile of the batch-256 inference path (profiles/r*_infer_kernel_stats.txt) -- the small shapes reach every member, none is excused.

Then entry points no other test calls in this form: yogo_conv_bf16_pack WITH a scale (training never passes one), the bytes of
yogo_conv_bf16_pack and yogo_conv_bf16_pack_multi against a numpy packing of the documented layout, and the direct layer-0 kernel
yogo_conv_first_fwd_bf16 alone against float64 with a derived bound."""
import glob
import os
import re

import pytest
import torch

import yogo_oracle as O

pytestmark = pytest.mark.gpu

AW, AH = 0.0425, 0.0555

# (id, architecture, classes, (H, W), rgb, batch, float input, BatchNorm state)
CASES = [
    ("base_104x136_trained", "base_model", 7, (104, 136), False, 3, False, "trained"),      # matrix-core layer 0; ws, ws3, both staged
    ("base_104x136_edges", "base_model", 7, (104, 136), False, 3, False, "edges"),
    ("base_104x136_initial", "base_model", 7, (104, 136), False, 3, False, "initial"),
    ("base_97x131_direct_u8", "base_model", 7, (97, 131), False, 3, False, "trained"),       # odd sizes: yogo_conv_first_fwd_bf16 on uint8
    ("base_104x136_float_input", "base_model", 7, (104, 136), False, 2, True, "trained"),    # the direct kernel with in_dtype = 1
    ("quarter_130x70_rgb", "quarter_filters", 7, (130, 70), True, 2, False, "trained"),      # three input channels; 4 / 8 channel layers
    ("silu_96x128", "silu_model", 7, (96, 128), False, 2, False, "trained"),                 # SiLU epilogues
    ("depth0_104x136", "depth_ver_0", 7, (104, 136), False, 2, False, "trained"),            # BatchNorm under the head
    ("triple_64x96", "triple_filters", 7, (64, 96), False, 2, False, "trained"),             # widths to 384: the tiled kernels
    ("half_193x258", "half_filters", 7, (193, 258), False, 2, False, "trained"),             # larger planes, several tiles per band
    ("base_104x136_P6", "base_model", 1, (104, 136), False, 2, False, "trained"),            # the smallest fusable head
    ("base_104x136_P16", "base_model", 11, (104, 136), False, 2, False, "trained"),          # the largest fusable head
    ("base_104x136_P17", "base_model", 12, (104, 136), False, 2, False, "trained"),          # the unfused head: the fallback
]
IDS = [c[0] for c in CASES]


def _images(case):
    _, name, classes, (H, W), rgb, B, as_float, kind = case
    g = torch.Generator().manual_seed(11)
    x = torch.randint(0, 256, (B, 3 if rgb else 1, H, W), dtype=torch.uint8, generator=g)
    if as_float:   # not 8-bit values: fractions, a sign, a few large pixels
        x = x.float() - 100.0 + torch.rand(x.shape, generator=g)
        x[:, :, ::17, ::13] *= 8.0
    return x


def _model(case, sd=None):
    from yogo_amd.model import YOGO
    from yogo_amd.model_defns import MODELS

    _, name, classes, (H, W), rgb, B, as_float, kind = case
    torch.manual_seed(21)
    m = YOGO((H, W), AW, AH, classes, is_rgb=rgb, model_func=MODELS[name]).cuda().eval()
    if sd is not None:
        m.load_state_dict(sd)
    return m


def _conv_kernels(log):
    """name<template arguments> of the convolution launches of a launch log"""
    out = set()
    for ln in log:
        k = re.sub(r"\s+", "", ln.split("|")[0])
        if k.startswith("conv_bf16") or k.startswith("conv_first"):
            out.add(k)
    return out


def _logged(fn):
    from yogo_amd import _hip

    _hip.launch_log(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        log = _hip.read_launch_log()
    finally:
        _hip.launch_log(False)
    return out, log


def _assert_head_plan(case, log_model_call):
    """stated from the rule of the fused head + decode kernel (engine.head_decode_fusable: a bare 1x1 head of 6 .. 16 channels over a
    multiple of 16 and at most 128 channels), not from what the engine did"""
    P = 5 + case[2]
    cin = O.arch(case[1], case[2])[-2][0]
    names = [ln.split("|")[0].strip() for ln in log_model_call]
    if 6 <= P <= 16 and cin % 16 == 0 and cin <= 128:
        assert any(n.startswith("conv_bf16_1x1_f32_kernel<") and n.endswith(", true>") for n in names), (case[0], "head + decode must be one launch", names)
        assert not any(n.startswith("decode_fwd_kernel") for n in names), (case[0], names)
    else:
        if cin % 16 == 0 and cin <= 128:   # (wider inputs, triple_filters' 384: the tiled kernel with the fp32 epilogue)
            assert any(n.startswith("conv_bf16_1x1_f32_kernel<") and n.endswith(", false>") for n in names), (case[0], "the unfused head", names)
        assert any(n.startswith("decode_fwd_kernel") for n in names), (case[0], "the fallback decodes in a launch of its own", names)
        assert not any(n.endswith(", true>") and n.startswith("conv_bf16_1x1_f32_kernel<") for n in names), (case[0], names)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_inference_forward_layer_by_layer_against_the_bf16_oracle(case):
    from _util import BF16_INFER_E2E_RTOL, infer_bn_state, teacher_forced_infer_check
    from yogo_amd.engine import get_engine

    cid, name, classes, hw, rgb, B, as_float, kind = case
    spec = O.arch(name, classes)
    x = _images(case)
    m = _model(case)
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    sd = infer_bn_state(O, spec, sd0, x, kind, seed=len(cid))
    m.load_state_dict(sd)
    xc = x.cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        m.model(xc)   # (folds and packs: the two logged forwards below start from the same cache)
        inf = get_engine(m.model)._infer_bf16
        assert inf is not None and inf.supported() and inf.trace is None
        raw_u, log_u = _logged(lambda: m.model(xc))
        inf.trace = {}
        try:
            raw, log_t = _logged(lambda: m.model(xc))
            assert log_t == log_u and len(log_t) == len(spec), ("a trace must not change the plan", log_u, log_t)
            assert torch.equal(raw.view(torch.int32), raw_u.view(torch.int32))
            assert raw.dtype == torch.float32 and raw.shape[:2] == (B, 5 + classes)
            print("\n".join(log_t))
            # ---- layer by layer, given the forward's own stored inputs
            teacher_forced_infer_check(O, m, x, spec, sd, cid)
        finally:
            inf.trace = None
        # ---- end to end, raw head output
        want = O.bf16_infer_forward(x, sd, spec)
        e2e = float((raw.cpu() - want).abs().max() / want.abs().max())
        print(f"[{cid}] end to end: max|d| / max|ref| = {e2e:.3e} (bound {BF16_INFER_E2E_RTOL})")
        assert e2e <= BF16_INFER_E2E_RTOL, (cid, e2e)
        # ---- model(x): the head's plan, and the bits of the two launches
        m.inference = True
        dec, log_d = _logged(lambda: m(xc))
        _assert_head_plan(case, log_d)
        two = m.forward_raw(xc).decoded()
        assert torch.equal(dec.view(torch.int32), two.view(torch.int32))


def test_cases_reach_every_convolution_kernel_of_the_inference_profile():
    """the dispatch does not depend on tensor contents: the cases' launches are taken from freshly initialised models"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    profs = sorted(glob.glob(os.path.join(root, "profiles", "r*_infer_kernel_stats.txt")))
    assert profs
    want = set()
    for ln in open(profs[-1]):
        if ln.startswith("# rocprofv3") and "post" in ln:
            break   # (the second table is the post-process alone on synthetic predictions)
        mm = re.match(r"(?:void\s+)?((?:conv_bf16|conv_first)\w*(?:<[^>]*>)?)", ln)
        if mm:
            want.add(re.sub(r"\s+", "", mm.group(1)))
    assert len(want) >= 8, want
    launched = set()
    for case in CASES:
        m = _model(case)
        xc = _images(case).cuda()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            _, log_a = _logged(lambda: m.model(xc))   # (the first forward: the weight packing is part of the path)
            _, log_b = _logged(lambda: m(xc))
        launched |= _conv_kernels(log_a) | _conv_kernels(log_b)
    print(sorted(launched))
    assert not (want - launched), (sorted(want - launched), sorted(launched))
    # the direct layer-0 kernel is in no profile of the 772x1032 path; the odd, rgb and float cases must have reached it
    assert {"conv_first_bf16_kernel<uint8_t,1>", "conv_first_bf16_kernel<uint8_t,3>", "conv_first_bf16_kernel<float,1>"} <= launched, sorted(launched)


# ---- yogo_conv_bf16_pack with a scale ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cin,Cout,k", [(16, 32, 3), (128, 128, 3), (24, 40, 3), (128, 12, 1), (64, 7, 1)])
def test_pack_with_a_scale_is_the_pack_of_the_scaled_weights(Cin, Cout, k):
    """mode 0: pack(w, scale) == pack(w * scale[:, None, None, None]) bit for bit (the product formed in fp32 by torch: the same single
    rounding before the bf16 one).  Modes 1 and 2 (the data gradients' packings) ignore the scale: the same bits with and without it."""
    from yogo_amd import _hip

    g = torch.Generator().manual_seed(Cin * 1000 + Cout)
    w = (torch.randn(Cout, Cin, k, k, generator=g) * 0.1).cuda()
    scale = torch.randn(Cout, generator=g)
    scale[0] = 0.0
    scale[-1] = 316.2
    scale = scale.cuda()
    st = _hip.stream_ptr()

    def pack(wt, sc, mode):
        nbytes = _hip.query_size("yogo_conv_bf16_packed_bytes", Cin, Cout, k, mode)
        buf = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
        _hip.call("yogo_conv_bf16_pack", wt.contiguous(), sc, buf, Cin, Cout, k, mode, st)
        torch.cuda.synchronize()
        return buf.cpu()

    a = pack(w, scale, 0)
    b = pack(w * scale[:, None, None, None], None, 0)
    assert torch.equal(a, b), int((a != b).sum())
    assert not torch.equal(a, pack(w, None, 0))   # (the scale does reach the kernel)
    for mode in (1, 2) if k == 3 else (1,):
        assert torch.equal(pack(w, scale, mode), pack(w, None, mode)), mode


# ---- the two packing kernels write one layout ---------------------------------------------------------------------------------------
# (Cin, Cout, ks, mode): channel counts 7 and 12 are padded to 16 contraction channels / 32 GEMM rows; 128 -> 7 has Mpad = 32 (one
# 32-row tile) against Kb = 16 channel blocks; mode 2 stores the taps in the parity-class order of the stride-2 data gradient
PACK_CASES = ((16, 32, 3, 0), (32, 16, 3, 1), (64, 128, 3, 2), (128, 7, 1, 0), (12, 7, 1, 1), (7, 12, 3, 0))


def _pack_numpy(w, scale, ks, mode):
    """the layout comment of conv_bf16_pack.hip: [T][Kb][Mpad] units of 8 contraction channels of one GEMM row; mode 0: k = ci, m = co,
    weights times scale[co]; modes 1 / 2: k = co, m = ci, taps flipped; mode 2: slice t holds tap nibble t of 0x862071534; zero padding"""
    import numpy as np

    Cout, Cin = w.shape[:2]
    Kc, Mc = (Cout, Cin) if mode else (Cin, Cout)
    Kb = (Kc + 15) // 16 * 2
    tile = 32 * (1 if Mc <= 32 else 2 if Mc <= 64 else 4)
    Mpad = (Mc + tile - 1) // tile * tile
    T = ks * ks
    full = np.zeros((T, Kb * 8, Mpad), dtype=np.float32)
    for t in range(T):
        ts = (0x862071534 >> (4 * t)) & 15 if mode == 2 else t
        tt = T - 1 - ts if mode else ts
        tap = w[:, :, tt // ks, tt % ks]   # [co][ci]
        if mode:
            full[t, :Cout, :Cin] = tap
        else:
            full[t, :Cin, :Cout] = (tap * scale[:, None] if scale is not None else tap).T
    units = np.ascontiguousarray(full.reshape(T, Kb, 8, Mpad).transpose(0, 1, 3, 2))
    u = units.view(np.uint32)
    bf = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype("<u2")   # round to nearest even (finite values)
    return bf.tobytes()


@pytest.mark.parametrize("scaled", [False, True])
def test_pack_multi_and_pack_write_the_layout_of_the_comment(scaled):
    """yogo_conv_bf16_pack_multi for a table of all the cases == one yogo_conv_bf16_pack per case == the numpy packing, byte for byte
    (scaled: the mode-0 cases take a per-output-channel scale)"""
    from yogo_amd import _hip

    st = _hip.stream_ptr()
    g = torch.Generator().manual_seed(7)
    ws, scs, singles, multis, rows, blk = [], [], [], [], [], 0
    for Cin, Cout, ks, mode in PACK_CASES:
        w = (torch.randn(Cout, Cin, ks, ks, generator=g) * 0.1).cuda()
        sc = (torch.randn(Cout, generator=g) + 2.0).cuda() if scaled and mode == 0 else None
        nbytes = _hip.query_size("yogo_conv_bf16_packed_bytes", Cin, Cout, ks, mode)
        one = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
        _hip.call("yogo_conv_bf16_pack", w, sc, one, Cin, Cout, ks, mode, st)
        multi = torch.full((nbytes,), 0xCD, dtype=torch.uint8, device="cuda")
        rows.append([w.data_ptr(), sc.data_ptr() if sc is not None else 0, multi.data_ptr(), Cin, Cout, ks, mode, blk])
        blk += _hip.query_ints("yogo_conv_bf16_pack_blocks", 1, Cin, Cout, ks, mode)[0]
        ws.append(w); scs.append(sc); singles.append(one); multis.append(multi)
    table = torch.tensor(rows, dtype=torch.int64, device="cuda")
    _hip.call("yogo_conv_bf16_pack_multi", table, len(rows), blk, st)
    torch.cuda.synchronize()
    for case, w, sc, one, multi in zip(PACK_CASES, ws, scs, singles, multis):
        want = _pack_numpy(w.cpu().numpy(), sc.cpu().numpy() if sc is not None else None, case[2], case[3])
        assert len(want) == one.numel(), (case, len(want), one.numel())
        assert one.cpu().numpy().tobytes() == want, (case, "yogo_conv_bf16_pack")
        assert multi.cpu().numpy().tobytes() == want, (case, "yogo_conv_bf16_pack_multi")


# ---- yogo_conv_first_fwd_bf16 alone -----------------------------------------------------------------------------------------------
# Bound (derived, not measured), per element, ref = the float64 result:
#   one bf16 rounding of the fp32 value                         2^-8 |ref|
#   the fp32 fma chain of 9 Cin products, the bias add and the activation's multiply: (9 Cin + 2) roundings of at most 2^-24 of the
#     running magnitude, which sum |w x| + |bias| bounds          (9 Cin + 2) 2^-24 (sum |w x| + |bias|)
#     (LeakyReLU scales it by <= 1, SiLU by <= 1.1 = max |silu'|; the bf16 rounding acts on the fp32 value: a factor 1 + 2^-8)
#   SiLU = v / (1 + __expf(-v)) (common.h: act_fwd).  The compiler's HIP math header defines __expf(t) as the hardware exp2 of
#     fl(log2(e)) * t (__clang_hip_math.h: __builtin_amdgcn_exp2f, the v_exp_f32 instruction, 1 ulp = 2^-23 in AMD's instruction set
#     reference).  Rounding the constant and the product moves the exponent by 1.5 * 2^-24 |t| log2(e), i.e. the result by
#     1.5 * 2^-24 |t| relative; the add and the correctly rounded division (-fhip-fp32-correctly-rounded-divide-sqrt) are one rounding
#     each: relative (1.5 |v| + 4) 2^-24 of |ref| in all, taken here as                2^-22 (2 + |v|) |ref|
NONE, LEAKY, SILU = 0, 1, 2


@pytest.mark.parametrize("Cin,as_float", [(1, False), (1, True), (3, False), (3, True)])
def test_conv_first_fwd_bf16_against_float64(Cin, as_float):
    import torch.nn.functional as F

    from yogo_amd import _hip

    st = _hip.stream_ptr()
    B = 2
    worst = 0.0
    for (H, W) in ((37, 53), (9, 7), (1, 1), (2, 1)):   # (the last two: every tap but the centre is padding; stride 2 leaves one output)
        g = torch.Generator().manual_seed(H * 100 + Cin)
        n = B * Cin * H * W
        esz = 4 if as_float else 1
        lead = (-n * esz) % 512 // esz + 512 // esz   # the batch is the TAIL of its allocation: the second image ends it
        if as_float:
            vals = (torch.rand(lead + n, generator=g) * 300.0 - 40.0)
        else:
            vals = torch.randint(0, 256, (lead + n,), dtype=torch.uint8, generator=g)
        big = vals.cuda()
        xd = big[lead:].view(B, Cin, H, W)
        assert xd.is_contiguous() and xd.data_ptr() + n * esz == big.data_ptr() + big.numel() * esz
        x64 = vals[lead:].view(B, Cin, H, W).double()
        for Cout in (7, 16, 20):
            w = torch.randn(Cout, Cin, 3, 3, generator=g) * 0.05
            bias_t = torch.randn(Cout, generator=g) * 3.0
            mb = _hip.lib().yogo_bf16_channel_blocks(Cout)
            assert mb == ((Cout + 15) // 16) * 2
            for stride in (1, 2):
                OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
                pre0 = F.conv2d(x64, w.double(), None, stride=stride, padding=1)
                mag0 = F.conv2d(x64.abs(), w.double().abs(), None, stride=stride, padding=1)
                for has_bias in (True, False):
                    pre = pre0 + bias_t.double()[None, :, None, None] if has_bias else pre0
                    mag = mag0 + bias_t.double().abs()[None, :, None, None] if has_bias else mag0
                    for act in (NONE, LEAKY, SILU):
                        out = torch.full((B, mb, OH, OW, 8), float("nan"), dtype=torch.bfloat16, device="cuda")
                        _hip.call("yogo_conv_first_fwd_bf16", xd, 1 if as_float else 0, w.cuda(), bias_t.cuda() if has_bias else None, out,
                                  B, Cin, Cout, H, W, stride, act, st)
                        torch.cuda.synchronize()
                        full = out.cpu().float().permute(0, 1, 4, 2, 3).reshape(B, mb * 8, OH, OW)   # (host permute: no helper kernel measures)
                        assert bool(torch.isfinite(full).all()), (H, W, Cout, stride, act, "every element is written")
                        assert int((full[:, Cout:] != 0).sum()) == 0, (H, W, Cout, stride, act, "padding channels")
                        if act == LEAKY:
                            ref = torch.where(pre > 0, pre, O.LEAKY_SLOPE * pre)
                        elif act == SILU:
                            ref = pre * torch.sigmoid(pre)
                        else:
                            ref = pre
                        bound = 2.0 ** -8 * ref.abs() + (1 + 2.0 ** -8) * 1.1 * (9 * Cin + 2) * 2.0 ** -24 * mag
                        if act == SILU:
                            bound = bound + 2.0 ** -22 * (2 + pre.abs()) * ref.abs()
                        d = (full[:, :Cout].double() - ref).abs()
                        ratio = float((d / bound.clamp_min(1e-300)).max())
                        worst = max(worst, ratio)
                        assert ratio <= 1.0, (H, W, Cout, stride, has_bias, act, ratio)
    print(f"conv_first_fwd_bf16 Cin={Cin} {'float32' if as_float else 'uint8'}: worst |d| / bound = {worst:.3f}")
