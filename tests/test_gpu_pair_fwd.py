"""Layers 1 + 2 forward in one launch (yogo_conv2d_fwd_bf16_signs_pair -> conv_bf16_staged_pair_kernel: layer 2 reads y1 from LDS) against
the pair it replaces: yogo_conv2d_fwd_bf16_signs called twice.  Every stored tensor -- y1, y2, both sign maps -- must be the SAME BYTES
(torch.equal): the fused kernel issues the same products in the same order per accumulator and the same epilogue, and layer 2 multiplies the
very bf16 units layer 1 stores.  The output buffers start as NaN / 0xA5, so a unit that no tile owns shows, and one that two tiles own with
different values (a neighbour's halo column evaluated on other inputs) shows against the reference.

The shapes are the edges of the tiling: a tile is 1 row x 31 columns of y2 = 3 x 63 of y1 (two 32-pixel MFMA blocks), so 7x63 / 8x64 / 9x65 is
one tile +- 1 column with odd and even row counts, 6x125 / 126 / 127 two tiles +- 1, 33x130 several of both, and the 1- and 2-pixel planes
put every tap of layer 2 on the padding.  Layer 2's taps outside y1's plane must read ZEROS, never layer 1 evaluated on padded y0: the
adversarial case makes every y1 value near the border strongly positive (bias 8), so that a non-zero "padding" moves y2 by whole units.

Independent reference on the small shapes: torch's CPU float64 convolution of the same bf16-rounded operands (layer 2 on the STORED y1) at
the bound the staged kernels are held to in tests/test_gpu_ws.py: 2^-8 |want| + 2e-5 max |want| (one bf16 rounding of the result).
Reference rows: yogo/model_defns.py:39-46."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

PAIR = "conv_bf16_staged_pair_kernel<"
STAGED1, STAGED2 = "conv_bf16_staged_kernel<1,", "conv_bf16_staged_kernel<2,"


def _blocks(c):
    return ((c + 15) // 16) * 2


def _names(log):
    return {ln.split("|")[0].replace(" ", "") for ln in log}


def _inputs(B, C1, C2, IH, IW, scales, seed, bias_shift=0.0):
    from yogo_amd import _hip as Hh

    st = Hh.stream_ptr()
    g = torch.Generator(device="cuda").manual_seed(seed)
    x8 = torch.randn(B, 2, IH, IW, 8, device="cuda", generator=g).to(torch.bfloat16)
    w1 = torch.randn(C1, 16, 3, 3, device="cuda", generator=g) * 0.08
    w2 = torch.randn(C2, C1, 3, 3, device="cuda", generator=g) * 0.06
    b1 = torch.randn(C1, device="cuda", generator=g) * 0.5 + bias_shift
    b2 = torch.randn(C2, device="cuda", generator=g) * 0.5
    m1 = (torch.rand(B, C1, device="cuda", generator=g) > 0.2).float() / 0.8 if scales else None
    m2 = (torch.rand(B, C2, device="cuda", generator=g) > 0.2).float() / 0.8 if scales else None
    pk = []
    for w, ci, co in ((w1, 16, C1), (w2, C1, C2)):
        p = torch.empty(Hh.query_size("yogo_conv_bf16_packed_bytes", ci, co, 3, 0), dtype=torch.uint8, device="cuda")
        Hh.call("yogo_conv_bf16_pack", w, None, p, ci, co, 3, 0, st)
        pk.append(p)
    return dict(B=B, C1=C1, C2=C2, IH=IH, IW=IW, x8=x8, w1=w1, w2=w2, b1=b1, b2=b2, m1=m1, m2=m2, pk1=pk[0], pk2=pk[1])


def _outputs(d):
    from yogo_amd import _hip as Hh

    B, C1, C2, IH, IW = d["B"], d["C1"], d["C2"], d["IH"], d["IW"]
    OH, OW = (IH - 1) // 2 + 1, (IW - 1) // 2 + 1
    y1 = torch.full((B, _blocks(C1), IH, IW, 8), float("nan"), dtype=torch.bfloat16, device="cuda")
    y2 = torch.full((B, _blocks(C2), OH, OW, 8), float("nan"), dtype=torch.bfloat16, device="cuda")
    s1 = torch.full((Hh.query_size("yogo_bf16_signs_bytes", B, C1, IH, IW),), 0xA5, dtype=torch.uint8, device="cuda")
    s2 = torch.full((Hh.query_size("yogo_bf16_signs_bytes", B, C2, OH, OW),), 0xA5, dtype=torch.uint8, device="cuda")
    return y1, s1, y2, s2


def _run(d, fused):
    """(y1, signs1, y2, signs2, launch log) of the one call (fused) or of yogo_conv2d_fwd_bf16_signs twice"""
    from yogo_amd import _hip as Hh

    st = Hh.stream_ptr()
    B, C1, C2, IH, IW = d["B"], d["C1"], d["C2"], d["IH"], d["IW"]
    y1, s1, y2, s2 = _outputs(d)
    Hh.launch_log(True)
    try:
        if fused:
            Hh.call("yogo_conv2d_fwd_bf16_signs_pair", d["x8"], d["pk1"], d["b1"], y1, s1, d["m1"], d["pk2"], d["b2"], y2, s2, d["m2"],
                    B, 16, C1, C2, IH, IW, 1, st)
        else:
            Hh.call("yogo_conv2d_fwd_bf16_signs", d["x8"], d["pk1"], d["b1"], y1, s1, d["m1"], B, 16, C1, IH, IW, 3, 1, 1, st)
            Hh.call("yogo_conv2d_fwd_bf16_signs", y1, d["pk2"], d["b2"], y2, s2, d["m2"], B, C1, C2, IH, IW, 3, 2, 1, st)
        torch.cuda.synchronize()
        log = Hh.read_launch_log()
    finally:
        Hh.launch_log(False)
    return y1, s1, y2, s2, log


def _assert_same_bytes(a, b, what):
    for name, u, v in zip(("y1", "signs1", "y2", "signs2"), a[:4], b[:4]):
        if u.dtype == torch.bfloat16:
            u, v = u.view(torch.int16), v.view(torch.int16)
        assert torch.equal(u, v), (what, name, f"{int((u != v).sum())} of {u.numel()} elements differ")


def _from8c(t, C):
    from yogo_amd import _hip as Hh

    B, _, Hh_, W, _ = t.shape
    out = torch.empty(B, C, Hh_, W, device="cuda")
    Hh.call("yogo_bf16_8c_to_nchw_f32", t, out, B, C, Hh_ * W, Hh.stream_ptr())
    return out.double().cpu()


def _assert_fp64(d, y1, y2, what):
    """each layer against the CPU float64 convolution of the operands the kernel was given (layer 2: the stored y1, zero-padded by conv2d)"""
    C1, C2 = d["C1"], d["C2"]
    for tag, xin, cin, w, b, m, got, cout, s in (("y1", d["x8"], 16, d["w1"], d["b1"], d["m1"], y1, C1, 1), ("y2", y1, C1, d["w2"], d["b2"], d["m2"], y2, C2, 2)):
        want = F.leaky_relu(F.conv2d(_from8c(xin, cin), w.to(torch.bfloat16).double().cpu(), b.double().cpu(), stride=s, padding=1), 0.01)
        if m is not None:
            want = want * m.double().cpu()[:, :, None, None]
        gotd = _from8c(got, cout)
        tol = 2.0 ** -8 * want.abs() + 2e-5 * float(want.abs().max())
        err = (gotd - want).abs() - tol
        print(f"{what} {tag}: max |got - want| - tol = {float(err.max()):.3e}")
        assert bool((err <= 0).all()), (what, tag, float(err.max()))


SHAPES = [(1, 1), (1, 70), (70, 1), (2, 2), (3, 3), (4, 5), (5, 4), (7, 63), (8, 64), (9, 65), (6, 125), (6, 126), (6, 127), (33, 130)]
# (B, C1, C2, channel scales): both batch sizes, both widths of either layer, with and without scales -- always with a bias
COMBOS = [(1, 32, 64, True), (3, 24, 48, False), (3, 32, 48, True), (1, 24, 64, False)]


@pytest.mark.parametrize("B,C1,C2,scales", COMBOS)
@pytest.mark.parametrize("IH,IW", SHAPES)
def test_pair_is_bit_identical_to_the_two_launches_and_matches_cpu(IH, IW, B, C1, C2, scales):
    from yogo_amd import _hip as Hh

    # C1 = 24: layer 2 of the two launches is the tiled kernel (the staged one takes 16 or 32 input channels), whose order of the sums the
    # pair kernel does not reproduce -- the entry point then runs the two launches itself, and the bytes are theirs either way
    fuses = C1 == 32
    assert Hh.lib().yogo_conv2d_fwd_bf16_signs_pair_eligible(B, 16, C1, C2, IH, IW) == int(fuses)
    d = _inputs(B, C1, C2, IH, IW, scales, seed=1000 + 7 * IH + IW)
    ref = _run(d, fused=False)
    got = _run(d, fused=True)
    assert not any(k.startswith(PAIR) for k in _names(ref[4])), ref[4]
    if fuses:
        assert any(k.startswith(PAIR) for k in _names(got[4])) and not any(k.startswith("conv_bf16_staged_kernel<") for k in _names(got[4])), got[4]
        assert "l1_mfma_factor=" in next(ln for ln in got[4] if ln.replace(" ", "").startswith(PAIR))
    else:
        assert _names(got[4]) == _names(ref[4]) and len(got[4]) == 2, got[4]
    what = f"{IH}x{IW} B={B} 16->{C1}->{C2} scales={scales}"
    _assert_same_bytes(got, ref, what)
    _assert_fp64(d, got[0], got[2], what)


@pytest.mark.parametrize("IH,IW", [(7, 63), (9, 65), (6, 126), (2, 2)])
def test_padding_of_y1_is_zero_not_layer1_on_padded_y0(IH, IW):
    """bias 8 on layer 1: conv(0) + bias = 8 wherever y0 is padding, so a y1 "padding" evaluated instead of zeroed adds whole units to y2's border"""
    d = _inputs(2, 32, 64, IH, IW, False, seed=77, bias_shift=8.0)
    ref = _run(d, fused=False)
    got = _run(d, fused=True)
    border = _from8c(got[0], 32)
    assert float(border[:, :, 0, :].min()) > 1.0 and float(border[:, :, :, 0].min()) > 1.0 and float(border[:, :, -1, :].min()) > 1.0 and float(border[:, :, :, -1].min()) > 1.0
    _assert_same_bytes(got, ref, f"adversarial {IH}x{IW}")
    _assert_fp64(d, got[0], got[2], f"adversarial {IH}x{IW}")


def test_pair_repeats_itself_across_many_tiles_per_wavefront():
    """B = 12 images of 257x126: 36 column strips of 129 tiles, cut into runs of 13 -- a wavefront walks a run down its strip and the last y1 row
    of a tile reaches the next one through registers, not through layer 1 again; the runs start inside strips (that row computed afresh) and
    at their top (zeros), the last run of a strip is short, the last strip group has four wavefronts without a strip, and a wavefront goes
    from unit to unit, image to image"""
    d = _inputs(12, 32, 64, 257, 126, True, seed=5)
    ref = _run(d, fused=False)
    for _ in range(2):
        _assert_same_bytes(_run(d, fused=True), ref, "B=12 257x126")


def test_pair_at_the_production_plane():
    """386x516 = layers 1 + 2 of base_model at 772x1032, B = 2, 16 -> 32 -> 64 with the step's channel masks: the same bytes as the two
    launches; the instantiation joins the set test_gpu_production_shapes.py wants covered by a parity test"""
    import test_gpu_production_shapes as P

    d = _inputs(2, 32, 64, 386, 516, True, seed=9)
    ref = _run(d, fused=False)
    got = _run(d, fused=True)
    mine = P.kernels_of(got[4])
    assert any(k.startswith(PAIR) for k in mine), sorted(mine)
    _assert_same_bytes(got, ref, "386x516")
    P.SEEN.update(mine)


@pytest.mark.parametrize("C1,C2,IH,IW", [(16, 64, 20, 22), (24, 64, 20, 22), (32, 32, 20, 22), (32, 128, 20, 22)])
def test_ineligible_shapes_take_the_two_launches(C1, C2, IH, IW):
    from yogo_amd import _hip as Hh

    assert Hh.lib().yogo_conv2d_fwd_bf16_signs_pair_eligible(2, 16, C1, C2, IH, IW) == 0
    d = _inputs(2, C1, C2, IH, IW, True, seed=3)
    ref = _run(d, fused=False)
    got = _run(d, fused=True)
    assert not any(k.startswith(PAIR) for k in _names(got[4])), got[4]
    assert _names(got[4]) == _names(ref[4]) and len(got[4]) == 2
    _assert_same_bytes(got, ref, f"ineligible 16->{C1}->{C2}")


def test_training_step_routes_the_pair_and_the_hook_switches_it_off():
    """a base_model step launches the pair kernel and neither staged forward; with yogo_hook_conv_bf16_staged_pair(0) (the hooks library) the
    two staged kernels and not the pair; and the engine's saved records of the two layers are the same tensors either way"""
    from _util import hooks_library
    from yogo_amd import _hip as Hh
    from yogo_amd.model import YOGO
    from yogo_amd.train import HipTrainer
    from yogo_amd.yogo_loss import YOGOLoss

    import yogo_oracle as O

    HI, WI, C = 128, 192, 7
    torch.manual_seed(4)
    m0 = YOGO((HI, WI), 0.0425, 0.0555, C).cuda()
    m0.train()
    for mod in m0.modules():
        if isinstance(mod, torch.nn.Dropout2d):
            mod.p = 0.0
    sd0 = {k: v.detach().clone() for k, v in m0.state_dict().items()}
    x = O.synthetic_images(2, HI, WI, seed=5).cuda()
    lab = O.synthetic_labels(2, m0.Sx, m0.Sy, K=8, num_classes=C, seed=6).cuda()

    def step():
        m0.load_state_dict(sd0)
        t = HipTrainer(m0, YOGOLoss().cuda(), total_steps=10, half=True)
        Hh.launch_log(True)
        try:
            t.step(x, lab)
            torch.cuda.synchronize()
            log = Hh.read_launch_log()
        finally:
            Hh.launch_log(False)
        return _names(log), t

    on, tr = step()
    assert any(k.startswith(PAIR) for k in on) and not any(k.startswith((STAGED1, STAGED2)) for k in on), sorted(on)
    with hooks_library() as hl:
        hook = hl.yogo_hook_conv_bf16_staged_pair
        hook.restype, hook.argtypes = ctypes.c_int, [ctypes.c_int]
        hook(0)
        try:
            off, _ = step()
        finally:
            hook(1)
    assert not any(k.startswith(PAIR) for k in off), sorted(off)
    assert any(k.startswith(STAGED1) for k in off) and any(k.startswith(STAGED2) for k in off), sorted(off)
    assert on - {k for k in on if k.startswith(PAIR)} == off - {k for k in off if k.startswith((STAGED1, STAGED2))}
    # the engine's records of layers 1 and 2 (what the backward pass reads) are the two calls' records, tensor by tensor
    from yogo_amd import engine as E

    recs = {}
    for flag in (True, False):
        prev, E._PAIR_FWD = E._PAIR_FWD, flag
        try:
            m0.load_state_dict(sd0)
            recs[flag] = E.forward_bf16_train(tr.engine, x)[1]
            torch.cuda.synchronize()
        finally:
            E._PAIR_FWD = prev
    assert len(recs[True]) == len(recs[False])
    for i in (1, 2, 3):
        for f in ("x_in", "y", "z", "pre", "signs", "mask"):
            a, b = getattr(recs[True][i], f), getattr(recs[False][i], f)
            assert (a is None) == (b is None), (i, f)
            if a is not None and not (i == 3 and f != "x_in"):
                assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (i, f)
