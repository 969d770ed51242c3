"""Training through autograd on the bf16 path: ``model(x)`` under ``torch.autocast("cuda", dtype=torch.bfloat16)`` with gradients on,
a loss, ``loss.backward()`` -- the reference's own loop (yogo/train.py:315-325) -- runs the kernels of HipTrainer(half=True).step.

  1. gradients, loss and BatchNorm running buffers are bit-identical to HipTrainer(half=True) (with and without its fused
     decode + loss kernel), on several architectures, at the production image size and with a clamp that bites;
  2. the kernels launched are HipTrainer's bf16 backbone kernels and none of the fp32 convolution / weight-gradient kernels;
  3. no autocast, fp16 autocast and no_grad() keep today's fp32 path bit for bit;
  4. two live graphs and gradient accumulation; 5. a second backward and an in-place parameter update raise;
  6. frozen lower layers get no gradient and cost no backward work below the lowest trainable layer (>= 2);
  7. a custom loss on the decoded prediction; 8. five optimiser steps with torch's AdamW + CosineAnnealingLR track HipTrainer.
Every model of a test comes from one state_dict, and torch.manual_seed is set in front of every forward so the Dropout2d masks
(one torch.rand per forward) are the same."""
import contextlib

import pytest
import torch

import yogo_oracle as O
from _util import BF16_STEP_COS_MIN, BF16_STEP_LOSS_RTOL, assert_grads_match_bf16_oracle

pytestmark = pytest.mark.gpu

C = 7


def _imports():
    from yogo_amd import _hip, engine, train
    from yogo_amd.model import YOGO, _DecodeFn, _decode
    from yogo_amd.model_defns import MODELS
    from yogo_amd.yogo_loss import YOGOLoss

    return _hip, engine, train, YOGO, _DecodeFn, _decode, MODELS, YOGOLoss


class Case:
    """one architecture / image size / clamp: a reference state_dict, a batch, and fresh models built from the state_dict"""

    def __init__(self, name="base_model", hw=(96, 128), rgb=False, clip=1.0, B=4, seed=0, K=6):
        _, _, _, YOGO, _, _, MODELS, _ = _imports()
        self.args = dict(img_size=hw, anchor_w=0.0425, anchor_h=0.0555, num_classes=C, is_rgb=rgb, model_func=MODELS[name],
                         clip_value=clip)
        torch.manual_seed(seed)
        m0 = YOGO(**self.args).cuda()
        self.sd = {k: v.detach().clone() for k, v in m0.state_dict().items()}
        g = torch.Generator().manual_seed(seed + 1)
        self.x = torch.randint(0, 256, (B, 3 if rgb else 1, hw[0], hw[1]), dtype=torch.uint8, generator=g).cuda()
        self.lab = O.synthetic_labels(B, m0.Sx, m0.Sy, K=K, num_classes=C, seed=seed + 2).cuda()

    def model(self, no_dropout=False):
        YOGO = _imports()[3]
        m = YOGO(**self.args).cuda()
        m.load_state_dict(self.sd)
        m.train()
        if no_dropout:
            for mod in m.modules():
                if isinstance(mod, torch.nn.Dropout2d):
                    mod.p = 0.0
        return m


def _grads(m):
    return {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in m.named_parameters()}


def _buffers(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}


def module_step(m, x, lab, seed, dtype=torch.bfloat16, loss_fn=None):
    """zero_grad, forward under autocast (dtype None: none), loss, backward; returns the detached loss"""
    YOGOLoss = _imports()[7]
    m.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    ctx = torch.autocast("cuda", dtype=dtype) if dtype is not None else contextlib.nullcontext()
    with ctx:
        pred = m(x)
        loss = loss_fn(pred) if loss_fn is not None else YOGOLoss().cuda()(pred, lab)[0]
    loss.backward()
    return loss.detach()


def trainer_step(case, seed, fused):
    """HipTrainer(half=True).step on a fresh model; returns (loss, gradients by name from flat.grad, BatchNorm buffers)"""
    _, _, train, _, _, _, _, YOGOLoss = _imports()
    m = case.model()
    tr = train.HipTrainer(m, YOGOLoss().cuda(), total_steps=10, half=True)
    prev = train._FUSED_DECODE_LOSS
    train._FUSED_DECODE_LOSS = fused
    try:
        torch.manual_seed(seed)
        out = tr.step(case.x, case.lab)
    finally:
        train._FUSED_DECODE_LOSS = prev
    grads, off = {}, 0
    for n, p in m.named_parameters():
        grads[n] = tr.flat.grad[off:off + p.numel()].view(p.shape).clone()
        off += p.numel()
    return out[0].clone(), grads, _buffers(m)


@contextlib.contextmanager
def entry_points():
    """names of the C-ABI entry points called (from any thread: autograd runs backward on its own) while the block runs"""
    _hip = _imports()[0]
    names = []
    orig = _hip.call

    def rec(name, *args):
        names.append(name)
        return orig(name, *args)

    _hip.call = rec
    try:
        yield names
    finally:
        _hip.call = orig


@contextlib.contextmanager
def launched():
    """kernel instantiations of the library's launch log (the text in front of " | ") while the block runs"""
    _hip = _imports()[0]
    out = set()
    _hip.launch_log(True)
    try:
        yield out
    finally:
        torch.cuda.synchronize()
        _hip.launch_log(False)
        out.update("".join(ln.split("|")[0].split()) for ln in _hip.read_launch_log())


# ---- 1. bit-identical to HipTrainer(half=True) ---------------------------------------------------------------------------------
_EQ_CASES = {
    "base_96x128": dict(name="base_model", hw=(96, 128), B=4),
    "depth_ver_0": dict(name="depth_ver_0", hw=(96, 128), B=4),            # head-BN fusion
    "silu_model": dict(name="silu_model", hw=(96, 128), B=4),
    "quarter_rgb": dict(name="quarter_filters", hw=(130, 70), rgb=True, B=2),
    "base_772x1032": dict(name="base_model", hw=(772, 1032), B=2, K=64),  # layer-0 MFMA / Gram, fused layer-1/0 sweep
    "small_clip": dict(name="base_model", hw=(96, 128), B=4, clip=2e-3),
}


@pytest.mark.parametrize("case", sorted(_EQ_CASES))
def test_module_path_is_bit_identical_to_hip_trainer(case):
    cs = Case(**_EQ_CASES[case])
    m = cs.model()
    loss = module_step(m, cs.x, cs.lab, seed=11)
    got, bufs = _grads(m), _buffers(m)
    assert all(g is not None for g in got.values())
    for fused in (False, True):
        tloss, want, tbufs = trainer_step(cs, seed=11, fused=fused)
        assert torch.equal(loss, tloss), (case, fused, float(loss), float(tloss))
        for n in want:
            assert torch.equal(got[n], want[n]), (case, fused, n, float((got[n] - want[n]).abs().max()))
        for k in tbufs:
            assert torch.equal(bufs[k], tbufs[k]), (case, fused, k)
    if case == "small_clip":   # the fused clamp bites
        clip = float(cs.sd["clip_value"])
        assert any(bool((g.abs() == clip).any()) for g in got.values())
        assert all(float(g.abs().max()) <= clip for g in got.values())


# ---- 2. which kernels run ------------------------------------------------------------------------------------------------------
_FP32_ENTRY_POINTS = {"yogo_conv2d_fwd_f32", "yogo_conv2d_dgrad_f32", "yogo_conv2d_wgrad_f32", "yogo_conv_pack_f32", "yogo_conv_first_fwd",
                      "yogo_conv_first_wgrad", "yogo_bn_apply_act", "yogo_bn_bwd", "yogo_decode_bwd"}
_BACKBONE_PREFIXES = ("yogo_conv_first", "yogo_conv2d_", "yogo_conv_bf16", "yogo_bn_", "yogo_wgrad_", "yogo_partials_reduce")


@pytest.mark.parametrize("hw,B", [((96, 128), 4), ((772, 1032), 2)])
def test_module_path_launches_the_bf16_kernels(hw, B):
    cs = Case(hw=hw, B=B, K=64)
    m = cs.model()
    with launched() as kern, entry_points() as calls:
        module_step(m, cs.x, cs.lab, seed=3)
    m2 = cs.model()
    _, _, train, _, _, _, _, YOGOLoss = _imports()
    tr = train.HipTrainer(m2, YOGOLoss().cuda(), total_steps=10, half=True)
    with launched() as tkern, entry_points() as tcalls:
        torch.manual_seed(3)
        tr.step(cs.x, cs.lab)
    tback = {c for c in tcalls if c.startswith(_BACKBONE_PREFIXES)}
    for pre in ("yogo_conv_first", "yogo_conv2d_fwd_bf16", "yogo_conv2d_wgrad_bf16", "yogo_bn_"):
        assert any(c.startswith(pre) for c in tback), (pre, sorted(tback))
    assert tback <= set(calls), sorted(tback - set(calls))
    assert not (set(calls) & _FP32_ENTRY_POINTS), sorted(set(calls) & _FP32_ENTRY_POINTS)
    tk = {k for k in tkern if k.startswith(("conv_bf16", "wgrad_bf16", "wgrad_reduce"))}
    assert tk and tk <= kern, sorted(tk - kern)
    assert not any(k.startswith("conv_igemm_f32") for k in kern), sorted(kern)


# ---- 3. the paths that stay fp32 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [None, torch.float16])
def test_no_autocast_and_fp16_autocast_keep_the_fp32_path(dtype):
    _hip, engine, _, _, _DecodeFn, _, _, YOGOLoss = _imports()
    cs = Case()
    m = cs.model()
    with entry_points() as calls:
        loss = module_step(m, cs.x, cs.lab, seed=5, dtype=dtype)
    assert "yogo_conv2d_wgrad_f32" in calls and not any("bf16" in c for c in calls)
    r = cs.model()
    eng = engine.get_engine(r.model)
    eng.clip = r._clip
    torch.manual_seed(5)
    raw = engine._BackboneFn.apply(cs.x, r.model, *r.model.parameters())
    pred = _DecodeFn.apply(raw, r._Cxs, r._Cys, *r._decode_scalars(), bool(r.inference))
    rloss = YOGOLoss().cuda()(pred, cs.lab)[0]
    rloss.backward()
    assert torch.equal(loss, rloss.detach())
    want = _grads(r)
    for n, g in _grads(m).items():
        assert torch.equal(g, want[n]), n


@pytest.mark.parametrize("dtype", [None, torch.bfloat16])
def test_no_grad_in_train_mode_keeps_the_fp32_forward(dtype):
    _, engine, _, _, _, _decode, _, _ = _imports()
    cs = Case()
    m = cs.model()
    torch.manual_seed(6)
    ctx = torch.autocast("cuda", dtype=dtype) if dtype is not None else contextlib.nullcontext()
    with torch.no_grad(), ctx:
        out = m(cs.x)
    r = cs.model()
    torch.manual_seed(6)
    raw, _ = engine.get_engine(r.model).forward(cs.x, need_grad=False)
    want = _decode(raw, r._Cxs, r._Cys, *r._decode_scalars(), bool(r.inference))
    assert torch.equal(out, want)
    wb = _buffers(r)
    for k, v in _buffers(m).items():
        assert torch.equal(v, wb[k]), k


def test_backbone_alone_under_bf16_autocast():
    """``model.model(x)`` (the HipBackbone) on its own: forward_bf16_train's head output, and backward_bf16_train on the fp32 gradient"""
    _, engine, _, _, _, _, _, _ = _imports()
    cs = Case()
    m, r = cs.model(), cs.model()
    ea, er = engine.get_engine(m.model), engine.get_engine(r.model)
    ea.clip = er.clip = m._clip
    torch.manual_seed(7)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        raw = m.model(cs.x)
    graw = torch.randn(raw.shape, generator=torch.Generator(device="cuda").manual_seed(8), device="cuda")
    raw.backward(graw)
    torch.manual_seed(7)
    rraw, saved = engine.forward_bf16_train(er, cs.x)
    want = engine.backward_bf16_train(er, saved, graw)
    assert torch.equal(raw.detach(), rraw)
    for (n, p), w in zip(m.model.named_parameters(), want):
        assert torch.equal(p.grad, w), n


# ---- 4. several live graphs, accumulation --------------------------------------------------------------------------------------
def test_two_live_graphs_accumulate():
    YOGOLoss = _imports()[7]
    cs = Case(B=2)
    g = torch.Generator().manual_seed(40)
    xb = torch.randint(0, 256, cs.x.shape, dtype=torch.uint8, generator=g).cuda()
    m = cs.model()
    labb = O.synthetic_labels(2, m.Sx, m.Sy, K=6, num_classes=C, seed=41).cuda()
    L = YOGOLoss().cuda()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        torch.manual_seed(1)
        la = L(m(cs.x), cs.lab)[0]
        torch.manual_seed(2)
        lb = L(m(xb), labb)[0]
    lb.backward()
    la.backward()
    ma, mb = cs.model(), cs.model()
    module_step(ma, cs.x, cs.lab, seed=1)
    module_step(mb, xb, labb, seed=2)
    ga, gb = _grads(ma), _grads(mb)
    for n, got in _grads(m).items():
        assert torch.equal(got, gb[n] + ga[n]), n


# ---- 5. misuse raises, never returns numbers -----------------------------------------------------------------------------------
def test_second_backward_raises():
    YOGOLoss = _imports()[7]
    cs = Case()
    m = cs.model()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = YOGOLoss().cuda()(m(cs.x), cs.lab)[0]
    loss.backward(retain_graph=True)
    first = _grads(m)
    with pytest.raises(RuntimeError, match="second backward"):
        loss.backward()
    for n, g in _grads(m).items():
        assert torch.equal(g, first[n]), n


def test_in_place_update_between_forward_and_backward_raises():
    YOGOLoss = _imports()[7]
    cs = Case()
    m = cs.model()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = YOGOLoss().cuda()(m(cs.x), cs.lab)[0]
    _, engine, _, _, _, _, _, _ = _imports()
    with torch.no_grad():
        engine.get_engine(m.model).layers[3].conv.weight.add_(1e-3)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()
    assert all(p.grad is None for p in m.parameters())


# ---- 6. frozen lower layers ----------------------------------------------------------------------------------------------------
def test_frozen_lower_layers():
    _, engine, _, _, _, _, _, _ = _imports()
    cs = Case()
    full = cs.model()
    module_step(full, cs.x, cs.lab, seed=9)
    want = _grads(full)
    n = len(engine.get_engine(full.model).layers)
    for k in (1, 2, 5, n - 1):
        m = cs.model()
        eng = engine.get_engine(m.model)
        frozen = set()
        for i, L in enumerate(eng.layers[:k]):
            for mod in (L.conv, L.bn):
                if mod is not None:
                    for p in mod.parameters():
                        p.requires_grad_(False)
                        frozen.add(id(p))
        YOGOLoss = _imports()[7]
        torch.manual_seed(9)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = YOGOLoss().cuda()(m(cs.x), cs.lab)[0]
        eng.prof = []
        try:
            with entry_points() as calls:
                loss.backward()
            torch.cuda.synchronize()
            ticks = [(r[0], r[1]) for r in eng.prof]
        finally:
            eng.prof = None
        for name, p in m.named_parameters():
            if id(p) in frozen:
                assert p.grad is None, (k, name)
            else:
                assert torch.equal(p.grad, want[name]), (k, name)
        if k >= 2:
            assert {i for kind, i in ticks if kind == "wgrad"} == set(range(k, n)), (k, ticks)
            assert all(i > k for kind, i in ticks if kind == "dgrad"), (k, ticks)
            low = [c for c in calls if c.startswith(("yogo_conv_first", "yogo_conv2d_dgrad_wgrad_bf16_first_bwd"))]
            assert not low, (k, low)


# ---- 7. a custom loss ----------------------------------------------------------------------------------------------------------
def _custom(pred):
    return (pred[:, 4] ** 2).mean()


def _oracle_custom_step(cs, spec):
    """the oracle's bf16-storage emulation of a step (O.bf16_train_step, block by block) with _custom in place of YOGOLoss: forward
    blocks, fp32 decode and loss, d loss / d raw rounded to bf16 (what yogo_decode_bwd_bf16 writes), backward blocks"""
    sd = {k: v.cpu() for k, v in cs.sd.items()}
    x = cs.x.cpu()
    l0 = O.l0_on_matrix_cores(spec, x)
    cur, saved = x.float(), []
    for i in range(len(spec)):
        saved.append(O.bf16_block_forward(i, cur, sd, spec, l0))
        cur = saved[-1]["y"]
    raw = cur.detach().clone().requires_grad_(True)
    loss = _custom(O.decode(raw, sd["_Cxs"], sd["_Cys"], 0.0425, 0.0555))
    loss.backward()
    g = raw.grad.to(torch.bfloat16).float()
    grads = {}
    for i in range(len(spec) - 1, -1, -1):
        r = O.bf16_block_backward(i, g, saved[i], saved[i - 1] if i > 0 else None, spec, l0,
                                  l0_no_z=(i == 0 and O.l0_keeps_no_z(spec, l0)))
        pre = O.conv_prefix(spec, i)
        grads[pre + "weight"] = r["dW"]
        if "db" in r:
            grads[pre + "bias"] = r["db"]
        if "dgamma" in r:
            grads[f"model.{i}.1.weight"], grads[f"model.{i}.1.bias"] = r["dgamma"], r["dbeta"]
        if i > 0:
            g = r["dx"]
    return float(loss.detach()), grads


def test_custom_loss():
    """a loss of the user's own on the decoded prediction: against the oracle's bf16-storage emulation of the same step, the bounds of
    every bf16 whole-step test (loss BF16_STEP_LOSS_RTOL, per-tensor cosine >= BF16_STEP_COS_MIN); against the fp32 module path, the
    bound of test_gpu_bf16.py's bf16-vs-fp32 step (cosine > 0.95: layer 0's weight gradient sums cancel ~1000-fold, tests/_util.py)"""
    cs = Case(clip=1e9)   # unclamped: compare the raw gradients
    m16, m32 = cs.model(no_dropout=True), cs.model(no_dropout=True)
    l16 = float(module_step(m16, cs.x, cs.lab, seed=4, loss_fn=_custom))
    l32 = float(module_step(m32, cs.x, cs.lab, seed=4, dtype=None, loss_fn=_custom))
    lref, gref = _oracle_custom_step(cs, O.arch("base_model", C))
    print(f"custom loss: bf16 module path {l16:.6f}, bf16-storage oracle {lref:.6f}, fp32 module path {l32:.6f}")
    assert abs(l16 - lref) < BF16_STEP_LOSS_RTOL * abs(lref)
    got = {k: v.cpu() for k, v in _grads(m16).items()}
    assert set(got) == set(gref)
    assert_grads_match_bf16_oracle(got, gref, "custom loss vs bf16-storage oracle", cos_min=BF16_STEP_COS_MIN)
    ref32 = {k: v.cpu() for k, v in _grads(m32).items()}
    assert_grads_match_bf16_oracle(got, ref32, "custom loss vs fp32 module path", cos_min=0.95)


# ---- 8. torch's optimiser and scheduler ----------------------------------------------------------------------------------------
def test_short_trajectory_with_torch_adamw_tracks_hip_trainer():
    _, _, train, _, _, _, _, YOGOLoss = _imports()
    cs = Case()
    steps, lr = 5, 3e-4
    m = cs.model()
    opt = torch.optim.AdamW(m.parameters(), lr=lr, weight_decay=5e-2, betas=(0.9, 0.999), eps=1e-8, foreach=True)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=steps, eta_min=lr / 10.0)
    mt = cs.model()
    tr = train.HipTrainer(mt, YOGOLoss().cuda(), learning_rate=lr, weight_decay=5e-2, total_steps=steps, half=True)
    for s in range(steps):
        loss = float(module_step(m, cs.x, cs.lab, seed=100 + s))
        opt.step()
        sched.step()
        torch.manual_seed(100 + s)
        tl = float(tr.step(cs.x, cs.lab)[0])
        print(f"step {s}: module path {loss:.6f}  HipTrainer {tl:.6f}")
        if s == 0:
            assert loss == tl
        assert abs(loss - tl) < BF16_STEP_LOSS_RTOL * abs(tl), (s, loss, tl)
