"""Host-side executor of the backbone on the HIP kernels (libyogo_hip.so).

Walks a :class:`~yogo_amd.model_defns.HipBackbone` (block grammar of yogo/model_defns.py: Conv2d, [BatchNorm2d],
[LeakyReLU|SiLU], [Dropout2d]) into a layer table and runs forward / backward by calling the C ABI with raw device
pointers on the current HIP stream.  PyTorch supplies device memory, the stream and the autograd edge only.

Fusion plan (fp32):
  block without BN :  conv + bias + activation + Dropout2d channel mask            -> 1 kernel
  block with BN    :  conv (+bias) + per-workgroup BN partial sums | finalize | normalise + activation
  backward         :  [BN backward] -> wgrad (+bias grad, +clamp) -> dgrad whose epilogue applies the previous block's
                      activation derivative and dropout mask, so no separate element-wise backward passes exist.
The per-parameter gradient clamp of yogo/model.py:76-77 is fused into the gradient-finishing kernels.

bf16 training (forward_bf16_train / backward_bf16_train): activations and their gradients in NCHW8c bf16, everything else fp32.
  layer 0          :  uint8 image + BatchNorm on the matrix cores: statistics from the exact integer patch Gram matrix, then
                      conv + BatchNorm + activation in one sweep; any other first layer through yogo_conv_first_fwd_train_bf16
                      with the statistics from its epilogue
  layers > 0       :  conv (+bias, activation, dropout mask; sign map or pre-activation for the data gradient below) | BatchNorm
                      statistics by a sweep over the stored output | finalize | normalise + activation
  backward         :  per layer BatchNorm backward -> weight gradient -> hook -> data gradient, all on the current stream; the
                      fused kernels that replace some of these passes are named by the five switches defined above _packed_bf16
"""
from __future__ import annotations

import threading
import weakref
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch
from torch import nn

from yogo_amd import _hip

ACT_NONE, ACT_LEAKY, ACT_SILU = 0, 1, 2


@dataclass
class Layer:
    conv: nn.Conv2d
    bn: Optional[nn.BatchNorm2d] = None
    act: int = ACT_NONE
    drop: Optional[nn.Dropout2d] = None

    @property
    def cin(self) -> int:
        return self.conv.in_channels

    @property
    def cout(self) -> int:
        return self.conv.out_channels

    @property
    def k(self) -> int:
        return self.conv.kernel_size[0]

    @property
    def s(self) -> int:
        return self.conv.stride[0]

    def out_hw(self, h: int, w: int) -> Tuple[int, int]:
        p = 1 if self.k == 3 else 0
        return (h + 2 * p - self.k) // self.s + 1, (w + 2 * p - self.k) // self.s + 1


@dataclass
class Saved:
    x_in: torch.Tensor
    y: Optional[torch.Tensor] = None
    z: Optional[torch.Tensor] = None       # conv output of a BN block
    pre: Optional[torch.Tensor] = None     # pre-activation (SiLU blocks)
    signs: Optional[torch.Tensor] = None   # sign map of y (LeakyReLU blocks without BatchNorm, bf16 path)
    signs0: Optional[torch.Tensor] = None  # layer 0 on the matrix cores: sign map of its BatchNorm output -- kept INSTEAD of z
    w_used: Optional[torch.Tensor] = None  # layer 0 on the matrix cores: the bf16-rounded weights the forward multiplied with
    gram: Optional[torch.Tensor] = None    # layer 0: float[90] patch sums P and Gram matrix G of the batch (reused by backward)
    mask: Optional[torch.Tensor] = None    # Dropout2d channel mask, already scaled
    mean: Optional[torch.Tensor] = None
    invstd: Optional[torch.Tensor] = None
    bn_train: bool = False


def parse_backbone(backbone: nn.Sequential) -> List[Layer]:
    layers: List[Layer] = []
    for blk in backbone:
        mods = [blk] if isinstance(blk, nn.Conv2d) else list(blk)
        if not mods or not isinstance(mods[0], nn.Conv2d):
            raise RuntimeError(f"yogo_amd: unsupported block {blk!r}: every block must start with nn.Conv2d")
        conv = mods[0]
        k, s, p = conv.kernel_size, conv.stride, conv.padding
        ok = k[0] == k[1] and s[0] == s[1] and conv.dilation == (1, 1) and conv.groups == 1 and conv.padding_mode == "zeros"
        ok = ok and ((k[0] == 3 and p == (1, 1) and s[0] in (1, 2)) or (k[0] == 1 and p == (0, 0) and s[0] == 1))
        if not ok:
            raise RuntimeError(f"yogo_amd: unsupported convolution {conv!r} (3x3 pad 1 stride 1|2, or 1x1)")
        L = Layer(conv=conv)
        for m in mods[1:]:
            if isinstance(m, nn.BatchNorm2d):
                L.bn = m
            elif isinstance(m, nn.LeakyReLU):
                if abs(m.negative_slope - 0.01) > 1e-12:
                    raise RuntimeError("yogo_amd: LeakyReLU slope must be 0.01")
                L.act = ACT_LEAKY
            elif isinstance(m, nn.SiLU):
                L.act = ACT_SILU
            elif isinstance(m, nn.Dropout2d):
                L.drop = m
            else:
                raise RuntimeError(f"yogo_amd: unsupported module {m!r} in block")
        if L.bn is not None and L.drop is not None:
            raise RuntimeError("yogo_amd: BatchNorm + Dropout2d in one block is not part of the block grammar")
        layers.append(L)
    return layers


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.contiguous().float()


def _bn_affine(L: Layer, dev) -> Tuple[torch.Tensor, torch.Tensor]:
    """(gamma, beta) of the block's BatchNorm as fp32 device tensors; ones / zeros for affine=False"""
    bn = L.bn
    gamma = _f32(bn.weight.detach()) if bn.weight is not None else torch.ones(L.cout, device=dev)
    beta = _f32(bn.bias.detach()) if bn.bias is not None else torch.zeros(L.cout, device=dev)
    return gamma, beta


def _bn_grad_dst(bn: nn.BatchNorm2d, dst, grads: Dict[int, torch.Tensor], cout: int, dev) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dgamma, dbeta) destinations: the parameters' own through ``dst``, entered into ``grads``; scratch for affine=False (the
    kernels always write them)"""
    dgamma = dst(bn.weight) if bn.weight is not None else torch.empty(cout, dtype=torch.float32, device=dev)
    dbeta = dst(bn.bias) if bn.bias is not None else torch.empty(cout, dtype=torch.float32, device=dev)
    if bn.weight is not None:
        grads[id(bn.weight)] = dgamma
        grads[id(bn.bias)] = dbeta
    return dgamma, dbeta


def _bn_finalize(eng: "Engine", L: Layer, fn: str, *lead_args, count: int, dev, st) -> Tuple[torch.Tensor, torch.Tensor]:
    """Batch (mean, invstd) of the block's BatchNorm by ``fn`` (yogo_bn_finalize over partial sums, or yogo_bn_stats_from_gram), which
    also updates the running statistics when the module tracks them"""
    bn = L.bn
    mean = torch.empty(L.cout, dtype=torch.float32, device=dev)
    invstd = torch.empty(L.cout, dtype=torch.float32, device=dev)
    track = bn.track_running_stats and bn.running_mean is not None
    _hip.call(fn, *lead_args, L.cout, count, float(bn.eps), float(bn.momentum if bn.momentum is not None else 0.0), mean, invstd,
              bn.running_mean if track else None, bn.running_var if track else None, bn.num_batches_tracked if track else None, st)
    if track:
        eng.generation += 1   # running statistics rewritten by raw pointer
    return mean, invstd


def _first_wgrad(fn: str, L: Layer, x_in: torch.Tensor, g: torch.Tensor, dw: torch.Tensor, db: Optional[torch.Tensor], clip: float, st) -> None:
    """Plain weight gradient of a direct layer 0 by ``fn`` (yogo_conv_first_wgrad for an fp32 NCHW gradient, yogo_conv_first_wgrad_bf16g
    for bf16 NCHW8c): partial sums over the image rows, then one reduction of weight and bias gradient together"""
    B, _, IH, IW = x_in.shape
    rows = _hip.query_ints("yogo_conv_first_wgrad_rows", 1, B, IH, IW, L.s)[0]
    nj = L.cin * 9 + 1
    part = torch.empty(rows * L.cout * nj, dtype=torch.float32, device=x_in.device)
    red = torch.empty(L.cout, nj, dtype=torch.float32, device=x_in.device)
    _hip.call(fn, x_in, 0 if x_in.dtype == torch.uint8 else 1, g, part, B, L.cin, L.cout, IH, IW, L.s, st)
    _hip.call("yogo_partials_reduce", part, rows, L.cout * nj, clip, red, st)
    dw.view(L.cout, nj - 1).copy_(red[:, : nj - 1])
    if db is not None:
        db.copy_(red[:, nj - 1])


def _pack_hit(eng: "Engine", key: Tuple[int, int], w: torch.Tensor) -> Optional[torch.Tensor]:
    """the cached packing ``key`` of weight ``w``, unless torch has seen ``w`` written or moved since it was made"""
    hit = eng._pack.get(key)
    return hit[2] if hit is not None and hit[0] == w._version and hit[1] == w.data_ptr() else None


class Engine:
    def __init__(self, backbone: nn.Sequential):
        self.backbone_ref = weakref.ref(backbone)
        self.layers = parse_backbone(backbone)
        self._pack: Dict[Tuple[int, int], Tuple[int, int, torch.Tensor]] = {}
        self.clip: float = 0.0  # > 0: clamp parameter gradients to +-clip (set by YOGO from clip_value)
        # optional per-launch HIP-event timing (bench.py): list of (kind, layer, mw, flops, start_event, end_event)
        self.prof: Optional[list] = None
        self.prof_only: Optional[set] = None   # bracket only the launches whose `mw` tag is in this set (bench.py's timed region)
        self._open = None
        # bumped whenever a kernel writes parameters or BatchNorm buffers through raw pointers (AdamW on the flat buffer,
        # bn_finalize / bn_stats_from_gram on the running statistics): torch's _version does not see those writes, so every
        # cache of derived tensors (packed weights, folded inference weights) keys on this counter as well
        self.generation: int = 0
        self._pack_multi = None     # (weight pointers, buffers, job table, blocks) of _pack_all_bf16
        self._drop_consts = None    # (key, sizes, p, 1 / (1 - p)) of _dropout_masks
        self._infer_bf16: Optional["InferEngineBF16"] = None

    def _tick(self, kind: str, layer: int, flops: float, mw: int = 0, nbytes: float = 0.0) -> None:
        """open a HIP-event bracket around one kernel call (bench.py): algorithmic FLOPs and bytes of that call"""
        if self.prof is not None and (self.prof_only is None or mw in self.prof_only):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self._open = (kind, layer, mw, flops, e0, e1, nbytes)

    def _tock(self) -> None:
        if self._open is not None:
            self._open[5].record()
            self.prof.append(self._open)
            self._open = None

    # ------------------------------------------------------------------------------------------------------
    def invalidate_packed(self) -> None:
        """parameters / BatchNorm buffers were rewritten behind torch's back: drop every derived tensor"""
        self._pack.clear()
        self.generation += 1

    def _packed(self, i: int, mode: int) -> torch.Tensor:
        L = self.layers[i]
        w = L.conv.weight
        key = (i, mode)
        buf = _pack_hit(self, key, w)
        if buf is not None:
            return buf
        nbytes = _hip.query_size("yogo_conv_packed_bytes", L.cin, L.cout, L.k, L.s, mode)
        buf = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
        _hip.call("yogo_conv_pack_f32", _f32(w.detach()), buf, L.cin, L.cout, L.k, L.s, mode, _hip.stream_ptr())
        self._pack[key] = (w._version, w.data_ptr(), buf)
        return buf

    def _first_direct(self, i: int) -> bool:
        L = self.layers[i]
        return i == 0 and L.cin in (1, 3) and L.k == 3

    # ------------------------------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor, need_grad: bool) -> Tuple[torch.Tensor, List[Saved]]:
        _hip.require_cuda(x, "the input batch")
        if x.ndim != 4:
            raise RuntimeError(f"yogo_amd: expected a [B,C,H,W] batch, got {tuple(x.shape)}")
        dev = x.device
        st = _hip.stream_ptr()
        B = x.shape[0]
        if x.dtype == torch.uint8:
            cur = x.contiguous()
        else:
            cur = _f32(x)
        saved: List[Saved] = []
        for i, L in enumerate(self.layers):
            if cur.shape[1] != L.cin:
                raise RuntimeError(f"yogo_amd: layer {i} expects {L.cin} channels, got {cur.shape[1]}")
            IH, IW = int(cur.shape[2]), int(cur.shape[3])
            OH, OW = L.out_hw(IH, IW)
            if OH <= 0 or OW <= 0:
                raise RuntimeError(f"yogo_amd: image too small at layer {i}")
            w = L.conv.weight
            _hip.require_cuda(w, "the model parameters")
            bias = _f32(L.conv.bias.detach()) if L.conv.bias is not None else None
            S = Saved(x_in=cur)
            mask = None
            if L.drop is not None and L.drop.training and L.drop.p > 0:
                p = float(L.drop.p)
                mask = (torch.rand(B, L.cout, device=dev) >= p).to(torch.float32) / (1.0 - p)
                S.mask = mask
            has_bn = L.bn is not None
            bn_train = has_bn and (L.bn.training or L.bn.running_mean is None)
            out = torch.empty(B, L.cout, OH, OW, dtype=torch.float32, device=dev)
            pre = None
            if (not has_bn) and need_grad and L.act == ACT_SILU:
                pre = torch.empty_like(out)
            stats = None
            rows = mpad = 0
            direct = self._first_direct(i)
            if bn_train:
                if direct:
                    rows = _hip.query_ints("yogo_conv_first_stats_rows", 1, B, IH, IW, L.s)[0]
                    mpad = L.cout
                else:
                    rows, mpad = _hip.query_ints("yogo_conv2d_fwd_stats_shape", 2, B, L.cin, L.cout, IH, IW, L.k, L.s)
                stats = torch.empty(rows * mpad * 2, dtype=torch.float32, device=dev)
            fused_act = ACT_NONE if has_bn else L.act
            if direct:
                _hip.call("yogo_conv_first_fwd", cur, 0 if cur.dtype == torch.uint8 else 1, _f32(w.detach()), bias, out, pre,
                          mask, stats, B, L.cin, L.cout, IH, IW, L.s, fused_act, st)
            else:
                if cur.dtype != torch.float32:
                    cur = cur.float()
                    S.x_in = cur
                pk = self._packed(i, 0)
                self._tick("fwd", i, 2.0 * B * L.cout * L.cin * L.k * L.k * OH * OW, mw=4 if L.cout > 64 else (2 if L.cout > 32 else 1))
                _hip.call("yogo_conv2d_fwd_f32", cur, pk, bias, out, pre, mask, stats, B, L.cin, L.cout, IH, IW, L.k, L.s,
                          fused_act, st)
                self._tock()
            if has_bn:
                bn = L.bn
                gamma, beta = _bn_affine(L, dev)
                y = torch.empty_like(out) if need_grad else out
                if bn_train:
                    if bn.track_running_stats and bn.running_mean is not None and bn.momentum is None:
                        raise RuntimeError("yogo_amd: BatchNorm2d(momentum=None) is not supported")
                    mean, invstd = _bn_finalize(self, L, "yogo_bn_finalize", stats, rows, mpad, count=B * OH * OW, dev=dev, st=st)
                    _hip.call("yogo_bn_apply_act", out, y, mean, invstd, 0, float(bn.eps), gamma, beta, B, L.cout, OH * OW,
                              L.act, st)
                    S.mean, S.invstd = mean, invstd
                else:
                    _hip.call("yogo_bn_apply_act", out, y, bn.running_mean, bn.running_var, 1, float(bn.eps), gamma, beta, B,
                              L.cout, OH * OW, L.act, st)
                    if need_grad:
                        invstd = torch.empty(L.cout, dtype=torch.float32, device=dev)
                        _hip.call("yogo_bn_invstd", bn.running_var, float(bn.eps), invstd, L.cout, st)
                        S.mean, S.invstd = bn.running_mean, invstd
                S.bn_train = bn_train
                S.z = out if need_grad else None
                S.y = y
                cur = y
            else:
                S.y = out
                S.pre = pre
                cur = out
            saved.append(S if need_grad else Saved(x_in=cur))
        return cur, saved

    # ------------------------------------------------------------------------------------------------------
    def backward(self, saved: List[Saved], graw: torch.Tensor,
                 grad_out: Optional[Dict[int, torch.Tensor]] = None, on_layer=None) -> List[Optional[torch.Tensor]]:
        """returns gradients in the order of ``backbone.parameters()``.  ``grad_out`` maps id(param) to a preallocated
        contiguous destination (views of one flat gradient buffer in the trainer).  ``on_layer(i)`` is called once every
        gradient kernel of layers >= i has been enqueued (the trainer starts the all-reduce of that part there)."""
        st = _hip.stream_ptr()
        dev = graw.device
        clip = float(self.clip)
        grads: Dict[int, torch.Tensor] = {}

        def dst(param: torch.Tensor) -> torch.Tensor:
            if grad_out is not None and id(param) in grad_out:
                return grad_out[id(param)]
            return torch.empty(param.shape, dtype=torch.float32, device=dev)
        g = _f32(graw)
        n = len(self.layers)
        if g is graw and self.layers[-1].bn is not None:
            g = g.clone()   # yogo_bn_bwd writes dz in place: never into the gradient autograd handed us
        for i in range(n - 1, -1, -1):
            L, S = self.layers[i], saved[i]
            B, _, OH, OW = g.shape
            IH, IW = int(S.x_in.shape[2]), int(S.x_in.shape[3])
            if L.bn is not None:
                bn = L.bn
                gamma, beta = _bn_affine(L, dev)
                dgamma, dbeta = _bn_grad_dst(bn, dst, grads, L.cout, dev)
                rows = _hip.query_ints("yogo_bn_bwd_rows", 1, B, OH * OW)[0]
                part = torch.empty(rows * L.cout * 2, dtype=torch.float32, device=dev)
                sums = torch.empty(2 * L.cout, dtype=torch.float32, device=dev)
                # g arrives as dL/d(block output): the BN-backward kernels apply the activation derivative themselves
                _hip.call("yogo_bn_bwd", g, S.z, g, S.mean, S.invstd, gamma, beta, L.act, dgamma, dbeta, part, sums, B, L.cout,
                          OH * OW, 1 if S.bn_train else 0, clip, st)
            # ---- weight / bias gradient -------------------------------------------------------------------------
            dw = dst(L.conv.weight)
            db = dst(L.conv.bias) if L.conv.bias is not None else None
            if self._first_direct(i):
                _first_wgrad("yogo_conv_first_wgrad", L, S.x_in, g, dw, db, clip, st)
            else:
                wsb = _hip.query_size("yogo_conv2d_wgrad_workspace_bytes", B, L.cin, L.cout, IH, IW, L.k, L.s)
                ws = torch.empty(wsb // 4, dtype=torch.float32, device=dev)
                self._tick("wgrad", i, 2.0 * B * L.cout * L.cin * L.k * L.k * OH * OW)
                _hip.call("yogo_conv2d_wgrad_f32", S.x_in, g, dw, db, ws, B, L.cin, L.cout, IH, IW, L.k, L.s, clip, st)
                self._tock()
            if db is not None:
                grads[id(L.conv.bias)] = db
            grads[id(L.conv.weight)] = dw
            if on_layer is not None:
                on_layer(i)
            # ---- data gradient, with the previous block's activation derivative and dropout mask fused -------------
            if i > 0:
                Lp, Sp = self.layers[i - 1], saved[i - 1]
                ref_act = Lp.act
                if Lp.bn is not None:
                    act_ref, ref_act = None, ACT_NONE   # BatchNorm backward applies the activation derivative
                elif Lp.act == ACT_SILU:
                    act_ref = Sp.pre
                    if act_ref is None:
                        raise RuntimeError("yogo_amd: missing saved pre-activation for a SiLU block")
                elif Lp.act == ACT_LEAKY:
                    act_ref = Sp.y
                else:
                    act_ref = None
                dx = torch.empty(B, L.cin, IH, IW, dtype=torch.float32, device=dev)
                pk = self._packed(i, 1)
                # mw tags the kernel instantiation for bench.py's roofline: stride-2 dgrad runs the fused <.,4,true> kernel
                mw_tag = 20 if L.s == 2 else (4 if L.cin > 64 else (2 if L.cin > 32 else 1))
                self._tick("dgrad", i, 2.0 * B * L.cout * L.cin * L.k * L.k * OH * OW, mw=mw_tag)
                _hip.call("yogo_conv2d_dgrad_f32", g, pk, dx, act_ref, ref_act, Sp.mask, B, L.cin, L.cout, IH, IW, L.k, L.s, st)
                self._tock()
                g = dx
        bb = self.backbone_ref()
        return [grads.get(id(p)) for p in bb.parameters()]



# ---------------------------------------------------------------------------------------------------------------------
# bf16 training: activations / activation gradients in NCHW8c bf16, fp32 weights, statistics and parameter gradients
# (the reference's `--half` training is fp16 autocast, yogo/train.py:315-318; bf16 needs no loss scaling)
# ---------------------------------------------------------------------------------------------------------------------
def _blocks(c: int) -> int:
    return ((c + 15) // 16) * 2


# Fused kernels of the bf16 backward pass.  Each switch names one fused kernel; True is what the product runs, and the test named
# beside it rebinds the switch (``E._NAME = False``) to compare the kernel with the separate passes it replaces -- so they are
# plain module globals read at call time.  tools/ab_flag.py times a step either way.
_FUSE_LAYER0_BWD = True     # BatchNorm backward + activation derivative + first-conv weight gradient in one sweep (tests/test_gpu_bf16.py)
_L0_NO_Z = True             # ... without layer 0's conv output in memory: sign map + derived sums, yogo_conv_first_*_xs (tests/test_gpu_bf16.py)
_WGRAD_DEFER_REDUCE = True  # the per-layer split-K reductions of the weight gradients in one launch at the end of the backward pass (tests/test_gpu_bf16.py)
_L01_FUSE_BWD = True        # layer 1's data gradient folded into layer 0's backward sums, yogo_conv2d_dgrad_wgrad_bf16_first_bwd: no dy of layer 0 in memory (tests/test_gpu_first_fused_bwd.py)
_PAIR_FWD = True            # the forward of a stride-1 16 -> 32 and the stride-2 32 -> 64 block behind it in one launch, yogo_conv2d_fwd_bf16_signs_pair (tests/test_gpu_pair_fwd.py)
_HEAD_BN_FUSE = True        # the 1x1 head's data gradient computed inside the BatchNorm backward of the block under it, yogo_bn_bwd_bf16_head (tests/test_gpu_head_bn_fused.py)


def _packed_bf16(eng: Engine, i: int, mode: int) -> torch.Tensor:
    L = eng.layers[i]
    w = L.conv.weight
    key = (i, 10 + mode)
    buf = _pack_hit(eng, key, w)
    if buf is not None:
        return buf
    nbytes = _hip.query_size("yogo_conv_bf16_packed_bytes", L.cin, L.cout, L.k, mode)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    _hip.call("yogo_conv_bf16_pack", _f32(w.detach()), None, buf, L.cin, L.cout, L.k, mode, _hip.stream_ptr())
    eng._pack[key] = (w._version, w.data_ptr(), buf)
    return buf


def _pack_all_bf16(eng: Engine) -> None:
    """Forward and data-gradient packings of every matrix-core layer in ONE launch (the weights change every step)."""
    jobs = [(i, mode) for i in range(1, len(eng.layers)) for mode in (0, 2 if (eng.layers[i].s == 2 and eng.layers[i].k == 3) else 1)]
    ws = [eng.layers[i].conv.weight for i, _ in jobs]
    if any(w.dtype != torch.float32 or not w.is_contiguous() for w in ws) or not jobs:
        return   # (the per-layer path converts)
    if all(_pack_hit(eng, (i, 10 + m), w) is not None for (i, m), w in zip(jobs, ws)):
        return
    dev = ws[0].device
    key = tuple(w.data_ptr() for w in ws)
    st = eng._pack_multi
    if st is None or st[0] != key:
        bufs, rows, blk = [], [], 0
        for (i, mode), w in zip(jobs, ws):
            L = eng.layers[i]
            buf = torch.empty(_hip.query_size("yogo_conv_bf16_packed_bytes", L.cin, L.cout, L.k, mode), dtype=torch.uint8, device=dev)
            bufs.append(buf)
            rows.append([w.data_ptr(), 0, buf.data_ptr(), L.cin, L.cout, L.k, mode, blk])
            blk += _hip.query_ints("yogo_conv_bf16_pack_blocks", 1, L.cin, L.cout, L.k, mode)[0]
        st = (key, bufs, torch.tensor(rows, dtype=torch.int64, device=dev), blk)
        eng._pack_multi = st
    _, bufs, table, blk = st
    _hip.call("yogo_conv_bf16_pack_multi", table, len(jobs), blk, _hip.stream_ptr())
    for (i, mode), w, buf in zip(jobs, ws, bufs):
        eng._pack[(i, 10 + mode)] = (w._version, w.data_ptr(), buf)


def _dropout_masks(eng: Engine, B: int, dev) -> Dict[int, torch.Tensor]:
    """Dropout2d channel masks (already scaled by 1 / (1 - p)) of all layers from ONE torch.rand call."""
    act = [(i, float(L.drop.p)) for i, L in enumerate(eng.layers) if L.drop is not None and L.drop.training and L.drop.p > 0]
    if not act:
        return {}
    key = (B, tuple(act), str(dev))
    cached = eng._drop_consts
    if cached is None or cached[0] != key:
        sizes = [B * eng.layers[i].cout for i, _ in act]
        pvec = torch.cat([torch.full((n,), p, dtype=torch.float32) for n, (_, p) in zip(sizes, act)]).to(dev)
        cached = (key, sizes, pvec, 1.0 / (1.0 - pvec))
        eng._drop_consts = cached
    _, sizes, pvec, inv_keep = cached
    m = (torch.rand(pvec.numel(), device=dev) >= pvec).to(torch.float32) * inv_keep
    out, off = {}, 0
    for n, (i, _) in zip(sizes, act):
        out[i] = m[off:off + n].view(B, eng.layers[i].cout)
        off += n
    return out


def _check_bf16_train_input(eng: Engine, x: torch.Tensor) -> None:
    _hip.require_cuda(x, "the input batch")
    if x.ndim != 4:
        raise RuntimeError(f"yogo_amd: expected a [B,C,H,W] batch, got {tuple(x.shape)}")
    if x.shape[1] != eng.layers[0].cin:
        raise RuntimeError(f"yogo_amd: layer 0 expects {eng.layers[0].cin} channels, got {x.shape[1]}")
    for j in range(1, len(eng.layers)):
        if eng.layers[j].cin != eng.layers[j - 1].cout:
            raise RuntimeError(f"yogo_amd: layer {j} expects {eng.layers[j].cin} channels, layer {j - 1} produces {eng.layers[j - 1].cout}")
    for Lj in eng.layers:
        bnj = Lj.bn
        if (bnj is not None and (bnj.training or bnj.running_mean is None) and bnj.track_running_stats
                and bnj.running_mean is not None and bnj.momentum is None):
            raise RuntimeError("yogo_amd: BatchNorm2d(momentum=None) is not supported")
    if not eng._first_direct(0):
        raise RuntimeError("yogo_amd: bf16 training needs a 1- or 3-channel 3x3 first convolution")


def _first_mfma_fwd_bf16(eng: Engine, L: Layer, S: Saved, bias, bn_train: bool, B: int, H: int, W: int, st) -> torch.Tensor:
    """Layer 0 (uint8 image, 1 -> <= 16 channels, stride 2, BatchNorm) on the matrix cores: fills ``S``, returns the block output"""
    cur, dev = S.x_in, S.x_in.device
    OH, OW = L.out_hw(H, W)
    bn = L.bn
    gamma, beta = _bn_affine(L, dev)
    w32 = _f32(L.conv.weight.detach())
    y = torch.empty(B, _blocks(L.cout), OH, OW, 8, dtype=torch.bfloat16, device=dev)
    if bn_train:   # sweep 1: exact integer patch sums -> statistics of all channels (and backward's G)
        rows = _hip.query_ints("yogo_conv_first_gram_rows", 1, B, H, W)[0]
        gpart = torch.empty(rows * 54, dtype=torch.int32, device=dev)
        gram64 = torch.empty(90, dtype=torch.float64, device=dev)
        S.gram = torch.empty(90, dtype=torch.float32, device=dev)
        _hip.call("yogo_conv_first_gram", cur, gpart, gram64, S.gram, B, H, W, st)
        mean, invstd = _bn_finalize(eng, L, "yogo_bn_stats_from_gram", gram64, w32, bias, count=B * OH * OW, dev=dev, st=st)
    else:
        invstd = torch.empty(L.cout, dtype=torch.float32, device=dev)
        _hip.call("yogo_bn_invstd", bn.running_var, float(bn.eps), invstd, L.cout, st)
        mean = bn.running_mean
    # sweep 2: the convolution again, y = act(BatchNorm(z)) and what backward needs of z: its sign map when the fused backward
    # sweep can take that (it derives everything else from its own sums), else z itself
    # (the sign-map sweep has no byte-wise route: a batch at an odd address -- a view into a byte buffer -- keeps z)
    no_z = (_L0_NO_Z and _FUSE_LAYER0_BWD and S.gram is not None and L.conv.bias is None and cur.data_ptr() % 2 == 0
            and _hip.lib().yogo_conv_first_bn_wgrad_xs_supported(0, L.cin, L.cout, H, W, L.s, L.act))
    if no_z:
        out8 = None
        S.signs0 = torch.empty(B, OH * OW * 2, dtype=torch.uint8, device=dev)
        _hip.call("yogo_conv_first_mfma_signs", cur, w32, bias, None, y, S.signs0, mean, invstd, gamma, beta, B, L.cout, H, W, L.act, st)
    else:
        out8 = torch.empty_like(y)
        _hip.call("yogo_conv_first_mfma", cur, w32, bias, out8, y, mean, invstd, gamma, beta, None, B, L.cout, H, W, L.act, st)
    S.mean, S.invstd, S.bn_train, S.z, S.y = mean, invstd, bn_train, out8, y
    S.w_used = w32.to(torch.bfloat16).to(torch.float32)
    return y


def _layer_fwd_bf16(eng: Engine, i: int, L: Layer, S: Saved, bias, bn_train: bool, last: bool, B: int, H: int, W: int, st) -> torch.Tensor:
    """One block: the convolution (+bias, activation and dropout mask without BatchNorm), then BatchNorm + activation over its stored
    output.  The last layer writes fp32 NCHW.  Fills ``S``, returns the block output"""
    cur, mask, dev = S.x_in, S.mask, S.x_in.device
    OH, OW = L.out_hw(H, W)
    has_bn = L.bn is not None
    if last and (has_bn or mask is not None):
        raise RuntimeError("yogo_amd: BatchNorm / Dropout on the last layer is not supported by the bf16 path")
    fused_act = ACT_NONE if has_bn else L.act
    out8 = None if last else torch.empty(B, _blocks(L.cout), OH, OW, 8, dtype=torch.bfloat16, device=dev)
    out32 = torch.empty(B, L.cout, OH, OW, dtype=torch.float32, device=dev) if last else None
    stats = None
    rows = mpad = 0
    if i == 0:
        if bn_train:   # the only conv whose epilogue sums the BatchNorm statistics
            rows, mpad = _hip.query_ints("yogo_conv_first_stats_rows", 1, B, H, W, L.s)[0], L.cout
            stats = torch.empty(rows * mpad * 2, dtype=torch.float32, device=dev)
        _hip.call("yogo_conv_first_fwd_train_bf16", cur, 0 if cur.dtype == torch.uint8 else 1, _f32(L.conv.weight.detach()), bias,
                  out8, mask, stats, B, L.cin, L.cout, H, W, L.s, fused_act, st)
    else:
        pk = _packed_bf16(eng, i, 0)
        # algorithmic bytes: input + output once at storage precision (bf16 NCHW8c, channels padded to 16; fp32 head)
        nbytes = B * (_blocks(L.cin) * 8 * H * W * 2 + (L.cout * OH * OW * 4 if last else _blocks(L.cout) * 8 * OH * OW * 2))
        # mw tags the kernel variant for bench.py: 34 = conv_bf16_kernel<4,2,8,...> (128 output channels, stride 1)
        eng._tick("fwd", i, 2.0 * B * L.cout * L.cin * L.k * L.k * OH * OW, mw=34 if (L.cout > 64 and L.s == 1) else (35 if (L.cout > 64 and L.cin > 64 and L.k == 3) else 30), nbytes=nbytes)
        if L.act == ACT_SILU and not has_bn:   # silu'(z) needs the pre-activation: the conv writes it next to the output
            S.pre = torch.empty_like(out8)
            _hip.call("yogo_conv2d_fwd_bf16_pre", cur, pk, bias, out8, S.pre, mask, B, L.cin, L.cout, H, W, L.k, L.s, fused_act, st)
        elif L.act == ACT_LEAKY and not has_bn and not last:   # the data gradient below takes a 1-bit sign map, not the bf16 output
            S.signs = torch.empty(_hip.query_size("yogo_bf16_signs_bytes", B, L.cout, OH, OW), dtype=torch.uint8, device=dev)
            _hip.call("yogo_conv2d_fwd_bf16_signs", cur, pk, bias, out8, S.signs, mask, B, L.cin, L.cout, H, W, L.k, L.s, fused_act, st)
        else:
            _hip.call("yogo_conv2d_fwd_bf16", cur, pk, bias, out8, out32, mask, None, B, L.cin, L.cout, H, W, L.k, L.s, fused_act, st)
        eng._tock()
    if not has_bn:
        S.y = out32 if last else out8
        return S.y
    bn = L.bn
    gamma, beta = _bn_affine(L, dev)
    y = torch.empty_like(out8)
    if bn_train:
        if i > 0:   # statistics by a sweep over the stored bf16 output
            rows, mpad = _hip.query_ints("yogo_bn_bwd_bf16_rows", 1, B, OH * OW)[0], L.cout
            stats = torch.empty(rows * mpad * 2, dtype=torch.float32, device=dev)
            _hip.call("yogo_bn_stats_bf16", out8, stats, B, L.cout, OH * OW, st)
        mean, invstd = _bn_finalize(eng, L, "yogo_bn_finalize", stats, rows, mpad, count=B * OH * OW, dev=dev, st=st)
    else:
        invstd = torch.empty(L.cout, dtype=torch.float32, device=dev)
        _hip.call("yogo_bn_invstd", bn.running_var, float(bn.eps), invstd, L.cout, st)
        mean = bn.running_mean
    _hip.call("yogo_bn_apply_act_bf16", out8, y, mean, invstd, 0, float(bn.eps), gamma, beta, B, L.cout, OH * OW, L.act, st)
    S.mean, S.invstd, S.bn_train, S.z, S.y = mean, invstd, bn_train, out8, y
    return y


def _pair_fwd_eligible(eng: Engine, i: int, B: int, H: int, W: int) -> bool:
    """layers i and i + 1 are a stride-1 3x3 16 -> 32 and a stride-2 3x3 32 -> <= 64 LeakyReLU block without BatchNorm, neither the first
    nor the last layer, at a shape the one-launch pair takes (yogo_conv2d_fwd_bf16_signs_pair: layer i + 1 reads layer i's output from LDS)"""
    if i < 1 or i + 2 >= len(eng.layers):
        return False
    La, Lb = eng.layers[i], eng.layers[i + 1]
    if not all(L.k == 3 and L.bn is None and L.act == ACT_LEAKY for L in (La, Lb)) or La.s != 1 or Lb.s != 2:
        return False
    return bool(_hip.lib().yogo_conv2d_fwd_bf16_signs_pair_eligible(B, La.cin, La.cout, Lb.cout, H, W))


def _pair_fwd_bf16(eng: Engine, i: int, Sa: Saved, Sb: Saved, B: int, H: int, W: int, st) -> torch.Tensor:
    """_layer_fwd_bf16 of layers i and i + 1 (both the sign-map branch) in one call: fills both records as the two calls do"""
    La, Lb = eng.layers[i], eng.layers[i + 1]
    dev = Sa.x_in.device
    OH, OW = Lb.out_hw(H, W)
    bias_a = _f32(La.conv.bias.detach()) if La.conv.bias is not None else None
    bias_b = _f32(Lb.conv.bias.detach()) if Lb.conv.bias is not None else None
    pk_a, pk_b = _packed_bf16(eng, i, 0), _packed_bf16(eng, i + 1, 0)
    y1 = torch.empty(B, _blocks(La.cout), H, W, 8, dtype=torch.bfloat16, device=dev)
    y2 = torch.empty(B, _blocks(Lb.cout), OH, OW, 8, dtype=torch.bfloat16, device=dev)
    Sa.signs = torch.empty(_hip.query_size("yogo_bf16_signs_bytes", B, La.cout, H, W), dtype=torch.uint8, device=dev)
    Sb.signs = torch.empty(_hip.query_size("yogo_bf16_signs_bytes", B, Lb.cout, OH, OW), dtype=torch.uint8, device=dev)
    # one event for the pair, under layer i: the summed FLOPs, and the bytes the pair has to move (y0 in, y1 and y2 out; y1 is not read back)
    flops = 2.0 * B * 9 * (La.cout * La.cin * H * W + Lb.cout * Lb.cin * OH * OW)
    nbytes = B * 16 * ((_blocks(La.cin) + _blocks(La.cout)) * H * W + _blocks(Lb.cout) * OH * OW)
    eng._tick("fwd", i, flops, mw=30, nbytes=nbytes)
    _hip.call("yogo_conv2d_fwd_bf16_signs_pair", Sa.x_in, pk_a, bias_a, y1, Sa.signs, Sa.mask, pk_b, bias_b, y2, Sb.signs, Sb.mask,
              B, La.cin, La.cout, Lb.cout, H, W, ACT_LEAKY, st)
    eng._tock()
    Sb.x_in = y1
    Sa.y, Sb.y = y1, y2
    return y2


def forward_bf16_train(eng: Engine, x: torch.Tensor) -> Tuple[torch.Tensor, List[Saved]]:
    _check_bf16_train_input(eng, x)
    dev, st, B = x.device, _hip.stream_ptr(), x.shape[0]
    _pack_all_bf16(eng)
    masks = _dropout_masks(eng, B, dev)
    cur = x.contiguous() if x.dtype == torch.uint8 else _f32(x)
    H, W = int(cur.shape[2]), int(cur.shape[3])
    saved: List[Saved] = []
    n = len(eng.layers)
    paired = -1   # the layer the pair call of the layer before it has already run
    for i, L in enumerate(eng.layers):
        if i == paired:
            H, W = L.out_hw(H, W)
            continue
        OH, OW = L.out_hw(H, W)
        if OH <= 0 or OW <= 0:
            raise RuntimeError(f"yogo_amd: image too small at layer {i}")
        last = i == n - 1
        has_bn = L.bn is not None
        if L.act == ACT_SILU and not has_bn and (i == 0 or last):
            raise RuntimeError("yogo_amd: bf16 training of a first / last SiLU block without BatchNorm is not implemented (use fp32)")
        bias = _f32(L.conv.bias.detach()) if L.conv.bias is not None else None
        S = Saved(x_in=cur, mask=masks.get(i))
        bn_train = has_bn and (L.bn.training or L.bn.running_mean is None)
        if _PAIR_FWD and _pair_fwd_eligible(eng, i, B, H, W):
            OH2, OW2 = eng.layers[i + 1].out_hw(OH, OW)
            if OH2 <= 0 or OW2 <= 0:
                raise RuntimeError(f"yogo_amd: image too small at layer {i + 1}")
            S2 = Saved(x_in=None, mask=masks.get(i + 1))
            cur = _pair_fwd_bf16(eng, i, S, S2, B, H, W, st)
            saved += [S, S2]
            paired = i + 1
            H, W = OH, OW
            continue
        if (i == 0 and has_bn and S.mask is None and not last and cur.dtype == torch.uint8
                and _hip.lib().yogo_conv_first_mfma_supported(0, L.cin, L.cout, H, W, L.s)):
            cur = _first_mfma_fwd_bf16(eng, L, S, bias, bn_train, B, H, W, st)
        else:
            cur = _layer_fwd_bf16(eng, i, L, S, bias, bn_train, last, B, H, W, st)
        saved.append(S)
        H, W = OH, OW
    return cur, saved


def backward_bf16_train(eng: Engine, saved: List[Saved], graw: torch.Tensor,
                        grad_out: Optional[Dict[int, torch.Tensor]] = None, on_layer=None,
                        trace: Optional[dict] = None, flush_layers=None, stop_at: int = 0) -> List[Optional[torch.Tensor]]:
    """``on_layer(i)`` is called once every gradient kernel of layer i has been enqueued.  With ``flush_layers`` (layer indices) the
    hook only needs COMPLETE parameter gradients at those layers: the split-K reductions stay deferred and are flushed in front of
    the hook there (and behind the last layer) -- two launches for the data-parallel trainer's two-part exchange instead of one
    reduction per layer, the same bits.  Without it a hook gets every layer's gradients reduced as soon as the layer is through.
    ``trace`` (tests / probes only): a dict that receives clones of the activation gradients as they exist between the
    kernels -- ("g", i): gradient w.r.t. block i's output, ("dz", i): BatchNorm-backward output of block i; a tensor that a fused
    kernel never writes (layer 0's g under _L01_FUSE_BWD, the g of the block under the head under _HEAD_BN_FUSE) has no entry: a
    trace records the plan the product runs, it does not change it -- so that every
    kernel of a real step can be checked against the oracle given its ACTUAL inputs (tests/_util.py, teacher-forced check).
    ``stop_at`` (frozen lower layers, the autograd path): the pass ends with the parameter gradients of layer ``stop_at`` -- no data
    gradient of that layer and nothing of the layers below it is computed; their entries of the result are None."""
    n = len(eng.layers)
    if not 0 <= stop_at < n:
        raise ValueError(f"yogo_amd: stop_at {stop_at} is not a layer of this {n}-layer network")
    st, dev, clip = _hip.stream_ptr(), graw.device, float(eng.clip)
    grads: Dict[int, torch.Tensor] = {}

    def dst(param: torch.Tensor) -> torch.Tensor:
        if grad_out is not None and id(param) in grad_out:
            return grad_out[id(param)]
        return torch.empty(param.shape, dtype=torch.float32, device=dev)

    # Everything runs on the current stream, so the caching allocator orders each tensor's reuse behind its last use -- except the
    # split-K workspaces of a deferred reduction: the flush that reads them is enqueued layers later, so they stay referenced here
    # until the pass returns (freed earlier, a later layer's tensors would be handed their memory and overwrite the partial sums).
    queued_ws: List[torch.Tensor] = []
    # the split-K reductions of the weight gradients: deferred to ONE launch behind the last layer -- unless a per-layer hook wants
    # each layer's gradients as soon as the layer is through
    wq = _wgrad_queue() if (_WGRAD_DEFER_REDUCE and (on_layer is None or flush_layers is not None)) else None
    flush_at = frozenset(flush_layers) if flush_layers is not None else frozenset()
    if wq is not None:
        _hip.call("yogo_wgrad_reduce_queue_reset", wq)   # (a pass that raised half way must not leave its reductions behind)
    if graw.dtype == torch.bfloat16 and graw.ndim == 5:   # already NCHW8c (yogo_decode_bwd_bf16)
        g = graw
        B = g.shape[0]
    else:
        graw = _f32(graw)
        B, P, Sy, Sx = graw.shape
        g = torch.empty(B, _blocks(P), Sy, Sx, 8, dtype=torch.bfloat16, device=dev)
        _hip.call("yogo_nchw_f32_to_bf16_8c", graw, g, B, P, Sy * Sx, st)

    def bn_backward(L, S, g, head_g, OH, OW):
        """dz of the block (in place of g); given ``head_g``, the head's data gradient is computed inside both sweeps"""
        gamma, beta = _bn_affine(L, dev)
        dgamma, dbeta = _bn_grad_dst(L.bn, dst, grads, L.cout, dev)
        rows = _hip.query_ints("yogo_bn_bwd_bf16_rows", 1, B, OH * OW)[0]
        part = torch.empty(rows * L.cout * 2, dtype=torch.float32, device=dev)
        sums = torch.empty(2 * L.cout, dtype=torch.float32, device=dev)
        if head_g is not None:
            dz = torch.empty(B, _blocks(L.cout), OH, OW, 8, dtype=torch.bfloat16, device=dev)
            _hip.call("yogo_bn_bwd_bf16_head", *head_g, S.z, dz, S.mean, S.invstd, gamma, beta, L.act, dgamma, dbeta,
                      part, sums, B, L.cout, OH * OW, 1 if S.bn_train else 0, clip, st)
        else:
            dz = g
            _hip.call("yogo_bn_bwd_bf16", g, S.z, dz, S.mean, S.invstd, gamma, beta, L.act, dgamma, dbeta, part, sums, B, L.cout, OH * OW,
                      1 if S.bn_train else 0, clip, st)
        return dz

    def wgrad_first_bn(L, S, g, fused01, dw, IH, IW):
        """layer 0 with BatchNorm and no conv bias: BatchNorm backward, activation derivative and the weight gradient share ONE sweep
        over (image, g, z or its sign map) -- dz is never written (see conv_first_bn_wgrad_kernel).  ``g`` is None exactly when
        ``fused01`` is set: layer 1's sweep has then already folded its data gradient into the partial sums"""
        gamma, beta = _bn_affine(L, dev)
        dgamma, dbeta = _bn_grad_dst(L.bn, dst, grads, L.cout, dev)
        cols = _hip.query_ints("yogo_conv_first_bn_wgrad_cols", 1, L.cin, L.cout)[0]
        sums = torch.empty(cols, dtype=torch.float32, device=dev)
        xg = "_xs" if S.signs0 is not None else "_xg" if S.gram is not None else ""
        if fused01 is not None:   # layer 1's data gradient has filled the partial sums
            part, rows = fused01[:2]
        else:
            rows = _hip.query_ints("yogo_conv_first_wgrad_rows", 1, B, IH, IW, L.s)[0]
            part = torch.empty(rows * cols, dtype=torch.float32, device=dev)
            _hip.call("yogo_conv_first_bn_wgrad_bf16" + xg, S.x_in, 0 if S.x_in.dtype == torch.uint8 else 1, g,
                      S.signs0 if S.signs0 is not None else S.z, S.mean, S.invstd, gamma, beta, part, B, L.cin, L.cout, IH, IW, L.s, L.act, st)
        _hip.call("yogo_partials_reduce", part, rows, cols, 0.0, sums, st)
        _hip.call("yogo_conv_first_bn_wgrad_finalize" + xg, sums, *((S.gram,) if S.gram is not None else ()), S.mean, S.invstd, gamma,
                  S.w_used if S.w_used is not None else _f32(L.conv.weight.detach()), dw, dgamma,
                  dbeta, B, L.cin, L.cout, IH, IW, L.s, 1 if S.bn_train else 0, clip, st)

    def wgrad_dgrad_first(L, S, g, dw, db, IH, IW, OH, OW):
        """layer 1 above a matrix-core layer 0 that kept its sign map: ONE sweep over g does layer 1's weight gradient and folds its
        data gradient straight into layer 0's backward sums, which it returns as (part, rows, IH, IW)"""
        L0, S0 = eng.layers[0], saved[0]
        ws = torch.empty(_hip.query_size("yogo_conv2d_dgrad_wgrad_first_bwd_workspace_bytes", B, IH, IW) // 4, dtype=torch.float32, device=dev)
        rows = _hip.query_ints("yogo_conv2d_dgrad_first_bwd_rows", 1, B, IH, IW, 1)[0]
        cols = _hip.query_ints("yogo_conv_first_bn_wgrad_cols", 1, L0.cin, L0.cout)[0]
        part = torch.empty(rows * cols, dtype=torch.float32, device=dev)
        queued_ws.append(ws)
        eng._tick("wgrad", 1, 2.0 * B * L.cout * L.cin * L.k * L.k * OH * OW * 2, mw=30,
                  nbytes=B * (16 * (_blocks(L.cout) + _blocks(L.cin)) * OH * OW + 2 * IH * IW + 4 * IH * IW))
        _hip.call("yogo_conv2d_dgrad_wgrad_bf16_first_bwd", g, _packed_bf16(eng, 1, 1), S.x_in, S0.x_in, S0.signs0, part, dw, db, ws,
                  B, L.cin, L.cout, IH, IW, L0.act, clip, wq, st)
        eng._tock()
        return part, rows, IH, IW

    def wgrad(i, L, S, g, dw, db, IH, IW, OH, OW):
        """layers > 0 on the bf16 matrix cores; with the queue, the split-K reduction waits for the next flush"""
        ws = torch.empty(_hip.query_size("yogo_conv2d_wgrad_bf16_workspace_bytes", B, L.cin, L.cout, IH, IW, L.k, L.s) // 4,
                         dtype=torch.float32, device=dev)
        eng._tick("wgrad", i, 2.0 * B * L.cout * L.cin * L.k * L.k * OH * OW, mw=30,
                  nbytes=B * 2 * 8 * (_blocks(L.cout) * OH * OW + _blocks(L.cin) * IH * IW))
        if wq is not None:
            queued_ws.append(ws)
            _hip.call("yogo_conv2d_wgrad_bf16_deferred", S.x_in, g, dw, db, ws, B, L.cin, L.cout, IH, IW, L.k, L.s, clip, wq, st)
        else:
            _hip.call("yogo_conv2d_wgrad_bf16", S.x_in, g, dw, db, ws, B, L.cin, L.cout, IH, IW, L.k, L.s, clip, st)
        eng._tock()

    def dgrad(i, L, g, Sp, act_ref, ref_act, IH, IW, OH, OW):
        """data gradient of layer i with the activation derivative and dropout mask of the block below fused into its epilogue"""
        pk = _packed_bf16(eng, i, 2 if (L.s == 2 and L.k == 3) else 1)
        dx = torch.empty(B, _blocks(L.cin), IH, IW, 8, dtype=torch.bfloat16, device=dev)
        signs = Sp.signs if ref_act == ACT_LEAKY else None   # one byte per 16-byte unit in place of the reference
        if signs is not None:
            nbytes = B * (16 * _blocks(L.cout) * OH * OW + 17 * _blocks(L.cin) * IH * IW)
        else:
            nbytes = B * 2 * 8 * (_blocks(L.cout) * OH * OW + _blocks(L.cin) * IH * IW * (2 if act_ref is not None else 1))
        eng._tick("dgrad", i, 2.0 * B * L.cout * L.cin * L.k * L.k * OH * OW, mw=34 if (L.cin > 64 and L.s == 1 and act_ref is None) else 30, nbytes=nbytes)
        if signs is not None:
            _hip.call("yogo_conv2d_dgrad_bf16_signs", g, pk, dx, signs, Sp.mask, B, L.cin, L.cout, IH, IW, L.k, L.s, st)
        else:
            _hip.call("yogo_conv2d_dgrad_bf16", g, pk, dx, act_ref, ref_act, Sp.mask, B, L.cin, L.cout, IH, IW, L.k, L.s, st)
        eng._tock()
        return dx

    head_g = None    # (head gradient, head weights, head channels) while the head's data gradient is left to the BatchNorm backward below
    fused01 = None   # (part, rows, OH, OW) of layer 0's backward sums when layer 1's sweep produced them (g is then None at layer 0)
    for i in range(n - 1, stop_at - 1, -1):
        L, S = eng.layers[i], saved[i]
        OH, OW = (int(g.shape[2]), int(g.shape[3])) if g is not None else fused01[2:]
        IH, IW = int(S.x_in.shape[2]), int(S.x_in.shape[3])
        Lp, Sp = (eng.layers[i - 1], saved[i - 1]) if i > stop_at else (None, None)
        # ---- the plan of this layer --------------------------------------------------------------------------------------
        # layer 0's BatchNorm backward and weight gradient in one sweep (wgrad_first_bn)
        fuse0 = _FUSE_LAYER0_BWD and i == 0 and L.bn is not None and L.conv.bias is None and L.act in (ACT_NONE, ACT_LEAKY)
        # layer 1's weight gradient and data gradient in one sweep that feeds layer 0's (wgrad_dgrad_first): layer 0 has no data
        # gradient of its own, so its dy need not exist; a trace then has no ("g", 0)
        fuse01 = False
        if _L01_FUSE_BWD and i == 1 and stop_at == 0 and _FUSE_LAYER0_BWD:
            fuse01 = bool(Sp.signs0 is not None and Sp.x_in.dtype == torch.uint8 and Lp.bn is not None and Lp.conv.bias is None and Lp.cin == 1
                          and Lp.s == 2 and Lp.act in (ACT_NONE, ACT_LEAKY) and L.k == 3 and L.s == 1 and Sp.mask is None
                          and _hip.lib().yogo_conv2d_dgrad_first_bwd_supported(L.cin, L.cout, IH, IW, B, Lp.act))
        # the 1x1 head above a BatchNorm block leaves its data gradient to that block's BatchNorm backward: 12 multiply-adds per element
        # there are cheaper than writing and twice reading the 128-channel data gradient (a trace then has no ("g", n - 2))
        head_below = bool(_HEAD_BN_FUSE and i == n - 1 and Lp is not None and i - 1 > 0 and L.k == 1 and L.s == 1 and L.cout <= 16
                          and Lp.bn is not None and Lp.cout % 16 == 0 and g.shape[1] == 2)
        # the reference the data gradient takes for the activation derivative of the block below: none when that block's BatchNorm
        # backward applies it, its output for LeakyReLU (sign of the output = sign of the pre-activation), its pre-activation for SiLU
        act_ref, ref_act = None, ACT_NONE
        if Lp is not None and Lp.bn is None and Lp.act != ACT_NONE:
            act_ref, ref_act = (Sp.y if Lp.act == ACT_LEAKY else Sp.pre), Lp.act
        if trace is not None and g is not None and head_g is None:   # (under head_g, g is still the head's gradient: recorded above)
            trace[("g", i)] = g.clone()
        # ---- BatchNorm backward ------------------------------------------------------------------------------------------
        if L.bn is not None and not fuse0:
            g, head_g = bn_backward(L, S, g, head_g, OH, OW), None
            if trace is not None:
                trace[("dz", i)] = g.clone()
        # ---- weight / bias gradient --------------------------------------------------------------------------------------
        dw = dst(L.conv.weight)
        db = dst(L.conv.bias) if L.conv.bias is not None else None
        if fuse0:
            wgrad_first_bn(L, S, g, fused01, dw, IH, IW)
        elif fuse01:
            fused01 = wgrad_dgrad_first(L, S, g, dw, db, IH, IW, OH, OW)
        elif i == 0:   # any other layer 0
            _first_wgrad("yogo_conv_first_wgrad_bf16g", L, S.x_in, g, dw, db, clip, st)
        else:
            wgrad(i, L, S, g, dw, db, IH, IW, OH, OW)
        if db is not None:
            grads[id(L.conv.bias)] = db
        grads[id(L.conv.weight)] = dw
        # ---- hook --------------------------------------------------------------------------------------------------------
        if on_layer is not None:
            if wq is not None and i in flush_at:   # the hook takes the gradients of layers >= i: their reductions run now, as one launch
                _hip.call("yogo_wgrad_reduce_flush", wq, st)
            on_layer(i)
        # ---- data gradient -----------------------------------------------------------------------------------------------
        if fuse01:   # (went into layer 0's sums above)
            g = None
        elif head_below:
            head_g = (g, _f32(L.conv.weight.detach()).reshape(L.cout, L.cin), L.cout)
        elif i > stop_at:
            g = dgrad(i, L, g, Sp, act_ref, ref_act, IH, IW, OH, OW)
    if wq is not None:   # every layer's split-K reduction in ONE launch (they are ~21 us each, mostly launch and tail latency)
        _hip.call("yogo_wgrad_reduce_flush", wq, st)
    bb = eng.backbone_ref()
    return [grads.get(id(p)) for p in bb.parameters()]


_WGRAD_QUEUE = None


def _wgrad_queue() -> int:
    """the process's queue of deferred weight-gradient reductions (yogo_wgrad_reduce_queue_create; one host thread drives a GPU)"""
    global _WGRAD_QUEUE
    if _WGRAD_QUEUE is None:
        import ctypes
        h = ctypes.c_void_p(0)
        _hip.call("yogo_wgrad_reduce_queue_create", ctypes.addressof(h))
        _WGRAD_QUEUE = int(h.value)
    return _WGRAD_QUEUE


_ENGINES: "weakref.WeakKeyDictionary[nn.Module, Engine]" = weakref.WeakKeyDictionary()


def get_engine(backbone: nn.Sequential) -> Engine:
    eng = _ENGINES.get(backbone)
    if eng is None:
        eng = Engine(backbone)
        _ENGINES[backbone] = eng
    return eng


class _BackboneFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, backbone, *params):  # type: ignore[override]
        eng = get_engine(backbone)
        raw, saved = eng.forward(x, need_grad=True)
        ctx.eng = eng
        ctx.saved = saved
        return raw

    @staticmethod
    def backward(ctx, graw):  # type: ignore[override]
        with torch.cuda.device(graw.device):
            grads = ctx.eng.backward(ctx.saved, graw)
        ctx.saved = None
        return (None, None, *grads)


# ---- bf16 training through autograd: the module surface under torch.autocast("cuda", dtype=torch.bfloat16) -------------------------
# The same kernel sequence as HipTrainer(half=True), with the autograd semantics a torch training loop relies on: the parameters are
# saved for backward (an in-place update between forward and backward raises torch's version error instead of differentiating repacked
# new weights), one backward per graph (the Saved records are handed over to it), several live graphs, gradients accumulated by autograd,
# and frozen parameters -- None for them, and the backward pass ends at the lowest trainable layer when that layer is >= 2.
_BF16_BWD_LOCK = threading.Lock()   # autograd runs backward on one thread per device; the deferred-reduction queue is one per process


def bf16_training_requested() -> bool:
    """True inside `torch.autocast("cuda", dtype=torch.bfloat16)` -- how the reference's training loop asks for half precision
    (yogo/train.py:315-318, there in fp16; fp16 autocast keeps the fp32 kernels here)"""
    return bf16_inference_requested()


def bf16_train_supported(eng: Engine) -> bool:
    """the network is one forward_bf16_train / backward_bf16_train take: False for everything forward_bf16_train refuses (which still
    raises on its own) -- a first convolution that is not a 1- or 3-channel 3x3, a first or last SiLU block without BatchNorm,
    BatchNorm or Dropout2d on the last layer, BatchNorm2d(momentum=None) -- and for a network of one layer"""
    layers = eng.layers
    n = len(layers)
    if n < 2 or not eng._first_direct(0):
        return False
    for i, L in enumerate(layers):
        if i > 0 and L.cin != layers[i - 1].cout:
            return False
        if L.act == ACT_SILU and L.bn is None and i in (0, n - 1):
            return False
        if L.bn is not None and L.bn.momentum is None:
            return False
    return layers[-1].bn is None and layers[-1].drop is None


def _param_layers(eng: Engine) -> Dict[int, int]:
    """id(parameter) -> index of the layer it belongs to"""
    out: Dict[int, int] = {}
    for i, L in enumerate(eng.layers):
        for m in (L.conv, L.bn):
            if m is not None:
                for p in m.parameters(recurse=False):
                    out[id(p)] = i
    return out


def bf16_autograd_backward(eng: Engine, saved: List[Saved], g: torch.Tensor, needs) -> List[Optional[torch.Tensor]]:
    """backward of the autograd functions: ``g`` = head gradient (bf16 NCHW8c or fp32 NCHW), ``needs`` = ctx.needs_input_grad of the
    backbone's parameters in ``backbone.parameters()`` order.  Gradients of the parameters that need none are None; when the lowest
    layer holding a trainable parameter is >= 2 the pass stops there (layers 0 / 1 keep their fused sweep: the full pass runs)."""
    bb = eng.backbone_ref()
    params = list(bb.parameters())
    needs = list(needs)
    if len(needs) != len(params):
        raise RuntimeError("yogo_amd: the backbone's parameters changed between forward and backward")
    if not any(needs):
        return [None] * len(params)
    layer_of = _param_layers(eng)
    lo = min(layer_of[id(p)] for p, nd in zip(params, needs) if nd)
    with _BF16_BWD_LOCK:
        grads = backward_bf16_train(eng, saved, g, stop_at=lo if lo >= 2 else 0)
    return [gr if nd else None for gr, nd in zip(grads, needs)]


class _BackboneBF16Fn(torch.autograd.Function):
    """the backbone alone on the bf16 training path: returns the fp32 head output; backward takes its fp32 gradient"""

    @staticmethod
    def forward(ctx, x, backbone, *params):  # type: ignore[override]
        eng = get_engine(backbone)
        with torch.cuda.device(x.device):
            raw, saved = forward_bf16_train(eng, x)
        ctx.save_for_backward(*params)
        ctx.eng, ctx.saved = eng, saved
        return raw

    @staticmethod
    def backward(ctx, graw):  # type: ignore[override]
        if ctx.saved is None:
            raise RuntimeError("yogo_amd: a second backward through a bf16 training graph is not supported (its forward records "
                               "belong to the first backward); run the forward again")
        ctx.saved_tensors   # (raises torch's version error if a parameter was modified in place since the forward)
        saved, ctx.saved = ctx.saved, None
        with torch.cuda.device(graw.device):
            grads = bf16_autograd_backward(ctx.eng, saved, graw, ctx.needs_input_grad[2:])
        return (None, None, *grads)


def backbone_apply(backbone: nn.Sequential, x: torch.Tensor) -> torch.Tensor:
    _hip.require_cuda(x, "the input batch")
    params = list(backbone.parameters())
    if not backbone.training and not torch.is_grad_enabled() and (
            bf16_inference_requested() or getattr(backbone, "bf16_inference", False)):
        raw = backbone_infer_bf16(backbone, x)
        if raw is not None:
            return raw
    with torch.cuda.device(x.device):
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            if bf16_training_requested() and bf16_train_supported(get_engine(backbone)):
                return _BackboneBF16Fn.apply(x, backbone, *params)
            return _BackboneFn.apply(x, backbone, *params)
        raw, _ = get_engine(backbone).forward(x, need_grad=False)
        return raw

class InferEngineBF16:
    """Eval-mode forward on the bf16 matrix cores (the reference runs `yogo infer` under bf16 autocast, yogo/infer.py:313-317).

    Activations live in NCHW8c bf16 ([B][C/8][H][W][8]); eval-mode BatchNorm is folded into the packed weights (per-output-
    channel scale) and the bias; bias + activation are fused into the conv epilogue; the last layer writes fp32 NCHW for the
    decode / NMS kernels.  Folded tensors and packed weights are cached and rebuilt when any parameter or buffer changes.
    """

    def __init__(self, engine: Engine):
        self.engine = engine
        self._key = None
        self._prep: List[Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]] = []
        self._fold: List[Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]] = []   # per layer: the folded (scale, bias) _prep was made of
        # tests: when a dict, forward() stores a clone of every layer's output under ("y", i) and the folded ("scale", i) / ("bias", i)
        # of _prepare (None where a layer has none; under the fused head + decode the last "y" is the decoded tensor) -- the teacher-forced check of
        # tests/_util.py.  It records the plan, it does not change it
        self.trace: Optional[dict] = None

    def _state_key(self):
        k = [self.engine.generation]
        for L in self.engine.layers:
            ts = [L.conv.weight, L.conv.bias]
            if L.bn is not None:
                ts += [L.bn.weight, L.bn.bias, L.bn.running_mean, L.bn.running_var]
            for t in ts:
                k.append(None if t is None else (t.data_ptr(), t._version))
        return tuple(k)

    def supported(self) -> bool:
        L0 = self.engine.layers[0]
        if not (L0.cin in (1, 3) and L0.k == 3):
            return False
        return all(L.bn is None or (not L.bn.training and L.bn.running_mean is not None) for L in self.engine.layers)

    @torch.no_grad()
    def _prepare(self) -> None:
        key = self._state_key()
        if key == self._key:
            return
        st = _hip.stream_ptr()
        prep, fold = [], []
        for i, L in enumerate(self.engine.layers):
            w = _f32(L.conv.weight.detach())
            bias = L.conv.bias.detach().float() if L.conv.bias is not None else None
            scale = None
            if L.bn is not None:
                bn = L.bn
                gamma = bn.weight.detach().float() if bn.weight is not None else torch.ones_like(bn.running_var)
                beta = bn.bias.detach().float() if bn.bias is not None else torch.zeros_like(bn.running_var)
                scale = gamma / torch.sqrt(bn.running_var.float() + bn.eps)
                base = bias if bias is not None else torch.zeros_like(scale)
                bias = beta + (base - bn.running_mean.float()) * scale
            fold.append((scale, bias))
            if i == 0:
                wf = w * scale[:, None, None, None] if scale is not None else w
                prep.append((wf.contiguous(), bias.contiguous() if bias is not None else None))
            else:
                nbytes = _hip.query_size("yogo_conv_bf16_packed_bytes", L.cin, L.cout, L.k, 0)
                packed = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
                _hip.call("yogo_conv_bf16_pack", w, scale.contiguous() if scale is not None else None, packed, L.cin, L.cout, L.k, 0, st)
                prep.append((packed, bias.contiguous() if bias is not None else None))
        self._prep, self._fold = prep, fold
        self._key = key

    @torch.no_grad()
    def forward(self, x: torch.Tensor, decode=None) -> torch.Tensor:
        """raw head output [B, 5 + C, Sy, Sx] -- or, given the decode's operands ``(cxs, cys, anchor_w, anchor_h, width_mult,
        height_mult, inference)`` and a 1x1 head the fused kernel takes, the DECODED tensor of yogo/model.py:277-313 (one launch for
        head + decode, bit-identical to the two)"""
        _hip.require_cuda(x, "the input batch")
        if x.ndim != 4:
            raise RuntimeError(f"yogo_amd: expected a [B,C,H,W] batch, got {tuple(x.shape)}")
        self._prepare()
        st = _hip.stream_ptr()
        dev = x.device
        B = x.shape[0]
        cur = x.contiguous() if x.dtype == torch.uint8 else _f32(x)
        H, W = int(cur.shape[2]), int(cur.shape[3])
        n = len(self.engine.layers)
        tc = self.trace
        if tc is not None:
            for i, (sc, bs) in enumerate(self._fold):
                tc[("scale", i)] = None if sc is None else sc.clone()
                tc[("bias", i)] = None if bs is None else bs.clone()
        for i, L in enumerate(self.engine.layers):
            OH, OW = L.out_hw(H, W)
            if OH <= 0 or OW <= 0:
                raise RuntimeError(f"yogo_amd: image too small at layer {i}")
            wq, bias = self._prep[i]
            last = i == n - 1
            if i == 0:
                if cur.shape[1] != L.cin:
                    raise RuntimeError(f"yogo_amd: layer 0 expects {L.cin} channels, got {cur.shape[1]}")
                mb = _hip.lib().yogo_bf16_channel_blocks(L.cout)
                out = torch.empty(B, mb, OH, OW, 8, dtype=torch.bfloat16, device=dev)
                if cur.dtype == torch.uint8 and _hip.lib().yogo_conv_first_mfma_supported(0, L.cin, L.cout, H, W, L.s):
                    _hip.call("yogo_conv_first_mfma", cur, wq, bias, out, None, None, None, None, None, None, B, L.cout, H, W, L.act, st)
                else:
                    _hip.call("yogo_conv_first_fwd_bf16", cur, 0 if cur.dtype == torch.uint8 else 1, wq, bias, out, B, L.cin, L.cout, H, W,
                              L.s, L.act, st)
                if last:
                    raise RuntimeError("yogo_amd: a one-layer network is not supported by the bf16 inference path")
            elif last:
                out = torch.empty(B, L.cout, OH, OW, dtype=torch.float32, device=dev)
                if decode is not None and head_decode_fusable(L):
                    cxs, cys, aw, ah, wm, hm, inference = decode
                    cxs, cys = _hip.grid_buffers(cxs, cys, OH, OW, dev)   # (the kernel indexes them as [OH * OW])
                    _hip.call("yogo_head1x1_decode_fwd_bf16", cur, wq, bias, out, cxs, cys, B, L.cin, L.cout, OH, OW, aw, ah, wm, hm, 1 if inference else 0, st)
                    self.decoded = True
                else:
                    _hip.call("yogo_conv2d_fwd_bf16", cur, wq, bias, None, out, None, None, B, L.cin, L.cout, H, W, L.k, L.s, L.act, st)
                    self.decoded = False
            else:
                mb = _hip.lib().yogo_bf16_channel_blocks(L.cout)
                out = torch.empty(B, mb, OH, OW, 8, dtype=torch.bfloat16, device=dev)
                _hip.call("yogo_conv2d_fwd_bf16", cur, wq, bias, out, None, None, None, B, L.cin, L.cout, H, W, L.k, L.s, L.act, st)
            if tc is not None:
                tc[("y", i)] = out.clone()
            cur, H, W = out, OH, OW
        return cur


def head_decode_fusable(L) -> bool:
    """the last layer is a plain 1x1 head the fused head + decode kernel takes (yogo_head1x1_decode_fwd_bf16)"""
    return L.k == 1 and L.s == 1 and L.bn is None and L.act == 0 and 6 <= L.cout <= 16 and L.cin % 16 == 0 and L.cin <= 128


def bf16_inference_requested() -> bool:
    """True inside `torch.autocast("cuda", dtype=torch.bfloat16)` -- how the reference's predict() asks for half inference"""
    try:
        return bool(torch.is_autocast_enabled()) and torch.get_autocast_gpu_dtype() == torch.bfloat16
    except Exception:
        return False


def backbone_infer_bf16(backbone: nn.Sequential, x: torch.Tensor, decode=None):
    """raw head output via the bf16 path, or None when the model state does not allow it (train-mode BatchNorm, ...).  With ``decode``
    (the decode's operands, see InferEngineBF16.forward) the result is ``(tensor, decoded)``: decoded = True when head + decode ran as one
    launch and ``tensor`` already is the decoded prediction"""
    eng = get_engine(backbone)
    inf = eng._infer_bf16
    if inf is None:
        inf = eng._infer_bf16 = InferEngineBF16(eng)
    if not inf.supported():
        return None
    with torch.cuda.device(x.device):
        if decode is None:
            return inf.forward(x)
        out = inf.forward(x, decode=decode)
        return out, bool(inf.decoded)
