"""Every route of the bf16 convolution engine -- forward, data gradient, weight gradient -- held to EXACT integer sums at its tile, band,
parity and channel-padding edges (tests/_conv_bf16_exact.py says why no tolerance is needed).

Every case runs through the public entry points under the product library's plan and, wherever the launch log shows a specialised kernel
(conv_bf16_ws / ws16 / ws3 / staged / staged_pair / s2d_direct / 1x1_f32), once more under the test-hooks library with those kernels switched
off, so that the tiled conv_bf16_kernel they shadow is held to the same bits -- and, where conv_bf16_ws16_kernel ran, once with only that
member off (conv_bf16_ws_kernel<0> on the bias-free launches) and once with it on every eligible launch (conv_bf16_ws16_kernel<true>, the
biased form, which the hooks library alone can select).  Nothing is compared with another route: everything is compared with the float64 reference.
Outputs start as NaN / 0xA5 between sentinel regions (tests/_util.py: Guarded).  `pytest -s` prints the route table (profiles/conv_bf16_exact.log)."""
import contextlib
import ctypes
import re

import pytest
import torch

import _conv_bf16_exact as X
import test_gpu_bf16 as TB
import test_gpu_ws as TW
from _util import TF_ULP

pytestmark = pytest.mark.gpu

MAX_ELEMS = 4 * 1024 * 1024     # entries whose largest tensor exceeds this are left out (listed in EXCLUDED below)


# ---- the cases: (B, Cin, Cout, IH, IW, k, s) of the FORWARD convolution; every case runs every entry point -------------------------
def _imported():
    """the shape lists the project has curated for edges, by import, each as (source, forward-convolution case)"""
    out = [("bf16.CASES", c) for c in TB.CASES]
    out += [("bf16.workspace", c) for c in TB.test_wgrad_bf16_workspace_is_large_enough.pytestmark[0].args[1]]
    for kind, B, Cin, H, W in TW.CASES + TW.WS16_CASES:
        # a data-gradient entry (B, Cin, H, W) is the gradient of a forward convolution 128 -> Cin (test_gpu_ws.py: _run_in)
        out.append(("ws." + kind, (B, 128, Cin, H, W, 3, 1) if kind.startswith("dgrad") else (B, Cin, 128, H, W, 3, 1)))
    out += [("ws.s2f." + kind, (B, Cin, 128, H, W, 3, 2)) for kind, B, Cin, H, W in TW.S2F_CASES]
    out += [("ws.s2d." + kind, (B, M, K, OH, OW, 3, 2)) for kind, B, K, M, OH, OW in TW.S2D_THIN_CASES]   # dx [M] <- dy [K]: forward M -> K
    out += [("ws.thin." + kind, (B, Cin, Cout, H, W, 3, s)) for kind, B, Cin, Cout, H, W, s in TW.THIN_CASES]
    out += [("ws.head." + kind, (B, Cin, Cout, H, W, 1, 1)) for kind, B, Cin, Cout, H, W in TW.HEAD_CASES]
    return out


def _largest(case):
    B, Cin, Cout, IH, IW, k, s = case
    OH, OW = X.out_hw(IH, IW, k, s)
    return max(B * X.blocks(Cin) * 8 * IH * IW, B * X.blocks(Cout) * 8 * OH * OW)


EDGES = [
    # H or W of 1, 2 and 3 (the persistent kernels refuse IH, IW < 3: the tiled kernel takes these also under the product's plan)
    (1, 128, 128, 1, 9, 3, 1), (2, 128, 128, 2, 2, 3, 1), (1, 128, 128, 3, 1, 3, 1), (1, 64, 128, 2, 3, 3, 1), (1, 128, 128, 1, 1, 3, 1),
    (1, 128, 128, 2, 5, 3, 2), (1, 128, 128, 1, 1, 3, 2), (1, 64, 64, 1, 2, 3, 1), (1, 32, 32, 3, 2, 3, 1), (1, 128, 12, 1, 1, 1, 1), (1, 128, 12, 2, 3, 1, 1),
    # stride 2 with odd and even H, W in all four combinations
    (1, 32, 64, 5, 6, 3, 2), (1, 32, 64, 6, 5, 3, 2), (1, 128, 128, 7, 7, 3, 2), (1, 128, 128, 8, 8, 3, 2),
    # widths one below, at and one above the row-staged pitches: 62, 63, 64 and 126, 127 at stride 1; 31 and 32 output columns at stride 2
    (1, 16, 32, 10, 62, 3, 1), (1, 16, 32, 10, 63, 3, 1), (1, 16, 32, 10, 64, 3, 1), (1, 16, 32, 6, 126, 3, 1), (1, 16, 32, 6, 127, 3, 1),
    (1, 32, 64, 9, 61, 3, 2), (1, 32, 64, 9, 62, 3, 2), (1, 32, 64, 9, 63, 3, 2), (1, 32, 64, 9, 64, 3, 2),
    # plane sizes one below, at and one above the 32-, 128- and 256-pixel tiles of the staged, ws3, ws, ws16 and head kernels
    (1, 128, 128, 3, 85, 3, 1), (1, 128, 128, 3, 86, 3, 1), (1, 128, 128, 16, 16, 3, 1), (1, 128, 128, 3, 11, 3, 1),
    (1, 128, 128, 3, 85, 3, 2), (1, 128, 128, 16, 16, 3, 2), (1, 128, 12, 3, 11, 1, 1), (1, 128, 12, 4, 8, 1, 1), (1, 16, 32, 3, 11, 3, 1), (1, 32, 64, 7, 21, 3, 2),
    # B = 3: persistent workgroups cross image seams with a partial last tile
    (3, 128, 128, 5, 9, 3, 1), (3, 128, 128, 9, 7, 3, 2), (3, 16, 32, 9, 35, 3, 1), (3, 32, 64, 7, 9, 3, 2), (3, 64, 128, 6, 11, 3, 1),
    # channel counts that are no multiple of 16 on both sides; M = 65 and 127 into the direct stride-2 data gradient
    (1, 7, 12, 6, 9, 3, 1), (2, 12, 24, 5, 8, 3, 2), (1, 24, 40, 7, 6, 3, 2), (1, 40, 7, 6, 7, 3, 1), (1, 40, 24, 4, 5, 1, 1), (2, 65, 128, 7, 9, 3, 2),
    (1, 127, 128, 6, 8, 3, 2),
    # the wide64 tile: 64 -> 64 with OH * OW >= 4096
    (1, 64, 64, 64, 66, 3, 1),
    # three rows of 8000 / 10000 columns: 24 bands are not enough for the input tile to fit the LDS-DMA slots, the tiled kernel stages through
    # registers (dma=0; conv_bf16.hip, bf_plan: `ni + nw <= PF`)
    (1, 16, 32, 3, 8000, 3, 1), (1, 128, 128, 3, 10000, 3, 1),
    # the wgrad_bf16_kernel instantiations no imported list reaches (WGRAD_EXPECTED below, in its order): <4,1,1> at 3x3 stride 1, 1x1 and
    # stride 2; <2,2,1> at 1x1 and at stride 2 on 64 output channels (MPW 1); <2,1,2> at 1x1; <1,4,1> and <1,2,2> at stride 2; the tall
    # R = 8 tiling on 32 input channels (no PACK2) with 1 and 3 steps per row
    (1, 32, 128, 5, 9, 3, 1), (1, 32, 128, 4, 5, 1, 1), (1, 32, 128, 7, 9, 3, 2), (1, 64, 64, 4, 5, 1, 1), (1, 64, 64, 7, 9, 3, 2), (1, 32, 64, 4, 5, 1, 1),
    (1, 128, 32, 7, 9, 3, 2), (1, 64, 32, 7, 9, 3, 2), (1, 32, 32, 70, 9, 3, 1), (1, 32, 32, 70, 40, 3, 1),
    # LEAN2 + PACK2 with 2 steps per row (WGRAD_LOOPS below: the one (loop, steps per row) pair the lists above lack)
    (1, 16, 32, 70, 20, 3, 1),
]

CASES, SOURCES, EXCLUDED = [], {}, []
for _src, _c in _imported() + [("edge", c) for c in EDGES]:
    _c = tuple(_c)
    if _largest(_c) > MAX_ELEMS:
        EXCLUDED.append((_src, _c))
        continue
    SOURCES.setdefault(_c, []).append(_src)
    if _c not in CASES:
        CASES.append(_c)

# Left out by the 4M-element rule (their largest tensor, in elements of the padded NCHW8c layout) -- by name:
#   ws.CASES:   ("fwd_signs", 2, 64, 193, 258) 12.7M, ("fwd_plain", 40, 128, 97, 129) 64M, ("fwd_signs", 24, 64, 193, 258) 153M,
#               ("dgrad_mask", 7, 128, 50, 131) 5.9M
#   ws.WS16:    ("fwd_plain", 40, 128, 97, 129) 64M, ("dgrad", 7, 128, 50, 131) 5.9M
#   ws.S2F:     ("nobias", 2, 128, 193, 258) 12.7M, ("plain", 40, 128, 97, 129) 64M
#   ws.S2D:     ("signs", 2, 64, 32, 386, 516) 12.7M, ("signs", 2, 128, 128, 193, 258) 12.7M, ("signs", 40, 128, 128, 30, 30) 4.6M
#   ws.THIN:    ("signs", 2, 16, 32, 386, 516, 1) 12.7M, ("signs", 2, 32, 64, 386, 516, 2) 12.7M
# (the B = 24 and B = 40 entries, the 772x1032 production planes of layers 1 - 4 and the B = 7 entry; all keep their tolerance tests in
#  test_gpu_ws.py and test_gpu_production_shapes.py).  test_case_lists pins this list.
EXCLUDED_EXPECTED = 13

# Long walks of wgrad_bf16_kernel, through _wgrad alone (no forward, no data gradient): (case, loop, ring depth).  In every other case of this
# file a workgroup walks at most 3 units, so the prologue fills the ring and the in-loop LDS-DMA issue -- the slot schedule riding behind the
# MFMAs, the counted vmcnt, the ring index wrapping -- hardly runs.  Here units_per_split >= 2 * depth + 1 (several wraps, every value of the
# counted wait) and units % units_per_split != 0 (a short last split), asserted from the launch log; one entry per loop of the kernel and ring
# depth that loop can get (tools/wgrad_plan_sweep.cpp; its table: profiles/wgrad_bf16_one_definition.log).  Up to 16M elements per tensor.
WALK_MAX_ELEMS = 16 * 1024 * 1024
WGRAD_WALKS = [
    ((2, 128, 128, 1027, 7, 3, 1), "BLK4", 2), ((4, 128, 128, 521, 33, 3, 1), "BLK4", 2),        # ordinary chunks; wide (33-column) chunks: 9 steps
    ((3, 128, 64, 1027, 7, 3, 1), "LEAN", 3), ((3, 96, 128, 1027, 7, 3, 2), "LEAN", 3), ((2, 128, 64, 1027, 17, 3, 1), "LEAN", 2),
    ((5, 32, 64, 2041, 3, 3, 1), "LEAN2", 3), ((5, 64, 32, 1034, 33, 3, 2), "LEAN2", 2),
    ((5, 16, 16, 515, 65, 3, 1), "LEAN2+PACK2", 3), ((5, 16, 16, 2065, 49, 3, 1), "LEAN2+PACK2", 2),   # (the first: 5 chunks per row)
    ((5, 16, 32, 2041, 3, 3, 2), "generic32", 3), ((5, 16, 64, 1033, 49, 3, 1), "generic32", 2),
    ((5, 32, 32, 2041, 3, 3, 2), "generic64", 3), ((5, 32, 32, 1034, 97, 3, 2), "generic64", 2),
]

PAIR_CASES = [(B, 32, C2, IH, IW) for C2 in (64, 40) for (B, IH, IW) in ((2, 9, 34), (1, 4, 2), (3, 21, 63))]


def _id(case):
    return "x".join(str(v) for v in case)


# ---- running one case ---------------------------------------------------------------------------------------------------------------
SPECIALISED = ("conv_bf16_ws_kernel", "conv_bf16_ws16_kernel", "conv_bf16_ws3_kernel", "conv_bf16_staged_kernel", "conv_bf16_staged_pair_kernel",
               "conv_bf16_s2d_direct_kernel", "conv_bf16_1x1_f32_kernel")
_REFS, _LOGS, _FAILED = {}, {}, {}


def _ref(case, cls=None):
    if case not in _REFS:
        r = cls(case) if cls else (X.Ref(case) if len(case) == 7 else X.PairRef(case))
        r.check_preconditions()     # on the reference alone, before any GPU result is looked at
        _REFS[case] = r
    return _REFS[case]


def _kernel_of(line):
    return line.split("|")[0].split("<")[0].strip()


class _Plan:
    """one pass over the entry points under one library / switch setting: collects launch-log lines and mismatches"""

    def __init__(self, case, tag):
        from _util import Guarded
        from yogo_amd import _hip

        self.h, self.G, self.case, self.tag = _hip, Guarded, case, tag
        self.st = _hip.stream_ptr()
        self.lines, self.errors, self.guards, self.by_name = [], [], [], {}
        self.plan = None

    def out(self, shape, dtype):
        n = 1
        for v in shape:
            n *= v
        g = self.G(n, dtype)
        self.guards.append(g)
        return g.view.view(shape)

    def packed(self, w, Cin, Cout, k, mode):
        p = torch.empty(self.h.query_size("yogo_conv_bf16_packed_bytes", Cin, Cout, k, mode), dtype=torch.uint8, device="cuda")
        self.h.call("yogo_conv_bf16_pack", w.float().cuda(), None, p, Cin, Cout, k, mode, self.st)
        return p

    def launch(self, name, entry, *args):
        """one entry-point call with the launch log on; remembers the plan line of its (last) compute kernel"""
        h = self.h
        h.launch_log(True)
        try:
            h.call(entry, *args)
            torch.cuda.synchronize()
            lines = [ln for ln in h.read_launch_log() if not ln.startswith(("conv_bf16_pack", "wgrad_reduce"))]
        finally:
            h.launch_log(False)
        self.plan = " ;; ".join(lines)
        self.by_name[name] = lines
        self.lines += lines

    def route(self, base=None):
        """one line of the route table: the kernels of this plan, each with the entry points it took (``base``: the product plan's routes -- only
        the entry points that took another kernel than there are named).  Short forms: conv_bf16_X_kernel<..> -> X<..>, the tiled kernel ->
        tiled<..>{CKb, dma, rowpitch, TW}, true / false -> T / F."""
        def short(ln):
            k = ln.split("|")[0].strip().replace("conv_bf16_kernel", "tiled").replace("conv_bf16_", "").replace("_kernel", "")
            k = k.replace("true", "T").replace("false", "F").replace(", ", ",")
            if ln.startswith("conv_bf16_kernel"):
                kv = dict(re.findall(r"\b(CKb|dma|rowpitch|TW)=(\d+)", ln))
                k += "{%s,%s,%s,%s}" % (kv["CKb"], kv["dma"], kv["rowpitch"], kv["TW"])
            return k
        routes = {name: " + ".join(short(ln) for ln in lines) or "(no launch-log line)" for name, lines in self.by_name.items()}
        groups = {}
        for name, r in routes.items():
            if base is None or base.get(name) != r:
                groups.setdefault(r, []).append(name)
        head = f"{_id(self.case)} ({', '.join(SOURCES.get(self.case, ['pair']))})" if base is None else "   "
        print(f"\n{head} [{self.tag}] " + "; ".join(f"{r}: {', '.join(names)}" for r, names in groups.items()), end="")   # (pytest's dot ends the line)
        return routes

    def check(self, fn, what, *args):
        try:
            fn(f"{_id(self.case)} [{self.tag}] {what}", *args, self.plan)
        except AssertionError as e:
            print("\n  MISMATCH", e, end="")
            self.errors.append(str(e))

    def finish(self):
        for g in self.guards:
            try:
                g.check(f"{_id(self.case)} [{self.tag}]")
            except AssertionError as e:
                self.errors.append(str(e))


def _forward_and_dgrad(P, ref):
    h, st = P.h, P.st
    B, Cin, Cout, IH, IW, k, s = ref.case
    OH, OW = ref.OH, ref.OW
    cbi, cbo = X.blocks(Cin), X.blocks(Cout)
    bf16, u8, f32 = torch.bfloat16, torch.uint8, torch.float32
    x8 = X.to8c(ref.x).cuda()
    bias = ref.bias.float().cuda()
    so, si = ref.so.float().cuda(), ref.si.float().cuda()
    pk = P.packed(ref.w, Cin, Cout, k, 0)
    shape = (B, Cin, Cout, IH, IW, k, s)
    oshape = (B, cbo, OH, OW, 8)
    # ---- forward: bf16 output + BatchNorm partials (the general epilogue)
    rows, mpad = h.query_ints("yogo_conv2d_fwd_bf16_stats_shape", 2, *shape)
    out, stats = P.out(oshape, bf16), P.out((rows, mpad, 2), f32)
    P.launch("f.stats", "yogo_conv2d_fwd_bf16", x8, pk, bias, out, None, so, stats, *shape, 1, st)
    P.check(X.compare_8c, "forward with statistics", out.cpu(), ref.stored())
    P.check(X.compare, "BatchNorm partials (sum y, sum y^2), index (channel, 0 / 1)", stats.cpu().double().sum(0)[:Cout], ref.stats)
    # ---- fp32 NCHW output (the head's mode)
    o32 = P.out((B, Cout, OH, OW), f32)
    P.launch("f.f32", "yogo_conv2d_fwd_bf16", x8, pk, bias, None, o32, None, None, *shape, 0, st)
    P.check(X.compare, "forward, fp32 output", o32.cpu(), ref.y.float())
    # ---- the lean epilogue: LeakyReLU + scale; bias only; nothing at all (the bias-free plain launches: conv_bf16_ws16_kernel's)
    for name, b_, act, sc in (("f.lean", True, 1, True), ("f.plain", True, 0, False), ("f.nobias", False, 0, False), ("f.leaky", True, 1, False)):
        out = P.out(oshape, bf16)
        P.launch(name, "yogo_conv2d_fwd_bf16", x8, pk, bias if b_ else None, out, None, so if sc else None, None, *shape, act, st)
        P.check(X.compare_8c, name, out.cpu(), ref.stored(act, b_, sc))
    # ---- with the sign map
    out, sg = P.out(oshape, bf16), P.out((h.query_size("yogo_bf16_signs_bytes", B, Cout, OH, OW),), u8)
    P.launch("f.signs", "yogo_conv2d_fwd_bf16_signs", x8, pk, bias, out, sg, so, *shape, 1, st)
    P.check(X.compare_8c, "forward with sign map", out.cpu(), ref.stored())
    P.check(X.compare_signs, "forward with sign map", sg.cpu(), ref.stored())
    # ---- SiLU with the pre-activation kept: out_pre exact, the SiLU output at TF_ULP
    out, pre = P.out(oshape, bf16), P.out(oshape, bf16)
    P.launch("f.pre", "yogo_conv2d_fwd_bf16_pre", x8, pk, bias, out, pre, so, *shape, 2, st)
    P.check(X.compare_8c, "pre-activation output", pre.cpu(), ref.stored(0, True, False))
    full, want = X.from8c(out.cpu()).double(), ref.silu()
    d = (full[:, :Cout] - want).abs()
    nbad = int((~(d <= TF_ULP * torch.maximum(full[:, :Cout].abs(), want.abs()))).sum())
    if nbad or bool((full[:, Cout:] != 0).any()):
        P.errors.append(f"{_id(ref.case)} [{P.tag}] SiLU output: {nbad} beyond TF_ULP (max |d| {float(d.nan_to_num(1e30).max())}) or padding channels not zero | {P.plan}")
    # ---- data gradient: no reference; scale only; bf16 LeakyReLU reference + scale; sign map + scale
    dmode = 2 if (s == 2 and k == 3) else 1
    pd = P.packed(ref.w, Cin, Cout, k, dmode)
    dy8 = X.to8c(ref.dy).cuda()
    ishape = (B, cbi, IH, IW, 8)
    dx = P.out(ishape, bf16)
    P.launch("d", "yogo_conv2d_dgrad_bf16", dy8, pd, dx, None, 0, None, *shape, st)
    P.check(X.compare_8c, "data gradient", dx.cpu(), ref.dx())
    dx = P.out(ishape, bf16)
    P.launch("d.scale", "yogo_conv2d_dgrad_bf16", dy8, pd, dx, None, 0, si, *shape, st)
    P.check(X.compare_8c, "data gradient with scale", dx.cpu(), ref.dx(False, True))
    dx = P.out(ishape, bf16)
    P.launch("d.ref", "yogo_conv2d_dgrad_bf16", dy8, pd, dx, X.to8c(ref.refy).cuda(), 1, si, *shape, st)
    P.check(X.compare_8c, "data gradient with a bf16 LeakyReLU reference", dx.cpu(), ref.dx(True, True))
    dx = P.out(ishape, bf16)
    P.launch("d.signs", "yogo_conv2d_dgrad_bf16_signs", dy8, pd, dx, ref.ref_signs().cuda(), si, *shape, st)
    P.check(X.compare_8c, "data gradient with a sign-map reference", dx.cpu(), ref.dx(True, True))


def _wgrad(P, ref):
    h, st = P.h, P.st
    B, Cin, Cout, IH, IW, k, s = ref.case
    shape = (B, Cin, Cout, IH, IW, k, s)
    f32 = torch.float32
    x8, dy8 = X.to8c(ref.x).cuda(), X.to8c(ref.dy).cuda()
    ws_in = torch.empty(h.query_size("yogo_conv2d_wgrad_workspace_bytes", *shape) // 4 + 1, device="cuda")
    nws = h.query_size("yogo_conv2d_wgrad_bf16_workspace_bytes", *shape) // 4
    qh = ctypes.c_void_p(0)
    h.call("yogo_wgrad_reduce_queue_create", ctypes.addressof(qh))
    q = int(qh.value)
    try:
        for clip in (0.0, X.CLIP):
            wdw, wdb = ref.wgrad(clip)
            for name, entry in (("w", "yogo_conv2d_wgrad_bf16"), ("w.bf16in", "yogo_conv2d_wgrad_bf16in"), ("w.defer", "yogo_conv2d_wgrad_bf16_deferred")):
                dw, db = P.out((Cout, Cin, k, k), f32), P.out((Cout,), f32)
                ws = ws_in if entry.endswith("bf16in") else P.out((nws,), f32)
                if entry.endswith("deferred"):
                    P.launch(name, entry, x8, dy8, dw, db, ws, *shape, clip, q, st)
                    h.call("yogo_wgrad_reduce_flush", q, st)
                    torch.cuda.synchronize()
                else:
                    P.launch(name, entry, x8, dy8, dw, db, ws, *shape, clip, st)
                P.check(X.compare, f"{name} dw, clip {clip}", dw.cpu(), wdw.float())
                P.check(X.compare, f"{name} db, clip {clip}", db.cpu(), wdb.float())
    finally:
        h.call("yogo_wgrad_reduce_queue_destroy", q)


def _pair(P, ref):
    h, st = P.h, P.st
    B, C1, C2, IH, IW = ref.case
    OH, OW = ref.OH, ref.OW
    bf16, u8 = torch.bfloat16, torch.uint8
    x8 = X.to8c(ref.x).cuda()
    pk1, pk2 = P.packed(ref.w1, 16, C1, 3, 0), P.packed(ref.w2, C1, C2, 3, 0)
    y1, y2 = P.out((B, X.blocks(C1), IH, IW, 8), bf16), P.out((B, X.blocks(C2), OH, OW, 8), bf16)
    s1 = P.out((h.query_size("yogo_bf16_signs_bytes", B, C1, IH, IW),), u8)
    s2 = P.out((h.query_size("yogo_bf16_signs_bytes", B, C2, OH, OW),), u8)
    P.launch("pair", "yogo_conv2d_fwd_bf16_signs_pair", x8, pk1, ref.b1.float().cuda(), y1, s1, ref.s1.float().cuda(), pk2, ref.b2.float().cuda(), y2, s2,
             ref.s2.float().cuda(), B, 16, C1, C2, IH, IW, 1, st)
    P.check(X.compare_8c, "pair y1", y1.cpu(), ref.y1)
    P.check(X.compare_signs, "pair signs1", s1.cpu(), ref.y1)
    P.check(X.compare_8c, "pair y2", y2.cpu(), ref.y2)
    P.check(X.compare_signs, "pair signs2", s2.cpu(), ref.y2)


@contextlib.contextmanager
def _library(tag):
    """"product": libyogo_hip.so as it is; "tiled": the hooks library with every specialised kernel off; "ws": with only the 16x16x32 member off;
    "ws16b": with the 16x16x32 member on every eligible launch, the biased forward too"""
    if tag == "product":
        yield
        return
    from _util import hooks_library

    with hooks_library() as L:
        if tag == "tiled":
            for name in ("persistent", "direct", "staged", "staged_pair", "head"):
                getattr(L, "yogo_hook_conv_bf16_" + name)(0)
        else:
            L.yogo_hook_conv_bf16_ws16(0 if tag == "ws" else 2)
        yield


def run_case(case):
    """every entry point of one case under every plan it has; memoised (launch log and failures)"""
    if case in _LOGS:
        return _LOGS[case], _FAILED[case]
    ref = _ref(case)
    body = _pair if len(case) == 5 else _forward_and_dgrad
    lines, errors = [], []
    tags = ["product"]
    while tags:
        tag = tags.pop(0)
        with _library(tag):
            P = _Plan(case, tag)
            body(P, ref)
            if tag == "product" and len(case) == 7:
                _wgrad(P, ref)
            P.finish()
        routes = P.route(None if tag == "product" else base)
        if tag == "product":
            base = routes
        lines += P.lines
        errors += P.errors
        if tag == "product":
            seen = {_kernel_of(ln) for ln in P.lines}
            if "conv_bf16_ws16_kernel" in seen:
                tags += ["ws", "ws16b"]
            fwd_on_ws16 = any(ln.startswith("conv_bf16_ws16_kernel") for ln in P.by_name.get("f.nobias", []))
            if seen & set(SPECIALISED):
                tags.append("tiled")
        elif tag == "ws16b":
            if fwd_on_ws16 and not any(ln.startswith("conv_bf16_ws16_kernel<true>") for ln in P.by_name["f.plain"]):
                errors.append(f"{_id(case)} [ws16b]: the biased forward did not run on conv_bf16_ws16_kernel<true>")
        elif tag == "tiled":
            left = {_kernel_of(ln) for ln in P.lines} & set(SPECIALISED)
            if left:
                errors.append(f"{_id(case)} [tiled]: specialised kernels still launched with their switches off: {sorted(left)}")
    _LOGS[case], _FAILED[case] = lines, errors
    return lines, errors


def test_case_lists():
    """the imported lists are all here; what the 4M-element rule leaves out is what the comment above names"""
    assert len(EXCLUDED) == EXCLUDED_EXPECTED, EXCLUDED
    assert all(c[0] in (7, 24, 40) or max(c[3], c[4]) >= 258 for _, c in EXCLUDED), EXCLUDED
    assert len({c for _, c in _imported()} - {c for _, c in EXCLUDED} - set(CASES)) == 0


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_every_route_gives_the_exact_integers(case):
    _, errors = run_case(case)
    assert not errors, "\n".join(errors)


@pytest.mark.parametrize("case", PAIR_CASES, ids=_id)
def test_pair_gives_the_exact_values(case):
    _, errors = run_case(case)
    assert not errors, "\n".join(errors)


def test_small_planes_run_on_the_tiled_kernel_under_the_product_plan():
    """IH or IW below 3 with 128 output channels: conv_bf16_ws_eligible / conv_bf16_ws3_eligible refuse, the tiled kernel takes the launch"""
    for case in ((1, 128, 128, 1, 9, 3, 1), (2, 128, 128, 2, 2, 3, 1), (1, 128, 128, 2, 5, 3, 2)):
        lines, _ = run_case(case)
        assert not any(_kernel_of(ln).startswith(("conv_bf16_ws", "conv_bf16_ws3")) for ln in lines), (case, lines)
        assert any(ln.startswith("conv_bf16_kernel<4,") for ln in lines), (case, lines)


# ---- coverage -------------------------------------------------------------------------------------------------------------------------
TILED_RE = re.compile(r"conv_bf16_kernel<(\d+), (\d+), (\d+), (true|false), (\d+), (true|false), (\d+), (true|false), (true|false)> \| (.*)")
# every wgrad_bf16_kernel instantiation the dispatcher can launch (wgrad_bf16.hip: WbTable), as logged: <MBW, NBW, KS, T, S, R, MPW, PACK2, BLK4>
WGRAD_EXPECTED = [
    "wgrad_bf16_kernel<1, 1, 4, 1, 1, 4, 1, false, false>", "wgrad_bf16_kernel<1, 1, 4, 9, 1, 4, 1, false, false>",
    "wgrad_bf16_kernel<1, 1, 4, 9, 1, 8, 1, true, false>", "wgrad_bf16_kernel<1, 1, 4, 9, 2, 2, 1, false, false>",
    "wgrad_bf16_kernel<1, 2, 2, 1, 1, 4, 1, false, false>", "wgrad_bf16_kernel<1, 2, 2, 9, 1, 4, 1, false, false>",
    "wgrad_bf16_kernel<1, 4, 1, 1, 1, 4, 1, false, false>", "wgrad_bf16_kernel<1, 4, 1, 9, 1, 4, 1, false, false>",
    "wgrad_bf16_kernel<2, 1, 2, 9, 1, 4, 1, false, false>", "wgrad_bf16_kernel<2, 1, 2, 9, 2, 2, 1, false, false>",
    "wgrad_bf16_kernel<2, 2, 1, 9, 1, 4, 1, false, false>", "wgrad_bf16_kernel<2, 2, 1, 9, 1, 4, 2, false, true>",
    "wgrad_bf16_kernel<2, 2, 1, 9, 2, 2, 2, false, false>",
    # ... and the nine the EDGES entries above add
    "wgrad_bf16_kernel<4, 1, 1, 9, 1, 4, 1, false, false>", "wgrad_bf16_kernel<4, 1, 1, 1, 1, 4, 1, false, false>",
    "wgrad_bf16_kernel<4, 1, 1, 9, 2, 2, 1, false, false>", "wgrad_bf16_kernel<2, 2, 1, 1, 1, 4, 1, false, false>",
    "wgrad_bf16_kernel<2, 2, 1, 9, 2, 2, 1, false, false>", "wgrad_bf16_kernel<2, 1, 2, 1, 1, 4, 1, false, false>",
    "wgrad_bf16_kernel<1, 4, 1, 9, 2, 2, 1, false, false>", "wgrad_bf16_kernel<1, 2, 2, 9, 2, 2, 1, false, false>",
    "wgrad_bf16_kernel<1, 1, 4, 9, 1, 8, 1, false, false>",
]   # 22: the instantiations of the planner sweep's table (profiles/wgrad_bf16_one_definition.log)
WGRAD_RE = re.compile(r"wgrad_bf16_kernel<(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (true|false), (true|false)> \| (.*)")
# every (loop of the kernel, 16-pixel steps per staged row) pair a plan can ask for.  LEAN (KS = 1) never gets 4 steps per row: the planner
# sweep finds no KS = 1 plan with wce = 64.  BLK4's steps are 4 x 4 pixels: 8 per chunk, 9 for a wide chunk (33 - 36 columns).
WGRAD_LOOPS = ([("LEAN", n) for n in (1, 2, 3)] + [("LEAN2", n) for n in (1, 2, 3, 4)] + [("LEAN2+PACK2", n) for n in (1, 2, 3, 4)] +
               [("BLK4", "ordinary"), ("BLK4", "wide"), ("generic32", None), ("generic64", None)])


def _wgrad_plan(ln):
    """a wgrad_bf16_kernel launch-log line -> dict(loop, steps, depth, units, units_per_split): the loop as the kernel picks it (wgrad_bf16.hip,
    the dispatch at the end of the kernel) from the template arguments and the plan text"""
    m = WGRAD_RE.match(ln)
    assert m, ln
    MBW, NBW, KS, T, S, R, MPW = (int(v) for v in m.groups()[:7])
    PACK2, BLK4 = m.group(8) == "true", m.group(9) == "true"
    kv = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", m.group(10))}
    if BLK4:
        loop, steps = "BLK4", "wide" if kv["base_w"] + (1 if kv["rem_w"] else 0) > 32 else "ordinary"
    elif KS == 1:
        loop, steps = "LEAN", kv["wce"] >> 4
    elif R % KS == 0 and MPW == 1 and kv["xcb"] == (2 if PACK2 else 4):
        loop, steps = ("LEAN2+PACK2" if PACK2 else "LEAN2"), kv["wce"] >> 4
    else:
        loop, steps = "generic%d" % (16 * kv["xcb"]), None
    return dict(loop=loop, steps=steps, depth=kv["depth"], units=kv["units"], units_per_split=kv["units_per_split"])


@pytest.mark.parametrize("walk", WGRAD_WALKS, ids=lambda w: _id(w[0]) + "-" + w[1])
def test_wgrad_long_walks_give_the_exact_integers(walk):
    case, loop, depth = walk
    B, Cin, Cout, IH, IW, k, s = case
    ref = _ref(case, X.WgradRef)
    P = _Plan(case, "product")
    _wgrad(P, ref)
    P.finish()
    assert not P.errors, "\n".join(P.errors)
    plans = [_wgrad_plan(ln) for ln in P.lines if ln.startswith("wgrad_bf16_kernel")]
    print("\n" + _id(case), sorted({ln for ln in P.lines if ln.startswith("wgrad_bf16_kernel")}), end="")
    assert len(plans) >= 4 and all(p == plans[0] for p in plans), plans     # (both clips of the immediate and the deferred entry at least)
    p = plans[0]
    assert (p["loop"], p["depth"]) == (loop, depth), p
    assert p["units_per_split"] >= 2 * p["depth"] + 1 and p["units"] % p["units_per_split"] != 0, p


def test_wgrad_walks_cover_every_loop_and_ring_depth():
    """host side of the list: one entry per loop and per ring depth the planner sweep's table has for it (BLK4: 2 only), BLK4 with ordinary and wide chunks"""
    have = {(loop, depth) for _, loop, depth in WGRAD_WALKS}
    want = {("BLK4", 2)} | {(loop, d) for loop in ("LEAN", "LEAN2", "LEAN2+PACK2", "generic32", "generic64") for d in (2, 3)}
    assert have == want, (sorted(have - want), sorted(want - have))
    assert all(_largest(c) <= WALK_MAX_ELEMS for c, _, _ in WGRAD_WALKS)


def test_coverage_of_kernel_families_and_tiled_variants():
    lines = []
    for case in CASES + PAIR_CASES:
        lines += run_case(case)[0]
    families = {_kernel_of(ln) for ln in lines}
    for fam in ("conv_bf16_kernel",) + SPECIALISED + ("wgrad_bf16_kernel",):
        assert fam in families, (fam, sorted(families))
    seen = dict(MW=set(), S2D=set(), F32=set(), REF=set(), PP=set(), PP8=set(), LEPI=set(), dma=set(), CKb=set(), rowpitch=set(), ring=set(), wide64=set())
    for ln in lines:
        m = TILED_RE.match(ln)
        if not m:
            continue
        MW, NW, NWV, S2D, PF, F32, REF, PP, LEPI, txt = m.groups()
        kv = dict(re.findall(r"(\w+)=(\d+)", txt))
        seen["MW"].add(int(MW)); seen["S2D"].add(S2D); seen["F32"].add(F32); seen["REF"].add(int(REF)); seen["PP"].add(PP); seen["LEPI"].add(LEPI)
        seen["dma"].add(int(kv["dma"])); seen["CKb"].add(int(kv["CKb"])); seen["rowpitch"].add(int(kv["rowpitch"]))
        # the ring plan: the stride-2 data gradient of the 128-channel tile in 16-channel chunks on the fixed 2 + 3 slot layout
        seen["ring"].add(S2D == "true" and int(MW) == 4 and kv["CKb"] == "2" and int(kv["nchunk"]) >= 4 and txt.find("slots=2+3") >= 0)
        seen["wide64"].add((int(MW), int(NW), int(NWV)) == (2, 4, 8))
        seen["PP8"].add(PP == "true" and int(NWV) == 8)     # the ping-pong main loop proper (PP = true on 4 wavefronts names the lean4 loop)
    print("\ntiled variants seen:", {k: sorted(v) for k, v in seen.items()})
    wg = sorted({ln.split("|")[0].strip() for ln in lines if ln.startswith("wgrad_bf16_kernel")})
    names = [ln.split("|")[0].strip() for ln in lines]
    items = [f"{w} ({names.count(w)})" for w in sorted(set(names))]
    print("instantiations seen (launches):\n    " + "\n    ".join("; ".join(items[i:i + 3]) for i in range(0, len(items), 3)))
    assert seen["MW"] >= {1, 2, 4} and seen["S2D"] == {"true", "false"} and "true" in seen["F32"], seen
    assert seen["REF"] >= {0, 1, 2, 3} and "true" in seen["PP"] and True in seen["PP8"] and seen["LEPI"] == {"true", "false"}, seen
    assert seen["dma"] >= {0, 1, 2} and seen["CKb"] >= {2, 4, 8} and seen["rowpitch"] >= {0, 64, 128}, seen
    assert True in seen["ring"] and True in seen["wide64"], seen
    assert any(ln.startswith("conv_bf16_ws16_kernel<true>") for ln in lines) and any(ln.startswith("conv_bf16_ws16_kernel<false>") for ln in lines)
    assert len(set(WGRAD_EXPECTED)) == 22 and set(wg) == set(WGRAD_EXPECTED), (sorted(set(WGRAD_EXPECTED) - set(wg)), sorted(set(wg) - set(WGRAD_EXPECTED)))
    loops = {}
    for ln in lines:
        if ln.startswith("wgrad_bf16_kernel"):
            p = _wgrad_plan(ln)
            loops.setdefault((p["loop"], p["steps"]), ln.split("|")[1].strip().split(" B=")[0])
    print("wgrad_bf16_kernel loop bodies seen (loop, steps per row): first shape\n    " + "\n    ".join(f"{k}: {v}" for k, v in sorted(loops.items(), key=str)))
    assert set(loops) == set(WGRAD_LOOPS), (sorted(set(WGRAD_LOOPS) - set(loops), key=str), sorted(set(loops) - set(WGRAD_LOOPS), key=str))
