"""The head's decode / loss / NMS entry points of two builds of the library on the same device inputs, in one process: every output
compared as integer bit patterns (NaN positions included).  For a change that must not move a bit of yogo_amd/csrc/head_math.h's
arithmetic: build the earlier commit's library from a worktree, then
    python tools/cmp_head_bits.py EARLIER/libyogo_hip.so yogo_amd/lib/libyogo_hip.so
Exits non-zero at the first difference, naming the entry point, the shape and the index.

Inputs: every groups() batch and raw_batch() of tests/_loss_cases.py on its 17 x 19 grid (one workgroup plus a partial wavefront), and
random raw head outputs and labels, batch 3, grids 17 x 19 and 9 x 31, P in (6, 7, 12, 16, 17, 69): one class, the model's P, the last P
of one 16-channel block, the first of a second, MAX_CLASSES; a third of the cells labelled (mask values 1, 0.5, 2), a few raw sizes
above 80 and a few logits beyond +-16."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("tests", "oracle", ""):
    sys.path.insert(0, os.path.join(ROOT, d))
import _loss_cases as L
import yogo_oracle as O
from yogo_amd import _hip as H

BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
LIBS, WORDS, CALLS = [], [0], [0]


def call(lib, name, *args):
    rc = getattr(lib, name)(*[H._ptr(a) for a in args])
    if rc != 0:
        sys.exit(f"{name} failed (code {rc}): {lib.yogo_hip_last_error().decode()}")


def query_size(name, *args):
    out = ctypes.c_size_t(0)
    call(LIBS[0], name, *args, ctypes.addressof(out))
    return int(out.value)


def both(what, run):
    """run(lib) -> {output name: tensor} for either library; the first one's outputs are returned (the next call's inputs)"""
    a, b = (run(lib) for lib in LIBS)
    torch.cuda.synchronize()
    for k in a:
        if a[k].is_floating_point() and bool(torch.isnan(a[k]).all()):
            sys.exit(f"NOT WRITTEN {what} -> {k}: the output is still its NaN prefill")
        ia, ib = (t.contiguous().view(BITS[t.element_size()]) for t in (a[k], b[k]))
        if not torch.equal(ia, ib):
            bad = (ia != ib).flatten().nonzero().flatten()
            idx = tuple(int(v) for v in np.unravel_index(int(bad[0]), tuple(ia.shape)))
            sys.exit(f"DIFFERENT {what} -> {k} {tuple(ia.shape)}: {len(bad)} words, the first at {idx}: "
                     f"{int(ia[idx]):#x} != {int(ib[idx]):#x}")
        WORDS[0] += ia.numel()
    CALLS[0] += 1
    return a


def nans(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def loss(what, pred, label, w):
    B, P, Sy, Sx = pred.shape
    nws = query_size("yogo_loss_workspace_bytes", B, Sy, Sx) // 4

    def run(lib):
        o = dict(grad=nans(*pred.shape), loss=nans(4), ws=torch.zeros(nws, device="cuda"))
        call(lib, "yogo_loss_fwd_bwd", pred, label, o["grad"], o["loss"], o["ws"], B, P, Sy, Sx, *w, H.stream_ptr())
        return o
    return both(f"yogo_loss_fwd_bwd {what} {tuple(pred.shape)} w={w}", run)


def raw_level(what, raw, label, gout, cxs, cys, anchors, w):
    """every entry point that starts from the raw head output"""
    B, P, Sy, Sx = raw.shape
    Pb = ((P + 15) // 16) * 2
    st = H.stream_ptr()
    nws = query_size("yogo_loss_workspace_bytes", B, Sy, Sx) // 4
    shape = f"{what} {tuple(raw.shape)}"
    for inference in (0, 1):
        def fwd(lib):
            o = dict(out=nans(*raw.shape))
            call(lib, "yogo_decode_fwd", raw, o["out"], cxs, cys, B, P, Sy, Sx, *anchors, inference, st)
            return o
        out = both(f"yogo_decode_fwd {shape} inference={inference}", fwd)["out"]

        def bwd(lib):
            o = dict(graw=nans(*raw.shape))
            call(lib, "yogo_decode_bwd", raw, out, gout, o["graw"], B, P, Sy, Sx, inference, st)
            return o
        both(f"yogo_decode_bwd {shape} inference={inference}", bwd)

        def bwd16(lib):
            o = dict(graw8c=nans(B, Pb, Sy, Sx, 8, dtype=torch.bfloat16))
            call(lib, "yogo_decode_bwd_bf16", raw, out, gout, o["graw8c"], B, P, Sy, Sx, inference, st)
            return o
        both(f"yogo_decode_bwd_bf16 {shape} inference={inference}", bwd16)
        if inference == 0:
            loss(f"{what} (decoded)", out, label, w)

    def fused(lib):
        o = dict(graw8c=nans(B, Pb, Sy, Sx, 8, dtype=torch.bfloat16), loss=nans(4), ws=torch.zeros(nws, device="cuda"))
        call(lib, "yogo_decode_loss_bwd_bf16", raw, label, cxs, cys, o["graw8c"], o["loss"], o["ws"], B, P, Sy, Sx, *anchors, *w, st)
        return o
    both(f"yogo_decode_loss_bwd_bf16 {shape} w={w}", fused)
    cap = Sy * Sx
    nbytes = query_size("yogo_format_preds_workspace_bytes", B, Sy, Sx)
    for inference in (0, 1):
        for iou, min_cls, fmt in ((0.5, 0.0, 1), (0.0, 0.3, 0)):     # with NMS; without, and the class-confidence filter
            def nms(lib):
                o = dict(rows=nans(B, cap, P), cells=torch.full((B, cap), -1, dtype=torch.int64, device="cuda"),
                         counts=torch.full((B,), -1, dtype=torch.int32, device="cuda"))
                ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
                call(lib, "yogo_decode_format_preds_batched", raw, cxs, cys, o["rows"], o["cells"], o["counts"], ws, B, P, Sy, Sx, cap,
                     *anchors, inference, 0.5, iou, fmt, min_cls, st)
                return o
            both(f"yogo_decode_format_preds_batched {shape} inference={inference} iou_thresh={iou}", nms)


def head(gen, B, Cin, P, Sy, Sx, cxs, cys, anchors):
    st = H.stream_ptr()
    x = (torch.randn(B, Cin // 8, Sy, Sx, 8, generator=gen, device="cuda") * 2).to(torch.bfloat16)
    w = torch.randn(P, Cin, 1, 1, generator=gen, device="cuda") * 0.3
    bias = torch.randn(P, generator=gen, device="cuda")
    packed = torch.zeros(query_size("yogo_conv_bf16_packed_bytes", Cin, P, 1, 0), dtype=torch.uint8, device="cuda")
    call(LIBS[0], "yogo_conv_bf16_pack", w, None, packed, Cin, P, 1, 0, st)
    for inference in (0, 1):
        def run(lib):
            o = dict(out=nans(B, P, Sy, Sx))
            call(lib, "yogo_head1x1_decode_fwd_bf16", x, packed, bias, o["out"], cxs, cys, B, Cin, P, Sy, Sx, *anchors, inference, st)
            return o
        both(f"yogo_head1x1_decode_fwd_bf16 B={B} Cin={Cin} P={P} grid={Sy}x{Sx} inference={inference}", run)


def random_case(gen, B, P, Sy, Sx):
    """-> raw [B, P, Sy, Sx], label [B, 6, Sy, Sx], gout like raw"""
    C = P - 5
    r = lambda *s: torch.rand(*s, generator=gen, device="cuda")
    raw = torch.randn(B, P, Sy, Sx, generator=gen, device="cuda") * 2
    raw[:, 2:4][r(B, 2, Sy, Sx) < 0.03] = 85.0                       # past the exp clamp
    big = r(B, C, Sy, Sx)
    raw[:, 5:][big < 0.02] = -40.0                                   # beyond LSE_FOLD_MAX
    raw[:, 5:][big > 0.98] = 20.0
    raw[:, 5:][(big > 0.5) & (big < 0.503)] = 1e4
    label = torch.zeros(B, 6, Sy, Sx, device="cuda")
    pick = r(B, Sy, Sx)
    label[:, 0] = torch.where(pick < 1 / 3, torch.where(pick < 0.04, 0.5, torch.where(pick < 0.08, 2.0, 1.0)), 0.0)
    lo, ext = r(B, 2, Sy, Sx) * 0.7, r(B, 2, Sy, Sx) * 0.29 + 0.01
    label[:, 1:3], label[:, 3:5] = lo, lo + ext
    label[:, 5] = torch.randint(0, C, (B, Sy, Sx), generator=gen, device="cuda").float()
    return raw, label, torch.randn(B, P, Sy, Sx, generator=gen, device="cuda")


if __name__ == "__main__":
    protos = H.parse_header()
    LIBS[:] = [H.bind(os.path.abspath(p), protos) for p in sys.argv[1:3]]
    assert len(LIBS) == 2 and LIBS[0]._handle != LIBS[1]._handle, "two different library files"
    for i, g in enumerate(L.groups()):
        pred, label, _ = L.pack(g, fill=None if i <= 1 else "cycle")
        loss(g.name, dev(pred), dev(label), g.w)
    rb = L.raw_batch()
    gen = torch.Generator(device="cuda").manual_seed(7)
    gout = torch.randn(*rb.raw.shape, generator=gen, device="cuda")
    raw_level("raw_batch", dev(rb.raw), dev(rb.label), gout, rb.cxs.cuda().contiguous(), rb.cys.cuda().contiguous(), L.ANCHORS, rb.w)
    for Sy, Sx in (L.GRID, (9, 31)):
        cxs, cys = (t.cuda().contiguous() for t in O.make_grids(Sx, Sy))
        for P in (6, 7, 12, 16, 17, 69):
            raw, label, gout = random_case(gen, 3, P, Sy, Sx)
            raw_level("random", raw, label, gout, cxs, cys, L.ANCHORS, L.DEFAULT_W if P != 12 else (0.25, 2.0, 3.0, 0.1))
            if P <= 16:
                for Cin in (16, 128):
                    head(gen, 3, Cin, P, Sy, Sx, cxs, cys, L.ANCHORS)
    print(f"identical: {CALLS[0]} calls of each library, {WORDS[0]} words compared, 0 differ")
