"""wgrad_bf16_kernel on the production layer shapes, product library: LAYERS and bench() (tools/ab_variants.py alternates compile-time
variants over them), and the A/B against another BUILD of the library:
    python tools/bench_wgrad_bf16.py [B] [which]              one timing per layer
    python tools/bench_wgrad_bf16.py ab TAG [rounds] [B]      yogo_amd/lib/libyogo_hip_TAG.so (e.g. a parent commit's build copied to
        libyogo_hip_parent.so) against the product library: dw / db of every layer and of the long-walk shapes compared for EQUAL BITS on
        random bf16 inputs, then the layers alternating between the two in one process (first round dropped): the product's median must lie
        inside TAG's own min-max."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from yogo_amd import _hip as H

LAYERS = {"l1": (16, 32, 386, 516, 3, 1), "l2": (32, 64, 386, 516, 3, 2), "l3": (64, 128, 193, 258, 3, 1),
          "l4": (128, 128, 193, 258, 3, 2), "l5": (128, 128, 97, 129, 3, 1), "l7": (128, 12, 97, 129, 1, 1)}
# one shape per loop of the kernel with many units per workgroup (tests/test_gpu_conv_bf16_exact.py: WGRAD_WALKS), for the bit comparison
WALKS = [(2, 128, 128, 1027, 7, 3, 1), (4, 128, 128, 521, 33, 3, 1), (3, 128, 64, 1027, 7, 3, 1), (3, 96, 128, 1027, 7, 3, 2), (2, 128, 64, 1027, 17, 3, 1),
         (5, 32, 64, 2041, 3, 3, 1), (5, 64, 32, 1034, 33, 3, 2), (5, 16, 16, 515, 65, 3, 1), (5, 16, 16, 2065, 49, 3, 1), (5, 16, 32, 2041, 3, 3, 2),
         (5, 16, 64, 1033, 49, 3, 1), (5, 32, 32, 2041, 3, 3, 2), (5, 32, 32, 1034, 97, 3, 2)]


def blocks(c):
    return ((c + 15) // 16) * 2


def operands(B, Cin, Cout, IH, IW, k, s, seed=None):
    pad = 1 if k == 3 else 0
    OH, OW = (IH + 2 * pad - k) // s + 1, (IW + 2 * pad - k) // s + 1
    g = None if seed is None else torch.Generator(device="cuda").manual_seed(seed)
    x8 = torch.randn(B, blocks(Cin), IH, IW, 8, device="cuda", generator=g).to(torch.bfloat16)
    g8 = torch.randn(B, blocks(Cout), OH, OW, 8, device="cuda", generator=g).to(torch.bfloat16)
    return x8, g8, OH, OW


def bench(name, B, Cin, Cout, IH, IW, k, s, reps=10):
    st = H.stream_ptr()
    x8, g8, OH, OW = operands(B, Cin, Cout, IH, IW, k, s)
    ws = torch.empty(H.query_size("yogo_conv2d_wgrad_bf16_workspace_bytes", B, Cin, Cout, IH, IW, k, s) // 4, device="cuda")
    dw, db = torch.empty(Cout, Cin, k, k, device="cuda"), torch.empty(Cout, device="cuda")
    f = lambda: H.call("yogo_conv2d_wgrad_bf16", x8, g8, dw, db, ws, B, Cin, Cout, IH, IW, k, s, 1.0, st)
    for _ in range(2):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    print(f"{name} wgrad B={B} {Cin}->{Cout} {IH}x{IW} k{k} s{s}: {ms:.3f} ms  {2.0 * B * Cout * Cin * k * k * OH * OW / ms / 1e9:.1f} TF", flush=True)
    return ms


def ab(tag, rounds, B):
    import contextlib
    import io
    from ab_variants import load

    libs = {t: load(t) for t in (tag, "base")}
    bad = 0
    cases = [(n, (4,) + v) for n, v in LAYERS.items()] + [("walk", c) for c in WALKS]
    for name, (Bc, Cin, Cout, IH, IW, k, s) in cases:
        x8, g8, _, _ = operands(Bc, Cin, Cout, IH, IW, k, s, seed=1)
        res = {}
        for t, L in libs.items():
            H._lib = L
            ws = torch.full((H.query_size("yogo_conv2d_wgrad_bf16_workspace_bytes", Bc, Cin, Cout, IH, IW, k, s) // 4,), float("nan"), device="cuda")
            dw, db = torch.full((Cout, Cin, k, k), float("nan"), device="cuda"), torch.full((Cout,), float("nan"), device="cuda")
            H.call("yogo_conv2d_wgrad_bf16", x8, g8, dw, db, ws, Bc, Cin, Cout, IH, IW, k, s, 0.0, H.stream_ptr())
            torch.cuda.synchronize()
            res[t] = (dw.view(torch.int32).cpu(), db.view(torch.int32).cpu())
        nd = [int((res[tag][i] != res["base"][i]).sum()) for i in (0, 1)]
        bad += any(nd)
        print(f"bits  {name:5s} B={Bc} {Cin}->{Cout} {IH}x{IW} k{k} s{s}: dw {'same' if not nd[0] else 'DIFFER %d' % nd[0]}, db {'same' if not nd[1] else 'DIFFER %d' % nd[1]}"
              f"  (finite: {bool(torch.isfinite(res['base'][0].view(torch.float32)).all())})", flush=True)
    times = {(w, t): [] for w in LAYERS for t in libs}
    for r in range(rounds + 1):   # round 0 warms the clocks and is dropped
        for w in LAYERS:
            for t, L in libs.items():
                H._lib = L
                with contextlib.redirect_stdout(io.StringIO()):
                    ms = bench(w, B, *LAYERS[w])
                if r > 0:
                    times[(w, t)].append(ms)
    slow = 0
    print(f"# speed: ms per call at B={B}, {rounds} rounds of 10 calls (first round dropped); base's median must lie inside {tag}'s min-max")
    for w in LAYERS:
        p, v = times[(w, tag)], times[(w, "base")]
        med = sorted(v)[len(v) // 2]
        where = "inside" if min(p) <= med <= max(p) else ("below" if med < min(p) else "ABOVE")
        slow += where == "ABOVE"
        print(f"speed {w} {tag:7s} median {sorted(p)[len(p) // 2]:.3f} min {min(p):.3f} max {max(p):.3f} | base median {med:.3f} min {min(v):.3f} max {max(v):.3f}  {where}")
    return 1 if bad or slow else 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "ab":
        sys.exit(ab(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 15, int(sys.argv[4]) if len(sys.argv) > 4 else 128))
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    for w in (sys.argv[2].split(",") if len(sys.argv) > 2 else list(LAYERS)):
        bench(w, B, *LAYERS[w])
