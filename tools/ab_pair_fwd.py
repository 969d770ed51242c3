"""Kernel-level A/B of layers 1 + 2 forward (experiments; not part of the product): the one-launch pair (yogo_conv2d_fwd_bf16_signs_pair,
conv_bf16_staged_pair_kernel) against the two launches of yogo_conv2d_fwd_bf16_signs on the same tensors at the training step's shape
(bf16, 16 -> 32 -> 64 at 386x516, bias + LeakyReLU + channel masks + sign maps), alternating in one process on one device.
    python tools/ab_pair_fwd.py [TAGS] [rounds] [B] [reps]
TAGS: comma list of library variants whose pair kernel is timed ("base" = the product; another tiling is a variant build, e.g.
`bash yogo_amd/csrc/build.sh variant pair_r2 conv_bf16_staged_pair -DBF_PAIR_R2=2` -> tag pair_r2).  The two launches always run on the
product library.  Prints every round's times, the medians, and whether the outputs are the same bytes."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ab_variants import load
from yogo_amd import _hip as H

C0, C1, C2, IH, IW = 16, 32, 64, 386, 516


def timed(f, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


if __name__ == "__main__":
    tags = (sys.argv[1] if len(sys.argv) > 1 else "base").split(",")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    B = int(sys.argv[3]) if len(sys.argv) > 3 else 128
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 10
    libs = {t: load(t) for t in dict.fromkeys(["base"] + tags)}
    H._lib = libs["base"]
    st = H.stream_ptr()
    OH, OW = (IH - 1) // 2 + 1, (IW - 1) // 2 + 1
    x8 = torch.randn(B, 2, IH, IW, 8, device="cuda").to(torch.bfloat16)
    w1, w2 = torch.randn(C1, C0, 3, 3, device="cuda") * 0.08, torch.randn(C2, C1, 3, 3, device="cuda") * 0.06
    b1, b2 = torch.randn(C1, device="cuda"), torch.randn(C2, device="cuda")
    m1, m2 = (torch.rand(B, C1, device="cuda") > 0.05).float() / 0.95, (torch.rand(B, C2, device="cuda") > 0.1).float() / 0.9
    pk = []
    for w, ci, co in ((w1, C0, C1), (w2, C1, C2)):
        p = torch.empty(H.query_size("yogo_conv_bf16_packed_bytes", ci, co, 3, 0), dtype=torch.uint8, device="cuda")
        H.call("yogo_conv_bf16_pack", w, None, p, ci, co, 3, 0, st)
        pk.append(p)

    def outputs():
        return (torch.empty(B, 4, IH, IW, 8, dtype=torch.bfloat16, device="cuda"), torch.empty(H.query_size("yogo_bf16_signs_bytes", B, C1, IH, IW), dtype=torch.uint8, device="cuda"),
                torch.empty(B, 8, OH, OW, 8, dtype=torch.bfloat16, device="cuda"), torch.empty(H.query_size("yogo_bf16_signs_bytes", B, C2, OH, OW), dtype=torch.uint8, device="cuda"))

    ref, got = outputs(), outputs()

    def two():
        H._lib = libs["base"]
        H.call("yogo_conv2d_fwd_bf16_signs", x8, pk[0], b1, ref[0], ref[1], m1, B, C0, C1, IH, IW, 3, 1, 1, st)
        H.call("yogo_conv2d_fwd_bf16_signs", ref[0], pk[1], b2, ref[2], ref[3], m2, B, C1, C2, IH, IW, 3, 2, 1, st)

    def pair(tag):
        def f():
            H._lib = libs[tag]
            H.call("yogo_conv2d_fwd_bf16_signs_pair", x8, pk[0], b1, got[0], got[1], m1, pk[1], b2, got[2], got[3], m2, B, C0, C1, C2, IH, IW, 1, st)
        return f

    arms = [("two launches", two)] + [(f"pair[{t}]", pair(t)) for t in tags]
    two()
    for tag, (name, f) in zip(tags, arms[1:]):
        for t in got:
            t.view(torch.uint8).fill_(0x5A)
        H._lib = libs[tag]   # (every library has a launch log of its own)
        H.launch_log(True)
        f()
        torch.cuda.synchronize()
        H.launch_log(False)
        print(name, "|", "; ".join(H.read_launch_log()))
        print(name, "same bytes as the two launches:", all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(ref, got)), flush=True)
    res = {name: [] for name, _ in arms}
    for r in range(rounds + 1):   # round 0 warms the clocks and is dropped
        for name, f in arms:
            ms = timed(f, reps)
            if r > 0:
                res[name].append(ms)
    for name, _ in arms:
        v = sorted(res[name])
        print(f"{name:16s} ms per call: " + " ".join(f"{x:.3f}" for x in res[name]) + f"   median {v[len(v) // 2]:.3f}  min {v[0]:.3f}  max {v[-1]:.3f}", flush=True)
