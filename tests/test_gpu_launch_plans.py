"""Which kernel takes which bf16 convolution launch, and with what plan: one launch per case through the PRODUCT library (the one
without plan switches), its single launch-log line -- kernel name with template arguments | plan text -- compared with
tests/golden/launch_plans.json.

The family tests (test_gpu_ws.py) compare "hook off" with "default"; a gate of launch_conv_bf16 (yogo_amd/csrc/conv_bf16.hip) that
silently rejects turns that into tiled against tiled and still passes.  Here every gate has a case it must accept, and every reason a
gate rejects for has a case that must fall through to the tiled conv_bf16_kernel; `kernel` / `marks` below state that expectation from
the dispatcher's rules, the fixture holds the whole line.  Tensor contents do not matter (zeros): only the dispatch is under test.

    python tests/test_gpu_launch_plans.py --record     rewrites the fixture from the library of the tree the file lies in
"""
import json
import os
import re
import sys

import pytest

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plans.json")
B = 2
NONE, LEAKY, SILU = 0, 1, 2

# (id, op, Cin, Cout, H, W, ks, stride, act, options, kernel the line must start with, marks)
#   op "fwd": yogo_conv2d_fwd_bf16[_signs | _pre] of a Cin -> Cout convolution on an H x W input; options: bias, scale (per-image channel
#     factors), signs (writes the sign map), pre (second, pre-activation output), stats (BatchNorm partial sums), f32 (fp32 NCHW output)
#   op "dgrad": yogo_conv2d_dgrad_bf16[_signs] of the SAME forward convolution (the GEMM contracts over Cout and produces Cin channels);
#     options: scale, signs (reads the sign map of the reference), ref (reads the reference tensor itself, REF = 1)
#   marks (tiled kernel only): pp / lepi = the PP / LEPI template argument is true (PP: the ping-pong loop of the 8-wavefront tiles, the
#     lean step loop of the 4-wavefront ones); ring = the 128-row stride-2 data gradient with the fixed 2 + 3 slot
#     layout of its four-buffer ring; rows = the row-staged tiling (a non-zero row pitch)
CASES = [
    # ---- every gate accepts its smallest shape
    ("ws_bias", "fwd", 128, 128, 13, 17, 3, 1, NONE, {"bias"}, "conv_bf16_ws_kernel<0>", ()),
    ("ws16_no_bias", "dgrad", 128, 128, 13, 17, 3, 1, NONE, set(), "conv_bf16_ws16_kernel<false>", ()),
    ("ws_leaky_signs_scale", "fwd", 64, 128, 13, 17, 3, 1, LEAKY, {"bias", "signs", "scale"}, "conv_bf16_ws_kernel<7>", ()),
    ("ws3", "fwd", 64, 128, 37, 41, 3, 2, LEAKY, {"bias"}, "conv_bf16_ws3_kernel<1>", ()),
    ("head_1x1", "fwd", 128, 12, 5, 7, 1, 1, NONE, {"bias", "f32"}, "conv_bf16_1x1_f32_kernel<8, false>", ()),
    ("staged_stride1", "fwd", 16, 32, 20, 22, 3, 1, LEAKY, {"bias", "signs", "scale"}, "conv_bf16_staged_kernel<1, 1, 1, true, 4, 8, true>", ()),
    ("staged_stride2", "fwd", 32, 64, 20, 22, 3, 2, LEAKY, {"bias", "signs", "scale"}, "conv_bf16_staged_kernel<2, 2, 2, true, 8, 1, false>", ()),
    ("direct_s2d_m32_signs", "dgrad", 32, 64, 20, 22, 3, 2, NONE, {"signs", "scale"}, "conv_bf16_s2d_direct_kernel<4, 1, true>", ()),
    ("direct_s2d_m128", "dgrad", 128, 128, 20, 22, 3, 2, NONE, {"scale"}, "conv_bf16_s2d_direct_kernel<8, 2, false>", ()),
    # ---- every reason a gate rejects for: the tiled kernel
    ("tiled_pre", "fwd", 128, 128, 13, 17, 3, 1, SILU, {"bias", "pre"}, "conv_bf16_kernel<4, 2, 8, false, 10, false, 0,", ()),
    ("tiled_stats", "fwd", 128, 128, 13, 17, 3, 1, NONE, {"bias", "stats"}, "conv_bf16_kernel<4, 2, 8, false, 10, false, 0,", ()),
    ("tiled_f32_3x3", "fwd", 128, 128, 13, 17, 3, 1, NONE, {"bias", "f32"}, "conv_bf16_kernel<4, 2, 8, false, 10, true, 0,", ()),
    ("tiled_act_ref", "dgrad", 128, 128, 13, 17, 3, 1, NONE, {"ref"}, "conv_bf16_kernel<4, 2, 8, false, 10, false, 1,", ()),
    ("tiled_thin_stride1_signs_dgrad", "dgrad", 16, 32, 20, 22, 3, 1, NONE, {"signs"}, "conv_bf16_kernel<1, 4, 4, false, 16, false, 2,", ()),
    ("tiled_128_to_64_dgrad", "dgrad", 64, 128, 13, 17, 3, 1, NONE, set(), "conv_bf16_kernel<2, 2, 4, false, 16, false, 0,", ()),
    ("tiled_s2d_m64", "dgrad", 64, 128, 20, 22, 3, 2, NONE, set(), "conv_bf16_kernel<2, 1, 4, true, 16, false, 0,", ("lepi",)),
    ("tiled_stride2_fwd_stats", "fwd", 128, 128, 37, 41, 3, 2, NONE, {"bias", "stats"}, "conv_bf16_kernel<4, 1, 8, false, 10, false, 0,", ()),
    ("tiled_head_1x1_bf16_out", "fwd", 128, 12, 5, 7, 1, 1, NONE, {"bias"}, "conv_bf16_kernel<1, 4, 4, false, 16, false, 0,", ()),
    # ---- the plans of the tiled kernel: ring, lean 4-wavefront loop (both epilogues), row-staged tiling, ping-pong loop, the wide 64-row tile
    ("tiled_ring", "dgrad", 128, 64, 37, 41, 3, 2, NONE, set(), "conv_bf16_kernel<4, 1, 8, true, 10, false, 0,", ("ring",)),
    ("tiled_lean4_signs_dgrad", "dgrad", 32, 16, 20, 22, 3, 1, NONE, {"signs", "scale"}, "conv_bf16_kernel<1, 4, 4, false, 16, false, 2,", ("pp", "lepi")),
    ("tiled_lean4_general", "dgrad", 32, 16, 20, 22, 3, 1, NONE, {"ref"}, "conv_bf16_kernel<1, 4, 4, false, 16, false, 1,", ("pp",)),
    ("tiled_rows_lean_fwd", "fwd", 16, 48, 33, 65, 3, 1, LEAKY, {"bias"}, "conv_bf16_kernel<2, 2, 4, false, 16, false, 0,", ("rows", "pp", "lepi")),
    ("tiled_ping_pong", "fwd", 128, 128, 97, 129, 3, 1, NONE, {"bias", "stats"}, "conv_bf16_kernel<4, 2, 8, false, 10, false, 0,", ("pp",)),
    ("tiled_wide64", "fwd", 64, 64, 97, 129, 3, 1, LEAKY, {"bias"}, "conv_bf16_kernel<2, 4, 8, false, 10, false, 0,", ("pp",)),
]
IDS = [c[0] for c in CASES]


def _blocks(c):
    return ((c + 15) // 16) * 2


def launch_line(case):
    """allocates the smallest tensors the entry point needs, calls it once with the launch log on, returns the one line it logged"""
    import torch

    from yogo_amd import _hip as Hh

    _, op, Cin, Cout, H, W, ks, stride, act, opts, _, _ = case
    pad = 1 if ks == 3 else 0
    OH, OW = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    st = Hh.stream_ptr()

    def z8(C, h, w):
        return torch.zeros(B, _blocks(C), h, w, 8, dtype=torch.bfloat16, device="cuda")

    def signs_of(C, h, w):
        return torch.zeros(Hh.query_size("yogo_bf16_signs_bytes", B, C, h, w), dtype=torch.uint8, device="cuda")

    def packed_of(mode):
        return torch.zeros(Hh.query_size("yogo_conv_bf16_packed_bytes", Cin, Cout, ks, mode), dtype=torch.uint8, device="cuda")

    x_in, x_out = z8(Cin, H, W), z8(Cout, OH, OW)   # the forward convolution's input and output
    keep = []   # (the operands stay referenced until the launch has run)
    Hh.launch_log(True)
    try:
        if op == "fwd":
            packed = packed_of(0)
            bias = torch.zeros(Cout, device="cuda") if "bias" in opts else None
            scale = torch.ones(B, Cout, device="cuda") if "scale" in opts else None
            if "signs" in opts:
                sg = signs_of(Cout, OH, OW)
                Hh.call("yogo_conv2d_fwd_bf16_signs", x_in, packed, bias, x_out, sg, scale, B, Cin, Cout, H, W, ks, stride, act, st)
            elif "pre" in opts:
                sg = z8(Cout, OH, OW)
                Hh.call("yogo_conv2d_fwd_bf16_pre", x_in, packed, bias, x_out, sg, scale, B, Cin, Cout, H, W, ks, stride, act, st)
            else:
                sg = None
                stats = None
                if "stats" in opts:
                    rows, mpad = Hh.query_ints("yogo_conv2d_fwd_bf16_stats_shape", 2, B, Cin, Cout, H, W, ks, stride)
                    stats = torch.zeros(rows, mpad, 2, device="cuda")
                f32 = torch.zeros(B, Cout, OH, OW, device="cuda") if "f32" in opts else None
                Hh.call("yogo_conv2d_fwd_bf16", x_in, packed, bias, None if f32 is not None else x_out, f32, scale, stats, B, Cin, Cout, H, W, ks, stride, act, st)
                keep += [stats, f32]
            keep += [packed, bias, scale, sg]
        else:
            packed = packed_of(2 if (stride == 2 and ks == 3) else 1)
            scale = torch.ones(B, Cin, device="cuda") if "scale" in opts else None
            if "signs" in opts:
                sg = signs_of(Cin, H, W)
                Hh.call("yogo_conv2d_dgrad_bf16_signs", x_out, packed, x_in, sg, scale, B, Cin, Cout, H, W, ks, stride, st)
            else:
                sg = z8(Cin, H, W) if "ref" in opts else None
                Hh.call("yogo_conv2d_dgrad_bf16", x_out, packed, x_in, sg, LEAKY if sg is not None else NONE, scale, B, Cin, Cout, H, W, ks, stride, st)
            keep += [packed, scale, sg]
        torch.cuda.synchronize()
        log = Hh.read_launch_log()
    finally:
        Hh.launch_log(False)
    assert len(log) == 1, (case[0], "one entry point call, one kernel launch", log)
    return log[0]


def check_expectation(case, line):
    """the part of a line that the dispatcher's rules fix, whatever the fixture says"""
    name, kernel, marks = case[0], case[10], case[11]
    assert line.startswith(kernel), (name, "must run", kernel, "ran", line)
    if kernel.startswith("conv_bf16_kernel<"):
        targs = [a.strip() for a in line.split("|")[0].strip()[len("conv_bf16_kernel<"):-1].split(",")]
        assert len(targs) == 9, line
        got = set()
        if targs[7] == "true":
            got.add("pp")
        if targs[8] == "true":
            got.add("lepi")
        if targs[0] == "4" and targs[3] == "true" and " slots=2+3 " in line and " CKb=2 " in line:
            got.add("ring")
        if re.search(r" rowpitch=[1-9]", line):
            got.add("rows")
        assert got == set(marks), (name, "plan marks", sorted(got), "expected", sorted(marks), line)


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_lists_exactly_the_cases(golden):
    assert sorted(golden) == sorted(IDS)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_launch_runs_the_recorded_kernel_and_plan(case, golden):
    line = launch_line(case)
    print(line)
    check_expectation(case, line)
    assert line == golden[case[0]], (case[0], "the launch differs from the recorded one", line, golden[case[0]])


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_gpu_launch_plans.py --record")
    lines = {}
    for c in CASES:
        lines[c[0]] = launch_line(c)
        print(c[0], "::", lines[c[0]], flush=True)
    with open(FIXTURE, "w") as f:
        json.dump(lines, f, indent=1, sort_keys=True)
        f.write("\n")
    for c in CASES:
        check_expectation(c, lines[c[0]])
    print("recorded", len(lines), "launches ->", FIXTURE)
