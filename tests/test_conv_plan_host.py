"""The tiled bf16 convolution planner's answers (yogo_amd/csrc/conv_bf16.hip: bf_plan_tiled) without a device:
yogo_conv2d_fwd_bf16_stats_shape runs the planner and returns (rows, mpad) of the BatchNorm partial-sum buffer -- rows is the batch
times the workgroups per image of the plan's tiling, so a changed band count or tile changes it.  The answers over a sweep of channel
counts, kernel sizes, strides, batches and image sizes (through every band boundary) are held to tests/golden/conv_bf16_stats_shape.json.

    python tests/test_conv_plan_host.py --record     rewrites the fixture from the library of the tree the file lies in
"""
import itertools
import json
import os
import subprocess
import sys

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_bf16_stats_shape.json")
CHANNELS = (16, 32, 64, 128, 12, 7)
KS_STRIDE = ((1, 1), (3, 1), (3, 2))   # a 1x1 convolution has stride 1
BATCHES = (1, 3)
# 1x1 and 3x5, widths on both sides of the band boundaries (31 | 32 | 33, 64 | 65, 129), then the planes of base_model at 772x1032
SIZES = ((1, 1), (3, 5), (7, 31), (7, 32), (7, 33), (9, 64), (9, 65), (5, 129), (97, 129), (193, 258), (386, 516))


def sweep():
    for (ks, s), B, Cin, Cout, (H, W) in itertools.product(KS_STRIDE, BATCHES, CHANNELS, CHANNELS, SIZES):
        yield B, Cin, Cout, H, W, ks, s


def answers():
    """[[B, Cin, Cout, H, W, ks, stride, rows, mpad], ...]; a shape the planner refuses: rows = -1 and the error text for mpad"""
    from yogo_amd import _hip

    out = []
    for shape in sweep():
        try:
            rows, mpad = _hip.query_ints("yogo_conv2d_fwd_bf16_stats_shape", 2, *shape)
        except RuntimeError as e:
            rows, mpad = -1, str(e)
        out.append([*shape, rows, mpad])
    return out


def test_stats_shape_answers_match_the_recorded_table():
    with open(FIXTURE) as f:
        want = json.load(f)
    got = answers()
    assert len(got) == len(want) == len(KS_STRIDE) * len(BATCHES) * len(CHANNELS) ** 2 * len(SIZES)
    diff = [(g, w) for g, w in zip(got, want) if g != w]
    assert not diff, (len(diff), "answers differ from the recorded table; the first (got, recorded):", diff[:5])


@pytest.mark.parametrize("shape", [(2, 16, 32, 20, 22, 5, 1), (2, 16, 32, 20, 22, 1, 2), (2, 16, 32, 20, 22, 3, 3), (2, 0, 32, 20, 22, 3, 1),
                                   (2, 16, 32, 0, 22, 3, 1), (-1, 16, 32, 20, 22, 3, 1)])
def test_unsupported_shape_keeps_its_error_text(shape):
    from yogo_amd import _hip

    with pytest.raises(RuntimeError) as e:
        _hip.query_ints("yogo_conv2d_fwd_bf16_stats_shape", 2, *shape)
    assert str(e.value) == "yogo_conv2d_fwd_bf16_stats_shape failed (code 1): conv_bf16: unsupported shape"


def test_stats_shape_needs_no_gpu():
    """in a process that sees no device at all (and never loads torch), the query gives the recorded answers"""
    from yogo_amd import _hip

    with open(FIXTURE) as f:
        want = [w for w in json.load(f) if w[0] == 3 and w[3:5] in ([97, 129], [3, 5])]
    code = ("import ctypes, json, sys\n"
            "L = ctypes.CDLL(sys.argv[1])\n"
            "out = []\n"
            "for s in json.loads(sys.argv[2]):\n"
            "    r, m = ctypes.c_int(0), ctypes.c_int(0)\n"
            "    rc = L.yogo_conv2d_fwd_bf16_stats_shape(*s, ctypes.byref(r), ctypes.byref(m))\n"
            "    out.append([*s, r.value if rc == 0 else -1, m.value])\n"
            "print(json.dumps(out))\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    res = subprocess.run([sys.executable, "-c", code, _hip.LIB_PATH, json.dumps([w[:7] for w in want])], env=env, capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    assert json.loads(res.stdout.strip().splitlines()[-1]) == want


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_conv_plan_host.py --record")
    table = answers()
    with open(FIXTURE, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(row) for row in table) + "\n]\n")
    print("recorded", len(table), "answers ->", FIXTURE, "; refused:", sum(1 for t in table if t[7] < 0))
