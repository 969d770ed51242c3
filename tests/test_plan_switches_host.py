"""The plan switches (yogo_amd/csrc/plan_switches.hip) have their setters in the test-hooks library and nowhere else, and the two libraries
run one planner: libyogo_hip_hooks.so is the product's objects with plan_switches.o alone compiled under -DYOGO_TEST_HOOKS.  No device."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_bf16_stats_shape.json")
# (name, default): the product's plan
HOOKS = (("yogo_hook_conv_bf16_persistent", 1), ("yogo_hook_conv_bf16_ws16", 1), ("yogo_hook_conv_bf16_direct", 1), ("yogo_hook_conv_bf16_staged", 1),
         ("yogo_hook_conv_bf16_head", 1), ("yogo_hook_conv_first_bn_wgrad_pairs", 1), ("yogo_hook_conv_first_mfma_pairs", 1))


def hooks_path():
    from yogo_amd import _hip

    return os.path.join(os.path.dirname(_hip.LIB_PATH), "libyogo_hip_hooks.so")


@pytest.mark.parametrize("name", [n for n, _ in HOOKS])
def test_product_library_exports_no_hook(name):
    from yogo_amd import _hip

    L = ctypes.CDLL(_hip.LIB_PATH)
    with pytest.raises(AttributeError):
        getattr(L, name)


@pytest.mark.parametrize("name,default", HOOKS)
def test_hooks_library_has_each_setter(name, default):
    fn = getattr(ctypes.CDLL(hooks_path()), name)
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int]
    assert fn(default) == 0


def test_hooks_library_runs_the_recorded_planner_without_a_gpu():
    """the subset of test_conv_plan_host.py::test_stats_shape_needs_no_gpu, asked of the hooks library in a process that sees no device"""
    with open(FIXTURE) as f:
        want = [w for w in json.load(f) if w[0] == 3 and w[3:5] in ([97, 129], [3, 5])]
    assert want
    code = ("import ctypes, json, sys\n"
            "L = ctypes.CDLL(sys.argv[1])\n"
            "out = []\n"
            "for s in json.loads(sys.argv[2]):\n"
            "    r, m = ctypes.c_int(0), ctypes.c_int(0)\n"
            "    rc = L.yogo_conv2d_fwd_bf16_stats_shape(*s, ctypes.byref(r), ctypes.byref(m))\n"
            "    out.append([*s, r.value if rc == 0 else -1, m.value])\n"
            "print(json.dumps(out))\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    res = subprocess.run([sys.executable, "-c", code, hooks_path(), json.dumps([w[:7] for w in want])], env=env, capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr
    assert json.loads(res.stdout.strip().splitlines()[-1]) == want
