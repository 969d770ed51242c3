"""yogo_amd/csrc/float_text.h on the host: ``format_f32_repr`` against ``repr(float(numpy.float32(v)))``, byte for byte.

tests/float_text_main.cpp (its own ``main``) is compiled with the host C++ compiler under ``-fsanitize=address,undefined`` and run as a
child process: it reads uint32 bit patterns and prints one formatted value per line.  Nothing is loaded into Python.  The header is
the one the device kernels of yogo_amd/csrc/pred_text.hip compile, so what passes here is the arithmetic the GPU runs."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
from _float_text_cases import python_reprs, structured_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yogo_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("float_text") / "float_text_main"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-I", CSRC, os.path.join(ROOT, "tests", "float_text_main.cpp"), "-o", str(exe)], check=True)

    def run(bits: np.ndarray, *args: str):
        bits = np.ascontiguousarray(bits, dtype="<u4")
        p = subprocess.run([str(exe), *args], input=bits.tobytes(), capture_output=True)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        lines = p.stdout.decode("ascii").split("\n")
        assert lines[-1] == "" and len(lines) == len(bits) + 1
        return lines[:-1]

    return run


def _compare(driver, bits: np.ndarray) -> None:
    got, want = driver(bits), python_reprs(bits)
    bad = [(f"{int(b):#010x}", g, w) for b, g, w in zip(bits.tolist(), got, want) if g != w]
    assert not bad, f"{len(bad)} of {len(bits)} differ, first {bad[:5]}"
    assert max(map(len, got)) <= 24


def test_reference_self_check():
    """the reference is what the issue says it is on this interpreter: the switch points of the notation and the longest text"""
    f32 = lambda x: repr(float(np.float32(x)))   # noqa: E731
    assert f32(1e-4) == "9.999999747378752e-05" and f32(1e-5) == "9.999999747378752e-06"
    assert f32(9999999198822400.0) == "9999999198822400.0" and f32(1e16) == "1.0000000272564224e+16"
    assert f32(100.0) == "100.0" and repr(float(np.uint32(1).view(np.float32))) == "1.401298464324817e-45"
    assert sys.float_repr_style == "short"
    bits = np.random.default_rng(11).integers(0, 1 << 32, size=400_000, dtype=np.uint64).astype(np.uint32)
    assert max(map(len, python_reprs(bits))) == 23


def test_structured_values(driver):
    bits = structured_bits()
    want = python_reprs(bits)
    for s in ("9.999999747378752e-05", "9.999999747378752e-06", "9999999198822400.0", "1.0000000272564224e+16", "inf", "-inf", "nan", "0.0",
              "-0.0", "1.401298464324817e-45", "100.0", "1.0"):
        assert s in want, s   # both switch points of the notation are among the cases
    _compare(driver, bits)


def test_random_bit_patterns(driver):
    _compare(driver, np.random.default_rng(2024).integers(0, 1 << 32, size=2_000_000, dtype=np.uint64).astype(np.uint32))


def test_uniform_values(driver):
    _compare(driver, np.random.default_rng(7).random(500_000, dtype=np.float32).view(np.uint32))


def test_small_fractions(driver):
    """k / 129 and k / 97 for all k up to the denominator: box coordinates as a grid of cells produces them"""
    v = np.concatenate([np.arange(130, dtype=np.float32) / np.float32(129), np.arange(98, dtype=np.float32) / np.float32(97)])
    _compare(driver, v.view(np.uint32))


def test_format_u32(driver):
    vals = np.array([0, 1, 9, 10, 11, 99, 100, 999, 1000, 65535, 99999, 100000, 999999999, 1000000000, 2147483647, 2147483648, 4294967295],
                    dtype=np.uint32)
    assert driver(vals, "u") == [str(int(v)) for v in vals]


def test_table_equals_big_integer_values():
    """the table in float_text.h is what tools/gen_float_text_tables.py computes afresh (which also checks the header's
    multiply-and-shift logarithms against exact ones)"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_float_text_tables.py"), "--check"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "equals" in p.stdout
