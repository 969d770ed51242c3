"""The powers-of-ten table of yogo_amd/csrc/float_text.h, from Python's big integers.

``format_f32_repr`` (float_text.h) prints a float32, widened exactly to a double, in shortest round-trip form (Schubfach: R. Giulietti,
"The Schubfach way to render doubles", 2020).  For a double c * 2^q it needs 10^j, j = -floor(log10(2^q)) (one less for the 3/4 rule of
the asymmetric interval), as a 128-bit integer

    g(j) = ceil(10^j / 2^r(j)),   r(j) = floor(log2(10^j)) - 127,   so that 2^127 <= g(j) < 2^128

(exact for 0 <= j <= 55, rounded up otherwise).  A widened float32 is a NORMAL double with 2^52 <= c < 2^53 and q = E - 52,
E = -149 .. 127 (the smallest subnormal float32 .. the largest binade), or zero; this file derives the range of j from that and emits
the rows between the two marker lines of the header.

  python tools/gen_float_text_tables.py            print the table rows
  python tools/gen_float_text_tables.py --check    compare the rows committed in float_text.h with freshly computed ones (exit 1 if not)
  python tools/gen_float_text_tables.py --write    rewrite the rows in float_text.h
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "yogo_amd", "csrc", "float_text.h")
BEGIN, END = "// --- generated table: begin ---", "// --- generated table: end ---"

Q_MIN, Q_MAX = -149 - 52, 127 - 52   # the binary exponents q of a widened float32 (c has 53 bits)


def _floor_log10(num: int, den: int) -> int:
    """floor(log10(num / den)) for positive integers"""
    k = 0
    while 10 ** (k + 1) * den <= num:
        k += 1
    while (num < den * 10 ** k) if k >= 0 else (num * 10 ** -k < den):
        k -= 1
    return k


def floor_log10_pow2_exact(e: int) -> int:
    return _floor_log10(1 << e, 1) if e >= 0 else _floor_log10(1, 1 << -e)


def floor_log10_three_quarters_pow2(e: int) -> int:
    return _floor_log10(3 << e, 4) if e >= 0 else _floor_log10(3, 4 << -e)


def floor_log2_pow10(j: int) -> int:
    """floor(log2(10^j)), exactly"""
    if j >= 0:
        return (10 ** j).bit_length() - 1
    # 10^j = 1 / 10^-j: floor(log2) = -ceil(log2(10^-j)); 10^-j is no power of two for j < 0
    return -(10 ** -j).bit_length()


def exponent_range():
    ks = [f(q) for q in range(Q_MIN, Q_MAX + 1) for f in (floor_log10_pow2_exact, floor_log10_three_quarters_pow2)]
    return -max(ks), -min(ks)   # j = -k


def g(j: int) -> int:
    r = floor_log2_pow10(j) - 127
    num, den = (10 ** j, 1) if j >= 0 else (1, 10 ** -j)
    if r >= 0:
        den <<= r
    else:
        num <<= -r
    v = -(-num // den)   # ceil
    assert 1 << 127 <= v < 1 << 128, j
    return v


def rows():
    j_min, j_max = exponent_range()
    out = [f"constexpr int kPow10Min = {j_min};   // 10^j for j = kPow10Min .. kPow10Max", f"constexpr int kPow10Max = {j_max};",
           "YOGO_FT_TABLE unsigned long long kPow10[kPow10Max - kPow10Min + 1][2] = {   // {high, low} words of g(j)"]
    for j in range(j_min, j_max + 1):
        v = g(j)
        out.append(f"    {{0x{v >> 64:016X}ull, 0x{v & (1 << 64) - 1:016X}ull}},   // {j}")
    out.append("};")
    return out


def check_integer_logs() -> None:
    """the shift-and-multiply logarithms float_text.h uses, against the exact ones, over everything it can be asked"""
    j_min, j_max = exponent_range()
    for q in range(Q_MIN - 4, Q_MAX + 5):
        assert (q * 1262611) >> 22 == floor_log10_pow2_exact(q), q
        assert (q * 1262611 - 524031) >> 22 == floor_log10_three_quarters_pow2(q), q
    for j in range(j_min - 2, j_max + 3):
        assert (j * 1741647) >> 19 == floor_log2_pow10(j), j


def main() -> int:
    check_integer_logs()
    fresh = rows()
    if "--write" in sys.argv or "--check" in sys.argv:
        src = open(HEADER).read()
        m = re.search(re.escape(BEGIN) + r"\n(.*?)\n" + re.escape(END), src, flags=re.S)
        if m is None:
            print(f"{HEADER}: the table markers are missing", file=sys.stderr)
            return 1
        if "--check" in sys.argv:
            same = m.group(1).split("\n") == fresh
            print("float_text.h: the committed table " + ("equals" if same else "DIFFERS from") + f" the freshly computed one ({len(fresh) - 4} rows)")
            return 0 if same else 1
        open(HEADER, "w").write(src[: m.start(1)] + "\n".join(fresh) + src[m.end(1):])
        print(f"wrote {len(fresh) - 4} rows to {HEADER}")
        return 0
    print("\n".join(fresh))
    return 0


if __name__ == "__main__":
    sys.exit(main())
