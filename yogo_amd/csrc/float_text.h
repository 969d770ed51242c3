// Decimal text of a float32 exactly as Python prints it -- repr(float(numpy.float32(v))) -- in one definition for the host (plain C++,
// no HIP include: tests/float_text_main.cpp) and for gfx950 (yogo_amd/csrc/pred_text.hip, which writes the prediction files of
// `yogo infer --save-preds --device-outputs` on the device; the host formatter is prediction_rows_to_text,
// yogo_amd/utils/prediction_formatting.py, the f-string of yogo/infer.py:52-55).
//
// Digits: the float32 is widened exactly to a double c * 2^q and printed as the SHORTEST decimal that converts back to that double,
// the one closest to the value where several are shortest -- what float.__repr__ (David Gay's mode 0), Ryu and Grisu-with-fallback
// give.  The algorithm is Schubfach (R. Giulietti, "The Schubfach way to render doubles", 2020): with k = floor(log10(2^q)) and
// g ~ 10^-k as a 128-bit integer (kPow10, rounded up), the value and the two ends of its rounding interval are scaled to
// integers + sticky bit ("round to odd") with two 64 x 64 -> 128-bit products each; the interval then holds at most two candidates
// at scale 10^(k+1) and, failing that, two at 10^k, and comparisons of small integers pick the result.  A float32 with mantissa
// field 0 widens to a double with mantissa field 0: the interval below such a value is half as wide as the one above (the next
// double down sits in the finer binade), k is then floor(log10(3/4 * 2^q)) and the lower end c - 1/4; ties and interval ends follow
// round-half-even (an even c owns its interval's ends).
// Notation (float_repr_style "short"): with the digits d1 d2 ... dn and the decimal point after `decpt` of them, fixed notation for
// -4 < decpt <= 16 (integers end in ".0"), otherwise d1[.d2...dn]e+XX with a sign and at least two exponent digits.  "inf", "-inf",
// "nan" for every NaN, "0.0", "-0.0".  The longest text has 23 characters ("-1.1754942106924411e-38").
//
// The table is emitted and verified by tools/gen_float_text_tables.py (Python big integers), which also derives its range: a widened
// float32 is zero or a NORMAL double with q = -201 .. 75.
#pragma once

#if defined(__HIPCC__)
#define YOGO_FT_HD __host__ __device__ inline
#else
#define YOGO_FT_HD inline
#endif
// the device copy of the table lives in constant memory; the host compilation (of hipcc too) sees a plain array
#if defined(__HIP_DEVICE_COMPILE__)
#define YOGO_FT_TABLE __constant__ static const
#else
#define YOGO_FT_TABLE static const
#endif

namespace float_text {

constexpr int kMaxF32Chars = 24;   // no value needs more (the longest has 23)
constexpr int kMaxU32Chars = 10;

// --- generated table: begin ---
constexpr int kPow10Min = -22;   // 10^j for j = kPow10Min .. kPow10Max
constexpr int kPow10Max = 61;
YOGO_FT_TABLE unsigned long long kPow10[kPow10Max - kPow10Min + 1][2] = {   // {high, low} words of g(j)
    {0xF1C90080BAF72CB1ull, 0x5324C68B12DD6339ull},   // -22
    {0x971DA05074DA7BEEull, 0xD3F6FC16EBCA5E04ull},   // -21
    {0xBCE5086492111AEAull, 0x88F4BB1CA6BCF585ull},   // -20
    {0xEC1E4A7DB69561A5ull, 0x2B31E9E3D06C32E6ull},   // -19
    {0x9392EE8E921D5D07ull, 0x3AFF322E62439FD0ull},   // -18
    {0xB877AA3236A4B449ull, 0x09BEFEB9FAD487C3ull},   // -17
    {0xE69594BEC44DE15Bull, 0x4C2EBE687989A9B4ull},   // -16
    {0x901D7CF73AB0ACD9ull, 0x0F9D37014BF60A11ull},   // -15
    {0xB424DC35095CD80Full, 0x538484C19EF38C95ull},   // -14
    {0xE12E13424BB40E13ull, 0x2865A5F206B06FBAull},   // -13
    {0x8CBCCC096F5088CBull, 0xF93F87B7442E45D4ull},   // -12
    {0xAFEBFF0BCB24AAFEull, 0xF78F69A51539D749ull},   // -11
    {0xDBE6FECEBDEDD5BEull, 0xB573440E5A884D1Cull},   // -10
    {0x89705F4136B4A597ull, 0x31680A88F8953031ull},   // -9
    {0xABCC77118461CEFCull, 0xFDC20D2B36BA7C3Eull},   // -8
    {0xD6BF94D5E57A42BCull, 0x3D32907604691B4Dull},   // -7
    {0x8637BD05AF6C69B5ull, 0xA63F9A49C2C1B110ull},   // -6
    {0xA7C5AC471B478423ull, 0x0FCF80DC33721D54ull},   // -5
    {0xD1B71758E219652Bull, 0xD3C36113404EA4A9ull},   // -4
    {0x83126E978D4FDF3Bull, 0x645A1CAC083126EAull},   // -3
    {0xA3D70A3D70A3D70Aull, 0x3D70A3D70A3D70A4ull},   // -2
    {0xCCCCCCCCCCCCCCCCull, 0xCCCCCCCCCCCCCCCDull},   // -1
    {0x8000000000000000ull, 0x0000000000000000ull},   // 0
    {0xA000000000000000ull, 0x0000000000000000ull},   // 1
    {0xC800000000000000ull, 0x0000000000000000ull},   // 2
    {0xFA00000000000000ull, 0x0000000000000000ull},   // 3
    {0x9C40000000000000ull, 0x0000000000000000ull},   // 4
    {0xC350000000000000ull, 0x0000000000000000ull},   // 5
    {0xF424000000000000ull, 0x0000000000000000ull},   // 6
    {0x9896800000000000ull, 0x0000000000000000ull},   // 7
    {0xBEBC200000000000ull, 0x0000000000000000ull},   // 8
    {0xEE6B280000000000ull, 0x0000000000000000ull},   // 9
    {0x9502F90000000000ull, 0x0000000000000000ull},   // 10
    {0xBA43B74000000000ull, 0x0000000000000000ull},   // 11
    {0xE8D4A51000000000ull, 0x0000000000000000ull},   // 12
    {0x9184E72A00000000ull, 0x0000000000000000ull},   // 13
    {0xB5E620F480000000ull, 0x0000000000000000ull},   // 14
    {0xE35FA931A0000000ull, 0x0000000000000000ull},   // 15
    {0x8E1BC9BF04000000ull, 0x0000000000000000ull},   // 16
    {0xB1A2BC2EC5000000ull, 0x0000000000000000ull},   // 17
    {0xDE0B6B3A76400000ull, 0x0000000000000000ull},   // 18
    {0x8AC7230489E80000ull, 0x0000000000000000ull},   // 19
    {0xAD78EBC5AC620000ull, 0x0000000000000000ull},   // 20
    {0xD8D726B7177A8000ull, 0x0000000000000000ull},   // 21
    {0x878678326EAC9000ull, 0x0000000000000000ull},   // 22
    {0xA968163F0A57B400ull, 0x0000000000000000ull},   // 23
    {0xD3C21BCECCEDA100ull, 0x0000000000000000ull},   // 24
    {0x84595161401484A0ull, 0x0000000000000000ull},   // 25
    {0xA56FA5B99019A5C8ull, 0x0000000000000000ull},   // 26
    {0xCECB8F27F4200F3Aull, 0x0000000000000000ull},   // 27
    {0x813F3978F8940984ull, 0x4000000000000000ull},   // 28
    {0xA18F07D736B90BE5ull, 0x5000000000000000ull},   // 29
    {0xC9F2C9CD04674EDEull, 0xA400000000000000ull},   // 30
    {0xFC6F7C4045812296ull, 0x4D00000000000000ull},   // 31
    {0x9DC5ADA82B70B59Dull, 0xF020000000000000ull},   // 32
    {0xC5371912364CE305ull, 0x6C28000000000000ull},   // 33
    {0xF684DF56C3E01BC6ull, 0xC732000000000000ull},   // 34
    {0x9A130B963A6C115Cull, 0x3C7F400000000000ull},   // 35
    {0xC097CE7BC90715B3ull, 0x4B9F100000000000ull},   // 36
    {0xF0BDC21ABB48DB20ull, 0x1E86D40000000000ull},   // 37
    {0x96769950B50D88F4ull, 0x1314448000000000ull},   // 38
    {0xBC143FA4E250EB31ull, 0x17D955A000000000ull},   // 39
    {0xEB194F8E1AE525FDull, 0x5DCFAB0800000000ull},   // 40
    {0x92EFD1B8D0CF37BEull, 0x5AA1CAE500000000ull},   // 41
    {0xB7ABC627050305ADull, 0xF14A3D9E40000000ull},   // 42
    {0xE596B7B0C643C719ull, 0x6D9CCD05D0000000ull},   // 43
    {0x8F7E32CE7BEA5C6Full, 0xE4820023A2000000ull},   // 44
    {0xB35DBF821AE4F38Bull, 0xDDA2802C8A800000ull},   // 45
    {0xE0352F62A19E306Eull, 0xD50B2037AD200000ull},   // 46
    {0x8C213D9DA502DE45ull, 0x4526F422CC340000ull},   // 47
    {0xAF298D050E4395D6ull, 0x9670B12B7F410000ull},   // 48
    {0xDAF3F04651D47B4Cull, 0x3C0CDD765F114000ull},   // 49
    {0x88D8762BF324CD0Full, 0xA5880A69FB6AC800ull},   // 50
    {0xAB0E93B6EFEE0053ull, 0x8EEA0D047A457A00ull},   // 51
    {0xD5D238A4ABE98068ull, 0x72A4904598D6D880ull},   // 52
    {0x85A36366EB71F041ull, 0x47A6DA2B7F864750ull},   // 53
    {0xA70C3C40A64E6C51ull, 0x999090B65F67D924ull},   // 54
    {0xD0CF4B50CFE20765ull, 0xFFF4B4E3F741CF6Dull},   // 55
    {0x82818F1281ED449Full, 0xBFF8F10E7A8921A5ull},   // 56
    {0xA321F2D7226895C7ull, 0xAFF72D52192B6A0Eull},   // 57
    {0xCBEA6F8CEB02BB39ull, 0x9BF4F8A69F764491ull},   // 58
    {0xFEE50B7025C36A08ull, 0x02F236D04753D5B5ull},   // 59
    {0x9F4F2726179A2245ull, 0x01D762422C946591ull},   // 60
    {0xC722F0EF9D80AAD6ull, 0x424D3AD2B7B97EF6ull},   // 61
};
// --- generated table: end ---

// the one place where the host and the device build differ: a * b as (low word, high word)
YOGO_FT_HD unsigned long long mul_64x64(unsigned long long a, unsigned long long b, unsigned long long* hi) {
#if defined(__HIP_DEVICE_COMPILE__)
  *hi = __umul64hi(a, b);
  return a * b;
#else
  const unsigned __int128 p = (unsigned __int128)a * b;
  *hi = (unsigned long long)(p >> 64);
  return (unsigned long long)p;
#endif
}

// floor(log10(2^e)), floor(log10(3/4 * 2^e)) and floor(log2(10^e)) by multiply and shift; the generator checks each against the
// exact value over every argument the formatter can pass
YOGO_FT_HD int floor_log10_pow2(int e) { return (e * 1262611) >> 22; }
YOGO_FT_HD int floor_log10_three_quarters_pow2(int e) { return (e * 1262611 - 524031) >> 22; }
YOGO_FT_HD int floor_log2_pow10(int e) { return (e * 1741647) >> 19; }

// floor(g * cp / 2^128), its lowest bit or-ed with "the discarded part was not zero" (g = {high, low})
YOGO_FT_HD unsigned long long round_to_odd(unsigned long long g_hi, unsigned long long g_lo, unsigned long long cp) {
  unsigned long long x_hi, y_hi;
  (void)mul_64x64(g_lo, cp, &x_hi);
  const unsigned long long y_lo = mul_64x64(g_hi, cp, &y_hi);
  const unsigned long long z = y_lo + x_hi;
  y_hi += z < y_lo ? 1u : 0u;
  return y_hi | (z > 1 ? 1u : 0u);
}

// the shortest decimal dec * 10^k of the double c * 2^q (2^52 <= c < 2^53: a widened float32 is never a subnormal double);
// mantissa_zero: the double's mantissa field is 0 (the asymmetric interval).  dec < 10^17 and may end in zeros.
YOGO_FT_HD unsigned long long shortest_decimal(unsigned long long c, int q, bool mantissa_zero, int* k_out) {
  const bool even = (c & 1) == 0;
  const unsigned long long cbl = 4 * c - 2 + (mantissa_zero ? 1 : 0);
  const unsigned long long cb = 4 * c;
  const unsigned long long cbr = 4 * c + 2;
  const int k = mantissa_zero ? floor_log10_three_quarters_pow2(q) : floor_log10_pow2(q);
  const int h = q + floor_log2_pow10(-k) + 1;   // 1 .. 4
  int j = -k - kPow10Min;                       // (in range for every float32: the generator derives the table's range from q)
  j = j < 0 ? 0 : (j > kPow10Max - kPow10Min ? kPow10Max - kPow10Min : j);
  const unsigned long long g_hi = kPow10[j][0], g_lo = kPow10[j][1];
  const unsigned long long vbl = round_to_odd(g_hi, g_lo, cbl << h);
  const unsigned long long vb = round_to_odd(g_hi, g_lo, cb << h);
  const unsigned long long vbr = round_to_odd(g_hi, g_lo, cbr << h);
  const unsigned long long lower = vbl + (even ? 0 : 1);
  const unsigned long long upper = vbr - (even ? 0 : 1);
  const unsigned long long s = vb / 4;
  if (s >= 10) {   // one digit fewer, if exactly one of the two neighbours at 10^(k+1) lies in the interval
    const unsigned long long sp = s / 10;
    const bool up_inside = lower <= 40 * sp;
    const bool wp_inside = 40 * sp + 40 <= upper;
    if (up_inside != wp_inside) {
      *k_out = k + 1;
      return sp + (wp_inside ? 1 : 0);
    }
  }
  *k_out = k;
  const bool u_inside = lower <= 4 * s;
  const bool w_inside = 4 * s + 4 <= upper;
  if (u_inside != w_inside) return s + (w_inside ? 1 : 0);
  const unsigned long long mid = 4 * s + 2;   // both inside: the closer one, the even one on a tie
  const bool round_up = vb > mid || (vb == mid && (s & 1) != 0);
  return s + (round_up ? 1 : 0);
}

// Output goes through `Out::put(char)`: the callers count, store, or store with a bound.
struct CountOut {
  int n = 0;
  YOGO_FT_HD void put(char) { ++n; }
};
struct BufOut {
  char* p;
  YOGO_FT_HD void put(char c) { *p++ = c; }
};

template <class Out>
YOGO_FT_HD void put_u32(unsigned v, Out& o) {
  unsigned p = 1;
  while (v / p >= 10) p *= 10;
  for (; p; p /= 10) o.put((char)('0' + v / p % 10));
}

// the `ndig` low decimal digits of x, leading zeros included; `pos` counts the digits of the whole number put so far and a '.' goes
// in front of digit number `dot_at`
template <class Out>
YOGO_FT_HD void put_digits(unsigned x, int ndig, int& pos, int dot_at, Out& o) {
  unsigned p = 1;
  for (int i = 1; i < ndig; ++i) p *= 10;
  for (; p; p /= 10) {
    if (pos == dot_at) o.put('.');
    o.put((char)('0' + x / p % 10));
    ++pos;
  }
}

template <class Out>
YOGO_FT_HD void format_f32_repr_to(float v, Out& o) {
  unsigned bits;
  __builtin_memcpy(&bits, &v, sizeof bits);
  const unsigned e8 = (bits >> 23) & 0xFFu, m = bits & 0x7FFFFFu;
  if (e8 == 0xFFu && m != 0) {
    o.put('n'), o.put('a'), o.put('n');
    return;
  }
  if (bits >> 31) o.put('-');
  if (e8 == 0xFFu) {
    o.put('i'), o.put('n'), o.put('f');
    return;
  }
  if (e8 == 0 && m == 0) {
    o.put('0'), o.put('.'), o.put('0');
    return;
  }
  // the double c * 2^q
  unsigned long long c;
  int q;
  bool mantissa_zero;
  if (e8 != 0) {
    c = (unsigned long long)(0x800000u | m) << 29;
    q = (int)e8 - 127 - 52;
    mantissa_zero = m == 0;
  } else {   // a subnormal float32, m * 2^-149, is a normal double: bring its leading bit to bit 23
    const int s = __builtin_clz(m) - 8;
    const unsigned mm = m << s;
    c = (unsigned long long)mm << 29;
    q = -149 - s - 29;
    mantissa_zero = (mm & 0x7FFFFFu) == 0;
  }
  int k;
  unsigned long long dec = shortest_decimal(c, q, mantissa_zero, &k);
  while (dec % 10 == 0) {
    dec /= 10;
    ++k;
  }
  int nd = 1;
  for (unsigned long long p = 10; nd < 17 && dec >= p; p *= 10) ++nd;
  const int decpt = nd + k;
  const unsigned hi = (unsigned)(dec / 100000000ull), lo = (unsigned)(dec % 100000000ull);   // hi < 10^9
  const bool fixed = -4 < decpt && decpt <= 16;
  int dot_at = -1;
  if (fixed) {
    if (decpt <= 0) {
      o.put('0'), o.put('.');
      for (int i = decpt; i < 0; ++i) o.put('0');
    } else if (decpt < nd) {
      dot_at = decpt;
    }
  } else if (nd > 1) {
    dot_at = 1;
  }
  int pos = 0;
  if (nd > 8) {
    put_digits(hi, nd - 8, pos, dot_at, o);
    put_digits(lo, 8, pos, dot_at, o);
  } else {
    put_digits(lo, nd, pos, dot_at, o);
  }
  if (fixed) {
    if (decpt >= nd) {
      for (int i = nd; i < decpt; ++i) o.put('0');
      o.put('.'), o.put('0');
    }
  } else {
    const int ex = decpt - 1;
    o.put('e');
    o.put(ex < 0 ? '-' : '+');
    const unsigned ax = (unsigned)(ex < 0 ? -ex : ex);
    if (ax < 10) o.put('0');
    put_u32(ax, o);
  }
}

// writes the characters of repr(float(numpy.float32(v))) (at most kMaxF32Chars, no terminator) and returns their number
YOGO_FT_HD int format_f32_repr(float v, char* out) {
  BufOut o{out};
  format_f32_repr_to(v, o);
  return (int)(o.p - out);
}

// the decimal digits of v (at most kMaxU32Chars, no terminator); returns their number
YOGO_FT_HD int format_u32(unsigned v, char* out) {
  BufOut o{out};
  put_u32(v, o);
  return (int)(o.p - out);
}

}  // namespace float_text
