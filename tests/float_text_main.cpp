// Stand-alone driver of yogo_amd/csrc/float_text.h for tests/test_float_text_host.py: reads raw little-endian uint32 bit patterns from
// standard input and prints format_f32_repr of each, one per line.  Built with the host C++ compiler (no HIP), under
// -fsanitize=address,undefined; a leading "u" argument prints format_u32 of the values instead.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "float_text.h"

int main(int argc, char** argv) {
  const bool as_u32 = argc > 1 && std::strcmp(argv[1], "u") == 0;
  std::vector<uint32_t> in(1 << 16);
  std::vector<char> out;
  size_t got;
  while ((got = std::fread(in.data(), sizeof(uint32_t), in.size(), stdin)) > 0) {
    out.clear();
    for (size_t i = 0; i < got; ++i) {
      // exactly the documented room and a guard behind it: a longer text is caught by the sanitizer
      std::vector<char> text(as_u32 ? float_text::kMaxU32Chars : float_text::kMaxF32Chars);
      int n;
      if (as_u32) {
        n = float_text::format_u32(in[i], text.data());
      } else {
        float v;
        std::memcpy(&v, &in[i], sizeof v);
        n = float_text::format_f32_repr(v, text.data());
      }
      out.insert(out.end(), text.begin(), text.begin() + n);
      out.push_back('\n');
    }
    if (std::fwrite(out.data(), 1, out.size(), stdout) != out.size()) return 1;
  }
  return 0;
}
