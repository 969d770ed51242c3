// Walks wb_plan (yogo_amd/csrc/wgrad_bf16_plan.h) over the shape space on the host and prints which (instantiation, loop, steps per
// row, ring depth) exist at all, each with its count and its smallest example -- the table of profiles/wgrad_bf16_one_definition.log
// that the case lists of tests/test_gpu_conv_bf16_exact.py are held against.  No GPU, no HIP:
//   c++ -std=c++17 -O2 -fsanitize=address,undefined -I yogo_amd/csrc tools/wgrad_plan_sweep.cpp -o /tmp/wgrad_plan_sweep
//   /tmp/wgrad_plan_sweep                          the sweep: Cin, Cout around every multiple of 32 up to 512, every IW up to 1100
//                                                  (2200 at stride 2), OH on both sides of 64, k 1 and 3, both strides
//   /tmp/wgrad_plan_sweep B Cin Cout IH IW k s     the plan of one case, as the launch log words it
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "wgrad_bf16_plan.h"

static const char* loop_of(const WbPlan& pl) {
  if (pl.blk4) return "BLK4";
  if (pl.lean) return "LEAN";
  if (pl.R % pl.KS == 0 && pl.g.xcb == (pl.pack2 ? 2 : 4)) return pl.pack2 ? "LEAN2+PACK2" : "LEAN2";
  return pl.g.xcb == 2 ? "generic, 32-byte pixels" : "generic, 64-byte pixels";
}

static std::string inst_of(const WbPlan& pl) {
  char b[96];
  snprintf(b, sizeof(b), "<%d, %d, %d, %d, %d, %d, %d, %s, %s>", pl.MBW, pl.NBW, pl.KS, pl.T, pl.S, pl.R, pl.MPW, pl.pack2 ? "true" : "false",
           pl.blk4 ? "true" : "false");
  return b;
}

static std::string steps_of(const WbPlan& pl) {
  if (!pl.blk4) return std::to_string(pl.g.wce >> 4);
  const bool wide = pl.g.base_w + (pl.g.rem_w ? 1 : 0) > 32, all = pl.g.base_w > 32;
  return all ? "9" : (wide ? "8 and 9" : "8");
}

int main(int argc, char** argv) {
  if (argc == 8) {
    int v[7];
    for (int i = 0; i < 7; ++i) v[i] = atoi(argv[i + 1]);
    WbPlan pl;
    if (!wb_plan(v[0], v[1], v[2], v[3], v[4], v[5], v[6], &pl)) { printf("no LDS plan\n"); return 1; }
    printf("wgrad_bf16_kernel%s | %s, %s steps per row | R=%d wce=%d nchunk_w=%d base_w=%d rem_w=%d xw=%d xcb=%d slots=%d+%d depth=%d lds=%d units=%d units_per_split=%d grid=%ux%ux%u\n",
           inst_of(pl).c_str(), loop_of(pl), steps_of(pl).c_str(), pl.R, pl.g.wce, pl.g.nchunk_w, pl.g.base_w, pl.g.rem_w, pl.g.xw, pl.g.xcb, pl.g.ngs, pl.g.nxs,
           pl.g.depth, pl.lds_bytes, pl.g.units, pl.g.units_per_split, pl.grid[0], pl.grid[1], pl.grid[2]);
    return 0;
  }
  std::set<int> chans = {1, 8, 15, 16, 17, 24, 48};
  for (int k = 1; k <= 16; ++k)
    for (int d = -1; d <= 1; ++d)
      if (32 * k + d <= 512) chans.insert(32 * k + d);
  const int ihs[] = {1, 2, 3, 7, 63, 64, 65, 66, 127, 128, 129, 130, 400};
  struct Row { long count = 0; int ex[7] = {0, 0, 0, 0, 0, 0, 0}; long size = 1L << 62; };
  std::map<std::tuple<std::string, std::string, std::string, int>, Row> table;
  long plans = 0, none = 0, lean_wce64 = 0, depth_other = 0;
  for (int ks : {1, 3})
    for (int s : {1, 2}) {
      if (ks == 1 && s == 2) continue;   // (the entry points refuse it)
      for (int N : chans)
        for (int M : chans)
          for (int IH : ihs)
            for (int IW = 1; IW <= 1100 * s; ++IW) {
              WbPlan pl;
              ++plans;
              if (!wb_plan(1, N, M, IH, IW, ks, s, &pl)) { ++none; continue; }
              if (pl.lean && !pl.blk4 && pl.g.wce == 64) ++lean_wce64;
              if (pl.g.depth != 2 && pl.g.depth != 3) ++depth_other;
              Row& r = table[{inst_of(pl), loop_of(pl), steps_of(pl), pl.g.depth}];
              ++r.count;
              const long size = (long)(N + M) * IH * IW;
              if (size < r.size) { r.size = size; const int e[7] = {1, N, M, IH, IW, ks, s}; for (int i = 0; i < 7; ++i) r.ex[i] = e[i]; }
            }
    }
  printf("%ld shapes planned, %ld without a plan, %ld KS = 1 row-step plans with wce == 64 (4 steps per row), %ld plans with a ring depth other than 2 or 3\n",
         plans, none, lean_wce64, depth_other);
  printf("%-44s %-24s %-8s %-5s %10s  %s\n", "instantiation <MBW,NBW,KS,T,S,R,MPW,PACK2,BLK4>", "loop", "steps", "depth", "shapes", "smallest (B, Cin, Cout, IH, IW, k, s)");
  std::set<std::string> insts;
  for (const auto& [k, r] : table) {
    insts.insert(std::get<0>(k));
    printf("%-44s %-24s %-8s %-5d %10ld  (%d, %d, %d, %d, %d, %d, %d)\n", std::get<0>(k).c_str(), std::get<1>(k).c_str(), std::get<2>(k).c_str(), std::get<3>(k), r.count,
           r.ex[0], r.ex[1], r.ex[2], r.ex[3], r.ex[4], r.ex[5], r.ex[6]);
  }
  printf("%zu instantiations, %zu (instantiation, loop, steps per row, depth) rows\n", insts.size(), table.size());
  return 0;
}
