// The table of plan switches (plan_switches.h).  Host code only: no kernel is compiled here, so the one object that differs between
// libyogo_hip.so and libyogo_hip_hooks.so holds no device code and every kernel of the two libraries is the same object file.
// The product has NO run-time plan switch (no mutable global state in the library besides the per-device launch state of
// api_common.hip): its accessors return constants.
#include "common.h"
#include "plan_switches.h"

// the two defaults an A/B variant build changes (a one-second compile):
//   bash build.sh variant nows16 plan_switches -DBF_WS16_MODE=0     bash build.sh variant slot plan_switches -DBF_NO_ROWDMA
#ifndef BF_WS16_MODE
#define BF_WS16_MODE 1
#endif
#ifdef BF_NO_ROWDMA
#define BF_ROWDMA_DEFAULT false
#else
#define BF_ROWDMA_DEFAULT true
#endif

// X(type, accessor, default, setter)
#define PLAN_HOOK_SWITCHES(X)                                                              \
  X(bool, plan_ws, true, yogo_hook_conv_bf16_persistent)                                   \
  X(int, plan_ws16_mode, BF_WS16_MODE, yogo_hook_conv_bf16_ws16)                           \
  X(bool, plan_direct, true, yogo_hook_conv_bf16_direct)                                   \
  X(bool, plan_staged, true, yogo_hook_conv_bf16_staged)                                   \
  X(bool, plan_staged_pair, true, yogo_hook_conv_bf16_staged_pair)                         \
  X(bool, plan_head, true, yogo_hook_conv_bf16_head)                                       \
  X(bool, plan_first_bn_wgrad_pairs, true, yogo_hook_conv_first_bn_wgrad_pairs)            \
  X(bool, plan_first_mfma_pairs, true, yogo_hook_conv_first_mfma_pairs)
#define PLAN_DIAG_SWITCHES(X)                                                              \
  X(bool, plan_tiled_pp, true, yogo_diag_conv_bf16_pp)                                     \
  X(bool, plan_tiled_ring, true, yogo_diag_conv_bf16_ring)                                 \
  X(bool, plan_tiled_lean4, true, yogo_diag_conv_bf16_lean4)                               \
  X(bool, plan_tiled_rowdma, BF_ROWDMA_DEFAULT, yogo_diag_conv_bf16_rowdma)

#define PLAN_CONSTANT(T, NAME, DEFAULT, SETTER) \
  T NAME() { return DEFAULT; }
// (a bool switch takes `on != 0`, the ws16 mode its argument: what the conversion to T does)
#define PLAN_VARIABLE(T, NAME, DEFAULT, SETTER)                                            \
  static T g_##NAME = DEFAULT;                                                             \
  T NAME() { return g_##NAME; }                                                            \
  extern "C" int SETTER(int v) { g_##NAME = static_cast<T>(v); return YOGO_OK; }

#if defined(YOGO_TEST_HOOKS) || defined(YOGO_DIAG)
PLAN_HOOK_SWITCHES(PLAN_VARIABLE)
#else
PLAN_HOOK_SWITCHES(PLAN_CONSTANT)
#endif
#ifdef YOGO_DIAG
PLAN_DIAG_SWITCHES(PLAN_VARIABLE)
#else
PLAN_DIAG_SWITCHES(PLAN_CONSTANT)
#endif
