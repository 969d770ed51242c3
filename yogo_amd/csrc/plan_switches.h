// Every plan switch of the library, one out-of-line accessor each (plan_switches.hip).  A launcher asks here which kernel family or
// loop variant a launch may take; no other file of csrc/ knows whether a switch is a constant or a variable.
//   product (libyogo_hip.so):              each accessor returns a constant -- no mutable plan state, no setter
//   -DYOGO_TEST_HOOKS (libyogo_hip_hooks.so, tests/ and tools/ only) and -DYOGO_DIAG: the eight below are variables with yogo_hook_* setters
//   -DYOGO_DIAG (libyogo_hip_diag.so):     the tiled planner's four are variables too (yogo_diag_conv_bf16_* setters)
#pragma once

// launch_conv_bf16 (conv_bf16.hip): the kernel families that take the launches they are eligible for
bool plan_ws();          // the persistent wavefront-specialised kernels (conv_bf16_ws.hip, conv_bf16_ws3.hip); off: the tiled conv_bf16_kernel
// conv_bf16_ws16_kernel (16x16x32 MFMAs) for the plain-epilogue launches: 0 = never (conv_bf16_ws_kernel<0> takes them), 1 = the product's
// rule (the launches WITHOUT a bias: the data gradients), 2 = every eligible launch (bias too: its tests and A/B runs)
int plan_ws16_mode();
bool plan_direct();      // the direct (weights-resident, no staging) stride-2 data gradients (conv_bf16_direct.hip)
bool plan_staged();      // the independent-wavefront kernel of the thin forward-type layers (conv_bf16_staged.hip)
bool plan_staged_pair(); // layers 1 + 2 forward in one launch (conv_bf16_staged_pair.hip); off: the two launches of yogo_conv2d_fwd_bf16_signs
bool plan_head();        // the 1x1 head's forward with the weights in registers (conv_bf16_head.hip)
// layer 0: two pixels per lane where the output width is even
bool plan_first_bn_wgrad_pairs();   // conv_first.hip, the sign-map sweep
bool plan_first_mfma_pairs();       // conv_first_mfma.hip
// bf_plan_tiled (conv_bf16.hip): loop variants of the tiled kernel, switched in the diagnostic build only
bool plan_tiled_pp();      // off: the interleaved main loop in place of the ping-pong one
bool plan_tiled_ring();    // off: the two-buffer loop of the stride-2 data gradient in place of the four-buffer ring
bool plan_tiled_lean4();   // off: the generic step loop of the 4-wavefront tiles
bool plan_tiled_rowdma();  // off: the per-lane slot staging of the lean 4-wavefront tiles in place of the row-by-row one
