#!/usr/bin/env bash
# Build libyogo_hip.so for gfx950 (MI355X).  hipcc cross-compiles without a GPU.
#   bash build.sh        -> yogo_amd/lib/libyogo_hip.so       (the product: no diagnostic code is compiled in)
#                           yogo_amd/lib/libyogo_hip_hooks.so (tests/ and tools/ only: the SAME objects, but for plan_switches.o compiled
#                           under -DYOGO_TEST_HOOKS -- the yogo_hook_* setters; every kernel is compiled once)
#   bash build.sh diag   -> yogo_amd/lib/libyogo_hip_diag.so  (-DYOGO_DIAG: ablation bits + s_memtime phase stamps in
#                           conv_bf16_kernel, driven by yogo_diag_conv_bf16(); tools/ only, never loaded by the package)
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
OUT="$HERE/../lib"
OBJ="$HERE/obj"
LIBNAME="libyogo_hip.so"
DEFS=()
if [[ "${1:-}" == "diag" ]]; then OBJ="$HERE/obj_diag"; LIBNAME="libyogo_hip_diag.so"; DEFS=(-DYOGO_DIAG -DYOGO_DIAG_PHASES); fi
# diag-coarse: start / loop / epilogue / end stamps only (the per-phase sums of the ping-pong loop cost it scalar registers)
if [[ "${1:-}" == "diag-coarse" ]]; then OBJ="$HERE/obj_diagc"; LIBNAME="libyogo_hip_diag.so"; DEFS=(-DYOGO_DIAG); fi
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
# The wavefront-specialised kernels keep their accumulators in AGPRs that only their asm statements name (cdna_hip_programming.md 5.7
# item 4): outside those statements the compiler must not spill, use scratch, move through v_accvgpr_*, or give an AGPR to any
# operand (gfx950 lets the allocator use AV-class registers for DS / VMEM data).  audit_ws FILE.s STRICT(1|0)
audit_ws() {
  local S="$1" strict="$2" bad scr spill
  [[ -f "$S" ]] || return 0
  bad=$(awk '/;;#ASMSTART/{a=1} /;;#ASMEND/{a=0} { if (!a && $0 !~ /^[ \t]*[;.]/ && ($0 ~ /v_accvgpr_/ || $0 ~ /[ ,\[]a[0-9]+([ ,\]:]|$)/ || $0 ~ /[ ,]a\[[0-9]+:[0-9]+\]/)) n++ } END { print n+0 }' "$S")
  scr=$(awk '/;;#ASMSTART/{a=1} /;;#ASMEND/{a=0} { if (!a && $0 !~ /^[ \t]*[;.]/ && $0 ~ /scratch_/) n++ } END { print n+0 }' "$S")
  spill=$(grep -E "\.vgpr_spill_count:|\.private_segment_fixed_size:" "$S" | awk '{ s += $2 } END { print s+0 }')
  if [[ "$bad" != 0 || "$scr" != 0 || "$spill" != 0 ]]; then
    echo "$(basename "$S") audit: $bad compiler accumulator / AGPR-operand instructions outside the asm statements, $scr scratch instructions, spill / scratch total $spill" >&2
    [[ "$strict" == 1 && ( "$bad" != 0 || "$WS_SPILL_OK" != 1 ) ]] && { echo "audit FAILED" >&2; return 1; }
  else
    echo "$(basename "$S" -hip-amdgcn-amd-amdhsa-gfx950.s) audit ok (no compiler v_accvgpr_* / AGPR operands / scratch outside the asm statements, no spills)"
  fi
  return 0
}
WS_FILES="conv_bf16_ws conv_bf16_ws3 conv_bf16_ws16"
# extra_flags BASE: the per-file flags, in `extra`
extra_flags() {
  extra=()
  case "$1" in
    nms|match|decode_loss|conv_bf16_head|draw_boxes) extra=(-ffp-contract=off) ;;
    conv_bf16_ws|conv_bf16_ws3|conv_bf16_ws16) extra=(-save-temps=obj -fno-slp-vectorize) ;;   # the assembly is audited below (asm-owned accumulator registers); no SLP packing: v_pk_*_f32 beside MFMAs costs more than it saves
    conv_bf16_tiled) extra=(-fno-slp-vectorize) ;;   # the same for the tiled kernels: the merged-epilogue forward instantiations -5 ... -9.5 % in the same-box A/B; the training step's launches take the lean epilogue with its explicit packed math and do not change
    conv_bf16_pack|conv_first_infer_bf16) extra=(-fno-slp-vectorize) ;;   # (these kernels were compiled beside the tiled one, with its flags: kept)
  esac
}
WS_SPILL_OK="${WS_SPILL_OK:-0}"   # (experiments: WS_SPILL_OK=1 turns a spill into a warning)
# variant TAG FILE [-DNAME=VALUE ...]: libyogo_hip_TAG.so = the product objects with FILE.hip recompiled under the given macros
# (in-process A/B of a compile-time choice: tools/ab_variants.py loads several such libraries side by side).  Build the product first.
# A choice of plan (BF_WS16_MODE, BF_NO_ROWDMA) is a macro of plan_switches.hip: variant TAG plan_switches -D... compiles no kernel.
if [[ "${1:-}" == "variant" ]]; then
  TAG="$2"; FILE="$3"; shift 3
  VOBJ="$HERE/obj_var"; mkdir -p "$VOBJ" "$OUT"
  extra_flags "$FILE"
  "$HIPCC" -O3 --offload-arch=gfx950 -fPIC -std=c++17 -fhip-fp32-correctly-rounded-divide-sqrt -Wall -Wno-unused-function -I"$HERE" -I"$HERE/../../include" "$@" "${extra[@]}" -c "$HERE/$FILE.hip" -o "$VOBJ/${TAG}_$FILE.o"
  audit_ws "$VOBJ/${TAG}_$FILE-hip-amdgcn-amd-amdhsa-gfx950.s" 0   # (ablation variants are timings, not results: a warning)
  objs=(); for f in "$HERE"/*.hip; do b="$(basename "$f" .hip)"; [[ "$b" == "$FILE" ]] || objs+=("$HERE/obj/$b.o"); done
  "$HIPCC" --offload-arch=gfx950 -shared -fPIC "${objs[@]}" "$VOBJ/${TAG}_$FILE.o" -ldl -o "$OUT/libyogo_hip_$TAG.so"
  echo "built $OUT/libyogo_hip_$TAG.so"
  exit 0
fi
HOBJ="$HERE/obj_hooks"
mkdir -p "$OUT" "$OBJ" "$HOBJ"
# (EXTRA_DEFS="-DNAME=VALUE ...": extra macros for an experiment, e.g. a diagnostic build of an ablation)
COMMON=(-O3 --offload-arch=gfx950 -fPIC -std=c++17 -fhip-fp32-correctly-rounded-divide-sqrt -Wall -Wno-unused-function -I"$HERE" -I"$HERE/../../include" "${DEFS[@]}" ${EXTRA_DEFS:-})
# compile_if_stale FILE.hip OBJECT [flags]: in the background, when the object is older than the file, a header or an .inc the file includes
pids=()
compile_if_stale() {
  local f="$1" o="$2" dep stale=0; shift 2
  for dep in "$f" "$HERE"/*.h "$HERE/../../include"/*.h $(grep -oE '[A-Za-z0-9_]+\.inc"' "$f" | sort -u | sed "s|^|$HERE/|; s|\"\$||"); do
    [[ -f "$dep" && ( ! -f "$o" || "$dep" -nt "$o" ) ]] && stale=1
  done
  if [[ "$stale" == 1 ]]; then
    "$HIPCC" "${COMMON[@]}" "$@" -c "$f" -o "$o" &
    pids+=($!)
  fi
}
for f in "$HERE"/*.hip; do
  base="$(basename "$f" .hip)"
  extra_flags "$base"
  compile_if_stale "$f" "$OBJ/$base.o" "${extra[@]}"
done
# the one object of the test-hooks library that is not the product's (see the end of this script)
[[ "${#DEFS[@]}" == 0 ]] && compile_if_stale "$HERE/plan_switches.hip" "$HOBJ/plan_switches.o" -DYOGO_TEST_HOOKS
for p in "${pids[@]:-}"; do [[ -n "$p" ]] && wait "$p"; done
# (the diagnostic build's stamps cost registers: its numbers are timings, not results -- a warning there, an error in the product)
for wsf in $WS_FILES; do
  if ! audit_ws "$OBJ/$wsf-hip-amdgcn-amd-amdhsa-gfx950.s" "$([[ "${#DEFS[@]}" == 0 ]] && echo 1 || echo 0)"; then rm -f "$OBJ/$wsf.o"; exit 1; fi
  # ... and no compiler instruction reads a register whose LDS read an asm statement left in flight (tools/audit_inflight.py)
  if [[ "${#DEFS[@]}" == 0 && -f "$OBJ/$wsf-hip-amdgcn-amd-amdhsa-gfx950.s" ]]; then
    if ! python3 "$HERE/../../tools/audit_inflight.py" "$OBJ/$wsf-hip-amdgcn-amd-amdhsa-gfx950.s"; then rm -f "$OBJ/$wsf.o"; exit 1; fi
  fi
done
objs=(); for f in "$HERE"/*.hip; do objs+=("$OBJ/$(basename "$f" .hip).o"); done
"$HIPCC" --offload-arch=gfx950 -shared -fPIC "${objs[@]}" -ldl -o "$OUT/$LIBNAME"
echo "built $OUT/$LIBNAME"
# libyogo_hip_hooks.so: the product's objects, every kernel among them, with plan_switches.o replaced by the one compiled under
# -DYOGO_TEST_HOOKS (the switches become variables with yogo_hook_* setters: tests/ and tools/ only -- the package never loads it)
if [[ "${#DEFS[@]}" == 0 ]]; then
  hobjs=(); for o in "${objs[@]}"; do [[ "$o" == "$OBJ/plan_switches.o" ]] && hobjs+=("$HOBJ/plan_switches.o") || hobjs+=("$o"); done
  "$HIPCC" --offload-arch=gfx950 -shared -fPIC "${hobjs[@]}" -ldl -o "$OUT/libyogo_hip_hooks.so"
  echo "built $OUT/libyogo_hip_hooks.so"
fi
