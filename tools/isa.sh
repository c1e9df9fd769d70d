#!/bin/bash
# Device assembly of one render kernel, for register / spill / instruction probes
# (seconds, not the full library's minutes).  The library it would link is never
# built: the other kernels are not instantiated (render.hip ZRT_ISA_KERNEL).
# usage: bash tools/isa.sh <out.s> ["MODE, PRNG, STATS, StackT[, LEAN]"] [extra hipcc flags...]
#   default kernel: the general C4 lockstep FAST kernel "3, 0, false, uint16_t";
#   "3, 0, false, uint16_t, true" is the lean kernel C4 runs (render.hip struct Lean);
#   a launch-size knob's variant: add e.g. -DZRT_STACK_ROWS_LOCK=12 -DZRT_SYNC_SAMPLES=2 -DZRT_PAXIS_LOG2M=8
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=$1; K=${2:-"3, 0, false, uint16_t"}; shift; [ $# -gt 0 ] && shift
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wno-unused-function \
  --offload-arch=gfx950 -munsafe-fp-atomics -fno-slp-vectorize --cuda-device-only -S \
  "-DZRT_ISA_KERNEL=$K" "$@" -o $OUT $R/zraytrace_amd/csrc/render.hip 2>&1 | grep -v 'unused-command-line' 
python $R/tools/kernel_regs.py $OUT
