#!/bin/bash
# Is the device code what it was at <git-ref>?  Emits the device assembly of every
# .hip file at the ref and in the working tree with the Makefile's HIPFLAGS, drops
# the lines naming the compilation unit's id (__hip_cuid_<hash of the source>) and
# compares the rest byte for byte.  Prints each file's md5 pair; exits non-zero on
# a difference.  usage: bash tools/isa_same.sh <git-ref>   (minutes: render.hip twice)
R=$(cd "$(dirname "$0")/.." && pwd); REF=${1:?usage: isa_same.sh <git-ref>}
T=$(mktemp -d); trap 'rm -rf "$T"' EXIT
mkdir -p $T/ref/zraytrace_amd $T/out && git -C $R archive $REF zraytrace_amd/csrc include | tar -x -C $T/ref || exit 2
FLAGS=$(make -s -C $R/zraytrace_amd/csrc --eval 'print-hipflags: ; @echo $(HIPFLAGS)' print-hipflags) || exit 2
for f in render denoise temporal bvh_gpu; do
  for side in ref new; do
    [ $side == ref ] && S=$T/ref || S=$R
    ( /opt/rocm/bin/hipcc $FLAGS --cuda-device-only -S -o $T/out/$f.$side.raw $S/zraytrace_amd/csrc/$f.hip 2> $T/out/$f.$side.err \
        && grep -v __hip_cuid_ $T/out/$f.$side.raw > $T/out/$f.$side.s ) &
  done
done
wait; rc=0
for f in render denoise temporal bvh_gpu; do
  [ -s $T/out/$f.ref.s ] && [ -s $T/out/$f.new.s ] || { echo "$f.hip: did not compile"; cat $T/out/$f.*.err; rc=2; continue; }
  a=$(md5sum < $T/out/$f.ref.s | cut -c1-32); b=$(md5sum < $T/out/$f.new.s | cut -c1-32)
  if cmp -s $T/out/$f.ref.s $T/out/$f.new.s; then echo "$f.hip  $a  $b  same"; else echo "$f.hip  $a  $b  DIFFERENT"; rc=1; fi
done
exit $rc
