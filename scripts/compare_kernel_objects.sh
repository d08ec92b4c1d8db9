#!/bin/sh
# Are the kernels of two builds the same?  sha256 of the four kernel objects, and of what the gfx950 code objects inside
# them hold: .text (the instructions), .rodata (the kernel descriptors) and .note (the kernels' metadata: registers, LDS,
# scratch, arguments).  Two trees at different paths never agree in more than that: hipcc names one symbol of every
# code object __hip_cuid_<hash of the source file's path>, so the symbol and hash tables are ordered differently, and the
# host part names the path itself.
#   scripts/compare_kernel_objects.sh <parent csrc/build> <new csrc/build>
set -eu
LLVM=${LLVM:-/opt/rocm/lib/llvm/bin}
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
rc=0
for k in nsk_kernels nsk_setup_kernels nsk_assembly_kernels nsk_amg_kernels; do
  for side in parent new; do
    [ $side = parent ] && dir=$1 || dir=$2
    o=$dir/$k.hip.o
    objcopy -O binary --only-section=.hip_fatbin "$o" "$tmp/$k.$side.fatbin"
    "$LLVM/clang-offload-bundler" --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input="$tmp/$k.$side.fatbin" --output="$tmp/$k.$side.co"
    line="$k.hip.o $side: object $(sha256sum < "$o" | cut -c1-64) gfx950 code object $(sha256sum < "$tmp/$k.$side.co" | cut -c1-64)"
    for sec in .text .rodata .note; do
      "$LLVM/llvm-objcopy" -O binary --only-section=$sec "$tmp/$k.$side.co" "$tmp/$k.$side$sec"
      line="$line $sec $(sha256sum < "$tmp/$k.$side$sec" | cut -c1-64) ($(wc -c < "$tmp/$k.$side$sec") bytes)"
    done
    echo "$line"
  done
  for sec in .text .rodata .note; do
    [ -s "$tmp/$k.new$sec" ] && cmp -s "$tmp/$k.parent$sec" "$tmp/$k.new$sec" || { echo "$k: $sec DIFFERS or is empty"; rc=1; }
  done
  [ $rc = 0 ] && echo "$k: .text, .rodata and .note of the gfx950 code objects are identical"
done
exit $rc
