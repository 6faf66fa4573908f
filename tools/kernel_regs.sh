#!/bin/bash
# registers / scratch / LDS / occupancy / code length of the device kernels whose (demangled) name matches a pattern,
# built with the flags of csrc/Makefile.  "sgprs" is the listing's `; NumSgprs:` line, or `; TotalNumSgprs:` (with the
# VCC and flat-scratch pairs) where the compiler prints that instead; "lds" is the static `; LDSByteSize:`.
#   tools/kernel_regs.sh [pattern]        e.g. tools/kernel_regs.sh 'kw_rows|kx_strided<512'
# MVN_KERNEL_LISTING=file keeps the listing there (default /tmp/mvn_kernels.s); MVN_KERNEL_CSRC=dir reads another tree's
# csrc, so that two commits can be compared kernel by kernel (diff of the two outputs).
cd "${MVN_KERNEL_CSRC:-$(dirname "$0")/../libmultiviewnative_amd/csrc}" || exit 1
S="${MVN_KERNEL_LISTING:-/tmp/mvn_kernels.s}"
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -fvisibility=hidden -fvisibility-inlines-hidden \
  -fno-fast-math -fno-slp-vectorize $MVN_EXTRA_FLAGS -S --cuda-device-only -o "$S" mvn_kernels.hip 2>/dev/null
awk '/^[_A-Za-z0-9]+:/ {name=$1; sub(":", "", name)}
     /; codeLenInByte =/ {c=$4} /; (Total)?NumSgprs:/ {sg=$3}
     /; NumVgprs:/ {v=$3} /; ScratchSize:/ {s=$3} /; LDSByteSize:/ {l=$3}
     /; Occupancy:/ {print name, "vgprs", v, "sgprs", sg, "scratch", s, "lds", l, "occupancy", $3, "code", c}' "$S" \
  | c++filt | grep -E "${1:-.}" | sort -u
