#!/usr/bin/env bash
# Prints, per (source file of csrc/, extra flags, device | host), the sha256 of the assembly hipcc emits for it with the flags
# csrc/build.sh compiles that file with, less the __hip_cuid_ lines (the only ones that differ between two compiles of one source).
# Two trees that print the same lines build the same code: the proof that a refactor of the kernels changed nothing.
#   tools/isa_digest.sh [CSRC_DIR] [FILE.hip ...]      (default: this tree's csrc, all files and the kept switches off their defaults)
set -euo pipefail
cd "${1:-$(dirname "$0")/../dn-splatter_amd/csrc}"; shift || true
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
COMMON=$(sed -n 's/^COMMON="\(.*\)"$/\1/p' build.sh)
digest() {   # FILE.hip [extra flags]: the file's own flags are read off its compile line in build.sh
    local f=$1 own side sum; shift
    own=$(sed -n "s/^\$HIPCC \$COMMON *\(.*\)-c $f .*/\1/p" build.sh)
    for side in device host; do
        sum=$($HIPCC $COMMON $own "$@" --cuda-$side-only -S "$f" -o - | grep -v __hip_cuid_ | sha256sum | cut -d' ' -f1)
        echo "$f [$*] $side $sum"
    done
}
if [ $# -gt 0 ]; then for f in "$@"; do digest "$f"; done; exit; fi
for f in *.hip; do digest "$f"; done
digest raster_bwd.hip -DDNS_BWD_TIMELINE
digest raster_bwd.hip -DDNS_BWD_WAVES_PER_EU=3
digest raster_fwd.hip -DDNS_FWD_PACKED=1
digest raster_fwd.hip -DDNS_FWD_X_VALU=4 -DDNS_FWD_X_LDS=1
digest raster_fwd.hip -DDNS_FWD_WAVES_PER_EU=8
