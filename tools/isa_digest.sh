#!/usr/bin/env bash
# Prints, per (source file of csrc/, extra flags, device | host), the sha256 of the assembly hipcc emits for it with the flags
# csrc/build.sh compiles that file with, less the __hip_cuid_ lines (the only ones that differ between two compiles of one source).
# Two trees that print the same lines build the same code: the proof that a refactor of the kernels changed nothing.
#   tools/isa_digest.sh [CSRC_DIR] [FILE.hip ...]      (default: this tree's csrc, all files and the kept switches off their defaults)
#   tools/isa_digest.sh --kernels FILE.hip [CSRC_DIR]  one line per function of the file's device code: sha256 of its assembly, its name
set -euo pipefail
KERNELS=; if [ "${1:-}" = --kernels ]; then KERNELS=$2; shift 2; fi
cd "${1:-$(dirname "$0")/../dn-splatter_amd/csrc}"; shift || true
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
COMMON=$(sed -n 's/^COMMON="\(.*\)"$/\1/p' build.sh)
own_flags() { sed -n "s/^\$HIPCC \$COMMON *\(.*\)-c $1 .*/\1/p" build.sh; }   # the file's own flags, off its compile line in build.sh
digest() {   # FILE.hip [extra flags]
    local f=$1 side sum; shift
    for side in device host; do
        sum=$($HIPCC $COMMON $(own_flags "$f") "$@" --cuda-$side-only -S "$f" -o - | grep -v __hip_cuid_ | sha256sum | cut -d' ' -f1)
        echo "$f [$*] $side $sum"
    done
}
if [ -n "$KERNELS" ]; then
    # the text from a function's label to its .Lfunc_end.  LLVM numbers the functions of a file and puts the number into every local label
    # (.LBB12_3, .Lfunc_end12, "Header=BB12_3"): taken out, with the padding in front of a label's comment that its length decides, so that a
    # function's digest does not depend on which functions precede it
    $HIPCC $COMMON $(own_flags "$KERNELS") --cuda-device-only -S "$KERNELS" -o - | sed -E 's/(BB|\.Lfunc_end)[0-9]+/\1/g; s/ +;/ ;/' |
        awk '/^\t\.type\t.*@function/ { want = 1 }
             want && /^[^.\t ][^ \t]*:/ { name = substr($1, 1, length($1) - 1); want = 0 }
             name { body = body $0 "\n" }
             name && /^\.Lfunc_end:/ { cmd = "sha256sum | cut -c1-65 | tr -d \"\\n\""; printf "%s", body | cmd; close(cmd); print name; fflush(); name = body = "" }' |
        c++filt | sort -k2
    exit
fi
if [ $# -gt 0 ]; then for f in "$@"; do digest "$f"; done; exit; fi
for f in *.hip; do digest "$f"; done
digest raster_bwd.hip -DDNS_BWD_TIMELINE
digest raster_bwd.hip -DDNS_BWD_WAVES_PER_EU=3
digest raster_fwd.hip -DDNS_FWD_PACKED=1
digest raster_fwd.hip -DDNS_FWD_X_VALU=4 -DDNS_FWD_X_LDS=1
digest raster_fwd.hip -DDNS_FWD_WAVES_PER_EU=8
