#!/usr/bin/env bash
# Builds libdnsplat.so for gfx950 (MI355X) in-tree.  project.hip is compiled without FMA contraction
# (bit-exact radii / tile counts against the oracle); the compositing kernels keep contraction on.
# raster_bwd.hip: SLP vectorisation off — its packed-fp32 pairs are written out by hand, and the SLP pass
# re-packs the remaining scalar chains at the price of extra v_mov (measured +5 % cycles per step).
set -euo pipefail
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
COMMON="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function"
mkdir -p _obj
pids=()
$HIPCC $COMMON -ffp-contract=off -c project.hip    -o _obj/project.o & pids+=($!)
$HIPCC $COMMON                   -c binning.hip    -o _obj/binning.o & pids+=($!)
$HIPCC $COMMON                   -c raster_fwd.hip -o _obj/raster_fwd.o & pids+=($!)
$HIPCC $COMMON -fno-slp-vectorize -c raster_bwd.hip -o _obj/raster_bwd.o & pids+=($!)
$HIPCC $COMMON                   -c c_api.hip      -o _obj/c_api.o & pids+=($!)
$HIPCC $COMMON -ffp-contract=off -c postops.hip    -o _obj/postops.o & pids+=($!)
$HIPCC $COMMON                   -c losses.hip     -o _obj/losses.o & pids+=($!)
$HIPCC $COMMON -ffp-contract=off -c pearson.hip    -o _obj/pearson.o & pids+=($!)
$HIPCC $COMMON -ffp-contract=off -c ags.hip        -o _obj/ags.o & pids+=($!)
$HIPCC $COMMON -ffp-contract=off -c pointcloud.hip -o _obj/pointcloud.o & pids+=($!)
$HIPCC $COMMON -ffp-contract=off -c metrics.hip    -o _obj/metrics.o & pids+=($!)
$HIPCC $COMMON -ffp-contract=off -c density.hip    -o _obj/density.o & pids+=($!)
$HIPCC $COMMON -ffp-contract=off -c levelset.hip   -o _obj/levelset.o & pids+=($!)
$HIPCC $COMMON -ffp-contract=off -c marching.hip   -o _obj/marching.o & pids+=($!)
$HIPCC $COMMON -ffp-contract=off -c geometry.hip   -o _obj/geometry.o & pids+=($!)
$HIPCC $COMMON -ffp-contract=off -c meshcull.hip   -o _obj/meshcull.o & pids+=($!)
$HIPCC $COMMON -ffp-contract=off -c tsdf.hip       -o _obj/tsdf.o & pids+=($!)
$HIPCC $COMMON -ffp-contract=off -c meshclusters.hip -o _obj/meshclusters.o & pids+=($!)
$HIPCC $COMMON -ffp-contract=off -c cloudfilter.hip -o _obj/cloudfilter.o & pids+=($!)
$HIPCC $COMMON -ffp-contract=off -c icp.hip        -o _obj/icp.o & pids+=($!)
$HIPCC $COMMON -ffp-contract=off -c subdivide.hip  -o _obj/subdivide.o & pids+=($!)
$HIPCC $COMMON -ffp-contract=off -c normals.hip    -o _obj/normals.o & pids+=($!)
for p in "${pids[@]}"; do wait "$p"; done
$HIPCC --offload-arch=gfx950 -shared -fPIC _obj/project.o _obj/binning.o _obj/raster_fwd.o _obj/raster_bwd.o _obj/c_api.o _obj/postops.o _obj/losses.o _obj/pearson.o _obj/ags.o _obj/pointcloud.o _obj/metrics.o _obj/density.o _obj/levelset.o _obj/marching.o _obj/geometry.o _obj/meshcull.o _obj/tsdf.o _obj/meshclusters.o _obj/cloudfilter.o _obj/icp.o _obj/subdivide.o _obj/normals.o -o ../libdnsplat.so
echo "built $(realpath ../libdnsplat.so)"
