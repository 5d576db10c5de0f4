"""Tensor-level wrappers over the C ABI and the autograd nodes everything else is built from.

Graph shape (same cut as gsplat 1.0.0, so the tensors dn-splatter reads back keep their meaning):

    params --_ProjectFn--> means2d, depths, conics, splats --_RasterFn----> render, alphas
              (stage 1/5)        ^ info["means2d"]: .grad / .absgrad   \\-_RasterDnFn--> rgb, depth, normal, accumulation, surface_normal
                                                                          (stages 2-4)

``_ProjectFn`` fuses what gsplat splits into fully_fused_projection + spherical_harmonics and what
dn_model.py:543-560 does in torch; ``_RasterFn`` fuses isect_tiles + sort + rasterize_to_pixels (the drop-in calls);
``_RasterDnFn`` is the same pass over the 7 fused channels with dn-splatter's per-pixel post-ops inside the kernels (the fused
get_outputs path).  ``_PackFn`` is the front end of the legacy rasterize_gaussians call.

One builder per C struct: ``_scene_struct``, ``_camera_struct``, ``_ShLayout`` + ``_proj_grads``, ``_raster_args``, ``bin_tiles``'
``enqueue``, ``_backproject_args``, ``_eval_metrics_args``, ``_density_args``, ``_level_rays_args``, ``_level_points_args``, ``_mc_args``, ``_mc_observed_args``, ``_tsdf_args``, ``_cloud_distances_args``, ``_mesh_sample_args``; ``_ProjectFn.backward`` loops over the cameras in one of the four modes of ``_ProjBwd``.
"""
from __future__ import annotations

import ctypes
import math
import os
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from ._lib import BackprojectArgs, BinArgs, Camera, CloudDistancesArgs, CloudNormalsArgs, CloudOutlierArgs, DensityArgs, EvalMetricsArgs, DnPost, IcpArgs, LevelPointsArgs, LevelRaysArgs, McArgs, McObservedArgs, MeshClustersArgs, MeshCutArgs, MeshDepthArgs, MeshFilterArgs, MeshSampleArgs, MeshVisibilityArgs, PoseGrads, ProjGrads, ProjOut, RasterArgs, Scene, SubdivideArgs, TsdfArgs, VoxelArgs, RECORD_FLOATS


def _ptr(t: Optional[Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream() -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_gpu(t: Tensor, name: str) -> None:
    if not t.is_cuda:
        raise _lib.DnsplatError(
            f"{name} is on {t.device}: the dn-splatter_amd renderer runs only on the GPU through libdnsplat.so "
            "(there is no CPU fallback; the CPU oracle under oracle/ is test infrastructure)")


def _f32c(t: Tensor, name: str) -> Tensor:
    _need_gpu(t, name)
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    return t.contiguous()


# --------------------------------------------------------------------------------------------------
# configuration records


@dataclass(frozen=True)
class ProjCfg:
    width: int
    height: int
    tile_size: int = 16
    eps2d: float = 0.3
    near_plane: float = 0.01
    far_plane: float = 1e10
    radius_clip: float = 0.0
    antialiased: bool = False
    scales_are_log: bool = False
    opacities_are_logit: bool = False
    sh_degree: int = -1          # -1: direct colours
    with_depth: bool = False
    with_normals: bool = False
    want_normals_world: bool = False
    colors_are_logit: bool = False   # direct colours: sigmoid() inside the kernel (dn_model.py:491-492, config.sh_degree == 0)
    skip_culled_records: bool = False   # dnsplat_proj_out.skip_culled_records: culled Gaussians' records are left unwritten
    tight_tiles: bool = False    # dnsplat_camera.tight_tiles: tile counts over the alpha >= 1/255 box instead of gsplat's 3-sigma box
    split_colours: bool = False  # dnsplat_proj_out.phase 1 + 2: the SH colours on a side stream, beside the binning kernels

    @property
    def tiles(self):
        return math.ceil(self.width / self.tile_size), math.ceil(self.height / self.tile_size)


class _Buffers:
    """Grow-only per-device scratch (binning workspace, pinned counters) so steady-state frames do not
    touch the allocator."""

    def __init__(self):
        self.ws: Dict[torch.device, Tensor] = {}
        self.pinned: Dict[torch.device, Tensor] = {}
        self.ring: Dict[tuple, dict] = {}
        self.side: Dict[tuple, "torch.cuda.Stream"] = {}
        self.static_cap: Dict[tuple, int] = {}
        self.n_max: Dict[tuple, Tensor] = {}     # "static" bin policy: running maximum of n_isects per (device, stream) + frame size key
        self.capacity_hint: Dict[tuple, int] = {}
        # Frames binned over list cells (BIN_CELL) keep a second set of the same records, in (cell, Gaussian) pairs and keyed by the frame
        # size key + the cell shifts: their buffers are sized by these.  The records above stay what they are for every reader —
        # per-tile pair counts, which such a frame reports as well — and bound the cell capacities from above (a cell list is never
        # longer than the tile lists it replaces).
        self.cell_hint: Dict[tuple, int] = {}
        self.static_cap_cells: Dict[tuple, int] = {}
        self.n_max_cells: Dict[tuple, Tensor] = {}

    @staticmethod
    def _key(device):
        # one set of scratch per (device, stream): frames rendered concurrently on different HIP streams
        # (model.get_outputs_batch) must not share the binning workspace or the pinned counter
        return (device, torch.cuda.current_stream(device).cuda_stream)

    def side_stream(self, device) -> "torch.cuda.Stream":
        """The stream work that may overlap the current stream's is put on (one per device and current stream)."""
        key = self._key(device)
        st = self.side.get(key)
        if st is None:
            # lowest priority: what runs there is meant to fill the gaps the current stream leaves, not to compete with it
            prio = int(os.environ.get("DNSPLAT_SIDE_PRIORITY", "1"))
            st = torch.cuda.Stream(device, priority=prio)
            self.side[key] = st
        return st

    def workspace(self, device, nbytes: int) -> Tensor:
        key = self._key(device)
        cur = self.ws.get(key)
        if cur is None or cur.numel() < nbytes:
            cur = torch.empty(int(nbytes * 1.25) + 1024, dtype=torch.uint8, device=device)
            self.ws[key] = cur
        return cur

    def pinned_i64(self, device) -> Tensor:
        key = self._key(device)
        cur = self.pinned.get(key)
        if cur is None:
            # two words: a frame binned over list cells reports (cell pairs, tile pairs), every other frame fills the first only
            cur = torch.zeros(2, dtype=torch.int64).pin_memory()
            self.pinned[key] = cur
        return cur

    RING = 8

    def ring_slot(self, device):
        """("deferred" bin policy) the next (pinned int64 [1], event) pair of a small per-(device, stream) ring: the count of a
        frame is copied into its own slot, so several frames can be in flight before the host looks at any of them."""
        key = self._key(device)
        ring = self.ring.get(key)
        if ring is None:
            mem = torch.zeros(2 * self.RING, dtype=torch.int64).pin_memory()      # two words per slot, as pinned_i64
            ring = {"mem": mem, "events": [torch.cuda.Event() for _ in range(self.RING)], "next": 0, "pending": []}
            self.ring[key] = ring
        i = ring["next"]
        ring["next"] = (i + 1) % self.RING
        slot = ring["mem"][2 * i:2 * i + 2]
        # the slot about to be reused must have been looked at — whoever owns it, also when counts were resolved out of order
        # through Binning.n_isects — and at most RING - 1 frames are ever unverified
        for p in [p for p in ring["pending"] if p.slot.data_ptr() == slot.data_ptr()]:
            p.resolve()
        while len(ring["pending"]) >= self.RING - 1:
            ring["pending"][0].resolve()
        return ring, slot, ring["events"][i]


BUFFERS = _Buffers()

# Optional flat gradient bucket (dp.GradArena): when set, stage 5 writes parameter gradients straight into
# it so that data-parallel training all-reduces ONE buffer without flatten copies.
GRAD_ARENA = None


def set_grad_arena(arena) -> None:
    global GRAD_ARENA
    GRAD_ARENA = arena


# Optional compact SH-gradient exchange (dp.ShFactorExchange): when set, stage 5 hands out the 6 factors per
# Gaussian instead of the 48 coefficient gradients; dp.allreduce_gradients all-gathers them and rebuilds the sum.
SH_EXCHANGE = None


def set_sh_exchange(exchange) -> None:
    global SH_EXCHANGE
    SH_EXCHANGE = exchange


def _grad_like(param: Tensor) -> Tensor:
    """Where stage 5 writes the gradient of ``param``: its slice of the flat bucket, unless ``param.grad`` already IS that
    slice (zero_grad(set_to_none=False), or a second camera accumulated into the same step).  In that case autograd will
    run ``param.grad += new``: had the kernel written into the bucket, old and new gradient would be the same memory and
    the sum would come out as 2 x new.  A fresh tensor keeps accumulation correct (the sum still lands in the bucket)."""
    a = GRAD_ARENA
    if a is not None and not a.in_use(param):
        t = a.take(param)
        if t is not None:
            return t.view(param.shape)
    if a is not None and a.in_use(param):
        a.invalidate_sh_state()        # autograd is about to `+=` into the bucket: its rows are no longer what the kernel last wrote
    return torch.empty_like(param)

# "sync": read n_isects back before emitting (one host round-trip per frame, what gsplat does).
# "capacity": size the intersection buffers from the previous frames (x1.25), enqueue everything,
#             then verify n_isects <= capacity while the compositing kernel already runs; an overflow
#             re-runs the emit+composite with exact sizes.  No GPU bubble, always correct.
# "deferred": as "capacity", but the host does not wait for the count at all: it is copied into a pinned ring slot and
#             verified as soon as it has arrived (the frame's own backward, the next frame's binning, or whoever asks for
#             n_isects first — whichever comes first, none of them blocks in the steady state).  The host can run a whole
#             frame ahead of the GPU.  An overflow cannot be repaired after the fact: it RAISES (never silently wrong) and
#             enlarges the capacity, so that re-running the step succeeds.  The first frame of a size runs in "sync" mode.
# "static":   for frames captured into a HIP graph (graph.GraphedStep): the capacity is whatever earlier eager frames established
#             and NOTHING on the host looks at the count; the device keeps a running maximum (dnsplat_bin_args.n_isects_max)
#             that static_overflow() reads on demand.
BIN_POLICY = {"mode": "sync"}


def set_bin_policy(mode: str) -> None:
    if mode not in ("sync", "capacity", "deferred", "static"):
        raise ValueError(mode)
    BIN_POLICY["mode"] = mode


def _capacity_guess(key, cells) -> int:
    """What earlier frames of this size say the lists of the next one need: per-tile pairs, or with list cells (cell, Gaussian) pairs
    — never more than the per-tile guess, and nothing once that one has been forgotten."""
    hint = BUFFERS.capacity_hint.get(key, 0)
    if cells is None or not hint:
        return hint
    return min(hint, BUFFERS.cell_hint.get(key + cells, hint))


def _learn_capacity(key, cells, n: int, n_tile: int) -> None:
    """A frame's counts have reached the host: the guesses grow to 1.25 x what it needed."""
    BUFFERS.capacity_hint[key] = max(BUFFERS.capacity_hint.get(key, 0), int(n_tile * 1.25) + 4096)
    if cells is not None:
        BUFFERS.cell_hint[key + cells] = max(BUFFERS.cell_hint.get(key + cells, 0), int(n * 1.25) + 4096)


class _PendingCount:
    """The intersection count of one frame binned under the "deferred" policy, until the host has looked at it."""

    def __init__(self, ring, slot, event, capacity, key, cells=None):
        self.ring, self.slot, self.event, self.capacity, self.key = ring, slot, event, capacity, key
        self.n: Optional[int] = None
        self.cells = cells              # list cells: n / capacity are (cell, Gaussian) pairs and n_tile the per-tile pair count
        self.n_tile: Optional[int] = None
        self.overflowed = False

    def ready(self) -> bool:
        return self.n is not None or self.event.query()

    def resolve(self) -> int:
        """Waits for the count if it has not arrived yet, verifies it, returns it.  Raises on overflow — on EVERY call for a frame
        that overflowed (its lists are truncated: nobody may read its count or its list as if it were complete)."""
        if self.n is None:
            self.event.synchronize()
            self.n = int(self.slot[0])
            self.n_tile = int(self.slot[1]) if self.cells else self.n
            if self in self.ring["pending"]:
                self.ring["pending"].remove(self)
            _learn_capacity(self.key, self.cells, self.n, self.n_tile)
            self.overflowed = self.n > self.capacity
        if self.overflowed:
            raise _lib.DnsplatError(
                f"tile binning: {self.n} intersections exceed the capacity {self.capacity} guessed from earlier frames "
                "(bin policy 'deferred' verifies the count after the fact): the outputs and gradients of that frame are "
                "invalid. The capacity has been enlarged; run the step again (or use set_bin_policy('capacity'), which "
                "repairs an overflow itself at the price of one host wait per frame)")
        return self.n


def static_overflow(device, stream=None) -> Optional[int]:
    """ "static" bin policy: the largest intersection count a frame binned on ``stream`` (default: the current one) produced, if
    it exceeded the capacity the frames of that size ran with (their lists were then truncated), else None.  Synchronises.
    An overflow is REPORTED ONCE and repaired for whoever captures next: the capacity guess of that frame size is raised to
    1.25 x the count seen, the sticky device maximum and the recorded static capacity are cleared — a re-capture after the error
    gets buffers that fit (before, a re-capture reused the same guess and overflowed again)."""
    skey = (device, (torch.cuda.current_stream(device) if stream is None else stream).cuda_stream)
    worst = None
    for k, t in list(BUFFERS.n_max.items()):
        if k[:2] != skey:
            continue
        n = int(t.item())
        # frames binned over list cells: their buffers hold (cell, Gaussian) pairs, counted and bounded beside the per-tile figures
        over_cells = [(ck, int(ct.item())) for ck, ct in BUFFERS.n_max_cells.items() if ck[:len(k)] == k]
        over_cells = [(ck, nc) for ck, nc in over_cells if nc > BUFFERS.static_cap_cells.get(ck, 0)]
        if n > BUFFERS.static_cap.get(k, 0) or over_cells:
            worst = n if worst is None else max(worst, n)
            hkey = k[2:]                                   # (device, N, width, height): the key of the capacity guesses
            BUFFERS.capacity_hint[hkey] = max(BUFFERS.capacity_hint.get(hkey, 0), int(n * 1.25) + 4096)
            t.zero_()
            BUFFERS.static_cap.pop(k, None)
            for ck, nc in over_cells:
                BUFFERS.cell_hint[ck[2:]] = max(BUFFERS.cell_hint.get(ck[2:], 0), int(nc * 1.25) + 4096)
            for ck in [ck for ck in BUFFERS.n_max_cells if ck[:len(k)] == k]:
                BUFFERS.n_max_cells[ck].zero_()
                BUFFERS.static_cap_cells.pop(ck, None)
    return worst


def forget_capacity_guesses(device=None) -> None:
    """Drops the capacity guesses earlier frames left behind — for ``device`` or for all: the Gaussian set changed size
    (densify.after_refinement), the next frame of a size starts in "sync".  The "static" policy's per-stream records (running
    maxima, static capacities) are NOT touched: the running maximum is a device word that the captured bin kernels of a live
    graph.GraphedStep still write on every replay, and this dict holds the reference that keeps it allocated — they go
    with their step (GraphedStep.close -> forget_static)."""
    for d in (BUFFERS.capacity_hint, BUFFERS.cell_hint):
        for k in [k for k in d if device is None or k[0] == device]:
            del d[k]


def carry_capacity_guesses(device, n_old: int, n_new: int, slack: float = 1.1) -> int:
    """The Gaussian set changed size (densify.after_refinement): instead of forgetting what the frames of the old size needed —
    which costs the next capture a round of eager frames over every pose just to size its buffers again — scale each guess by
    n_new / n_old x ``slack`` and file it under the new size.  A guess is a capacity, not a promise: a frame that outgrows it is
    reported by the bin policy in force (``GraphedStep.check()`` raises and enlarges it).  Returns the number of guesses carried."""
    carried = 0
    for d in (BUFFERS.capacity_hint, BUFFERS.cell_hint):      # the cell-pair guesses travel with the per-tile ones, uncounted
        for k in [k for k in d if (device is None or k[0] == device) and k[1] == n_old]:
            hint = d.pop(k)
            nk = (k[0], n_new) + tuple(k[2:])
            # never scaled DOWN: culling removes low-opacity, small-footprint Gaussians, so the intersections fall less than N does, and
            # an under-estimate would make the next capture's warm-up frame overflow instead of sizing itself
            ratio = max(1.0, n_new / max(n_old, 1))
            d[nk] = max(d.get(nk, 0), int(hint * ratio * slack) + 4096)
            carried += d is BUFFERS.capacity_hint
    return carried


def forget_static(device, stream) -> None:
    """Drops the "static" policy's per-stream records (running maxima, capacities) of ``stream``: called when the GraphedStep that
    owned the stream is discarded, so that they do not accumulate across re-captures."""
    skey = (device, stream.cuda_stream)
    for d in (BUFFERS.n_max, BUFFERS.static_cap, BUFFERS.n_max_cells, BUFFERS.static_cap_cells):
        for k in [k for k in d if k[:2] == skey]:
            del d[k]
    for d in (BUFFERS.ws, BUFFERS.pinned, BUFFERS.ring, BUFFERS.side):
        d.pop(skey, None)


def verify_pending_counts(device, block: bool = False) -> None:
    """Looks at every deferred intersection count of the current stream that has arrived (all of them with ``block``)."""
    ring = BUFFERS.ring.get(_Buffers._key(device))
    if ring is None:
        return
    for p in list(ring["pending"]):
        if block or p.ready():
            p.resolve()


# --------------------------------------------------------------------------------------------------
# stage 1 / 5


def _scene_struct(N, means, quats, scales, opacities, cfg: ProjCfg, sh0, sh0_stride, shN, shN_stride, sh_K, colors):
    s = Scene()
    s.N = N
    s.means, s.quats, s.scales, s.opacities = _ptr(means), _ptr(quats), _ptr(scales), _ptr(opacities)
    s.scales_are_log = int(cfg.scales_are_log)
    s.opacities_are_logit = int(cfg.opacities_are_logit)
    s.sh_degree = cfg.sh_degree
    s.sh_K = sh_K
    s.sh0, s.sh0_stride = _ptr(sh0), sh0_stride
    s.shN, s.shN_stride = _ptr(shN), shN_stride
    s.colors = _ptr(colors)
    s.n_colors = 0 if colors is None else colors.shape[-1]
    s.colors_are_logit = int(cfg.colors_are_logit and colors is not None)
    return s


def _camera_struct(viewmat, K, normal_frame, cfg: ProjCfg):
    c = Camera()
    c.viewmat, c.K, c.normal_frame = _ptr(viewmat), _ptr(K), _ptr(normal_frame)
    c.width, c.height, c.tile_size = cfg.width, cfg.height, cfg.tile_size
    c.eps2d, c.near_plane, c.far_plane, c.radius_clip = cfg.eps2d, cfg.near_plane, cfg.far_plane, cfg.radius_clip
    c.antialiased = int(cfg.antialiased)
    c.tight_tiles = int(cfg.tight_tiles)
    return c


def _backproject_args(width, height, depth, rgb, normal, mask, indices, counts, intrinsics, xform, crop, points, colors, normals,
                      state, scratch):
    a = BackprojectArgs()
    a.width, a.height = width, height
    a.depth, a.rgb, a.normal, a.mask = _ptr(depth), _ptr(rgb), _ptr(normal), _ptr(mask)
    a.indices, a.counts = _ptr(indices), _ptr(counts)
    a.n_rows = 0 if indices is None else indices.numel()
    a.fx, a.fy, a.cx, a.cy = intrinsics
    a.xform, a.crop = _ptr(xform), _ptr(crop)
    a.points, a.colors, a.normals = _ptr(points), _ptr(colors), _ptr(normals if normal is not None else None)
    a.capacity = points.shape[0]
    a.state, a.scratch = _ptr(state), _ptr(scratch)
    return a


def _eval_metrics_args(width, height, rgb, gt_rgb, depth, gt_depth, depth_tolerance, normal, gt_normal, normal_layout, scratch,
                       metrics, counts, sums):
    a = EvalMetricsArgs()
    a.width, a.height = width, height
    a.rgb, a.gt_rgb, a.depth, a.gt_depth = _ptr(rgb), _ptr(gt_rgb), _ptr(depth), _ptr(gt_depth)
    a.depth_tolerance, a.normal_layout = depth_tolerance, normal_layout
    a.normal, a.gt_normal = _ptr(normal), _ptr(gt_normal)
    a.scratch, a.metrics, a.counts, a.sums = _ptr(scratch), _ptr(metrics), _ptr(counts), _ptr(sums)
    return a


def _density_args(N, index, records, samples, lattice, mask, fill, neighbors, k, skip, num_closest, density, normals):
    """``lattice``: None, or the three coordinate arrays (X, Y, Z) that replace ``samples``."""
    a = DensityArgs()
    a.N, a.index, a.records = N, _ptr(index), _ptr(records)
    a.M, a.samples = (0, None) if samples is None else (samples.shape[0], _ptr(samples))
    if lattice is not None:
        X, Y, Z = lattice
        a.X, a.Y, a.Z = _ptr(X), _ptr(Y), _ptr(Z)
        a.Rx, a.Ry, a.Rz = X.numel(), Y.numel(), Z.numel()
    a.mask, a.fill = _ptr(mask), fill
    a.neighbors = _ptr(neighbors)
    a.neighbors_int64 = int(neighbors is not None and neighbors.dtype == torch.int64)
    a.k, a.skip, a.num_closest = k, skip, num_closest
    a.density, a.normals = _ptr(density), _ptr(normals)
    return a


def _level_rays_args(width, height, depth, mask, intrinsics, xform, range_table, N, index, records, scales_log, quats, neighbors, levels,
                     lane_map, t_hit, valid, closest, first_above, densities):
    a = LevelRaysArgs()
    a.width, a.height = width, height
    a.depth, a.mask = _ptr(depth), _ptr(mask)
    a.fx, a.fy, a.cx, a.cy = intrinsics
    a.xform, a.range = _ptr(xform), _ptr(range_table)
    a.N, a.index, a.records, a.scales_log, a.quats = N, _ptr(index), _ptr(records), _ptr(scales_log), _ptr(quats)
    a.neighbors = _ptr(neighbors)
    a.neighbors_int64 = int(neighbors is not None and neighbors.dtype == torch.int64)
    a.n_levels = len(levels)
    for l, v in enumerate(levels[:8]):
        a.levels[l] = v
    a.lane_map = lane_map
    a.t_hit, a.valid, a.closest = _ptr(t_hit), _ptr(valid), _ptr(closest)
    a.first_above, a.densities = _ptr(first_above), _ptr(densities)
    return a


def _level_points_args(width, height, depth, rgb, mask, indices, counts, intrinsics, xform, crop, t_hit, closest, normal_mode,
                       gauss_normals, N, index, records, points, colors, normals, state, scratch):
    a = LevelPointsArgs()
    a.width, a.height = width, height
    a.depth, a.rgb, a.mask = _ptr(depth), _ptr(rgb), _ptr(mask)
    a.indices, a.counts, a.n_rows = _ptr(indices), _ptr(counts), indices.numel()
    a.fx, a.fy, a.cx, a.cy = intrinsics
    a.xform, a.crop = _ptr(xform), _ptr(crop)
    a.t_hit, a.closest = _ptr(t_hit), _ptr(closest)
    a.normal_mode, a.gauss_normals = normal_mode, _ptr(gauss_normals)
    a.N, a.index, a.records = N, _ptr(index), _ptr(records)
    a.points, a.colors, a.normals = _ptr(points), _ptr(colors), _ptr(normals)
    a.capacity = points.shape[0]
    a.state, a.scratch = _ptr(state), _ptr(scratch)
    return a


def _mc_args(volume, level, scratch, counts, vertices=None, triangles=None, cap_v=0, cap_t=0, status=None):
    a = McArgs()
    a.volume, a.level = _ptr(volume), level
    a.nx, a.ny, a.nz = volume.shape
    a.scratch, a.scratch_bytes = _ptr(scratch), 0 if scratch is None else scratch.numel() * scratch.element_size()
    a.counts = _ptr(counts)
    a.cap_v, a.cap_t = cap_v, cap_t
    a.vertices, a.triangles, a.status = _ptr(vertices), _ptr(triangles), _ptr(status)
    return a


def _mc_observed_args(weight, min_weight, *mc):
    a = McObservedArgs()
    a.mc = _mc_args(*mc)
    a.weight, a.min_weight = _ptr(weight), min_weight
    return a


def _tsdf_args(tsdf, weight, color, origin, voxel, w2c, k, pixel_offset, depth, rgb, ray_scale, sdf_trunc, depth_trunc):
    a = TsdfArgs()
    a.tsdf, a.weight, a.color = _ptr(tsdf), _ptr(weight), _ptr(color)
    a.nx, a.ny, a.nz = tsdf.shape
    a.origin, a.voxel = (ctypes.c_double * 3)(*origin), voxel
    a.C, a.height, a.width = depth.shape
    a.w2c = _ptr(w2c)
    a.fx, a.fy, a.cx, a.cy = k[0], k[4], k[2], k[5]
    a.pixel_offset = pixel_offset
    a.depth, a.rgb, a.ray_scale = _ptr(depth), _ptr(rgb), _ptr(ray_scale)
    a.sdf_trunc, a.depth_trunc = sdf_trunc, depth_trunc
    return a


def _cloud_distances_args(N, index, src, src_normals, tgt_normals, threshold, percentile, dist2, idx, absdot, scalars, counts, scratch):
    a = CloudDistancesArgs()
    a.N, a.index = N, _ptr(index)
    a.M, a.src = src.shape[0], _ptr(src)
    a.src_normals, a.tgt_normals = _ptr(src_normals), _ptr(tgt_normals)
    a.threshold, a.percentile = threshold, percentile
    a.dist2, a.idx, a.absdot = _ptr(dist2), _ptr(idx), _ptr(absdot)
    a.scalars, a.counts, a.scratch = _ptr(scalars), _ptr(counts), _ptr(scratch)
    return a


def _mesh_sample_args(seed, cdf, vertices, triangles, face_normals, points, normals, faces):
    a = MeshSampleArgs()
    a.S, a.seed = points.shape[0], seed
    a.V, a.T = vertices.shape[0], triangles.shape[0]
    a.cdf, a.vertices, a.triangles, a.face_normals = _ptr(cdf), _ptr(vertices), _ptr(triangles), _ptr(face_normals)
    a.points, a.normals, a.faces = _ptr(points), _ptr(normals), _ptr(faces)
    return a


def _mesh_depth_args(vertices, triangles, w2c, k, width, height, znear, zfar, depth, scratch, stats=None):
    a = MeshDepthArgs()
    a.V, a.T, a.C = vertices.shape[0], triangles.shape[0], w2c.shape[0]
    a.width, a.height = width, height
    a.vertices, a.triangles, a.w2c = _ptr(vertices), _ptr(triangles), _ptr(w2c)
    a.fx, a.fy, a.cx, a.cy = k[0], k[4], k[2], k[5]
    a.znear, a.zfar = znear, zfar
    a.depth, a.scratch, a.stats = _ptr(depth), _ptr(scratch), _ptr(stats)
    return a


def _mesh_visibility_args(vertices, w2c, k, width, height, rendered, depth_gt, remove_occlusion, remove_missing_depth, obs, invalid):
    a = MeshVisibilityArgs()
    a.V, a.C = vertices.shape[0], w2c.shape[0]
    a.width, a.height = width, height
    a.vertices, a.w2c = _ptr(vertices), _ptr(w2c)
    a.K = (ctypes.c_double * 9)(*k)
    a.rendered, a.depth_gt = _ptr(rendered), _ptr(depth_gt)
    a.remove_occlusion, a.remove_missing_depth = int(remove_occlusion), int(remove_missing_depth)
    a.obs, a.invalid = _ptr(obs), _ptr(invalid)
    return a


def _mesh_cut_args(vertices, triangles, obs, invalid, obs_threshold, invalid_share, scratch, counts, out_vertices=None, out_triangles=None,
                   status=None):
    a = MeshCutArgs()
    a.V, a.T = vertices.shape[0], triangles.shape[0]
    a.vertices, a.triangles, a.obs, a.invalid = _ptr(vertices), _ptr(triangles), _ptr(obs), _ptr(invalid)
    a.obs_threshold, a.invalid_share = obs_threshold, invalid_share
    a.scratch, a.scratch_bytes = _ptr(scratch), scratch.numel() * scratch.element_size()
    a.counts = _ptr(counts)
    a.cap_v = 0 if out_vertices is None else out_vertices.shape[0]
    a.cap_t = 0 if out_triangles is None else out_triangles.shape[0]
    a.out_vertices, a.out_triangles, a.status = _ptr(out_vertices), _ptr(out_triangles), _ptr(status)
    return a


def _mesh_clusters_args(n_vertices, triangles, scratch, labels, sizes, counts, status):
    a = MeshClustersArgs()
    a.V, a.T = n_vertices, triangles.shape[0]
    a.triangles = _ptr(triangles)
    a.scratch, a.scratch_bytes = _ptr(scratch), scratch.numel() * scratch.element_size()
    a.labels, a.sizes, a.counts, a.status = _ptr(labels), _ptr(sizes), _ptr(counts), _ptr(status)
    return a


def _mesh_filter_args(n_vertices, triangles, labels, sizes, cluster_counts, keep_largest, min_triangles, scratch, threshold, counts,
                      vertex_index=None, out_triangles=None, status=None):
    a = MeshFilterArgs()
    a.V, a.T = n_vertices, triangles.shape[0]
    a.triangles, a.labels, a.sizes, a.cluster_counts = _ptr(triangles), _ptr(labels), _ptr(sizes), _ptr(cluster_counts)
    a.keep_largest, a.min_triangles = keep_largest, min_triangles
    a.scratch, a.scratch_bytes = _ptr(scratch), scratch.numel() * scratch.element_size()
    a.threshold, a.counts = _ptr(threshold), _ptr(counts)
    a.cap_v = 0 if vertex_index is None else vertex_index.shape[0]
    a.cap_t = 0 if out_triangles is None else out_triangles.shape[0]
    a.vertex_index, a.out_triangles, a.status = _ptr(vertex_index), _ptr(out_triangles), _ptr(status)
    return a


def _cloud_outlier_args(points, index, nb_neighbors, std_ratio, scratch, avg, stats, ind=None):
    a = CloudOutlierArgs()
    a.N, a.nb_neighbors = avg.shape[0], nb_neighbors
    a.points, a.index = _ptr(points), _ptr(index)
    a.std_ratio = std_ratio
    a.scratch, a.scratch_bytes = _ptr(scratch), scratch.numel() * scratch.element_size()
    a.avg, a.stats = _ptr(avg), _ptr(stats)
    a.capacity = 0 if ind is None else ind.shape[0]
    a.ind = _ptr(ind)
    return a


def _voxel_args(points, normals, colors, voxel_size, scratch, counts, voxel_of, out_points=None, out_normals=None, out_colors=None,
                out_counts=None):
    a = VoxelArgs()
    a.N = points.shape[0]
    a.points, a.normals, a.colors = _ptr(points), _ptr(normals), _ptr(colors)
    a.voxel_size = voxel_size
    a.scratch, a.scratch_bytes = _ptr(scratch), scratch.numel() * scratch.element_size()
    a.counts, a.voxel_of = _ptr(counts), _ptr(voxel_of)
    a.cap_v = 0 if out_points is None else out_points.shape[0]
    a.out_points, a.out_normals, a.out_colors, a.out_counts = _ptr(out_points), _ptr(out_normals), _ptr(out_colors), _ptr(out_counts)
    return a


def _icp_args(source, target, index, max_dist, relative_fitness, relative_rmse, max_iteration, state, scratch, trace=None, idx=None,
              dist2=None):
    a = IcpArgs()
    a.M, a.source = source.shape[0], _ptr(source)
    a.N, a.target, a.index = target.shape[0], _ptr(target), _ptr(index)
    a.max_dist, a.relative_fitness, a.relative_rmse, a.max_iteration = max_dist, relative_fitness, relative_rmse, max_iteration
    a.state, a.trace, a.idx, a.dist2 = _ptr(state), _ptr(trace), _ptr(idx), _ptr(dist2)
    a.scratch, a.scratch_bytes = _ptr(scratch), scratch.numel() * scratch.element_size()
    return a


def _subdivide_args(vertices, triangles, origin, max_edge, scratch, counts, status, vertex_base=0, out_vertices=None, out_triangles=None,
                    out_index=None, next_vertices=None, next_triangles=None, next_origin=None):
    a = SubdivideArgs()
    a.V, a.T = vertices.shape[0], triangles.shape[0]
    a.vertices, a.triangles, a.origin = _ptr(vertices), _ptr(triangles), _ptr(origin)
    a.max_edge = max_edge
    a.scratch, a.scratch_bytes = _ptr(scratch), scratch.numel() * scratch.element_size()
    a.counts, a.status = _ptr(counts), _ptr(status)
    a.vertex_base = vertex_base
    a.cap_v = 0 if out_vertices is None else out_vertices.shape[0]
    a.cap_t = 0 if out_triangles is None else out_triangles.shape[0]
    a.cap_long = 0 if next_origin is None else next_origin.shape[0] // 4
    a.cap_mid = 0 if next_vertices is None else next_vertices.shape[0] - vertices.shape[0]
    a.out_vertices, a.out_triangles, a.out_index = _ptr(out_vertices), _ptr(out_triangles), _ptr(out_index)
    a.next_vertices, a.next_triangles, a.next_origin = _ptr(next_vertices), _ptr(next_triangles), _ptr(next_origin)
    return a


def _cloud_normals_args(points, index, knn, radius, orient_toward, scratch, normals, status, covariance=None, neighbors=None, count=None):
    a = CloudNormalsArgs()
    a.N, a.knn = points.shape[0], knn
    a.points, a.index = _ptr(points), _ptr(index)
    a.radius = 0.0 if radius is None else radius
    a.orient = 0 if orient_toward is None else 1
    for k in range(3):
        a.toward[k] = 0.0 if orient_toward is None else orient_toward[k]
    a.scratch, a.scratch_bytes = _ptr(scratch), scratch.numel() * scratch.element_size()
    a.normals, a.covariance, a.neighbors, a.count, a.status = _ptr(normals), _ptr(covariance), _ptr(neighbors), _ptr(count), _ptr(status)
    return a


class _ShLayout:
    """How the colours of one projection arrive, resolved once in ``_ProjectFn.forward`` and kept on ``ctx``: ``kind`` "cat" (one
    tensor ``coeffs`` [N,K,3], gsplat's layout), "split" (``sh0`` [N,3] + ``shN`` [N,K-1,3], the model's own leaves) or "colors"
    (direct colours, no SH), ``sh_K``, and the row strides band 0 / bands 1.. go to the kernels with.  It holds NO tensor: the
    inputs are autograd's saved tensors, and a gradient tensor somebody else holds is cloned by autograd instead of adopted as
    ``.grad`` — ``bands`` turns whichever set it is given (the coefficients, or their gradients) into the kernels' two pointers."""
    __slots__ = ("kind", "sh_K", "s0", "sN")

    def __init__(self, kind: str, sh_K: int):
        self.kind, self.sh_K = kind, sh_K
        self.s0, self.sN = {"cat": (3 * sh_K, 3 * sh_K), "split": (3, 3 * (sh_K - 1)), "colors": (0, 0)}[kind]

    def bands(self, coeffs, sh0, shN, rows=None):
        """(band 0, bands 1..) of the coefficients — or of their gradients — for the rows ``rows`` = (g0, g1) of the Gaussians."""
        if rows is not None:
            coeffs, sh0, shN = (None if t is None else t[rows[0]:rows[1]] for t in (coeffs, sh0, shN))
        if self.kind == "cat":
            return coeffs, coeffs.view(-1)[3:]
        if self.kind == "split":
            return sh0, (shN if self.sh_K > 1 else None)
        return None, None

    def scene(self, cfg: ProjCfg, means, quats, scales, opacities, coeffs, sh0, shN, colors, rows=None) -> Scene:
        p0, pN = self.bands(coeffs, sh0, shN, rows)
        if rows is not None:
            means, quats, scales, opacities, colors = (None if t is None else t[rows[0]:rows[1]]
                                                       for t in (means, quats, scales, opacities, colors))
        return _scene_struct(means.shape[0], means, quats, scales, opacities, cfg, p0, self.s0, pN, self.sN, self.sh_K, colors)

    def new_grads(self, coeffs, sh0, shN, colors, bucket: bool):
        """Unwritten [v_coeffs, v_sh0, v_shN, v_colors] (None where the layout has no such input); ``bucket``: the leaves' gradients
        go where ``_grad_like`` says."""
        like = _grad_like if bucket else torch.empty_like
        if self.kind == "cat":
            return [torch.empty_like(coeffs), None, None, None]
        if self.kind == "split":
            return [None, like(sh0), like(shN) if self.sh_K > 1 else None, None]
        return [None, None, None, None if colors is None else torch.empty_like(colors)]


def _proj_grads(lay: _ShLayout, radii, v_splats, cots, geo, sh, rows=None) -> ProjGrads:
    """``radii`` / ``v_splats`` / ``cots`` = (v_means2d, v_depths, v_conics, v_compensations | None each): one camera's rows;
    ``geo`` = (v_means, v_quats, v_scales, v_opacities) and ``sh`` = [v_coeffs, v_sh0, v_shN, v_colors]: where the kernel writes.
    ``rows`` = (g0, g1) restricts every one of them to a slice of the Gaussians (dp.SlicedShExchange)."""
    v_colors = sh[3]
    if rows is not None:
        radii, v_splats, v_colors, *rest = (None if t is None else t[rows[0]:rows[1]] for t in (radii, v_splats, v_colors, *cots, *geo))
        cots, geo = rest[:4], rest[4:]
    g = ProjGrads()
    g.radii, g.v_splats = _ptr(radii), _ptr(v_splats)
    g.v_means2d, g.v_depths, g.v_conics, g.v_compensations = _ptr(cots[0]), _ptr(cots[1]), _ptr(cots[2]), _ptr(cots[3])
    g.v_means, g.v_quats, g.v_scales, g.v_opacities = _ptr(geo[0]), _ptr(geo[1]), _ptr(geo[2]), _ptr(geo[3])
    p0, pN = lay.bands(sh[0], sh[1], sh[2], rows)
    g.v_sh0, g.v_sh0_stride, g.v_shN, g.v_shN_stride = _ptr(p0), lay.s0, _ptr(pN), lay.sN
    g.v_colors = _ptr(v_colors)
    return g


class _ProjectFn(torch.autograd.Function):
    """Stage 1 forward / stage 5 backward.  SH coefficients come either as one tensor ``coeffs``
    [N,K,3] (gsplat layout, dn_model.py:466-468 concatenates it) or split ``sh0`` [N,3] +
    ``shN`` [N,K-1,3] (the model's own features_dc / features_rest — no 192 B/Gaussian cat copy)."""

    @staticmethod
    def forward(ctx, means, quats, scales, opacities, coeffs, sh0, shN, colors, viewmat, K, normal_frame, cfg: ProjCfg,
                saturation_flag=None, side=None):
        means = _f32c(means, "means"); quats = _f32c(quats, "quats"); scales = _f32c(scales, "scales")
        opacities = _f32c(opacities, "opacities")
        viewmat = _f32c(viewmat, "viewmats"); K = _f32c(K, "Ks")
        N = means.shape[0]
        dev = means.device
        lay = _ShLayout("colors", 0)
        if cfg.sh_degree >= 0:
            if coeffs is not None:
                coeffs = _f32c(coeffs, "colors")
                lay = _ShLayout("cat", coeffs.shape[1])
            else:
                sh0 = _f32c(sh0, "features_dc")
                if shN is not None and shN.shape[1] > 0:
                    shN = _f32c(shN, "features_rest")
                lay = _ShLayout("split", 1 + (shN.shape[1] if shN is not None else 0))
            if lay.sh_K < (cfg.sh_degree + 1) ** 2:
                raise ValueError(f"sh_degree={cfg.sh_degree} needs {(cfg.sh_degree + 1) ** 2} bases, got {lay.sh_K}")
        elif colors is not None:
            colors = _f32c(colors, "colors")
        if normal_frame is not None:
            normal_frame = _f32c(normal_frame, "normal_frame")

        # one launch per camera of the batch (C = 1 in training, dn_model.py:421; C > 1 for the batched render loops of the
        # offline consumers): per-camera outputs are the rows of [C,N,...] tensors, the records of camera c are rows
        # c*N .. (c+1)*N of one [C*N,16] buffer — the layout dnsplat_bin_* / dnsplat_raster_* take for a batch
        ctx.viewmat_shape = viewmat.shape
        viewmat = viewmat.reshape(-1, 4, 4)
        K = K.reshape(-1, 3, 3)
        C = viewmat.shape[0]
        if normal_frame is not None:
            normal_frame = normal_frame.reshape(-1, 12)
        radii = torch.empty(C, N, dtype=torch.int32, device=dev)
        tiles = torch.empty(C, N, dtype=torch.int32, device=dev)
        # tight tile boxes: gsplat's count for the caller (info["tiles_per_gauss"]), the tight one for the binning
        tiles_bin = torch.empty(C, N, dtype=torch.int32, device=dev) if cfg.tight_tiles else None
        tile_boxes = torch.empty(C, N, 2, dtype=torch.int32, device=dev)      # (first tile, width) of the box the binning walks
        means2d = torch.empty(C, N, 2, dtype=torch.float32, device=dev)
        depths = torch.empty(C, N, dtype=torch.float32, device=dev)
        conics = torch.empty(C, N, 3, dtype=torch.float32, device=dev)
        comp = torch.empty(C, N, dtype=torch.float32, device=dev) if cfg.antialiased else None
        splats = torch.empty(C * N, RECORD_FLOATS, dtype=torch.float32, device=dev)
        nworld = torch.empty(C, N, 3, dtype=torch.float32, device=dev) if cfg.want_normals_world else None

        scene = lay.scene(cfg, means, quats, scales, opacities, coeffs, sh0, shN, colors)
        # phase 1 here, phase 2 (the SH colours: most of the bytes) on a side stream while this stream goes on to the binning
        # kernels, which leave most of the chip idle; whoever reads the colour channels of the records waits for side["colours_ready"]
        split = bool(cfg.split_colours and side is not None and cfg.sh_degree >= 0)
        outs = []
        for c in range(C):
            cam = _camera_struct(viewmat[c], K[c], None if normal_frame is None else normal_frame[c], cfg)
            out = ProjOut()
            out.radii, out.means2d, out.depths, out.conics = _ptr(radii[c]), _ptr(means2d[c]), _ptr(depths[c]), _ptr(conics[c])
            out.compensations = _ptr(comp[c]) if comp is not None else None
            out.tiles_per_gauss, out.splats = _ptr(tiles[c]), _ptr(splats[c * N:])
            out.tiles_bin = _ptr(tiles_bin[c]) if tiles_bin is not None else None
            out.tile_boxes = _ptr(tile_boxes[c])
            out.normals_world = _ptr(nworld[c]) if nworld is not None else None
            out.with_depth_channel = int(cfg.with_depth)
            out.with_normal_channels = int(cfg.with_normals)
            out.saturation_flag = _ptr(saturation_flag)      # one word for all cameras of the batch (zeroed by camera_prepare)
            out.skip_culled_records = int(cfg.skip_culled_records)
            out.phase = 1 if split else 0
            _lib.run("dnsplat_project_fwd", _lib.lib().dnsplat_project_fwd, ctypes.byref(scene), ctypes.byref(cam), ctypes.byref(out), _stream())
            outs.append((cam, out))
        if split:
            main = torch.cuda.current_stream(dev)
            s2 = BUFFERS.side_stream(dev)
            s2.wait_stream(main)
            with torch.cuda.stream(s2):
                for cam, out in outs:
                    out.phase = 2
                    _lib.run("dnsplat_project_fwd_colours", _lib.lib().dnsplat_project_fwd, ctypes.byref(scene), ctypes.byref(cam),
                             ctypes.byref(out), _stream())
                ev = torch.cuda.Event()
                ev.record(s2)
            side["colours_ready"] = ev

        ctx.cfg = cfg
        ctx.sh = lay
        ctx.save_for_backward(means, quats, scales, opacities, coeffs, sh0, shN, colors, viewmat, K, normal_frame, radii, splats)
        ctx.set_materialize_grads(False)
        empty = torch.empty(0, device=dev)
        if tiles_bin is None:
            tiles_bin = torch.empty(0, dtype=torch.int32, device=dev)
        # ONE call: every call of mark_non_differentiable replaces the set of the previous one (normals_world with a grad_fn
        # would keep the frame's autograd graph alive through gauss_params["normals"])
        ctx.mark_non_differentiable(*([radii, tiles, tiles_bin, tile_boxes] + ([nworld] if nworld is not None else [])))
        return (means2d, depths, conics, comp if comp is not None else empty, splats, radii, tiles,
                nworld if nworld is not None else empty, tiles_bin, tile_boxes)

    @staticmethod
    def backward(ctx, v_means2d, v_depths, v_conics, v_comp, v_splats, _r, _t, _n, _tb, _bx):
        job = _ProjBwd(ctx, v_means2d, v_depths, v_conics, v_comp, v_splats)
        step = job.mode()
        total = step(0)      # running sum over the cameras of a batch (C > 1); a single camera writes its outputs directly
        for c in range(1, job.C):
            for acc, t in zip(total, step(c)):
                if acc is not None:
                    acc.add_(t)
        need = ctx.needs_input_grad
        return tuple(t if (t is not None and need[i]) else None for i, t in enumerate(total)) + (
            None if job.v_viewmat is None else job.v_viewmat.reshape(ctx.viewmat_shape), None, None, None, None, None)


class _ProjBwd:
    """One call of ``_ProjectFn.backward``: what the cameras of the batch share, and one method per mode of stage 5 — ``plain``,
    ``zero_state``, ``factors``, ``sliced`` — each of which launches camera ``c`` and returns its gradient list
    [v_means, v_quats, v_scales, v_opacities, v_coeffs, v_sh0, v_shN, v_colors].  Lives for the call only (it sees the gradient
    tensors: nothing that outlives the backward may hold them, or autograd clones them instead of adopting them as .grad)."""

    def __init__(self, ctx, v_means2d, v_depths, v_conics, v_comp, v_splats):
        self.saved = ctx.saved_tensors
        means, viewmat = self.saved[0], self.saved[8]
        cfg = self.cfg = ctx.cfg
        self.lay: _ShLayout = ctx.sh
        N = self.N = means.shape[0]
        C = self.C = viewmat.shape[0]
        dev = means.device
        if v_splats is None:
            v_splats = torch.zeros(C * N, RECORD_FLOATS, dtype=torch.float32, device=dev)
        self.v_splats = v_splats = v_splats.contiguous()
        # The screen-space gradient reaches this node in two parts that are ALWAYS added: columns 0-1 of the gradient records (what
        # the compositing backward accumulated and did not hand to autograd separately, _hand_over_means2d_grad) and whatever
        # autograd delivers for means2d itself (terms the caller hung on info["means2d"], the legacy pass fed with non-detached
        # xys, or — when means2d was not retained — the compositing term, whose record columns were then cleared).  The kernel
        # takes g.v_means2d INSTEAD of the record's columns, hence the sum here.  No state outside the autograd graph is involved:
        # records summed over two compositing calls, or a backward that stops at means2d, cannot be double counted.
        v_m2d = None
        if v_means2d is not None:
            v_m2d = (v_means2d.reshape(C * N, 2) + v_splats[:, 0:2]).reshape(C, N, 2).contiguous()
        v_dep = v_depths.reshape(C, N).contiguous() if v_depths is not None else None
        v_con = v_conics.reshape(C, N, 3).contiguous() if v_conics is not None else None
        v_cmp = v_comp.reshape(C, N).contiguous() if (v_comp is not None and cfg.antialiased) else None
        self.cots = (v_m2d, v_dep, v_con, v_cmp)
        # the camera pose (gsplat's viewmats.grad; the pose a camera optimiser trains): one [4,4] per camera from the pose twin of the
        # kernel, never summed over cameras and never all-reduced.  Not asked for: exactly the plain launch.
        self.v_viewmat = torch.empty(C, 4, 4, dtype=torch.float32, device=dev) if ctx.needs_input_grad[8] else None
        self.pose_rows = (torch.empty(_lib.lib().dnsplat_pose_partial_rows(N), 16, dtype=torch.float32, device=dev)
                          if self.v_viewmat is not None else None)
        self.fwd = ProjOut()
        self.fwd.with_depth_channel = int(cfg.with_depth)
        self.fwd.with_normal_channels = int(cfg.with_normals)

    def mode(self):
        """The mode every camera of this call runs in, as the bound method that launches one camera."""
        # The exchange and the tracked zero rows apply only to the model's own split layout (features_dc / features_rest are the leaf
        # parameters dp.allreduce_gradients rebuilds into, and the rows of the gradient arena), one camera per rank.  With the
        # concatenated gsplat layout the coefficient gradient is an intermediate autograd tensor that nobody could fill in
        # afterwards, so the kernel writes the rows itself.
        self.ex = ex = SH_EXCHANGE
        if self.lay.kind == "split" and self.lay.sh_K == 16 and self.C == 1:
            if ex is not None:
                return self.sliced if getattr(ex, "slices", 1) > 1 else self.factors
            if GRAD_ARENA is not None and GRAD_ARENA.sh_state is not None:
                return self.zero_state
        return self.plain

    def camera(self, c):
        # -> Camera, this camera's rows of radii / v_splats / the cotangents, the unwritten gradient tensors geo + sh
        means, quats, scales, opacities, coeffs, sh0, shN, colors, viewmat, K, normal_frame, radii = self.saved[:12]
        N, bucket = self.N, self.C == 1
        like = _grad_like if bucket else torch.empty_like
        geo = [like(means), like(quats), like(scales), like(opacities)]        # _grad_like: once per tensor, in this order
        sh = self.lay.new_grads(coeffs, sh0, shN, colors, bucket)
        cam = _camera_struct(viewmat[c], K[c], None if normal_frame is None else normal_frame[c], self.cfg)
        cots = tuple(None if t is None else t[c] for t in self.cots)
        return cam, radii[c], self.v_splats[c * N:(c + 1) * N], cots, geo, sh

    def launch(self, c, cam, g):
        scene = self.lay.scene(self.cfg, *self.saved[:8])
        if self.v_viewmat is not None:
            pg = PoseGrads()
            pg.partials, pg.v_viewmat = _ptr(self.pose_rows), _ptr(self.v_viewmat[c])
            _lib.run("dnsplat_project_bwd_pose", _lib.lib().dnsplat_project_bwd_pose, ctypes.byref(scene), ctypes.byref(cam),
                     ctypes.byref(self.fwd), ctypes.byref(g), ctypes.byref(pg), _stream())
        else:
            _lib.run("dnsplat_project_bwd", _lib.lib().dnsplat_project_bwd, ctypes.byref(scene), ctypes.byref(cam), ctypes.byref(self.fwd),
                     ctypes.byref(g), _stream())

    def plain(self, c):
        cam, radii, vs, cots, geo, sh = self.camera(c)
        self.launch(c, cam, _proj_grads(self.lay, radii, vs, cots, geo, sh))
        return geo + sh

    def zero_state(self, c):
        cam, radii, vs, cots, geo, sh = self.camera(c)
        g = _proj_grads(self.lay, radii, vs, cots, geo, sh)
        arena = GRAD_ARENA
        if arena.holds(sh[1]) and arena.holds(sh[2]):
            # the rows land in the flat bucket, whose zero rows are tracked: a Gaussian that is culled again is not re-zeroed
            g.sh_zero_state = _ptr(arena.sh_state)
            g.zero_state_geometry = int(all(arena.holds(t) for t in geo))
        self.launch(c, cam, g)
        return geo + sh

    def factors(self, c):
        # dp.ShFactorExchange: the coefficient-gradient tensors are handed to autograd unwritten; dp.allreduce_gradients fills them.
        # The factors come from their own small kernel so that their all-gather is already under way while the geometry gradients
        # are computed.
        ex = self.ex
        cam, radii, vs, cots, geo, sh = self.camera(c)
        g = _proj_grads(self.lay, radii, vs, cots, geo, sh)
        means, viewmat, splats_fwd = self.saved[0], self.saved[8], self.saved[12]
        N, dev = self.N, means.device
        fac = ex.begin(N, dev, self.cfg.sh_degree, self.lay.sh_K, means=means)
        own = ex.use_own_rows()
        if ex.packed:
            # slabs of visible rows only: header, masks and block offsets from the forward's radii (two small launches),
            # the rows from dnsplat_project_bwd itself
            if ex.scratch is None or ex.scratch.numel() < (N + 63) // 64 or ex.scratch.device != dev:
                ex.scratch = torch.empty((N + 63) // 64, dtype=torch.int32, device=dev)
            _lib.run("dnsplat_visible_index", _lib.lib().dnsplat_visible_index, N, ex.packed_capacity(N), _ptr(radii),
                     _ptr(viewmat[c]), _ptr(fac), _ptr(ex.scratch), _stream())
            g.sh_packed = _ptr(fac)
        elif ex.deferred or own:
            # a captured step (graph.GraphedDpStep): the exchange only starts behind the replay, so nothing is gained by
            # having the slab early — dnsplat_project_bwd writes it from the values it holds anyway (one launch less)
            g.sh_factors = _ptr(fac)
        else:
            _lib.run("dnsplat_sh_factors", _lib.lib().dnsplat_sh_factors, N, _ptr(radii), _ptr(viewmat[c]),
                     _ptr(splats_fwd), _ptr(vs), _ptr(fac), _stream())
            ex.launch()
        if own:
            # this camera's rows as on a single GPU, pre-scaled by 1 / world; the exchange adds the other cameras' shares
            from . import dp as _dp
            g.sh_grad_scale = ex.scale_override if ex.scale_override is not None else _dp.reduction_scale(_dp.world_size(ex.group))
        else:
            g.sh_grads_skip = 1
        self.launch(c, cam, g)
        return geo + sh

    def sliced(self, c):
        # dp.SlicedShExchange: the same entry point on K slices of the Gaussians (every row pointer advanced by g0, N = n_k),
        # each with its own mini slab.  Under capture (record_only) nothing is launched here: the argument structs stay with
        # the exchange, graph.GraphedDpStep issues launch k + all-gather k behind each replay; the geometry gradients are
        # then NOT handed to autograd (None): the launches write the bucket slices, which GraphedDpStep installs as .grad.
        ex = self.ex
        if self.v_viewmat is not None:
            raise _lib.DnsplatError("a camera pose gradient (viewmats / camera_to_world that requires grad) is not supported "
                                    "together with dp.SlicedShExchange: its launches cover slices of the Gaussians; use "
                                    "dp.ShFactorExchange or freeze the pose")
        cam, radii, vs, cots, geo, sh = self.camera(c)
        means = self.saved[0]
        slabs = ex.begin(self.N, means.device, self.cfg.sh_degree, self.lay.sh_K, means=means)
        # what the recorded launches read must stay allocated (graph-pool tensors of the captured backward).  NOT the gradient
        # tensors: they are slices of the bucket, which outlives the step — and autograd adopts a returned gradient as .grad
        # only while nobody else holds it (a second reference here made it clone v_sh0 / v_shN out of the bucket)
        keep = [*self.saved[:4], *self.saved[5:7], *self.saved[8:12], vs, *self.cots, slabs]
        if ex.record_only and (GRAD_ARENA is None or not all(GRAD_ARENA.holds(t) for t in (*geo, sh[1], sh[2]))):
            raise _lib.DnsplatError("the sliced exchange in recorded mode needs the gradients in a dp.GradArena (set_grad_arena) "
                                    "and .grad = None when the captured backward starts")
        launches = []
        for k, rows in enumerate(ex.bounds):
            sc_k = self.lay.scene(self.cfg, *self.saved[:8], rows=rows)
            g_k = _proj_grads(self.lay, radii, vs, cots, geo, sh, rows=rows)
            g_k.sh_factors, g_k.sh_grads_skip = _ptr(slabs[k]), 1
            launches.append((ctypes.byref(sc_k), ctypes.byref(cam), ctypes.byref(self.fwd), ctypes.byref(g_k)))
            keep += [sc_k, g_k]
        keep += [cam, self.fwd]
        if ex.record_only:
            ex.record(launches, keep)
            return [None] * 4 + sh
        # eager: slab k's all-gather is queued right behind launch k, so it travels while slices k+1.. compute
        works = []
        for k, args in enumerate(launches):
            _lib.run("dnsplat_project_bwd", _lib.lib().dnsplat_project_bwd, *args, _stream())
            works.append(ex.gather_slice(k))
        ex.works = works
        return geo + sh


def project(means, quats, scales, opacities, *, coeffs=None, sh0=None, shN=None, colors=None, viewmat, K,
            normal_frame=None, cfg: ProjCfg, saturation_flag: Optional[Tensor] = None, side: Optional[dict] = None):
    """``viewmat`` [4,4] or [C,4,4] (``K``, ``normal_frame`` alike) -> dict(means2d[C,N,2], depths[C,N], conics[C,N,3],
    compensations[C,N] | None, splats[C*N,16], radii[C,N], tiles_per_gauss[C,N], normals_world[C,N,3] | None)"""
    m2d, dep, con, comp, splats, radii, tiles, nworld, tiles_bin, tile_boxes = _ProjectFn.apply(
        means, quats, scales, opacities, coeffs, sh0, shN, colors, viewmat, K, normal_frame, cfg, saturation_flag, side)
    # tiles_per_gauss: gsplat's count (A.3), always.  tiles_bin: what dnsplat_bin_* must be given — the same tensor, or the count
    # over the tight boxes when cfg.tight_tiles (the flag travels WITH the counts: rasterize* take both from here)
    # "was it asked for", not "has it elements": with N == 0 every output is empty and still has to be there
    return dict(means2d=m2d, depths=dep, conics=con, compensations=comp if cfg.antialiased else None, splats=splats,
                radii=radii, tiles_per_gauss=tiles, normals_world=nworld if cfg.want_normals_world else None,
                tiles_bin=tiles_bin if cfg.tight_tiles else tiles, tight_tiles=bool(cfg.tight_tiles), tile_boxes=tile_boxes)


# --------------------------------------------------------------------------------------------------
# stage 2: binning


class Binning:
    """flatten_ids [capacity] int32 (first n_isects valid; entry = camera * N + gaussian), tile_offsets [C*T+1] int32.
    ``n_isects`` is known on return under the "sync" / "capacity" policies; under "deferred" reading it is what waits."""

    def __init__(self, flatten_ids: Tensor, tile_offsets: Tensor, n_isects, tile_width: int, tile_height: int,
                 n_cameras: int = 1, pending: Optional["_PendingCount"] = None, tile_ends: Optional[Tensor] = None,
                 n_dev: Optional[Tensor] = None):
        self.flatten_ids, self.tile_offsets = flatten_ids, tile_offsets
        # tile_ends [C*T] (fused path): the list of tile t is [tile_offsets[t], tile_ends[t]); tile_offsets of EMPTY tiles are then
        # not gsplat's (filled_offsets() gives those)
        self.tile_ends, self._n_dev = tile_ends, n_dev
        self._n, self.pending = n_isects, pending
        self.tile_width, self.tile_height, self.n_cameras = tile_width, tile_height, n_cameras
        # List cells (bin_tiles(cells=)): the lists above are per cell of 2^sx x 2^sy tiles — list_width x list_height of them per
        # camera — and n_isects counts (cell, Gaussian) pairs; the per-tile pair count travels beside it
        self.cells: Optional[Tuple[int, int]] = None
        self.list_width, self.list_height = tile_width, tile_height
        self._n_tile, self._n_tile_dev = None, None
        self.tile_boxes: Optional[Tensor] = None
        self.keep: Optional[dict] = None      # fused pass: the forward's keep masks over these lists ("masks", "stride")

    @property
    def n_isects(self) -> int:
        if self.pending is not None:
            self._n = self.pending.resolve()      # raises (every time) if that frame overflowed: self.pending stays
            self._n_tile = self.pending.n_tile
            self.pending = None
        if self._n is None:                      # "static" policy: nobody has asked yet — read the device scalar (synchronises)
            self._n = int(self._n_dev.item())
            if self._n > self.flatten_ids.numel():
                raise _lib.DnsplatError(f"tile binning: {self._n} intersections exceed the static capacity {self.flatten_ids.numel()}")
        return self._n

    @property
    def n_tile_pairs(self) -> int:
        """What n_isects would be with one list per tile (it is n_isects without list cells)."""
        n = self.n_isects                        # waits for / verifies the frame's counts
        if self.cells is None:
            return n
        if self._n_tile is None:
            self._n_tile = int(self._n_tile_dev.item())
        return self._n_tile

    def filled_offsets(self) -> Tensor:
        """gsplat's isect_offsets [C*T+1]: an empty tile carries the offset of the next non-empty one."""
        if self.tile_ends is None:
            return self.tile_offsets
        # the kernels left n_isects in the entries of the empty tiles: a suffix minimum is the same number
        return torch.flip(torch.cummin(torch.flip(self.tile_offsets, [0]), 0).values, [0])

    @n_isects.setter
    def n_isects(self, v) -> None:
        self._n, self.pending = v, None

    def verify_if_ready(self) -> None:
        if self.pending is not None and self.pending.ready():
            _ = self.n_isects


def bin_tiles(means2d: Tensor, radii: Tensor, depths: Tensor, tiles: Tensor, width: int, height: int,
              tile_size: int, after_emit=None, n_cameras: int = 1, tight_splats: Optional[Tensor] = None,
              defer_ok: bool = False, want_ends: bool = False, tile_boxes: Optional[Tensor] = None,
              cells: Optional[Tuple[int, int]] = None, exact: Optional[int] = None) -> Binning:
    """Stage 2 over ``n_cameras`` stacked projections (inputs flattened to [C*N, ...]).  ``after_emit(binning)`` (optional)
    is called right after the emit/sort kernels are enqueued and BEFORE any host wait, so the caller can queue the
    compositing kernel behind them; in "capacity" mode it is called again if the capacity guess turned out too small.
    ``cells`` = (shift_x, shift_y), with ``tile_boxes``: one list per cell of 2^shift_x x 2^shift_y tiles (dnsplat_bin_cells) — the
    lists, their offsets, the count and every capacity are then in (cell, Gaussian) pairs, and the per-tile pair count is
    ``Binning.n_tile_pairs``.  ``exact``: the count is known (a frame binned before): lists of exactly that size, no host wait,
    no record of it kept."""
    lib = _lib.lib()
    dev = means2d.device
    N = radii.numel()
    tw, th = math.ceil(width / tile_size), math.ceil(height / tile_size)
    if cells is not None and cells == (0, 0):
        cells = None
    lw, lh = (tw, th) if cells is None else (-(-tw >> cells[0]), -(-th >> cells[1]))      # lists per camera: tiles, or cells
    T = lw * lh * n_cameras
    # with cells: (cell pairs, tile pairs), written by one launch and copied to the host together
    n_dev = torch.empty(1 if cells is None else 2, dtype=torch.int64, device=dev)
    n_host = BUFFERS.pinned_i64(dev)
    key = (dev, N, width, height)
    skey = _Buffers._key(dev) + key      # the "static" policy's records are per (device, stream) and frame size
    bc = None
    if cells is not None:
        bc = _lib.BinCells()
        bc.shift_x, bc.shift_y, bc.n_tile_pairs = cells[0], cells[1], _ptr(n_dev[1:])

    prepared_ws = None      # the workspace dnsplat_bin_prepare last ran on in this call

    def prepare(capacity, flatten_ids, host_slot):
        """The arguments for lists of ``capacity`` entries; runs the depth sort unless this call has done so on the same workspace."""
        nonlocal prepared_ws
        nbytes = lib.dnsplat_bin_workspace_bytes(N, capacity, T)
        ws = BUFFERS.workspace(dev, nbytes)
        a = BinArgs()
        a.N, a.n_cameras, a.width, a.height, a.tile_size = N, n_cameras, width, height, tile_size
        a.means2d, a.radii, a.depths, a.tiles_per_gauss = _ptr(means2d), _ptr(radii), _ptr(depths), _ptr(tiles)
        a.isect_capacity = capacity
        a.flatten_ids, a.tile_offsets = _ptr(flatten_ids), _ptr(tile_offsets)
        a.n_isects, a.n_isects_host = _ptr(n_dev), _ptr(host_slot)
        a.workspace, a.workspace_bytes = _ptr(ws), ws.numel()
        # ``tiles`` were counted over the tight boxes (ProjCfg.tight_tiles): the emit kernel rebuilds them from the records
        a.splats, a.tight_tiles = _ptr(tight_splats), int(tight_splats is not None)
        # the fused path keeps its lists to itself: [start, end) per tile instead of gsplat's offsets (no fill launch)
        a.tile_ends, a.skip_offsets_fill = _ptr(tile_ends), int(tile_ends is not None)
        a.tile_boxes = _ptr(tile_boxes)          # the boxes ``tiles`` were counted over, from the same projection
        if exact is None:       # the running maxima of the "static" policy: of the list pairs and, with cells, of the tile pairs beside them
            a.n_isects_max = _ptr(BUFFERS.n_max.get(skey) if cells is None else BUFFERS.n_max_cells.get(skey + cells))
            if bc is not None:
                bc.n_tile_pairs_max = _ptr(BUFFERS.n_max.get(skey))
        # the N-sized front of the workspace has the same layout for every capacity, so a depth sort done earlier in this call
        # stays valid for a later emit as long as the buffer was not re-allocated
        if prepared_ws is None or prepared_ws.data_ptr() != ws.data_ptr():
            # (the timers know the entry points by their names without the suffix)
            if bc is None:
                _lib.run("dnsplat_bin_prepare", lib.dnsplat_bin_prepare, ctypes.byref(a), _stream())
            else:
                _lib.run("dnsplat_bin_prepare", lib.dnsplat_bin_prepare_cells, ctypes.byref(a), ctypes.byref(bc), _stream())
            prepared_ws = ws
        return a

    def enqueue(capacity, n_isects, host_slot=n_host, event=None, pending=None, n_tile=None) -> Binning:
        """Depth sort (unless this call has done it), ``event`` recorded behind it (the count is on its way to ``host_slot`` then),
        emit + tile sort into fresh lists of ``capacity`` entries, ``after_emit``."""
        flatten_ids = torch.empty(max(capacity, 1), dtype=torch.int32, device=dev)
        args = prepare(capacity, flatten_ids, host_slot)
        if event is not None:
            event.record()
        if bc is None:
            _lib.run("dnsplat_bin_emit_sort", lib.dnsplat_bin_emit_sort, ctypes.byref(args), _stream())
        else:
            _lib.run("dnsplat_bin_emit_sort", lib.dnsplat_bin_emit_sort_cells, ctypes.byref(args), ctypes.byref(bc), _stream())
        if pending is not None:
            pending.ring["pending"].append(pending)
        b = Binning(flatten_ids, tile_offsets, n_isects, tw, th, n_cameras, pending=pending, tile_ends=tile_ends, n_dev=n_dev[:1])
        if cells is not None:
            b.cells, b.list_width, b.list_height = cells, lw, lh
            b._n_tile, b._n_tile_dev = n_tile, n_dev[1:]
            b.tile_boxes = tile_boxes       # the compositing kernels read them beside the lists (dnsplat_raster_cells)
        if after_emit is not None:
            after_emit(b)
        return b

    def counts():
        """(list pairs, tile pairs) of the frame from the host words the depth sort's copy filled."""
        n = int(n_host[0])
        return n, (int(n_host[1]) if cells is not None else n)

    tile_offsets = torch.empty(T + 1, dtype=torch.int32, device=dev)
    tile_ends = torch.empty(T, dtype=torch.int32, device=dev) if want_ends else None
    mode = BIN_POLICY["mode"]
    if mode in ("deferred", "static") and not defer_ok:
        mode = "capacity"      # callers that hand n_isects / flatten_ids[:n] straight back (the drop-in calls) gain nothing from deferring
    if exact is not None:
        return enqueue(exact, exact, host_slot=None)
    hint = _capacity_guess(key, cells)
    if mode == "static" and hint:
        # nothing on the host depends on the count (a frame captured into a HIP graph): the capacity is the hint, and the
        # device keeps a running maximum of n_isects that static_overflow() compares with it whenever the caller likes
        if skey not in BUFFERS.n_max:
            BUFFERS.n_max[skey] = torch.zeros(1, dtype=torch.int64, device=dev)
        tile_hint = BUFFERS.capacity_hint[key]
        BUFFERS.static_cap[skey] = min(BUFFERS.static_cap.get(skey, tile_hint), tile_hint)      # the smallest buffers any such frame got
        if cells is not None:
            if skey + cells not in BUFFERS.n_max_cells:
                BUFFERS.n_max_cells[skey + cells] = torch.zeros(1, dtype=torch.int64, device=dev)
            BUFFERS.static_cap_cells[skey + cells] = min(BUFFERS.static_cap_cells.get(skey + cells, hint), hint)
        return enqueue(hint, None, host_slot=None)
    if mode == "deferred" and hint:
        verify_pending_counts(dev)                     # earlier frames whose count has arrived meanwhile (no wait)
        ring, slot, ev = BUFFERS.ring_slot(dev)
        return enqueue(hint, None, host_slot=slot, event=ev, pending=_PendingCount(ring, slot, ev, hint, key, cells))
    if mode == "capacity" and hint:
        ev = torch.cuda.Event()
        b = enqueue(hint, -1, event=ev)
        ev.synchronize()  # waits for the (early) depth sort only; compositing keeps running
        n, n_tile = counts()
        if n <= hint:
            b.n_isects = n
            b._n_tile = n_tile
            _learn_capacity(key, cells, n, n_tile)
            return b
        # guess too small: fall through and redo with the exact size
    else:
        prepare(hint, None, n_host)      # the depth sort alone: the host reads the count before anything is emitted
        torch.cuda.current_stream().synchronize()
        n, n_tile = counts()
    _learn_capacity(key, cells, n, n_tile)
    return enqueue(n, n, n_tile=n_tile)


class _PerTileLists:
    """The per-tile face of a frame binned over list cells: what a ``Binning`` of the same frame without cells would show.  The count
    arrives with the cell count (no sort needed); the lists are sorted when somebody reads them — ``build(n)``: the per-tile tile
    sort of the frame's depths and boxes into lists of exactly n entries, buffers of its own."""

    def __init__(self, cell_binning: Binning, build):
        self._cells, self._build, self._lists = cell_binning, build, None
        self.tile_width, self.tile_height, self.n_cameras = cell_binning.tile_width, cell_binning.tile_height, cell_binning.n_cameras
        self.cells, self.tile_ends = None, None

    pending = property(lambda self: self._cells.pending)
    _n = property(lambda self: self._cells._n_tile)
    _n_dev = property(lambda self: self._cells._n_tile_dev)
    n_isects = property(lambda self: self._cells.n_tile_pairs)
    n_tile_pairs = n_isects

    def _sorted(self) -> Binning:
        if self._lists is None:
            self._lists = self._build(self.n_isects)
        return self._lists

    flatten_ids = property(lambda self: self._sorted().flatten_ids)
    tile_offsets = property(lambda self: self._sorted().tile_offsets)

    def filled_offsets(self) -> Tensor:
        return self._sorted().filled_offsets()

    def verify_if_ready(self) -> None:
        self._cells.verify_if_ready()


class LazyInfo(dict):
    """An ``info`` dict some of whose entries are only computed when read (``lazy``: key -> thunk).  The fused path under the
    "deferred" bin policy uses it for ``n_isects`` / ``flatten_ids[:n_isects]``, which need the intersection count on the
    host: reading them is what waits for it, rendering a frame is not."""

    def __init__(self, eager: dict, lazy: dict):
        super().__init__(eager)
        self._lazy = dict(lazy)
        for k in lazy:
            super().__setitem__(k, None)

    def _force(self, k):
        thunk = self._lazy.pop(k, None)
        if thunk is not None:
            super().__setitem__(k, thunk())

    def __getitem__(self, k):
        self._force(k)
        return super().__getitem__(k)

    def get(self, k, default=None):
        if k in self:
            return self[k]
        return default

    def items(self):
        for k in list(self._lazy):
            self._force(k)
        return super().items()

    def values(self):
        for k in list(self._lazy):
            self._force(k)
        return super().values()

    # dict(info), {**info}, info.copy() and pickling take CPython's dict-merge fast path for a dict subclass whose __iter__ is
    # dict's own, which reads the stored None of an entry nobody has asked for yet.  With __iter__ overridden they go
    # through keys() + __getitem__, i.e. through _force.
    def __iter__(self):
        return iter(list(super().keys()))

    def keys(self):
        return super().keys()          # a view, as for any dict (set operations on it keep working)

    def _forced(self) -> dict:
        for k in list(self._lazy):
            self._force(k)
        return {k: dict.__getitem__(self, k) for k in super().keys()}

    def copy(self):
        return self._forced()

    def __reduce__(self):
        return (dict, (self._forced(),))


def binning_status(b: Binning, n_entries: int) -> int:
    """The tile sort's status word of the frame that produced ``b`` (0 = fine; see dnsplat_bin_status_offset).  Reads the
    workspace of the current stream, i.e. call it before the next frame is binned there; synchronises."""
    ws = BUFFERS.ws.get(_Buffers._key(b.flatten_ids.device))
    if ws is None or b.n_isects <= 0:
        return 0
    off = _lib.lib().dnsplat_bin_status_offset(n_entries, b.flatten_ids.numel())
    return int(ws[off:off + 4].view(torch.int32).item())


def isect_ids(b: Binning, depths: Tensor) -> Tensor:
    """gsplat's 64-bit sorted keys (camera | tile << 32 | depth bits), rebuilt on demand for the info dict."""
    out = torch.empty(max(b.n_isects, 1), dtype=torch.int64, device=depths.device)
    _lib.run("dnsplat_bin_isect_ids", _lib.lib().dnsplat_bin_isect_ids, b.tile_width * b.tile_height, b.n_cameras, _ptr(b.tile_offsets),
             _ptr(b.flatten_ids), _ptr(depths.reshape(-1).contiguous()), _ptr(out), b.n_isects, _stream())
    return out[: b.n_isects]


# --------------------------------------------------------------------------------------------------
# stages 3/4: compositing



# Deterministic gradient scatter (DNSPLAT_DETERMINISTIC=1 / set_deterministic(True); a test / debug mode, about 3x the backward's time
# and 128 B per list entry of scratch): the compositing backward stores the row of every (half tile, splat) in its own slot
# (dnsplat_raster_args.det_partials) and dnsplat_det_reduce adds each Gaussian's rows up in list order in float64 — the same bits in
# every run, where the default path's fp32 atomics land in arrival order ("atomics-vs-deterministic-reduction mode").
DETERMINISTIC = {"on": os.environ.get("DNSPLAT_DETERMINISTIC", "0") == "1"}


def set_deterministic(on: bool) -> None:
    DETERMINISTIC["on"] = bool(on)


def _planes(b: "Binning") -> int:
    """Half tiles that share one list of ``b``: the planes of the keep masks and of the deterministic mode's slot buffer."""
    return 2 if b.cells is None else 2 << (b.cells[0] + b.cells[1])


def _raster_cells(b: "Binning"):
    """dnsplat_raster_cells for the lists of ``b`` (None: one list per tile)."""
    if b.cells is None:
        return None
    c = _lib.RasterCells()
    c.shift_x, c.shift_y = b.cells
    c.tile_boxes = _ptr(b.tile_boxes)       # a tile takes the entries of its cell's list whose own box holds the tile
    return c


def _run_raster(name: str, a: "RasterArgs", b: "Binning") -> None:
    """``name`` over the lists of ``b``: the entry point itself, or its ``_cells`` form where the lists are per cell (the timers and
    traces know both by the name without the suffix)."""
    cells = _raster_cells(b)
    if cells is None:
        _lib.run(name, getattr(_lib.lib(), name), ctypes.byref(a), _stream())
    else:
        _lib.run(name, getattr(_lib.lib(), name + "_cells"), ctypes.byref(a), ctypes.byref(cells), _stream())


def _det_begin(a: "RasterArgs", b: "Binning", dev):
    """Deterministic mode: the zero-filled slot buffer for this launch (None when the mode is off)."""
    if not DETERMINISTIC["on"]:
        return None
    cap = max(int(b.flatten_ids.numel()), 1)
    # one plane per half tile that reads a list: its two halves, or every half tile of a list cell
    part = torch.zeros(_planes(b), cap, RECORD_FLOATS, dtype=torch.float32, device=dev)
    a.det_partials, a.det_capacity = _ptr(part), cap
    return part


def _det_finish(part: Optional[Tensor], b: "Binning", v_splats: Tensor) -> None:
    if part is None:
        return
    dev = v_splats.device
    cap = part.shape[1]
    n_dev = b._n_dev if b._n_dev is not None else torch.tensor([b.n_isects], dtype=torch.int64, device=dev)
    ws = torch.empty(_lib.lib().dnsplat_det_workspace_bytes(cap), dtype=torch.uint8, device=dev)
    d = _lib.DetArgs()
    d.n_records, d.capacity = v_splats.shape[0], cap
    d.n_isects, d.flatten_ids, d.partials, d.v_splats = _ptr(n_dev), _ptr(b.flatten_ids), _ptr(part), _ptr(v_splats)
    d.workspace, d.workspace_bytes = _ptr(ws), ws.numel()
    if part.shape[0] == 2:
        _lib.run("dnsplat_det_reduce", _lib.lib().dnsplat_det_reduce, ctypes.byref(d), _stream())
    else:
        _lib.run("dnsplat_det_reduce", _lib.lib().dnsplat_det_reduce_planes, ctypes.byref(d), part.shape[0], _stream())


def _hand_over_means2d_grad(means2d: Tensor, v_splats: Tensor):
    """gsplat's contract (dn_model.py:517-519): after ``info["means2d"].retain_grad()`` the screen-space gradient is found in
    ``info["means2d"].grad``.  Returning columns 0-1 of the gradient records as means2d's autograd gradient would make the
    retain_grad hook CLONE that strided view (a 13 us copy kernel per frame at 1 M Gaussians) although the projection
    backward reads the same numbers from the records anyway.  So with retain_grad() autograd gets no separate gradient for
    means2d (None: the records carry it) and the view itself is stored in ``.grad`` — added to whatever is already there, as
    the hook would.  WITHOUT retain_grad() the term goes back through autograd as usual, so that torch.autograd.grad(loss,
    info["means2d"]) and hooks registered on the tensor see it: a copy of the columns is returned and the columns themselves
    are cleared, because the projection backward always ADDS what autograd delivers for means2d to the records' columns
    (_ProjectFn.backward) — each term travels exactly one way, whatever else feeds the two tensors.
    Returns the gradient to hand to autograd for ``means2d``."""
    view = v_splats[:, 0:2].view(means2d.shape)
    if not means2d.retains_grad:
        if means2d.requires_grad:
            g = view.clone()
            v_splats[:, 0:2].zero_()
            return g
        return None
    means2d.grad = view if means2d.grad is None else means2d.grad + view
    return None


def _raster_args(C, width, height, tile_size, D, ed_channel, background, splats, flatten_ids, tile_offsets, tile_ends, render, alphas,
                 last_ids) -> RasterArgs:
    """What every compositing launch takes, forward or backward, drop-in or fused; the caller adds what only it has."""
    a = RasterArgs()
    a.n_cameras = C
    a.width, a.height, a.tile_size, a.D = width, height, tile_size, D
    a.splats, a.flatten_ids, a.tile_offsets, a.tile_ends = _ptr(splats), _ptr(flatten_ids), _ptr(tile_offsets), _ptr(tile_ends)
    a.background = _ptr(background)
    a.ed_channel = ed_channel
    a.render, a.alphas, a.last_ids = _ptr(render), _ptr(alphas), _ptr(last_ids)
    return a


def _bin_for(holder, composite, means2d, splats, depths, radii, tiles, width, height, tile_size, C, fused: bool) -> Binning:
    # stage 2 for a compositing node: ``composite(binning)`` is queued right behind the sort (bin_tiles' ``after_emit``).  The fused
    # path keeps its lists to itself: [start, end) per tile, and a count the host need not wait for
    tight = bool(holder is not None and holder.get("tight"))      # ``tiles`` were counted over the tight boxes
    tile_boxes = holder.get("tile_boxes") if holder is not None else None
    # the fused path over tight boxes keeps one list per cell of several tiles (BIN_CELL)
    cells = _cell_shifts(width, height, tile_size) if (fused and tight and tile_boxes is not None) else None
    cells = None if cells == (0, 0) else cells
    m2, rad, dep, til = means2d.detach().reshape(-1, 2), radii.reshape(-1), depths.detach().reshape(-1), tiles.reshape(-1)
    b = bin_tiles(m2, rad, dep, til, width, height, tile_size, after_emit=composite, n_cameras=C,
                  tight_splats=splats.detach() if tight else None, defer_ok=fused, want_ends=fused, tile_boxes=tile_boxes, cells=cells)
    if cells is not None:
        # what ``info`` shows of such a frame stays per tile: the count is on its way with the cell count, the lists are sorted on
        # request — the existing per-tile tile sort over the same depths and boxes, into buffers of its own (the cell lists are the
        # backward's)
        holder["tile_lists"] = _PerTileLists(b, lambda n: bin_tiles(m2, rad, dep, til, width, height, tile_size, n_cameras=C,
                                                                    tile_boxes=tile_boxes, exact=n))
    if holder is not None:
        holder["binning"] = b
    return b


def _tile_boxes_into(holder, tight, tile_boxes):
    """``tiles`` / ``tight`` / ``tile_boxes``: ``tiles_bin``, ``tight_tiles`` and ``tile_boxes`` of the project() result, always taken
    together (the binning walks the boxes the counts were taken over) — they travel to the node in ``holder``."""
    if tight or tile_boxes is not None:
        holder = {} if holder is None else holder
        holder["tight"] = bool(tight)
        holder["tile_boxes"] = tile_boxes          # (first tile, width) per entry, of the same projection as ``tiles``
    return holder


def _composite_bwd(a: RasterArgs, b: Binning, means2d: Tensor, v_splats: Tensor, absgrad: bool, det: bool = True):
    """Launches the compositing backward over ``a``; returns the gradient to hand to autograd for ``means2d``."""
    part = _det_begin(a, b, v_splats.device) if det else None
    _run_raster("dnsplat_raster_bwd", a, b)
    _det_finish(part, b, v_splats)
    if absgrad:
        # gsplat contract (dn_model.py:512, consumed by nerfstudio after_train via self.xys.absgrad)
        means2d.absgrad = v_splats[:, 14:16].reshape(means2d.shape)
    return _hand_over_means2d_grad(means2d, v_splats)


class _RasterFn(torch.autograd.Function):
    """Bins, then composites D channels.  ``means2d`` is an input only so that autograd routes the
    xy-gradient through the tensor dn-splatter calls retain_grad() on (dn_model.py:517-519); the
    kernels read xy from ``splats``."""

    @staticmethod
    def forward(ctx, means2d, splats, depths, radii, tiles, background, width, height, tile_size, D, ed_channel,
                xy_split, absgrad, holder):
        dev = splats.device
        C = means2d.shape[0] if means2d.dim() == 3 else 1      # cameras of the batch: means2d [C,N,2], splats [C*N,16]
        render = torch.empty(C, height, width, D, dtype=torch.float32, device=dev)
        alphas = torch.empty(C, height, width, dtype=torch.float32, device=dev)
        last_ids = torch.empty(C, height, width, dtype=torch.int32, device=dev)
        bg = _f32c(background, "background") if background is not None else None

        def composite(b: Binning):
            a = _raster_args(C, width, height, tile_size, D, ed_channel, bg, splats, b.flatten_ids, b.tile_offsets, None, render, alphas,
                             last_ids)
            _lib.run("dnsplat_raster_fwd", _lib.lib().dnsplat_raster_fwd, ctypes.byref(a), _stream())

        b = _bin_for(holder, composite, means2d, splats, depths, radii, tiles, width, height, tile_size, C, fused=False)
        ctx.save_for_backward(means2d, splats, b.flatten_ids, b.tile_offsets, render, alphas, last_ids)
        ctx.bg = bg
        ctx.binning = b
        ctx.cfg = (width, height, tile_size, D, ed_channel, xy_split, absgrad, C)
        ctx.set_materialize_grads(False)
        return render, alphas

    @staticmethod
    def backward(ctx, v_render, v_alphas):
        means2d, splats, flatten_ids, tile_offsets, render, alphas, last_ids = ctx.saved_tensors
        width, height, tile_size, D, ed_channel, xy_split, absgrad, C = ctx.cfg
        N = splats.shape[0]                      # records of the whole batch (cameras x Gaussians)
        dev = splats.device
        v_splats = torch.zeros(N, RECORD_FLOATS, dtype=torch.float32, device=dev)
        if v_render is None and v_alphas is None:
            return (None, v_splats) + (None,) * 12
        if v_render is None:
            v_render = torch.zeros_like(render)
        v_render = v_render.contiguous()
        v_alphas = v_alphas.contiguous() if v_alphas is not None else None
        a = _raster_args(C, width, height, tile_size, D, ed_channel, ctx.bg, splats, flatten_ids, tile_offsets, None, render, alphas, last_ids)
        a.v_render, a.v_alphas, a.xy_split, a.v_splats = _ptr(v_render), _ptr(v_alphas), xy_split, _ptr(v_splats)
        return (_composite_bwd(a, ctx.binning, means2d, v_splats, absgrad), v_splats) + (None,) * 12


def rasterize(means2d, splats, depths, radii, tiles, *, background=None, width, height, tile_size=16, D,
              ed_channel=-1, xy_split=None, absgrad=False, holder=None, tight=False, tile_boxes=None):
    """-> render [C,H,W,D], alphas [C,H,W] for the C cameras of ``means2d`` [C,N,2] / ``splats`` [C*N,16]."""
    holder = _tile_boxes_into(holder, tight, tile_boxes)
    if tile_size != 16:
        raise NotImplementedError("libdnsplat composites 16x16 tiles (dn_model.py:470-472 uses BLOCK_WIDTH = 16)")
    if xy_split is None:
        xy_split = D
    render, alphas = _RasterFn.apply(means2d, splats, depths, radii, tiles, background, width, height, tile_size, D,
                                     ed_channel, xy_split, absgrad, holder)
    return render, alphas


# The fused pass hands the forward's per-half-tile rectangle-test results to the backward (dnsplat_raster_args.keep_masks);
# DNSPLAT_KEEP_MASKS=0 makes the backward re-derive them (kernel A/B runs).
KEEP_MASKS = os.environ.get("DNSPLAT_KEEP_MASKS", "1") != "0"
# The fused get_outputs path keeps its tile lists to itself, so it bins over the tight tile boxes (dnsplat_camera.tight_tiles:
# ~1/3 fewer intersections on the benchmark scenes, same images and gradients).  DNSPLAT_TIGHT_TILES=0 (or setting this to
# False) makes it use gsplat's boxes, as the drop-in calls always do.
TIGHT_TILES = os.environ.get("DNSPLAT_TIGHT_TILES", "1") != "0"
# With tight tiles the fused path keeps ONE LIST PER CELL of several tiles (dnsplat_bin_cells): its compositing
# kernels re-test every list entry against their own half tile anyway, and the tile sort then handles a Gaussian once per cell.
# DNSPLAT_BIN_CELL=WxH (tiles; one of BIN_CELL_SHAPES) or set_bin_cell() picks the cell; 1x1 is one list per tile, the path without cells.
BIN_CELL_SHAPES = {"1x1": (0, 0), "2x1": (1, 0), "1x2": (0, 1), "2x2": (1, 1), "4x2": (2, 1)}
# Left to itself the path takes 2x2 cells from BIN_CELL_MIN_TILES tiles per image on: cells shorten the I-sized kernels of the tile sort,
# and a frame of a few hundred tiles has next to nothing of them — its binning is the fixed cost of its launches, while the compositing
# kernels would still stage the longer lists (C1, 256 tiles: profiles/ab_cell_lists.txt).  A shape that was ASKED for holds at every size.
BIN_CELL_MIN_TILES = 1024
BIN_CELL = {"shifts": (1, 1), "forced": False}


def set_bin_cell(shape: Optional[str]) -> None:
    """``shape``: one of BIN_CELL_SHAPES, at every frame size; None: 2x2 where it pays (BIN_CELL_MIN_TILES)."""
    if shape is None:
        BIN_CELL.update(shifts=(1, 1), forced=False)
        return
    if shape not in BIN_CELL_SHAPES:
        raise ValueError(f"DNSPLAT_BIN_CELL: {shape!r} is not one of {sorted(BIN_CELL_SHAPES)}")
    BIN_CELL.update(shifts=BIN_CELL_SHAPES[shape], forced=True)


def _cell_shifts(width: int, height: int, tile_size: int) -> Tuple[int, int]:
    if not BIN_CELL["forced"] and math.ceil(width / tile_size) * math.ceil(height / tile_size) < BIN_CELL_MIN_TILES:
        return (0, 0)
    return BIN_CELL["shifts"]


set_bin_cell(os.environ.get("DNSPLAT_BIN_CELL"))
# dnsplat_raster_args.saturation_flag for the fused path's backward (DNSPLAT_SATURATION_FLAG=0: always the clamping loop)
SATURATION_FLAG = os.environ.get("DNSPLAT_SATURATION_FLAG", "1") != "0"
# dnsplat_raster_args.zero_fill: the fused forward clears the gradient records its backward accumulates into
FORWARD_ZERO_FILL = os.environ.get("DNSPLAT_FORWARD_ZERO_FILL", "1") != "0"
# dnsplat_proj_out.skip_culled_records for the fused path (its records never leave the library; DNSPLAT_SKIP_CULLED_RECORDS=0: zero-filled)
SKIP_CULLED_RECORDS = os.environ.get("DNSPLAT_SKIP_CULLED_RECORDS", "1") != "0"
# the fused path's projection as two launches, the SH colour half on a side stream beside the binning kernels (ProjCfg.split_colours)
SPLIT_COLOURS = os.environ.get("DNSPLAT_SPLIT_COLOURS", "0") != "0"

# Measurement hook (bench.py's VALU roofline): a uint64 [8] device tensor makes the fused pass run the COUNTING instantiation of
# both compositing kernels, which tally list entries / splats walked / pairs evaluated / pairs blended / slots issued.
PAIR_COUNTERS: Optional[Tensor] = None

_BG7: Dict[torch.device, Tensor] = {}


def _bg7(device) -> Tensor:
    """Kernel-level background of the fused pass: none for rgb | depth, ones for the normal channels (the
    legacy gsplat.rasterize_gaussians default, dn_model.py:564-575 passes no background)."""
    t = _BG7.get(device)
    if t is None:
        t = torch.tensor([0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0], device=device)
        _BG7[device] = t
    return t


class _RasterDnFn(torch.autograd.Function):
    """Bins, composites the 7 fused channels AND applies dn-splatter's per-pixel post-ops in the same
    kernels (``dnsplat_dn_post``): returns the images ``get_outputs`` hands out — rgb, depth (filled),
    normal, accumulation, surface_normal — instead of the raw composite."""

    @staticmethod
    def forward(ctx, means2d, splats, depths, radii, tiles, bg_rgb, width, height, intr, absgrad, holder):
        dev = splats.device
        ctx.saturation_flag = holder.get("saturation_flag") if holder is not None else None
        C = means2d.shape[0]                     # cameras of the batch; intr = [(fx, fy, cx, cy)] * C
        f32 = dict(dtype=torch.float32, device=dev)
        render = torch.empty(C, height, width, 7, **f32)
        alphas = torch.empty(C, height, width, **f32)
        last_ids = torch.empty(C, height, width, dtype=torch.int32, device=dev)
        rgb = torch.empty(C, height, width, 3, **f32)
        depth_raw = torch.empty(C, height, width, **f32)
        normal = torch.empty(C, height, width, 3, **f32)
        # per-camera maximum of the expected depth: zeroed by the frame's camera_prepare launch when it came with the saturation
        # flag, otherwise (and again if the capacity guess forces a re-run) by a fill in composite()
        sat = holder.get("saturation_flag") if holder is not None else None
        depth_max = DEPTH_MAX_OF.pop(sat.data_ptr(), None) if sat is not None else None
        fresh = {"depth_max": depth_max is not None and depth_max.numel() == C}
        if not fresh["depth_max"]:
            depth_max = torch.empty(C, **f32)
        depth_out = torch.empty(C, height, width, 1, **f32)
        surface_normal = torch.empty(C, height, width, 3, **f32)
        bg_rgb = _f32c(bg_rgb, "background")
        bg7 = _bg7(dev)
        dn = DnPost()
        dn.background_rgb, dn.rgb, dn.depth, dn.normal = _ptr(bg_rgb), _ptr(rgb), _ptr(depth_raw), _ptr(normal)
        dn.depth_max = _ptr(depth_max)
        counters = holder.get("pair_counters") if holder is not None else None
        if counters is None:
            counters = PAIR_COUNTERS
        keep = {}
        # gradient records of the backward (atomically accumulated, so they must start at zero): allocated here and cleared by the
        # forward kernel itself when a backward can follow (FORWARD_ZERO_FILL = False: torch.zeros in the backward)
        fill = {"v_splats": torch.empty(splats.shape[0], RECORD_FLOATS, **f32)
                if (FORWARD_ZERO_FILL and ctx.needs_input_grad[1] and counters is None) else None}

        def composite(b: Binning):
            if not fresh["depth_max"]:
                depth_max.zero_()
            fresh["depth_max"] = False
            ready = holder.get("colours_ready") if holder is not None else None
            if ready is not None:          # the projection's colour phase runs on a side stream (ProjCfg.split_colours)
                torch.cuda.current_stream(dev).wait_event(ready)
            a = _raster_args(C, width, height, 16, 7, 3, bg7, splats, b.flatten_ids, b.tile_offsets, b.tile_ends, render, alphas, last_ids)
            if KEEP_MASKS:
                # the forward's rectangle-test ballots, one 64-bit word per (half tile, 64 list entries): the backward takes
                # them instead of re-testing (and re-gathering) every list entry
                stride = (b.flatten_ids.numel() >> 6) + C * b.list_width * b.list_height + 1
                keep["masks"], keep["stride"] = torch.empty(_planes(b) * stride, dtype=torch.int64, device=dev), stride
                a.keep_masks, a.keep_mask_stride = _ptr(keep["masks"]), stride
                b.keep = keep          # (for whoever inspects the lists: which of their entries each half tile kept)
            a.dn, a.pair_counters = ctypes.pointer(dn), _ptr(counters)
            if fill["v_splats"] is not None:      # the backward's accumulation buffer, cleared by this launch on the way
                a.zero_fill, a.zero_fill_bytes = _ptr(fill["v_splats"]), fill["v_splats"].numel() * 4
            _run_raster("dnsplat_raster_fwd", a, b)

        b = _bin_for(holder, composite, means2d, splats, depths, radii, tiles, width, height, 16, C, fused=True)
        for c in range(C):
            fx, fy, cx, cy = intr[c]
            _lib.run("dnsplat_dn_depth_normals", _lib.lib().dnsplat_dn_depth_normals, width, height, fx, fy, cx, cy,
                     _ptr(depth_raw[c]), _ptr(alphas[c]), _ptr(depth_max[c:]), _ptr(depth_out[c]), _ptr(surface_normal[c]), _stream())
        ctx.save_for_backward(means2d, splats, b.flatten_ids, b.tile_offsets, render, alphas, last_ids, bg_rgb)
        ctx.keep = keep
        ctx.binning = b
        ctx.v_splats = fill["v_splats"]
        ctx.cfg = (width, height, absgrad, C, counters)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(surface_normal)
        return rgb, depth_out, normal, alphas.unsqueeze(-1), surface_normal

    @staticmethod
    def backward(ctx, v_rgb, v_depth, v_normal, v_acc, _v_sn):
        means2d, splats, flatten_ids, tile_offsets, render, alphas, last_ids, bg_rgb = ctx.saved_tensors
        width, height, absgrad, C, counters = ctx.cfg
        N = splats.shape[0]
        dev = splats.device
        ctx.binning.verify_if_ready()     # "deferred" bin policy: the frame's count has normally arrived by now (never waits)
        # cleared by the forward launch of this frame; a second backward through the same graph gets a fresh one
        v_splats, ctx.v_splats = ctx.v_splats, None
        if v_splats is None:
            v_splats = torch.zeros(N, RECORD_FLOATS, dtype=torch.float32, device=dev)
        none = (None,) * 9
        if v_rgb is None and v_depth is None and v_normal is None and v_acc is None:
            return (None, v_splats) + none
        z = lambda t, c: torch.zeros(C, height, width, c, dtype=torch.float32, device=dev) if t is None else t.contiguous()  # noqa: E731
        v_rgb, v_depth, v_normal = z(v_rgb, 3), z(v_depth, 1), z(v_normal, 3)
        v_acc = v_acc.contiguous() if v_acc is not None else None
        dn = DnPost()
        dn.background_rgb = _ptr(bg_rgb)
        dn.v_rgb, dn.v_depth, dn.v_normal, dn.v_accumulation = _ptr(v_rgb), _ptr(v_depth), _ptr(v_normal), _ptr(v_acc)
        a = _raster_args(C, width, height, 16, 7, 3, _bg7(dev), splats, flatten_ids, tile_offsets, ctx.binning.tile_ends, render, alphas,
                         last_ids)
        a.xy_split, a.v_splats, a.dn, a.pair_counters = 4, _ptr(v_splats), ctypes.pointer(dn), _ptr(counters)
        if ctx.keep:
            a.keep_masks, a.keep_mask_stride = _ptr(ctx.keep["masks"]), ctx.keep["stride"]
        # "no visible opacity above the alpha cap in this frame" (written by the projection): lets the kernel drop the clamp handling
        a.saturation_flag = _ptr(ctx.saturation_flag) if SATURATION_FLAG else None
        return (_composite_bwd(a, ctx.binning, means2d, v_splats, absgrad, det=counters is None), v_splats) + none


def rasterize_dn(means2d, splats, depths, radii, tiles, *, background_rgb, width, height, intrinsics, absgrad=True,
                 holder=None, tight=False, tile_boxes=None):
    """``intrinsics``: one (fx, fy, cx, cy) per camera of ``means2d`` [C,N,2].
    -> rgb[C,H,W,3], depth[C,H,W,1], normal[C,H,W,3], accumulation[C,H,W,1], surface_normal[C,H,W,3].
    ``holder["pair_counters"]`` (optional uint64 [8] device tensor) switches both compositing kernels to their measurement
    instantiation (bench.py's VALU roofline)."""
    if isinstance(intrinsics[0], (int, float)):
        intrinsics = [tuple(intrinsics)]
    return _RasterDnFn.apply(means2d, splats, depths, radii, tiles, background_rgb, width, height, list(intrinsics), absgrad,
                             _tile_boxes_into(holder, tight, tile_boxes))


def camera_prepare(c2w: Tensor, fx: float, fy: float, cx: float, cy: float, with_normal_frame: bool = True, with_flag: bool = False,
                   n_depth_max: int = 0):
    """One-launch replacement of get_viewmat + intrinsics + normal frame (dn_model.py:475-479, 550-560).
    ``c2w`` [3,4] (or [1,3,4]) on the GPU -> viewmat[4,4], K[3,3], normal_frame[12] | None
    (+ with_flag: a zeroed int32 [1] device word, the frame's opacity-saturation flag for project(..., saturation_flag=);
    n_depth_max > 0: the flag is followed by that many zeroed floats, the per-camera depth maxima of the fused epilogue —
    ``flag.depth_max`` — so that the frame needs no fill launch for either).
    A ``c2w`` that requires grad (a camera optimiser's pose) makes ``viewmat`` an autograd function of it; K and the normal frame
    carry no gradient."""
    c2w = _f32c(c2w.reshape(-1)[:12], "camera_to_worlds")
    dev = c2w.device
    out = torch.empty(16 + 9 + 12, dtype=torch.float32, device=dev)
    viewmat, K, nf = out[:16], out[16:25], out[25:37]
    pose_leaf = c2w.requires_grad and torch.is_grad_enabled()
    if pose_leaf:
        viewmat = torch.empty(16, dtype=torch.float32, device=dev)      # an autograd output of its own, not a view of `out`
    # the words the launch zeroes live in their own buffer: autograd saves viewmat / K, and a later in-place fill of depth_max
    # (a re-run after a capacity overflow) must not touch their version counter
    zeros = torch.empty(1 + n_depth_max, dtype=torch.float32, device=dev) if with_flag else None
    flag = zeros[0:1].view(torch.int32) if with_flag else None
    _lib.run("dnsplat_camera_prepare", _lib.lib().dnsplat_camera_prepare, _ptr(c2w), fx, fy, cx, cy, _ptr(viewmat), _ptr(K),
             _ptr(nf) if with_normal_frame else None, _ptr(flag), 1 + n_depth_max, _stream())
    if with_flag and n_depth_max:
        DEPTH_MAX_OF[flag.data_ptr()] = zeros[1:1 + n_depth_max]
        while len(DEPTH_MAX_OF) > 16:          # prepared cameras nobody rendered (an exception in between): oldest first
            DEPTH_MAX_OF.pop(next(iter(DEPTH_MAX_OF)))
    if pose_leaf:
        viewmat = _ViewmatOfC2wFn.apply(c2w, viewmat)
    res = (viewmat.view(4, 4), K.view(3, 3), (nf if with_normal_frame else None))
    return res + (flag,) if with_flag else res


class _ViewmatOfC2wFn(torch.autograd.Function):
    """Makes the view matrix dnsplat_camera_prepare wrote an autograd function of the pose it was made from (a camera optimiser's
    output): the backward is the chain through nerfstudio's get_viewmat (columns 1, 2 negated, transpose, -R^T T) on twelve
    numbers.  K and the normal frame carry no gradient: the reference takes them from the raw camera (dn_model.py:476, 551, 560)."""

    @staticmethod
    def forward(ctx, c2w, viewmat):
        ctx.save_for_backward(c2w)
        return viewmat.view(16)

    @staticmethod
    def backward(ctx, v_viewmat):
        (c2w,) = ctx.saved_tensors
        c = c2w.view(3, 4)
        vV = v_viewmat.reshape(4, 4)
        R = torch.cat([c[:, :1], -c[:, 1:3]], 1)                       # get_viewmat's flipped rotation, rows k
        g = vV[:3, :3].t() - c[:, 3:4] * vV[:3, 3][None, :]            # viewmat[r][k] = R[k][r], viewmat[r][3] = -sum_k R[k][r] T[k]
        v_T = -(R @ vV[:3, 3])
        return torch.cat([g[:, :1], -g[:, 1:3], v_T[:, None]], 1).reshape(12), None


# zeroed depth_max words that came with a saturation flag (keyed by the flag's address; taken once by _RasterDnFn.forward)
DEPTH_MAX_OF: Dict[int, Tensor] = {}


def camera_prepare_batch(cameras, with_normal_frame: bool = True, with_flag: bool = False):
    """camera_prepare for a list of camera records (``camera_to_worlds`` [1,3,4], fx, fy, cx, cy) ->
    viewmats[C,4,4], Ks[C,3,3], normal_frames[C,12] | None (+ with_flag: ONE zeroed flag word for the whole batch)."""
    parts = [camera_prepare(c.camera_to_worlds, float(c.fx), float(c.fy), float(c.cx), float(c.cy), with_normal_frame,
                            with_flag=(with_flag and i == 0), n_depth_max=(len(cameras) if (with_flag and i == 0) else 0))
             for i, c in enumerate(cameras)]
    vm = torch.stack([p[0] for p in parts])
    K = torch.stack([p[1] for p in parts])
    nf = torch.stack([p[2] for p in parts]) if with_normal_frame else None
    return (vm, K, nf, parts[0][3]) if with_flag else (vm, K, nf)


class _PackFn(torch.autograd.Function):
    """(xys, conics, opacity, colors) -> records; front end of the legacy rasterize_gaussians call."""

    @staticmethod
    def forward(ctx, xys, conics, opacity, colors):
        xys = _f32c(xys, "xys"); conics = _f32c(conics, "conics")
        opacity = _f32c(opacity, "opacity"); colors = _f32c(colors, "colors")
        N, C = colors.shape
        splats = torch.empty(N, RECORD_FLOATS, dtype=torch.float32, device=xys.device)
        _lib.run("dnsplat_pack_splats", _lib.lib().dnsplat_pack_splats, N, _ptr(xys), _ptr(conics), _ptr(opacity.reshape(-1)), _ptr(colors), C,
                                                  _ptr(splats), _stream())
        ctx.C = C
        ctx.oshape = opacity.shape
        return splats

    @staticmethod
    def backward(ctx, v_splats):
        C = ctx.C
        return (v_splats[:, 0:2], v_splats[:, 2:5], v_splats[:, 5].reshape(ctx.oshape), v_splats[:, 6:6 + C])
