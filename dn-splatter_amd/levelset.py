"""Level-set surface points — the per-camera hot path of the reference's ``gs-mesh sugar-coarse`` exporter
(dn_splatter/export_mesh.py:514-697 ``LevelSetExtractor``; dn_model.py:1206-1447 ``DNSplatterModel.compute_level_surface_points``, the
SuGaR ray search) on HIP (``csrc/levelset.hip``).

Where the reference back-projects every pixel, runs sklearn's kd-tree on the CPU for 16 neighbours of each, gathers [n,16,3,3]
matrices for 21 samples along every ray in passes of 2 M samples, gathers by boolean mask per surface level and reads the number of
hits on the host for ``random.sample``, this module makes one ``dnsplat_level_rays`` call per frame (one thread per pixel: search,
21 density sums, the scan per level) and, per level, ``dnsplat_sample_valid_pixels`` on the level's validity bytes and
``dnsplat_level_points`` for the selected rows.  Nothing is read on the host.

  * ``level_rays``: the ray search alone (``t_hit``, ``valid``, ``closest`` and, for the tests, ``first_above`` and ``densities``);
  * ``LevelSetCloud``: one fixed-capacity buffer per level, ``add_frame`` per camera without any host synchronisation, ``finish`` once;
  * ``level_surface_points``: one camera, the reference's return shape ``{level: {"points", "normals", "colors"}}``;
  * ``export_level_set_points``: the exporter's loop over cameras, rendered through ``DNSplatterRenderer.get_outputs_batch``;
  * ``install_level_sets(model)``: ``compute_level_surface_points`` with the reference's signature, bound onto a model.

The draw is a deliberate departure, the one ``export.py`` documents: the same distribution (uniform without replacement) from the keyed
bijection of include/dnsplat.h instead of Python's ``random.sample``, which needs the number of hits on the host.  With ``num_samples``
at or above the number of hits every hit is kept, in raster order, as in the reference.  ``torch_levelset`` is the PyTorch restatement
and what ``install_level_sets`` runs for a model on the CPU."""
from __future__ import annotations

import types
from typing import Optional, Sequence

import torch
from torch import Tensor

from . import _lib
from . import torch_levelset
from ._lib import DnsplatError
from ._ops import _f32c, _level_points_args, _level_rays_args, _need_gpu, _stream
from .density import GaussianDensityField, _model_field
from .export import (MAX_PIXELS, AppendBuffers, _bytes2d, _check_append_buffers, _crop, _export_c2w, _image2d, _scratch, _without_outliers,
                     _xform, sample_valid_pixels)
from .torch_density import KNN, SKIP

RANGE_POINTS = 21           # include/dnsplat.h DNSPLAT_LEVEL_RANGE_POINTS
MAX_LEVELS = 8              # DNSPLAT_LEVEL_MAX_LEVELS
MAP_BLOCK, MAP_ROW = 0, 1   # DNSPLAT_LEVEL_MAP_*: a wave takes an 8 x 8 block of pixels / 64 consecutive pixels
LANE_MAP = MAP_BLOCK        # the faster of the two on the MI355X (profiles/level_set.txt)
NORMAL_MODES = {"closest_gaussian": 0, "analytical": 1}      # DNSPLAT_LEVEL_NORMAL_*

_RANGE = {}


def range_table(device) -> Tensor:
    """The 21 floats of ``torch.linspace(-3, 3, 21)`` on ``device``: formed on the host as the reference forms them, copied once."""
    device = torch.device(device)
    if device not in _RANGE:
        _RANGE[device] = torch_levelset.range_table(device)
    return _RANGE[device]


def level_seed(seed: int, level_index: int) -> int:
    """The sampler key of level ``level_index`` of a frame drawn with ``seed``."""
    return (int(seed) + level_index * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)


def _scalar(v):
    return v.item() if torch.is_tensor(v) else v


def _normal_mode(return_normal: str) -> int:
    if return_normal not in NORMAL_MODES:
        raise NotImplementedError(f"return_normal = {return_normal!r}: the reference implements 'closest_gaussian' and 'analytical'")
    return NORMAL_MODES[return_normal]


def _levels(surface_levels) -> tuple:
    levels = tuple(float(L) for L in surface_levels)
    if not 1 <= len(levels) <= MAX_LEVELS:
        raise ValueError(f"between 1 and {MAX_LEVELS} surface levels per call, got {len(levels)}")
    return levels


def _frame(field: GaussianDensityField, depth: Tensor, camera, mask):
    if field.N < KNN + SKIP:
        raise ValueError(f"level sets need at least {KNN + SKIP} Gaussians (knn_sk asks for 17), got {field.N}")
    depth = _f32c(_image2d(depth, "depth"), "depth")
    H, W = depth.shape
    if (H, W) != (int(_scalar(camera.height)), int(_scalar(camera.width))):
        raise ValueError(f"the depth image is {H} x {W}, the camera {int(_scalar(camera.height))} x {int(_scalar(camera.width))}")
    if H * W > MAX_PIXELS:
        raise DnsplatError(f"a frame of {W} x {H} pixels exceeds 2^31 - 1")
    intr = tuple(float(_scalar(getattr(camera, k))) for k in ("fx", "fy", "cx", "cy"))
    xform = _xform(_export_c2w(camera.camera_to_worlds), depth.device)
    return depth, H, W, intr, xform, _bytes2d(mask, H, W, "mask")


def level_rays(field: GaussianDensityField, depth: Tensor, camera, *, mask: Optional[Tensor] = None,
               surface_levels: Sequence[float] = (0.1, 0.3, 0.5), neighbors: Optional[Tensor] = None, lane_map: Optional[int] = None,
               first_above: bool = False, densities: bool = False, frame=None) -> dict:
    """``dnsplat_level_rays`` for one frame: ``t_hit`` float32 [L,P] (nan where empty), ``valid`` bool [L,P], ``closest`` int32 [P] (-1
    where the pixel took no part) and, on request, ``first_above`` int32 [L,P] and ``densities`` float32 [P,21].  ``neighbors``: an
    int32 or int64 [P,16] tensor that replaces the search in the thread.  ``frame``: what ``_frame`` made of (depth, camera, mask) for
    an earlier call on the same frame.  One launch, nothing read on the host."""
    levels = _levels(surface_levels)
    depth, H, W, intr, xform, mask = frame or _frame(field, depth, camera, mask)
    dev, P, nl = depth.device, H * W, len(levels)
    if neighbors is not None:
        _need_gpu(neighbors, "neighbors")
        if neighbors.dtype not in (torch.int32, torch.int64) or tuple(neighbors.shape) != (P, KNN):
            raise TypeError(f"neighbors must be an int32 or int64 [{P},{KNN}] tensor, got {neighbors.dtype} {tuple(neighbors.shape)}")
        neighbors = neighbors.contiguous()
    out = dict(t_hit=torch.empty(nl, P, dtype=torch.float32, device=dev), valid=torch.empty(nl, P, dtype=torch.bool, device=dev),
               closest=torch.empty(P, dtype=torch.int32, device=dev),
               first_above=torch.empty(nl, P, dtype=torch.int32, device=dev) if first_above else None,
               densities=torch.empty(P, RANGE_POINTS, dtype=torch.float32, device=dev) if densities else None)
    a = _level_rays_args(W, H, depth, mask, intr, xform, range_table(dev), field.N, field.index.buffer, field.records, field.scales_log,
                         field.quats, neighbors, levels, LANE_MAP if lane_map is None else int(lane_map), out["t_hit"], out["valid"],
                         out["closest"], out["first_above"], out["densities"])
    L = _lib.lib()
    _lib.run("dnsplat_level_rays", L.dnsplat_level_rays, a, _stream())
    return out


def level_points(field: GaussianDensityField, depth: Tensor, rgb: Tensor, camera, t_hit: Tensor, closest: Tensor, indices: Tensor,
                 counts: Optional[Tensor], *, points: Tensor, colors: Tensor, normals: Tensor, state: Tensor,
                 gauss_normals: Optional[Tensor] = None, mask: Optional[Tensor] = None, return_normal: str = "closest_gaussian",
                 crop_box=None, scratch: Optional[Tensor] = None, frame=None) -> None:
    """``dnsplat_level_points`` for one level: appends point, colour and normal of the pixels ``indices`` names (rows [0, counts[1]) if
    ``counts`` is given) to ``points`` / ``colors`` / ``normals`` [capacity,3] at the device cursor ``state[0]`` (``state``: int64 [3] =
    cursor, overflow, index out of range).  ``t_hit`` [P] is the level's row of ``level_rays``.  Three launches."""
    mode = _normal_mode(return_normal)
    depth, H, W, intr, xform, mask = frame or _frame(field, depth, camera, mask)
    dev = depth.device
    rgb = _f32c(rgb, "rgb")
    if rgb.numel() != 3 * H * W:
        raise ValueError(f"rgb has {rgb.numel()} entries for a {H} x {W} frame")
    if mode == 0:
        if gauss_normals is None:
            raise ValueError("return_normal='closest_gaussian' needs the model's normals parameter")
        gauss_normals = _f32c(gauss_normals.detach(), "normals")
        if tuple(gauss_normals.shape) != (field.N, 3):
            raise ValueError(f"normals must be [{field.N},3], got {tuple(gauss_normals.shape)}")
    _need_gpu(indices, "indices")
    if indices.dim() != 1 or indices.dtype != torch.int32 or not indices.is_contiguous():
        raise TypeError(f"indices must be a contiguous 1-D int32 tensor, got {indices.dtype} {tuple(indices.shape)}")
    if indices.numel() == 0:
        return
    _check_append_buffers(points, colors, normals, state)
    if t_hit.dtype != torch.float32 or t_hit.numel() != H * W or not t_hit.is_contiguous() or closest.dtype != torch.int32 or closest.numel() != H * W:
        raise ValueError("t_hit (float32) and closest (int32) must be the [P] rows of level_rays")
    if scratch is None:
        scratch = _scratch(W, H, indices.numel(), dev)
    a = _level_points_args(W, H, depth, rgb, mask, indices, counts, intr, xform, _crop(crop_box, dev), t_hit, closest, mode, gauss_normals,
                           field.N, field.index.buffer, field.records, points, colors, normals, state, scratch)
    L = _lib.lib()
    _lib.run("dnsplat_level_points", L.dnsplat_level_points, a, _stream())


class LevelSetCloud(AppendBuffers):
    """One caller-sized buffer of points, normals and colours per surface level that ``add_frame`` appends to on the device.

        cloud = LevelSetCloud((0.1, 0.3, 0.5), capacity, device)
        for outputs, camera in frames:
            cloud.add_frame(field, outputs, camera, num_samples=n, normals=model.normals, seed=i)
        result = cloud.finish()                      # {level: {"points", "normals", "colors"}}

    ``add_frame`` makes no host synchronisation; ``finish`` is the one place that does."""

    _ON_CPU = "the cloud is built on the GPU through libdnsplat.so (torch_levelset is the PyTorch restatement)"

    def __init__(self, surface_levels: Sequence[float], capacity: int, device):
        self.levels = _levels(surface_levels)
        super().__init__(capacity, device, lead=(len(self.levels),))      # one row of buffers and one state row per level

    def add_frame(self, field: GaussianDensityField, outputs, camera, *, num_samples: int, normals: Optional[Tensor] = None,
                  mask: Optional[Tensor] = None, return_normal: str = "closest_gaussian", seed: int = 0, crop_box=None,
                  neighbors: Optional[Tensor] = None, lane_map: Optional[int] = None) -> None:
        """``compute_level_surface_points`` for the rendered ``outputs`` (``depth``, ``rgb``) of ``camera``: the ray search of every
        pixel, then per level at most ``num_samples`` of the hits (level l draws with ``level_seed(seed, l)``; every hit in raster order
        if there are no more than that), their points, colours and normals, the ones inside ``crop_box`` appended to the level's
        buffers.  ``mask`` (bool [H,W]): pixels outside it take no part.  No host synchronisation."""
        _normal_mode(return_normal)
        if num_samples < 0:
            raise ValueError(f"num_samples must be >= 0, got {num_samples}")
        frame = _frame(field, outputs["depth"], camera, mask)               # the pose is inverted and sent to the device once per frame
        rays = level_rays(field, outputs["depth"], camera, mask=mask, surface_levels=self.levels, neighbors=neighbors, lane_map=lane_map,
                          frame=frame)
        H, W = _image2d(outputs["depth"], "depth").shape
        k = min(int(num_samples), H * W)
        if k == 0:
            return
        scratch = self._scratch_for(W, H, k)
        for l in range(len(self.levels)):
            indices, counts = sample_valid_pixels(rays["valid"][l].reshape(H, W), None, k, level_seed(seed, l), scratch)
            level_points(field, outputs["depth"], outputs["rgb"], camera, rays["t_hit"][l], rays["closest"], indices, counts,
                         points=self.points[l], colors=self.colors[l], normals=self.normals[l], state=self.state[l], gauss_normals=normals,
                         mask=mask, return_normal=return_normal, crop_box=crop_box, scratch=scratch, frame=frame)

    def finish(self, outlier_removal: bool = False, std_ratio: float = 2.0) -> dict:
        """{level: {"points", "normals", "colors"}} trimmed to the rows appended so far.  Synchronises; raises ``DnsplatError`` if a
        buffer was too small for what the frames produced.  ``outlier_removal`` is the exporter's switch (export_mesh.py:640): per
        level, the three arrays gathered with the ``ind`` of ``cloud_filter.remove_statistical_outlier(points, 20, std_ratio)``."""
        result = {}
        for l, (level, row) in enumerate(zip(self.levels, self.state.tolist())):
            cursor = self._cursor(row, f"LevelSetCloud overflow: level {level} produced more than capacity = {self.capacity} points",
                                  "LevelSetCloud: an index lies outside its frame")
            cloud = self.points[l, :cursor], self.normals[l, :cursor], self.colors[l, :cursor]
            if outlier_removal:
                cloud = _without_outliers(cloud, std_ratio)
            result[level] = {"points": cloud[0], "normals": cloud[1], "colors": cloud[2]}
        return result


def level_surface_points(field: GaussianDensityField, outputs, camera, num_samples: int, *, normals: Optional[Tensor] = None,
                         mask: Optional[Tensor] = None, surface_levels: Sequence[float] = (0.1, 0.3, 0.5),
                         return_normal: str = "closest_gaussian", seed: int = 0, crop_box=None) -> dict:
    """``compute_level_surface_points`` for one camera: {level: {"points", "normals", "colors"}}, the reference's return shape.  The
    lengths are data-dependent, so this call — unlike ``LevelSetCloud.add_frame`` — reads the cursors back once."""
    _normal_mode(return_normal)
    H, W = _image2d(outputs["depth"], "depth").shape
    cloud = LevelSetCloud(surface_levels, max(1, min(int(num_samples), H * W)), outputs["depth"].device)
    cloud.add_frame(field, outputs, camera, num_samples=num_samples, normals=normals, mask=mask, return_normal=return_normal, seed=seed,
                    crop_box=crop_box)
    return cloud.finish()


def export_level_set_points(renderer, cameras, total_points: int = 2_000_000, *, field: Optional[GaussianDensityField] = None,
                            surface_levels: Sequence[float] = (0.1, 0.3, 0.5), return_normal: str = "closest_gaussian", crop_box=None,
                            masks=None, seed: int = 0, max_batch: int = 8, outlier_removal: bool = False, std_ratio: float = 2.0) -> dict:
    """The camera loop of ``LevelSetExtractor.main`` (export_mesh.py:560-620): ``samples_per_frame = (total_points + F) // F`` hits per
    level of each of the F ``cameras``, rendered through ``renderer.get_outputs_batch``; frame f draws with seed ``seed + f`` and uses
    ``masks[f]`` if ``masks`` is given.  ``field`` defaults to a snapshot of ``renderer.gauss_params``.  ``outlier_removal`` /
    ``std_ratio``: the statistical outlier filter of :640 on each level's finished cloud.  Returns {level: {"points", "normals",
    "colors"}} on the device."""
    F_ = len(cameras)
    if F_ == 0:
        raise ValueError("export_level_set_points needs at least one camera")
    if masks is not None and len(masks) != F_:
        raise ValueError(f"{len(masks)} masks for {F_} cameras")
    _normal_mode(return_normal)
    gp = renderer.gauss_params
    if field is None:
        field = GaussianDensityField(gp["means"], gp["scales"], gp["quats"], gp["opacities"])
    samples_per_frame = (int(total_points) + F_) // F_
    cloud = LevelSetCloud(surface_levels, samples_per_frame * F_, cameras[0].camera_to_worlds.device)
    for i in range(0, F_, max_batch):
        chunk = cameras[i:i + max_batch]
        for j, out in enumerate(renderer.get_outputs_batch(chunk, max_batch=max_batch)):
            f = i + j
            cloud.add_frame(field, out, chunk[j], num_samples=samples_per_frame, normals=gp.get("normals"),
                            mask=None if masks is None else masks[f], return_normal=return_normal, seed=seed + f, crop_box=crop_box)
    return cloud.finish(outlier_removal=outlier_removal, std_ratio=std_ratio)


_CALLS = "_dnsplat_level_set_calls"


def install_level_sets(model):
    """Binds ``compute_level_surface_points(camera, num_samples, mask=None, surface_levels=(0.1, 0.3, 0.5),
    return_normal="closest_gaussian")`` — the reference's signature — onto ``model`` (anything with ``means``, ``scales``, ``quats``,
    ``opacities``, ``normals`` and ``get_outputs(camera=...)``).  On the GPU it runs on the ``GaussianDensityField`` snapshot that
    ``install_density`` shares (rebuilt when a parameter changes); for a model on the CPU it runs ``torch_levelset``.  Call c of a
    model draws with seed c.  Returns the names bound."""
    def compute_level_surface_points(self, camera, num_samples, mask=None, surface_levels=(0.1, 0.3, 0.5), return_normal="closest_gaussian"):
        _normal_mode(return_normal)
        outputs = self.get_outputs(camera=camera)
        assert "depth" in outputs
        seed = self.__dict__.get(_CALLS, 0)
        object.__setattr__(self, _CALLS, seed + 1)
        if mask is not None:
            mask = mask.to(outputs["depth"].device)
        if not self.means.is_cuda:
            cam = types.SimpleNamespace(camera_to_worlds=camera.camera_to_worlds, width=int(_scalar(camera.width)),
                                        height=int(_scalar(camera.height)), **{k: float(_scalar(getattr(camera, k))) for k in ("fx", "fy", "cx", "cy")})
            return torch_levelset.level_surface_points(self.means.data, self.scales.data, self.quats.data, self.opacities.data,
                                                       self.normals.data, outputs, cam, num_samples, mask, surface_levels, return_normal, seed)
        return level_surface_points(_model_field(self), outputs, camera, num_samples, normals=self.normals, mask=mask,
                                    surface_levels=surface_levels, return_normal=return_normal, seed=seed)

    object.__setattr__(model, "compute_level_surface_points", types.MethodType(torch.no_grad()(compute_level_surface_points), model))
    return ["compute_level_surface_points"]
