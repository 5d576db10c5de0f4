"""Oriented point clouds from rendered depth and normal maps — the per-frame tail of the reference's ``gs-mesh dn`` exporter
(dn_splatter/export_mesh.py:351-476 ``DepthAndNormalMapsPoisson``) on HIP (``csrc/pointcloud.hip``).

Where the reference runs, per training camera, eleven one-channel ``conv2d`` calls (``find_depth_edges``), a ``nonzero`` + CPU
``randperm`` + index upload (``pick_indices_at_random``), a back-projection of ALL pixels followed by a gather, a normal-map transform
of all pixels followed by the same gather, and a boolean-mask crop — two or three host round trips — this module makes three
entry-point calls that read nothing on the host: ``dnsplat_depth_edge_valid``, ``dnsplat_sample_valid_pixels``,
``dnsplat_backproject_points``.

  * drop-ins with the reference's names and signatures: ``find_depth_edges``, ``pick_indices_at_random``,
    ``get_colored_points_from_depth`` (three names to edit in export_mesh.py);
  * ``OrientedPointCloud``: ``add_frame`` per camera without any host synchronisation, ``finish`` once;
  * ``export_oriented_points``: the whole loop, frames rendered through ``DNSplatterRenderer.get_outputs_batch``.

The sampler is a deliberate departure: the reference draws with ``torch.randperm`` on the CPU generator, which needs the number of
valid pixels on the host; here the same distribution (uniform without replacement) comes from a keyed bijection evaluated on the
device (include/dnsplat.h).  ``add_frame(indices=...)`` takes the reference's own draw.  Open3D, Poisson reconstruction and file
writing are CPU work and stay outside.  ``torch_export`` is the PyTorch restatement.  There is no CPU fallback."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from ._lib import DnsplatError
from ._ops import _backproject_args, _f32c, _need_gpu, _ptr, _stream
from .torch_export import box_to_world, camera_points

EDGE_ROW_TILE = 32          # include/dnsplat.h DNSPLAT_EDGE_ROW_TILE: rows a workgroup of the dilation kernel finishes
EDGE_MAX_DILATION = 64      # DNSPLAT_EDGE_MAX_DILATION
SAMPLE_ROUNDS = 4           # DNSPLAT_SAMPLE_ROUNDS
MAX_PIXELS = 2 ** 31 - 1


def _scratch(width: int, height: int, k: int, device) -> Tensor:
    n = _lib.lib().dnsplat_pointcloud_scratch_bytes(int(width), int(height), int(k))
    if n == 0:
        raise DnsplatError(f"dnsplat point cloud: unsupported frame {width} x {height} with k = {k} (at most 2^31 - 1 pixels, k >= 0)")
    return torch.empty(n // 8, dtype=torch.int64, device=device)


def _image2d(t: Tensor, name: str) -> Tensor:
    if t.dim() == 3 and t.shape[-1] == 1:
        t = t[..., 0]
    if t.dim() != 2:
        raise ValueError(f"{name} must be [H,W] or [H,W,1], got {tuple(t.shape)}")
    return t


def _bytes2d(t: Optional[Tensor], H: int, W: int, name: str) -> Optional[Tensor]:
    """A [H,W] / [H,W,1] bool (or uint8) map as contiguous bytes on the GPU."""
    if t is None:
        return None
    _need_gpu(t, name)
    if t.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"{name} must be bool or uint8, got {t.dtype}")
    if t.numel() != H * W:
        raise ValueError(f"{name} has {t.numel()} entries for a {H} x {W} frame")
    return t.reshape(H, W).contiguous()


def depth_edge_valid(depth: Tensor, threshold: float = 0.01, dilation_itr: int = 3, scratch: Optional[Tensor] = None) -> Tensor:
    """bool [H,W]: ``find_depth_edges(depth, threshold, dilation_itr) < 0.2`` (export_mesh.py:379-386) in two launches."""
    depth = _f32c(_image2d(depth, "depth"), "depth")
    H, W = depth.shape
    if scratch is None:
        scratch = _scratch(W, H, 0, depth.device)
    valid = torch.empty(H, W, dtype=torch.bool, device=depth.device)
    L = _lib.lib()
    _lib.run("dnsplat_depth_edge_valid", L.dnsplat_depth_edge_valid, W, H, _ptr(depth), float(threshold), int(dilation_itr), _ptr(valid),
             _ptr(scratch), _stream())
    return valid


def sample_valid_pixels(valid: Optional[Tensor], depth: Optional[Tensor], k: int, seed: int = 0,
                        scratch: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """``min(k, n)`` of the n valid pixels, uniformly without replacement, n staying on the device: (indices int32 [k], counts int32
    [2] = {n, m}); rows [m, k) of ``indices`` are -1.  ``valid``: bool [H,W], or None — then the pixels with ``!(depth == 0)``, the
    reference's ``nonzero`` of the depth image."""
    if valid is None and depth is None:
        raise ValueError("sample_valid_pixels needs a validity map or a depth image")
    if k < 0:
        raise ValueError(f"k must be >= 0, got {k}")
    if valid is not None:
        valid = _image2d(valid, "valid")
        H, W = valid.shape
        valid = _bytes2d(valid, H, W, "valid")
        dev = valid.device
        depth = None
    else:
        depth = _f32c(_image2d(depth, "depth"), "depth")
        H, W = depth.shape
        dev = depth.device
    if scratch is None:
        scratch = _scratch(W, H, k, dev)
    indices = torch.empty(k, dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    L = _lib.lib()
    _lib.run("dnsplat_sample_valid_pixels", L.dnsplat_sample_valid_pixels, W, H, _ptr(valid), _ptr(depth), int(k), int(seed) & (2 ** 64 - 1),
             _ptr(indices) if k else None, _ptr(counts), _ptr(scratch), _stream())
    return indices, counts


def _export_c2w(camera_to_worlds: Tensor) -> Tensor:
    """``c2w @ diag(1, -1, -1, 1)`` of export_mesh.py:370-375 as a [3,4] tensor: the y and z columns negated, which is what the product
    with a diagonal matrix of ones and minus ones gives exactly.  Creates no tensor from host data."""
    c = camera_to_worlds.reshape(3, 4).float()
    return torch.cat([c[:, :1], -c[:, 1:3], c[:, 3:]], dim=1)


def _xform(c2w_cv: Tensor, device) -> Tensor:
    """[21] floats on ``device``: A = inverse of the rotation (as camera_utils.py:143 forms it), t, R.  A pose that lives on the host
    is inverted there, as the reference's CPU call is; one on the device stays there (``inv_ex``: no error check, no synchronisation)."""
    c2w_cv = c2w_cv.float()
    R = c2w_cv[:3, :3]
    A = torch.linalg.inv(R) if not R.is_cuda else torch.linalg.inv_ex(R)[0]
    return torch.cat([A.reshape(-1), c2w_cv[:3, 3].reshape(-1), R.reshape(-1)]).to(device).contiguous()


def _crop(crop_box, device) -> Optional[Tensor]:
    """[15] floats on ``device``: the world -> box affine B (the inverse of the box's pose) and the half extents S / 2."""
    if crop_box is None:
        return None
    on = torch.as_tensor(crop_box.R).device
    pose = box_to_world(crop_box, torch.float32, on)
    B = torch.linalg.inv(pose) if not pose.is_cuda else torch.linalg.inv_ex(pose)[0]
    half = torch.as_tensor(crop_box.S).to(device=on, dtype=torch.float32).reshape(3) / 2
    return torch.cat([B[:3, :4].reshape(-1), half]).to(device).contiguous()


def _check_append_buffers(points: Tensor, colors: Tensor, normals: Optional[Tensor], state: Tensor) -> None:
    """What ``dnsplat_backproject_points`` and ``dnsplat_level_points`` append to: [capacity,3] buffers of one capacity, the [3] state."""
    for name, buf in (("points", points), ("colors", colors), ("normals", normals)):
        if buf is None:
            continue
        _need_gpu(buf, name)
        if buf.dtype != torch.float32 or buf.dim() != 2 or buf.shape[1] != 3 or not buf.is_contiguous() or buf.shape[0] != points.shape[0]:
            raise ValueError(f"{name} must be a contiguous float32 [capacity,3] buffer")
    if state.dtype != torch.int64 or state.numel() != 3 or not state.is_cuda or not state.is_contiguous():
        raise ValueError("state must be a contiguous int64 [3] tensor on the GPU")


def backproject_points(depth: Tensor, rgb: Tensor, c2w_cv: Tensor, fx: float, fy: float, cx: float, cy: float, *, points: Tensor,
                       colors: Tensor, normals: Optional[Tensor] = None, state: Tensor, surface_normal: Optional[Tensor] = None,
                       mask: Optional[Tensor] = None, indices: Optional[Tensor] = None, counts: Optional[Tensor] = None, crop_box=None,
                       scratch: Optional[Tensor] = None) -> None:
    """Appends the world points, colours and world normals of the pixels ``indices`` names (rows [0, counts[1]) if ``counts`` is given;
    all pixels in raster order without ``indices``) to ``points`` / ``colors`` / ``normals`` [capacity,3] at the device cursor
    ``state[0]`` (``state``: int64 [3] = cursor, overflow, index out of range; the caller zeroes it once).  ``c2w_cv`` is the [3,4]
    OpenCV camera-to-world (``torch_export.export_c2w``).  Three launches, nothing read on the host."""
    depth = _f32c(_image2d(depth, "depth"), "depth")
    H, W = depth.shape
    dev = depth.device
    rgb = _f32c(rgb, "rgb")
    if rgb.numel() != 3 * H * W:
        raise ValueError(f"rgb has {rgb.numel()} entries for a {H} x {W} frame")
    if surface_normal is not None:
        surface_normal = _f32c(surface_normal, "surface_normal")
        if surface_normal.numel() != 3 * H * W:
            raise ValueError(f"surface_normal has {surface_normal.numel()} entries for a {H} x {W} frame")
        if normals is None:
            raise ValueError("a surface-normal image needs a normals buffer")
    mask = _bytes2d(mask, H, W, "mask")
    n_rows = H * W
    if indices is not None:
        _need_gpu(indices, "indices")
        if indices.dim() != 1 or indices.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"indices must be a 1-D int32 or int64 tensor, got {indices.dtype} {tuple(indices.shape)}")
        indices = indices.to(torch.int32).contiguous()
        n_rows = indices.numel()
        if n_rows == 0:
            return
    elif counts is not None:
        raise ValueError("counts without indices")
    _check_append_buffers(points, colors, normals, state)
    if scratch is None:
        scratch = _scratch(W, H, n_rows, dev)
    xform, crop = _xform(c2w_cv, dev), _crop(crop_box, dev)
    a = _backproject_args(W, H, depth, rgb, surface_normal, mask, indices, counts, (float(fx), float(fy), float(cx), float(cy)), xform, crop,
                          points, colors, normals, state, scratch)
    L = _lib.lib()
    _lib.run("dnsplat_backproject_points", L.dnsplat_backproject_points, a, _stream())


# ---- drop-ins with the reference's names and signatures -------------------------------------------------------------------------------


def find_depth_edges(depth_im: Tensor, threshold: float = 0.01, dilation_itr: int = 3) -> Tensor:
    """export_mesh.py:58-90: the dilated edge map of a depth image, 0 / 1 as float, [H,W,1]."""
    return (~depth_edge_valid(depth_im, threshold, dilation_itr)).to(depth_im.dtype)[..., None]


def pick_indices_at_random(valid_mask: Tensor, samples_per_frame: int, seed: int = 0) -> Tensor:
    """export_mesh.py:50-55: int64 flat indices of ``min(samples_per_frame, n)`` of the n nonzero entries of ``valid_mask`` (a bool map,
    or the depth image itself as the reference passes it without edge filtering).  The length of the result is data-dependent, so this
    call — unlike ``OrientedPointCloud.add_frame`` — reads one number back.  The draw is this library's (module docstring), keyed by
    ``seed``."""
    if valid_mask.dtype in (torch.bool, torch.uint8):
        indices, counts = sample_valid_pixels(valid_mask, None, int(samples_per_frame), seed)
    else:
        indices, counts = sample_valid_pixels(None, valid_mask, int(samples_per_frame), seed)
    return indices[:int(counts[1].item())].to(torch.int64)


def get_colored_points_from_depth(depths: Tensor, rgbs: Tensor, c2w: Tensor, fx: float, fy: float, cx: float, cy: float, img_size: tuple,
                                  mask: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """utils/camera_utils.py:175-210: (points, colors) of all pixels, or of the pixels the index tensor ``mask`` names."""
    W, H = int(img_size[0]), int(img_size[1])
    depth = depths.reshape(H, W)
    if mask is not None and not torch.is_tensor(mask):
        mask = torch.tensor(mask, device=depths.device)
    rows = H * W if mask is None else mask.numel()
    points = torch.empty(max(rows, 1), 3, dtype=torch.float32, device=depths.device)
    colors = torch.empty_like(points)
    state = torch.zeros(3, dtype=torch.int64, device=depths.device)
    backproject_points(depth.float(), rgbs.float(), c2w, fx, fy, cx, cy, points=points, colors=colors, state=state,
                       indices=None if mask is None else mask.reshape(-1))
    return points[:rows], colors[:rows]


def density_grad_samples(depth: Tensor, camera, c2w_cv: Tensor) -> Tensor:
    """export_mesh.py:431-441: every pixel of ``depth`` [H,W] back-projected at 0.99 of its depth, [H W, 3] on the device."""
    H, W = depth.shape
    c2w = c2w_cv.to(device=depth.device, dtype=torch.float32)
    A = torch.linalg.inv_ex(c2w[:3, :3])[0]
    return camera_points(depth * 0.99, camera.fx, camera.fy, camera.cx, camera.cy, (W, H)) @ A + c2w[:3, 3]


def density_grad_normal_image(field, depth: Tensor, camera, c2w_cv: Tensor) -> Tensor:
    """The ``density_grad`` branch of the exporter (export_mesh.py:430-457) as an image the back-projection kernel takes in place of
    ``outputs["surface_normal"]``: ``field.density_grad(..., num_closest_gaussians=1)`` at ``density_grad_samples`` (the second-nearest
    Gaussian, as ``knn_sk`` has it), flipped towards the camera, times the camera rotation and diag(1, -1, -1), normalised — the
    vector t the branch computes.  The kernel applies R normalize(diag(1, -1, -1) (2 s - 1)) to a stored s, so the image holds
    s = (diag(1, -1, -1) Rᵀ t + 1) / 2 and the appended normal is t to fp32 rounding.  [H,W,3] float32; the search and the gradient
    run in ``dnsplat_density_eval``, the elementwise frame around them in torch on the device.  No host synchronisation."""
    H, W = depth.shape
    c2w = c2w_cv.to(device=depth.device, dtype=torch.float32)
    R, t = c2w[:3, :3], c2w[:3, 3]
    xyz = density_grad_samples(depth, camera, c2w)
    n = field.density_grad(xyz, num_closest_gaussians=1)
    view = t - xyz
    view = view / view.norm(dim=-1, keepdim=True)
    n = torch.where(((n * view).sum(-1) < 0)[:, None], -n, n)
    flip = torch.cat([torch.ones_like(t[:1]), -torch.ones_like(t[:2])])          # diag(1, -1, -1) without host data
    n = (n @ R) * flip
    n = n / n.norm(dim=-1, keepdim=True)
    return (((n @ R) * flip + 1) / 2).reshape(H, W, 3)


# ---- the exporter's loop ---------------------------------------------------------------------------------------------------------------


class AppendBuffers:
    """What ``OrientedPointCloud`` and ``levelset.LevelSetCloud`` share: ``points``, ``normals`` and ``colors`` [*lead, capacity, 3] on
    the device, their ``state`` int64 [*lead, 3] (per row: cursor, overflow, index out of range), the scratch buffer of the last frame
    size and the read-back of a state row.  ``_ON_CPU``: what the subclass says to a device that is not the GPU."""

    def __init__(self, capacity: int, device, lead: tuple = ()):
        if capacity < 1:
            raise ValueError(f"capacity must be positive, got {capacity}")
        device = torch.device(device)
        if device.type != "cuda":
            raise DnsplatError(f"{type(self).__name__} on {device}: {self._ON_CPU}")
        self.capacity = int(capacity)
        self.points = torch.empty(*lead, self.capacity, 3, dtype=torch.float32, device=device)
        self.normals = torch.empty_like(self.points)
        self.colors = torch.empty_like(self.points)
        self.state = torch.zeros(*lead, 3, dtype=torch.int64, device=device)
        self._scratch_key = None
        self._scratch_buf = None

    def _scratch_for(self, W: int, H: int, k: int) -> Tensor:
        if self._scratch_key != (W, H, k):
            self._scratch_buf = _scratch(W, H, k, self.points.device)
            self._scratch_key = (W, H, k)
        return self._scratch_buf

    @staticmethod
    def _cursor(row, overflow_error: str, bad_error: str) -> int:
        """The cursor of ``row``, a state row read back to the host; raises the error its overflow or bad-index word stands for."""
        cursor, overflow, bad = (int(v) for v in row)
        if overflow or bad:
            raise DnsplatError(overflow_error if overflow else bad_error)
        return cursor


def _without_outliers(cloud, std_ratio: float):
    """The arrays of ``cloud`` (same rows) gathered with the ``ind`` of the statistical outlier filter over the first; an empty cloud
    passes through."""
    from .cloud_filter import remove_statistical_outlier

    if cloud[0].shape[0] == 0:
        return cloud
    ind, _ = remove_statistical_outlier(cloud[0], nb_neighbors=20, std_ratio=std_ratio)
    return tuple(x.index_select(0, ind) for x in cloud)


class OrientedPointCloud(AppendBuffers):
    """Caller-sized buffers of points, normals and colours that ``add_frame`` appends to on the device.

        cloud = OrientedPointCloud(capacity, device)
        for outputs, camera in frames:
            cloud.add_frame(outputs, camera, samples_per_frame=n, filter_edges=True, seed=i)
        points, normals, colors = cloud.finish()

    ``add_frame`` makes no host synchronisation; ``finish`` is the one place that does."""

    _ON_CPU = "the point cloud is built on the GPU through libdnsplat.so (there is no CPU fallback; torch_export is the PyTorch restatement)"

    def add_frame(self, outputs, camera, *, samples_per_frame: int, filter_edges: bool = False, edge_threshold: float = 0.004,
                  edge_dilation_iterations: int = 10, mask: Optional[Tensor] = None, indices: Optional[Tensor] = None, crop_box=None,
                  seed: int = 0, normal_method: str = "normal_maps", field=None) -> None:
        """One trip of the loop at export_mesh.py:360-472 for the ``outputs`` of ``camera`` (a
        ``model.Camera``): pick ``samples_per_frame`` of the valid pixels (off the dilated depth edges if ``filter_edges``, else with a
        nonzero depth), back-project them with ``camera_to_worlds · diag(1, -1, -1, 1)`` (:370-375), take their colours and world
        normals, keep those inside ``crop_box``, append.  ``mask`` (bool [H,W]) zeroes the depth of the pixels outside it AFTER the
        pick, as :391-396 does.  ``indices`` (int tensor) replaces the pick — the way to the reference's own ``randperm`` draw.
        ``crop_box``: anything with nerfstudio's ``OrientedBox`` attributes ``R`` [3,3], ``T`` [3], ``S`` [3]; a point is kept iff every
        coordinate of inverse(pose)·[p; 1] lies strictly inside ±S / 2 — ``OrientedBox.within`` restated from memory (nerfstudio is not
        a dependency): "parity unpinned", like the compositing rules.  Frames that contribute nothing (no valid pixel, nothing inside
        the box) simply append nothing, where the reference ``continue``s.  No host synchronisation.

        ``normal_method="density_grad"`` with ``field`` (a ``density.GaussianDensityField``) takes the normals from the density field
        instead of ``outputs["surface_normal"]`` (:430-457, ``density_grad_normal_image``).  The reference computes exactly this and
        then overwrites it with the rendered normal map at :459, so its two methods export the same normals; here the branch keeps what
        it computed — its documented intent.  The default, ``"normal_maps"``, is unchanged."""
        if normal_method not in ("normal_maps", "density_grad"):
            raise ValueError(f"normal_method must be 'normal_maps' or 'density_grad', got {normal_method!r}")
        if normal_method == "density_grad" and field is None:
            raise ValueError("normal_method='density_grad' needs field=GaussianDensityField(...)")
        if samples_per_frame < 0:
            raise ValueError(f"samples_per_frame must be >= 0, got {samples_per_frame}")
        depth = _f32c(_image2d(outputs["depth"], "depth"), "depth")
        H, W = depth.shape
        if (H, W) != (int(camera.height), int(camera.width)):
            raise ValueError(f"the depth image is {H} x {W}, the camera {int(camera.height)} x {int(camera.width)}")
        counts = None
        if indices is None:
            scratch = self._scratch_for(W, H, int(samples_per_frame))
            valid = depth_edge_valid(depth, edge_threshold, edge_dilation_iterations, scratch) if filter_edges else None
            indices, counts = sample_valid_pixels(valid, depth, int(samples_per_frame), seed, scratch)
        else:
            scratch = self._scratch_for(W, H, int(indices.numel()))
        c2w = _export_c2w(camera.camera_to_worlds)
        surface_normal = outputs["surface_normal"] if normal_method == "normal_maps" else density_grad_normal_image(field, depth, camera, c2w)
        backproject_points(depth, outputs["rgb"], c2w, camera.fx, camera.fy, camera.cx, camera.cy, points=self.points, colors=self.colors,
                           normals=self.normals, state=self.state, surface_normal=surface_normal, mask=mask, indices=indices,
                           counts=counts, crop_box=crop_box, scratch=scratch)

    def finish(self, outlier_removal: bool = False, std_ratio: float = 2.0) -> Tuple[Tensor, Tensor, Tensor]:
        """(points, normals, colors) trimmed to the rows appended so far.  Synchronises; raises ``DnsplatError`` if the buffers were
        too small for what the frames produced or an index lay outside its frame.  ``outlier_removal`` is the exporter's switch
        (export_mesh.py:487-491): the three arrays gathered with the ``ind`` of
        ``cloud_filter.remove_statistical_outlier(points, nb_neighbors=20, std_ratio=std_ratio)``."""
        cursor = self._cursor(self.state.tolist(),
                              f"OrientedPointCloud overflow: the frames produced more than capacity = {self.capacity} points",
                              "OrientedPointCloud: an index passed to add_frame lies outside its frame")
        cloud = self.points[:cursor], self.normals[:cursor], self.colors[:cursor]
        return _without_outliers(cloud, std_ratio) if outlier_removal else cloud


def export_oriented_points(renderer, cameras, total_points: int = 2_000_000, *, filter_edges: bool = False, edge_threshold: float = 0.004,
                           edge_dilation_iterations: int = 10, crop_box=None, masks=None, seed: int = 0, max_batch: int = 8,
                           outlier_removal: bool = False, std_ratio: float = 2.0):
    """The loop of ``DepthAndNormalMapsPoisson.main`` (export_mesh.py:351-476): ``samples_per_frame = (total_points + F) // F`` pixels
    of each of the F ``cameras``, rendered through ``renderer.get_outputs_batch``; frame f draws with seed ``seed + f`` and uses
    ``masks[f]`` if ``masks`` is given.  ``outlier_removal`` / ``std_ratio``: the statistical outlier filter of :487-491 on the finished
    cloud (``OrientedPointCloud.finish``).  Returns (points, normals, colors), [n,3] each, on the device."""
    F_ = len(cameras)
    if F_ == 0:
        raise ValueError("export_oriented_points needs at least one camera")
    if masks is not None and len(masks) != F_:
        raise ValueError(f"{len(masks)} masks for {F_} cameras")
    samples_per_frame = (int(total_points) + F_) // F_
    cloud = OrientedPointCloud(samples_per_frame * F_, cameras[0].camera_to_worlds.device)
    for i in range(0, F_, max_batch):
        chunk = cameras[i:i + max_batch]
        for j, out in enumerate(renderer.get_outputs_batch(chunk, max_batch=max_batch)):
            f = i + j
            cloud.add_frame(out, chunk[j], samples_per_frame=samples_per_frame, filter_edges=filter_edges, edge_threshold=edge_threshold,
                            edge_dilation_iterations=edge_dilation_iterations, mask=None if masks is None else masks[f], crop_box=crop_box,
                            seed=seed + f)
    return cloud.finish(outlier_removal=outlier_removal, std_ratio=std_ratio)
