"""The per-frame tail of the reference's ``gs-mesh dn`` exporter in plain PyTorch, restated from its behaviour
(dn_splatter/export_mesh.py:50-90 ``pick_indices_at_random`` / ``find_depth_edges``, :351-476 the loop of
``DepthAndNormalMapsPoisson.main``; utils/camera_utils.py:70-210 ``get_colored_points_from_depth``).

Dtype-generic: every function computes in the dtype of the images it is given, so that the same code is the float64 yardstick of
the tests and the float32 baseline of ``tools/pointcloud_timing.py``.  The edge map writes the Laplacian's four taps out: the
reference's conv2d pins its kernel to the image's dtype but multiplies by a float32 ``1.0`` on the way, which a float64 image does
not survive, and a convolution would also carry an infinite reciprocal to the diagonal neighbours as nan (0 x inf).  Pinned to the
reference's own functions by tests/golden/reference_export.npz.  ``export.py`` is the HIP path."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor


def _shifted(t: Tensor, dy: int, dx: int) -> Tensor:
    """t[y + dy, x + dx] with zeros outside the frame ([H,W])."""
    H, W = t.shape
    p = F.pad(t, (1, 1, 1, 1))
    return p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def depth_laplacian(depth: Tensor) -> Tensor:
    """up + down + left + right - 4 r of r = 1 / (depth + 1e-6), zeros outside the frame ([H,W])."""
    r = 1.0 / (depth + 1e-6)
    return _shifted(r, -1, 0) + _shifted(r, 1, 0) + _shifted(r, 0, -1) + _shifted(r, 0, 1) - 4 * r


def dilate(edge: Tensor, itr: int) -> Tensor:
    """bool [H,W]: an edge pixel lies within Chebyshev distance ``itr`` — ``itr`` rounds of a 3 x 3 all-ones convolution and ``> 0``."""
    if itr == 0:
        return edge.clone()
    k = 2 * itr + 1
    return F.max_pool2d(edge[None, None].to(torch.float32), kernel_size=k, stride=1, padding=itr)[0, 0] > 0


def find_depth_edges(depth_im: Tensor, threshold: float = 0.01, dilation_itr: int = 3) -> Tensor:
    """export_mesh.py:58-90: the dilated edge map of a depth image [H,W,1] as 0 / 1 in its dtype, [H,W,1]."""
    depth = depth_im.reshape(depth_im.shape[0], depth_im.shape[1])
    edge = depth_laplacian(depth) > threshold
    return dilate(edge, int(dilation_itr)).to(depth_im.dtype)[..., None]


def pick_indices_at_random(valid_mask: Tensor, samples_per_frame: int) -> Tensor:
    """export_mesh.py:50-55: the flat indices of the nonzero entries, or ``samples_per_frame`` of them drawn by ``torch.randperm`` on
    the CPU generator.  ``nonzero`` and the index upload synchronise with the host."""
    indices = torch.nonzero(torch.ravel(valid_mask))
    if samples_per_frame < len(indices):
        indices = indices[torch.randperm(len(indices))[:samples_per_frame]]
    return torch.ravel(indices)


def camera_points(depths: Tensor, fx: float, fy: float, cx: float, cy: float, img_size: tuple) -> Tensor:
    """[H W, 3] camera-frame points of every pixel, pixel centres at + 0.5 (camera_utils.py:122-131)."""
    W, H = int(img_size[0]), int(img_size[1])
    d = depths.reshape(-1)
    u = (torch.arange(W, device=d.device, dtype=d.dtype) + 0.5)[None, :].expand(H, W).reshape(-1)
    v = (torch.arange(H, device=d.device, dtype=d.dtype) + 0.5)[:, None].expand(H, W).reshape(-1)
    return torch.stack([(u - cx) * d / fx, (v - cy) * d / fy, d], dim=-1)


def get_colored_points_from_depth(depths: Tensor, rgbs: Tensor, c2w: Tensor, fx: float, fy: float, cx: float, cy: float, img_size: tuple,
                                  mask: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """camera_utils.py:175-210: world points and colours of all pixels, or of the pixels an index tensor ``mask`` names."""
    c2w = c2w.to(depths.dtype)
    points = camera_points(depths, fx, fy, cx, cy, img_size) @ torch.linalg.inv(c2w[..., :3, :3]) + c2w[..., :3, 3]
    colors = rgbs.reshape(-1, 3)
    if mask is not None:
        if not torch.is_tensor(mask):
            mask = torch.tensor(mask, device=depths.device)
        return points[mask], colors[mask]
    return points, colors


def world_normals(surface_normal: Tensor, c2w: Tensor) -> Tensor:
    """export_mesh.py:411-426: the [H,W,3] surface-normal image in [0, 1] as world-space unit normals [H W, 3] — 2 s - 1, y and z
    flipped, F.normalize, the camera's rotation."""
    n = (2 * surface_normal.reshape(-1, 3) - 1) @ torch.diag(torch.tensor([1, -1, -1], device=surface_normal.device, dtype=surface_normal.dtype))
    n = F.normalize(n.permute(1, 0), p=2, dim=0)
    return (c2w[:3, :3].to(n.dtype) @ n).permute(1, 0)


def export_c2w(camera_to_worlds: Tensor) -> Tensor:
    """export_mesh.py:370-375: the [3,4] OpenCV camera-to-world of a nerfstudio (OpenGL) pose."""
    c2w = torch.eye(4, dtype=camera_to_worlds.dtype, device=camera_to_worlds.device)
    c2w[:3, :4] = camera_to_worlds.reshape(3, 4)
    c2w = c2w @ torch.diag(torch.tensor([1, -1, -1, 1], device=c2w.device, dtype=c2w.dtype))
    return c2w[:3, :4]


def box_to_world(crop_box, dtype, device) -> Tensor:
    """The 4 x 4 pose of nerfstudio's ``OrientedBox`` (attributes R [3,3], T [3])."""
    Hm = torch.eye(4, dtype=dtype, device=device)
    Hm[:3, :3] = torch.as_tensor(crop_box.R).to(device=device, dtype=dtype)
    Hm[:3, 3] = torch.as_tensor(crop_box.T).to(device=device, dtype=dtype)
    return Hm


def within(crop_box, pts: Tensor) -> Tensor:
    """``OrientedBox.within`` as nerfstudio defines it — restated from memory, nerfstudio is not a dependency: "parity unpinned".
    A point is inside iff every coordinate of inverse(pose) [p; 1] lies strictly between -S / 2 and S / 2."""
    B = torch.linalg.inv(box_to_world(crop_box, pts.dtype, pts.device))
    q = (B[:3, :3] @ pts.T).T + B[:3, 3]
    half = torch.as_tensor(crop_box.S).to(device=pts.device, dtype=pts.dtype) / 2
    return ((q > -half) & (q < half)).all(dim=-1)


def frame_points(outputs, camera, samples_per_frame: int, filter_edges: bool = False, edge_threshold: float = 0.004,
                 edge_dilation_iterations: int = 10, mask: Optional[Tensor] = None, indices: Optional[Tensor] = None, crop_box=None):
    """One trip of the loop at export_mesh.py:360-472 with ``normal_method == "normal_maps"``: (points, normals, colors) of a frame, or
    None where the reference ``continue``s.  ``indices`` replaces the random draw."""
    depth_map = outputs["depth"]
    c2w = export_c2w(camera.camera_to_worlds.to(depth_map.dtype))
    W, H = int(camera.width), int(camera.height)
    if indices is None:
        valid = find_depth_edges(depth_map, edge_threshold, edge_dilation_iterations) < 0.2 if filter_edges else depth_map
        indices = pick_indices_at_random(valid, samples_per_frame)
    if len(indices) == 0:
        return None
    if mask is not None:
        depth_map = depth_map.clone()
        depth_map[~mask.reshape(depth_map.shape).bool()] = 0
    xyzs, rgbs = get_colored_points_from_depth(depth_map, outputs["rgb"], c2w, camera.fx, camera.fy, camera.cx, camera.cy, (W, H), indices)
    normals = world_normals(outputs["surface_normal"], c2w)[indices]
    if crop_box is not None:
        inside = within(crop_box, xyzs)
        if inside.sum() == 0:
            return None
        xyzs, rgbs, normals = xyzs[inside], rgbs[inside], normals[inside]
    return xyzs, normals, rgbs
