"""Restatements of the per-frame kernels of csrc/postops.hip that more than one test file compares against."""
import torch
import torch.nn.functional as F

from _scenes import FP32_ENVELOPE

NORMAL_FLOOR = 5e-6      # on the [0, 1] normal image


def _restated_surface_normal(depth, alphas, fx, fy, cx, cy, dtype):
    """dn_model.py:533-537 (alpha == 0: the image-wide maximum depth) and :589-603 through model.normal_from_depth_image."""
    from dn_splatter_amd import model

    H, W = depth.shape
    d = depth.to(dtype)
    filled = torch.where(alphas > 0, d, d.max())
    if dtype == torch.float32:
        n = model.normal_from_depth_image(filled[..., None], fx, fy, cx, cy, (W, H), torch.eye(4, device=depth.device))
    else:                       # the same back-projection (c2w = identity) in float64: normal_from_depth_image computes in float32
        gx = torch.arange(W, dtype=dtype, device=depth.device)[None, :] + 0.5
        gy = torch.arange(H, dtype=dtype, device=depth.device)[:, None] + 0.5
        n = model.pcd_to_normal(torch.stack([(gx - cx) * filled / fx, (gy - cy) * filled / fy, filled], dim=-1))
    n = n @ torch.diag(torch.tensor([1.0, -1.0, -1.0], dtype=dtype, device=depth.device))
    return filled, (1 + n) / 2


def surface_normal_allowance(sn32, sn64):
    """(allowance [H,W,1], e32 [1,1,H,W]) for a float32 normal image against ``sn64``: NORMAL_FLOOR + FP32_ENVELOPE x the float32
    restatement's own worst error over the pixel's 3 x 3 stencil support and its channels.
    The restatement's fp32 error is cancellation in (x +- 1 - cx) d / fx away from the image centre (up to ~5e-5 at fx = 1200).
    The kernel rounds the same products but multiplies by 1 / fx instead of dividing, so at a given entry the two fp32 errors need
    not be alike even where their sizes are: a pixel-by-pixel envelope leaves the kernel ~4x over it at a few thousand entries of a
    1080p frame."""
    e32 = (sn32.double() - sn64).abs().amax(dim=-1)[None, None]
    env = FP32_ENVELOPE * F.max_pool2d(e32, 3, 1, 1)[0, 0][..., None]
    return NORMAL_FLOOR + env, e32
