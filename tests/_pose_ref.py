"""fp64 reference of the camera pose gradient of the projection stage, one view matrix PER Gaussian.

The projection + SH colour of ``oracle/dense_ref.py`` (``project`` + ``sh_colors``), restated with an ``[N,4,4]`` stack of view matrices
whose slices are all the same matrix.  The gradient of a raster-level loss with respect to that stack is then every Gaussian's OWN
contribution ``g_n`` to the pose gradient, so that besides the sum ``S = sum_n g_n`` (what a kernel has to produce) the magnitude
``A = sum_n |g_n|`` is known entry by entry: the quantity an fp32 summation error is proportional to.  Pose gradients cancel heavily
(A / |S| in the thousands), so a tolerance relative to the entry or to the matrix' largest entry means nothing; ``k x 2^-24 x A`` does.

tests/test_pose_abi.py holds the helper to autograd through dense_ref itself with a single matrix.
"""
from __future__ import annotations

import torch

from oracle import dense_ref


def project_per_gaussian(means, quats, scales, V, K, W, H, eps2d=0.3, near=0.01, far=1e10, radius_clip=0.0, rotmats=None):
    """dense_ref.project with view matrix V[n] for Gaussian n.  ``rotmats`` [n,3,3]: the Gaussians' rotations, given instead of derived
    from ``quats``."""
    Rv, t = V[:, :3, :3], V[:, :3, 3]
    mean_c = torch.einsum("nij,nj->ni", Rv, means) + t
    Rq = dense_ref.quat_to_rotmat(quats) if rotmats is None else rotmats
    M = Rq * scales[:, None, :]
    covar = M @ M.transpose(1, 2)
    covar_c = Rv @ covar @ Rv.transpose(1, 2)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    x, y, z = mean_c.unbind(-1)
    lim_x = 1.3 * 0.5 * W / fx
    lim_y = 1.3 * 0.5 * H / fy
    rz = 1.0 / z
    tx = z * torch.minimum(lim_x, torch.maximum(-lim_x, x * rz))
    ty = z * torch.minimum(lim_y, torch.maximum(-lim_y, y * rz))
    zero = torch.zeros_like(z)
    J = torch.stack([torch.stack([fx * rz, zero, -fx * tx * rz * rz], -1),
                     torch.stack([zero, fy * rz, -fy * ty * rz * rz], -1)], dim=-2)
    cov2d = J @ covar_c @ J.transpose(1, 2)
    means2d = torch.stack([fx * x * rz + cx, fy * y * rz + cy], -1)
    det_orig = cov2d[:, 0, 0] * cov2d[:, 1, 1] - cov2d[:, 0, 1] * cov2d[:, 1, 0]
    c00 = cov2d[:, 0, 0] + eps2d
    c11 = cov2d[:, 1, 1] + eps2d
    c01 = 0.5 * (cov2d[:, 0, 1] + cov2d[:, 1, 0])
    det = c00 * c11 - c01 * c01
    comp = torch.sqrt(torch.clamp(det_orig / det, min=0.0))
    conics = torch.stack([c11 / det, -c01 / det, c00 / det], -1)
    with torch.no_grad():
        b = 0.5 * (c00 + c11)
        v1 = b + torch.sqrt(torch.clamp(b * b - det, min=0.01))
        radius = torch.ceil(3.0 * torch.sqrt(v1))
        ok = (z >= near) & (z <= far) & (det > 0) & (radius > radius_clip)
        ok &= ~((means2d[:, 0] + radius <= 0) | (means2d[:, 0] - radius >= W)
                | (means2d[:, 1] + radius <= 0) | (means2d[:, 1] - radius >= H))
        radii = torch.where(ok, radius, torch.zeros_like(radius)).to(torch.int32)
    return dict(radii=radii, means2d=means2d, depths=z, conics=conics, compensations=comp, ok=ok)


def stage_outputs(means, quats, scales, opacities, colors, V, K, W, H, sh_degree, antialiased=False, per_gaussian=True, **kw):
    """What the projection stage hands the compositing stage, as functions of the view matrix: means2d, conics, depths, the opacity
    (x compensation when antialiased) and the colours (SH: clamp_min(sum + 0.5, 0) of the visible Gaussians; direct: as given).
    ``per_gaussian``: V is [N,4,4]; otherwise [4,4] and the projection / colours are dense_ref's own functions."""
    if per_gaussian:
        pr = project_per_gaussian(means, quats, scales, V, K, W, H, **kw)
        cam = torch.inverse(V)[:, :3, 3]
    else:
        pr = dense_ref.project(means, quats, scales, V, K, W, H, **kw)
        cam = torch.inverse(V)[:3, 3][None]
    opac = opacities * pr["compensations"] if antialiased else opacities
    if sh_degree is None:
        cols = colors.reshape(means.shape[0], -1)
    else:
        cols = dense_ref.sh_colors(sh_degree, means - cam, colors)
        cols = torch.where((pr["radii"] > 0)[:, None], cols, torch.zeros_like(cols))
        cols = torch.clamp_min(cols + 0.5, 0.0)
    return dict(means2d=pr["means2d"], conics=pr["conics"], depths=pr["depths"], opacities=opac, colors=cols, radii=pr["radii"])


def contract(out, cot, visible=None):
    """sum of <cotangent, output> over the Gaussians ``visible`` (default: the reference's own radii > 0).  ``cot``: dict with any of
    means2d [N,2], conics [N,3], depths [N], opacities [N], colors [N,D]."""
    vis = (out["radii"] > 0) if visible is None else visible
    loss = 0.0
    for k, v in cot.items():
        if v is None:
            continue
        o = out[k]
        m = vis if o.dim() == 1 else vis[:, None]
        loss = loss + (torch.where(m, o, torch.zeros_like(o)) * v).sum()
    return loss


def pose_gradient_terms(means, quats, scales, opacities, colors, viewmat, K, W, H, sh_degree, cot, visible=None, **kw):
    """(S, A): the [4,4] pose gradient sum_n g_n and the magnitude sum_n |g_n| of the loss ``contract(stage_outputs, cot)``; all fp64."""
    N = means.shape[0]
    V = viewmat.detach().double().reshape(1, 4, 4).repeat(N, 1, 1).requires_grad_(True)
    out = stage_outputs(means, quats, scales, opacities, colors, V, K, W, H, sh_degree, per_gaussian=True, **kw)
    (g,) = torch.autograd.grad(contract(out, cot, visible), V)
    return g.sum(0), g.abs().sum(0)
