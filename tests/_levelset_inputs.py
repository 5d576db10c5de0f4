"""Inputs of the level-set tests (test_levelset_reference.py, test_gpu_levelset.py) and of the fixture's generator
(golden/make_reference_levelset_golden.py): one recipe.

``scene``: N Gaussians on a gently curved sheet in front of the camera of ``_export_inputs.camera`` — means on a jittered lattice of
the sheet (so that no two ranks of a pixel's neighbours tie), log-scales around the lattice spacing and anisotropic, rotations off unit
norm, opacity logits of both signs, unit ``normals`` — and a frame of that camera: the depth of the sheet along each pixel's ray
displaced by up to +-2 typical standard deviations, with a hole of zeros, a few negative values, a nan-free mask, and 8-bit colours.
``scene(H, W, N, seed)`` is the same law at another frame size and Gaussian count, for the GPU tests' edge shapes.

``flagged``: the rays whose hit decision fp32 rounding may turn, per level."""
import math

import numpy as np
import torch

import _export_inputs as frames
from _density_inputs import GAP, SWITCH_ENVELOPE, TOL_DENSITY, TOL_SWITCH_EXTRA, random_quats, smallest_rank_gap  # noqa: F401

W_FIX, H_FIX, N_FIX = 48, 40, 3600
SEED = 11
LEVELS = (0.1, 0.3, 0.5)
RANKS = 18                      # ranks 0 .. 17 of every pixel's point enter the gap condition
MAX_FLAGGED = 0.02              # share of the participating rays that may be flagged, per level
GOLDEN = "reference_levelset.npz"
SHEET_DEPTH, SHEET_HALF = 4.0, 2.2

# e_ref: the error of the reference's OWN fp32 outputs against the fp64 restatement on the unflagged hits of the fixture, as the
# generator printed it; test_levelset_reference.py holds the file to these numbers.
#   E_REF_T       the largest |t - t64| / (kappa (T_a - T_{a-1})), kappa = (|D_a| + |D_{a-1}| + L) / |D_a - D_{a-1}| the condition
#                 number of the interpolation
#   E_REF_NORMAL  the largest component error of the analytical normal
# The HIP outputs get 4 x each: the margin _density_inputs.py gives another summation order and another exp.
# Flagged rays of the fixture (levels 0.1 / 0.3 / 0.5), of the participating rays: see FLAGGED_SHARE.
# E_REF_DENSITY: the reference's own 21 densities per ray against the float64 restatement, relative to max(value, 1e-4).  It is above
# _density_inputs.TOL_DENSITY because the sample positions x_j = p + (r_j std) dir are themselves formed in fp32 here (half an ulp of
# |p| ~ 4 against scales of a few 1e-2), where get_density is handed its samples.  The HIP kernel forms x_j - mu_k as
# (p - mu_k) + (r_j std) dir instead, and on the fixture it is held to TOL_DENSITY.
# TOL_DENSITY_DRAWS, for the other draws of the scene's law (the GPU tests' frame sizes and Gaussian counts): TOL_DENSITY was measured
# on get_density's fixture, whose samples lie close to their neighbours.  A ray runs to +-3 std, where a neighbour's term
# o exp(-m^2 / 2) is still above the 1e-4 the error is relative to while m^2 / 2 reaches ln(o / 1e-4) <= 9.2, and a relative error
# delta of m^2 moves the term by (m^2 / 2) delta.  delta is set by the fp32 records of dnsplat_density_pack, which this kernel must
# read: M = R(q / |q|) exp(-s) formed in fp32 carries a few roundings per entry and m^2 twice their relative error.  On the host, the
# kernel's statements with M formed in double and rounded once give 2.2e-06 at most on these draws, with M formed in fp32 4.6e-06 ..
# 7.3e-06, the fixture 3.9e-06 — TOL_DENSITY holds there by its draw, not by the law.  The bound for the draws is therefore the
# reference's own fp32 error on the fixture, without a factor: no draw may be further from the exact densities than the reference is.
E_REF_T = 2.527e-06
E_REF_NORMAL = 4.720e-06
E_REF_DENSITY = 1.258e-05
FLAGGED_SHARE = (0.00061, 0.0, 0.0)
TOL_T = 4 * E_REF_T
TOL_NORMAL = 4 * E_REF_NORMAL
TOL_DENSITY_DRAWS = E_REF_DENSITY


def sheet(x, y):
    """Camera-frame depth of the sheet above (x, y)."""
    return SHEET_DEPTH + 0.06 * x * x - 0.04 * y * y + 0.05 * x * y + 0.1 * torch.sin(1.7 * x)


def camera(H, W):
    c2w, fx, fy, cx, cy = frames.camera(H, W)
    return frames.Cam(c2w, fx, fy, cx, cy, W, H)


def c2w_cv(cam):
    c = cam.camera_to_worlds.reshape(3, 4)
    return torch.cat([c[:, :1], -c[:, 1:3], c[:, 3:]], dim=1)


def gaussians(N, cam, seed):
    """dict of float32 host tensors: means [N,3], scales [N,3] (log), quats [N,4], opacities [N,1] (logit), normals [N,3]."""
    g = torch.Generator().manual_seed(seed)
    side = int(math.ceil(math.sqrt(N)))
    step = 2 * SHEET_HALF / side
    ij = torch.stack(torch.meshgrid(torch.arange(side), torch.arange(side), indexing="ij"), dim=-1).reshape(-1, 2)[:N].double()
    xy = -SHEET_HALF + (ij + 0.5 + 0.7 * (torch.rand(N, 2, generator=g, dtype=torch.float64) - 0.5)) * step
    z = sheet(xy[:, 0], xy[:, 1]) + 0.3 * step * torch.randn(N, generator=g, dtype=torch.float64)
    c = c2w_cv(cam).double()
    means = torch.stack([xy[:, 0], xy[:, 1], z], dim=-1) @ c[:, :3].T + c[:, 3]
    scales = math.log(step) - 0.25 + 0.35 * torch.randn(N, 3, generator=g)
    quats = random_quats(N, g) * (0.5 + torch.rand(N, 1, generator=g))
    opacities = 0.4 + 2.0 * torch.randn(N, 1, generator=g)
    normals = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    return {k: v.float().contiguous() for k, v in dict(means=means, scales=scales, quats=quats, opacities=opacities, normals=normals).items()}, step


def frame(H, W, cam, step, seed, special=True):
    """depth float32 [H,W,1], rgb float32 [H,W,3] (k / 255), mask bool [H,W,1]."""
    g = torch.Generator().manual_seed(seed + 1)
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float64) + 0.5, torch.arange(W, dtype=torch.float64) + 0.5, indexing="ij")
    ax, ay = (u - cam.cx) / cam.fx, (v - cam.cy) / cam.fy
    z = torch.full_like(ax, SHEET_DEPTH)
    for _ in range(8):                                                   # the sheet's depth along the pixel's ray
        z = sheet(ax * z, ay * z)
    depth = z + 2.0 * 0.8 * step * (2 * torch.rand(H, W, generator=g, dtype=torch.float64) - 1)
    rgb = torch.randint(0, 256, (H, W, 3), generator=g).float() / 255.0
    mask = torch.rand(H, W, generator=g) > 0.12
    if special and H >= 8 and W >= 8:
        depth[H // 4:H // 4 + 3, W // 3:W // 3 + 4] = 0.0                # a hole
        depth[H - 3, 1:W:5] = -1.5                                       # negative depths
        mask[H // 2:H // 2 + 2, W // 2:W // 2 + 5] = False
    return dict(depth=depth.float().reshape(H, W, 1), rgb=rgb, mask=mask.reshape(H, W, 1))


def scene(H=H_FIX, W=W_FIX, N=N_FIX, seed=SEED):
    """(Gaussians, frame, camera) of the fixture's law."""
    cam = camera(H, W)
    gp, step = gaussians(N, cam, seed)
    return gp, frame(H, W, cam, step, seed), cam


def flagged(ref64, level_index):
    """bool [P]: the participating rays of the float64 restatement ``ref64`` (torch_levelset.level_rays) whose decisions for level
    ``level_index`` lie within the rounding envelope — any of the 21 densities within TOL_DENSITY (relative to max(D, L)) of the level,
    or a bracketing density whose sum lies within SWITCH_ENVELOPE of the ``>= 1`` switch."""
    D = ref64["densities"]
    L = ref64["levels"][level_index]
    near = ((D - L).abs() <= TOL_DENSITY * torch.maximum(D.abs(), L)).any(dim=-1)
    a = ref64["first_above"][level_index].clamp(min=1)[:, None]
    bracket = torch.cat([ref64["sums"].gather(1, a), ref64["sums"].gather(1, a - 1)], dim=1)
    switch = ((bracket - 1.0).abs() <= SWITCH_ENVELOPE).any(dim=-1) & ~ref64["empty"][level_index]
    return (near | switch) & ref64["part"]


def load_golden(path):
    g = np.load(path)
    gp = {k: torch.from_numpy(g[k]) for k in ("means", "scales", "quats", "opacities", "normals")}
    H, W = (int(x) for x in g["size"])
    fr = dict(depth=torch.from_numpy(g["depth"]).reshape(H, W, 1), rgb=torch.from_numpy(g["rgb_u8"]).float().reshape(H, W, 3) / 255.0,
              mask=torch.from_numpy(np.unpackbits(g["mask"])[:H * W].astype(bool)).reshape(H, W, 1))
    return g, gp, fr, camera(H, W)


def ref_level(g, l, mode):
    """The reference's recorded (points, normals) of level index ``l`` for ``mode`` in ("closest", "analytical"), every hit in raster
    order.  The points are the same in both modes, and the colours are the frame's (the generator checked both)."""
    return torch.from_numpy(g[f"ref_closest_L{l}_points"]), torch.from_numpy(g[f"ref_{mode}_L{l}_normals"])


def reference_decisions(g, l):
    """(empty bool [n], first_above int64 [n]) of the reference for level index ``l`` over the participating rays in raster order: its
    own two comparisons (dn_model.py:1353-1357) on its own recorded float32 densities."""
    D = torch.from_numpy(g["ref_densities"])
    L = torch.tensor(LEVELS[l], dtype=torch.float32)
    first = (D - L > 0).max(dim=-1).indices
    empty = ~(D[:, 0] - L < 0) | (first == 0)
    return empty, first * ~empty
