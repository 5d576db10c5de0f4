"""Inputs of the AGS-Mesh normal-loss tests (test_ags_reference.py, test_gpu_ags.py) and of the fixture's generator
(golden/make_reference_ags_golden.py): one recipe, so that the GPU tests run on frames of the kind the reference's outputs were
recorded on.

The ground truth is a normal MAP as the dataparser delivers it — unit normals quantised to 8 bits per channel: three planes with
generic (not axis-aligned) normals and a sphere.  In [-1, 1] a component is then (2 k - 255) / 255 with an odd numerator, so every
|component| >= 1 / 255, and the Laplacian of 1 / (n + 1e-6) is flat up to an ulp inside a plane and many thresholds away from 0.01
across a boundary; on the sphere it takes the few values an 8-bit staircase allows.  The tests CHECK that no edge decision of a frame
they use hangs on fp32 rounding (the flagged-decision rule of test_gpu_ags.py) instead of assuming it.  ``surf`` is the ground truth plus 0.08 noise,
renormalised (about half the pixels within 0.1 rad), ``pred`` the ground truth plus 0.2 noise; both on a grid of 2^-13 so that a
fixture can hold them as int16."""
import math

import torch

GRID = 8192.0           # surf and pred are multiples of 1 / GRID: exact in fp32, int16 in a fixture

PLANES = ((0.31, -0.22, 0.92), (-0.45, 0.38, 0.81), (0.12, 0.57, -0.81))      # the third one faces away: negative z components


def _unit(v):
    n = math.sqrt(sum(c * c for c in v))
    return [c / n for c in v]


def gt_normal_image(H, W, col_cut=None, row_cut=None, sphere=True):
    """uint8 [H,W,3] normal map: plane 0 left of ``col_cut``; right of it plane 1 above ``row_cut`` and plane 2 below; a sphere
    of radius min(H, W) / 4 in the middle.  The cuts default to 0.45 W and 0.55 H; a test places them on a tile's edge."""
    col_cut = int(0.45 * W) if col_cut is None else col_cut
    row_cut = int(0.55 * H) if row_cut is None else row_cut
    n = torch.empty(H, W, 3, dtype=torch.float64)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    p0, p1, p2 = (torch.tensor(_unit(p), dtype=torch.float64) for p in PLANES)
    n[:] = p0
    right = xx >= col_cut
    n[right & (yy < row_cut)] = p1
    n[right & (yy >= row_cut)] = p2
    if sphere:
        rad = min(H, W) / 4.0
        dx, dy = (xx - (W - 1) / 2.0) / rad, (yy - (H - 1) / 2.0) / rad
        inside = dx * dx + dy * dy < 1.0
        z = torch.sqrt((1.0 - dx * dx - dy * dy).clamp_min(0.0))
        n[inside] = torch.stack([dx, dy, z], dim=-1)[inside]
    return torch.round((n + 1.0) / 2.0 * 255.0).to(torch.uint8)


def to_chw(image01):
    """(2 * image - 1).permute(2, 0, 1) of an [H,W,3] image in [0, 1] — dn_model.py:721-723."""
    return (2 * image01 - 1).permute(2, 0, 1)


def normal_inputs(H, W, seed=0, surf_noise=0.08, pred_noise=0.2, **scene):
    """(gt uint8 [H,W,3], surf, gt, pred float32 [3,H,W] in [-1, 1]); gt is ``to_chw(gt_u8 / 255)`` in fp32, as the model forms it."""
    g = torch.Generator().manual_seed(1000 * H + W + seed)
    gt_u8 = gt_normal_image(H, W, **scene)
    gt = to_chw(gt_u8.float() / 255.0).contiguous()
    surf = gt + surf_noise * torch.randn(3, H, W, generator=g)
    surf = surf / surf.norm(dim=0, keepdim=True)
    pred = gt + pred_noise * torch.randn(3, H, W, generator=g)
    q = lambda t: (torch.round(t * GRID) / GRID).float().contiguous()      # noqa: E731
    return gt_u8, q(surf), gt, q(pred)


# ---- decisions that fp32 rounding may turn -----------------------------------------------------------------------------------------
# A kernel that evaluates the same fp32 expressions in another order, or compares the dot product with cos 0.1 instead of calling
# arccos, may decide differently from exact arithmetic only where the decided quantity lies within a few roundings of its threshold.
# With u = 2^-24: the five-term sum of fp32 reciprocals is within 4 u sum|terms| of its exact value, the three-term dot product within
# 3 u sum|terms| (+ the rounding of the constant and of arccos near 0.1, below u); the bound used is 8 u, twice that.

U24 = 2.0 ** -24
EDGE_THRESHOLD = 0.01
COS_MAX_ANGLE = math.cos(0.1)
FLAG_CAP = 1e-3          # at most this share of a test frame's decisions may be flagged; none on the fixture's frames


def _taps(t):
    p = torch.nn.functional.pad(t, (1, 1, 1, 1))
    H, W = t.shape[-2], t.shape[-1]
    return [p[..., 1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1))]


def dilate(mask):
    """OR over the 3 x 3 neighbourhood, false outside the frame."""
    m = mask.to(torch.uint8)
    p = torch.nn.functional.pad(m, (1, 1, 1, 1))
    H, W = m.shape[-2], m.shape[-1]
    out = torch.zeros_like(m)
    for dy in range(3):
        for dx in range(3):
            out = out | p[..., dy:dy + H, dx:dx + W]
    return out > 0


def flagged_edge_decisions(gt):
    """bool [3,H,W]: the threshold decisions ``lap > 0.01`` of a float32 [3,H,W] normal map that lie within 8 u sum|terms| of the
    threshold — the Laplacian evaluated in float64 on the reciprocals ROUNDED TO float32 (what every fp32 side starts from)."""
    assert gt.dtype == torch.float32
    r = (1.0 / (gt + 1e-6)).double()
    taps = _taps(r)
    lap = taps[0] + taps[1] + taps[2] + taps[3] - 4 * r
    mag = taps[0].abs() + taps[1].abs() + taps[2].abs() + taps[3].abs() + 4 * r.abs()
    return (lap - EDGE_THRESHOLD).abs() <= 8 * U24 * mag


def flagged_confidence_decisions(surf, gt):
    """bool [H,W]: the decisions ``angle > 0.1`` whose dot product lies within 8 u (sum|terms| + 1) of cos 0.1."""
    prod = gt.double() * surf.double()
    return (prod.sum(dim=0) - COS_MAX_ANGLE).abs() <= 8 * U24 * (prod.abs().sum(dim=0) + 1)


# ---- the fixture tests/golden/reference_ags.npz (golden/make_reference_ags_golden.py) ------------------------------------------------

FIXTURE_FRAMES = ((45, 70), (33, 130))
FIXTURE_STEPS = (100, 7000, 7001, 14999, 15000)


def fixture_frame(g, H, W):
    """One strategy case of the fixture: surf, gt, pred float32 [3,H,W], the reference's dilated edge map bool [3,H,W] and its
    confident pixels bool [H,W]."""
    import numpy as np

    pre = f"f{H}x{W}_"
    gt_u8 = torch.from_numpy(g[pre + "gt_u8"])
    bits = lambda k, shape: torch.from_numpy(np.unpackbits(g[pre + k])[:int(np.prod(shape))].reshape(shape).astype(bool))   # noqa: E731
    return dict(gt_u8=gt_u8, gt=to_chw(gt_u8.float() / 255.0).contiguous(), surf=torch.from_numpy(g[pre + "surf_q"]).float() / GRID,
                pred=torch.from_numpy(g[pre + "pred_q"]).float() / GRID, edges=bits("edges", (3, H, W)),
                confident=bits("confident", (H, W)))


def fixture_result(g, H, W, step):
    """(value, d value / d surf, d value / d pred) of the reference's get_normal_loss at ``step``; the gradients are stored as their
    sign pattern and their one magnitude (weight / count)."""
    pre = f"f{H}x{W}_s{step}_"
    grad = lambda n: torch.from_numpy(g[pre + n + "_sign"]).float() * float(g[pre + n + "_mag"])      # noqa: E731
    return float(g[pre + "value"]), grad("v_surf"), grad("v_pred")
