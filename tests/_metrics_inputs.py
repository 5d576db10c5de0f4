"""Inputs of the evaluation-metric tests (test_metrics_reference.py, test_gpu_metrics.py) and of the fixture's generator
(golden/make_reference_metrics_golden.py): one recipe, so that the GPU tests run on frames of the kind the reference's outputs were
recorded on.

Everything lies on a grid, so that a fixture holds it as integers and every side starts from the same float32 bits: the sensor depth on
2^-10 (0.2 .. 6.2 m, one block below the tolerance), the predicted depth = the sensor depth x (1 + noise) on the same grid — the noise
wide enough that max(gt / pred, pred / gt) passes all three thresholds — the ground-truth normal and colour as 8-bit images / 255 (what a
dataparser delivers; the normals face away, so that the dot product of the stored values lies on both sides of the clamp at 1), the predictions on 2^-13 in [0, 1]."""
import torch

DEPTH_GRID = 1024.0
GRID = 8192.0
TOLERANCE = 0.1


def _q(t, grid):
    return (torch.round(t * grid) / grid).float().contiguous()


def frame(H, W, seed=0, identical=False):
    """dict of float32 host tensors: rgb, gt_rgb [H,W,3]; depth, gt_depth [H,W,1]; normal, gt_normal [H,W,3]; and the 8-bit / grid
    integers a fixture stores.  ``identical``: the predictions equal the ground truth (every difference in ONE histogram bin)."""
    g = torch.Generator().manual_seed(7000 * H + W + seed)
    gt_depth = _q(torch.rand(H, W, 1, generator=g) * 6 + 0.2, DEPTH_GRID)
    if H * W > 1:
        gt_depth[H // 4:H // 4 + max(1, H // 8), W // 3:W // 3 + max(1, W // 5)] = 51.0 / DEPTH_GRID          # below the tolerance
    depth = _q(gt_depth * torch.exp(0.35 * torch.randn(H, W, 1, generator=g)), DEPTH_GRID).clamp_min(1.0 / DEPTH_GRID)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    n = torch.stack([torch.sin(xx / 9.0) * 0.6, torch.cos(yy / 7.0) * 0.6, -0.6 * torch.ones_like(xx)], dim=-1)
    n = n / n.norm(dim=-1, keepdim=True)
    gt_normal_u8 = torch.round((n + 1) / 2 * 255).to(torch.uint8)
    gt_normal = gt_normal_u8.float() / 255.0
    normal = _q((gt_normal + 0.05 * torch.randn(H, W, 3, generator=g)).clamp(0, 1), GRID)
    gt_rgb_u8 = torch.randint(0, 256, (H, W, 3), generator=g).to(torch.uint8)
    gt_rgb = gt_rgb_u8.float() / 255.0
    rgb = _q((gt_rgb + 0.1 * torch.randn(H, W, 3, generator=g)).clamp(0, 1), GRID)
    if identical:
        depth, normal, rgb = gt_depth.clone(), gt_normal.clone(), gt_rgb.clone()
    return dict(rgb=rgb, gt_rgb=gt_rgb, depth=depth, gt_depth=gt_depth, normal=normal, gt_normal=gt_normal,
                gt_normal_u8=gt_normal_u8, gt_rgb_u8=gt_rgb_u8)


# ---- the fixture tests/golden/reference_metrics.npz (golden/make_reference_metrics_golden.py) ----------------------------------------

FIXTURE_FRAMES = ((45, 70), (33, 130))          # neither side a multiple of 16


def fixture_frame(g, H, W):
    """depth, gt_depth [H,W,1]; normal, gt_normal [H,W,3] of a stored frame, float32."""
    pre = f"f{H}x{W}_"
    t = lambda k: torch.from_numpy(g[pre + k].astype("int64"))      # noqa: E731
    return dict(depth=(t("depth_q").float() / DEPTH_GRID).reshape(H, W, 1), gt_depth=(t("gt_depth_q").float() / DEPTH_GRID).reshape(H, W, 1),
                normal=(t("normal_q").float() / GRID).reshape(H, W, 3), gt_normal=(t("gt_normal_u8").float() / 255.0).reshape(H, W, 3))


def _f(*v):
    return torch.tensor(v, dtype=torch.float32)


TOL32 = float(torch.tensor(TOLERANCE, dtype=torch.float32))          # 0.1f: NOT above the tolerance (0.1f > 0.1 is false in float32)
NAN, INF = float("nan"), float("inf")

# name -> (pred, gt): the explicit edge vectors of DepthMetrics
DEPTH_EDGES = {
    "zero_prediction": (_f(0.0, 1.0, 2.5, 0.7), _f(1.5, 1.0, 2.0, 0.05)),            # t = inf, rmse_log = inf
    "negative_prediction": (_f(-2.0, 1.0, 2.5, 3.0), _f(1.5, 1.0, 2.0, 2.0)),        # t < 0: inside all thresholds; a nan log term, dropped
    "nan_prediction": (_f(NAN, 1.0, 2.5, 3.0), _f(1.5, 1.0, 2.0, 2.0)),              # t nan: below no threshold; the means are nan
    "nothing_above_tolerance": (_f(1.0, 2.0, 3.0), _f(0.05, 0.0, TOL32)),             # nan everywhere
    "ground_truth_at_tolerance": (_f(1.0, 2.0, 0.3, 0.3), _f(TOL32, 2.5, 0.3, float(torch.nextafter(torch.tensor(TOL32), torch.tensor(1.0))))),      # the float32 above it IS
    "t_exactly_1_25": (_f(1.0, 1.25, 4.0, 1.0, 1.0), _f(1.25, 1.0, 5.0, 1.5625, 1.953125)),     # t == a threshold is not below it
    "only_negative_predictions": (_f(-1.0, -2.0), _f(1.0, 1.0)),                      # nanmean of nothing but nan: nan
}

# name -> (pred, gt) [1,3,H,W]: the explicit edge vectors of NormalMetrics (the median's rank, nan, inf)


def _normal_edge(H, W, seed, poke=None):
    g = torch.Generator().manual_seed(seed)
    gt = _q(torch.rand(1, 3, H, W, generator=g), GRID)
    pred = _q(torch.rand(1, 3, H, W, generator=g), GRID)
    if poke is not None:
        pred.reshape(-1)[poke[0]] = poke[1]
    return pred, gt


NORMAL_EDGES = {
    "even_count": _normal_edge(2, 3, 1),                         # 18 values: the LOWER middle, rank 8
    "odd_count": _normal_edge(3, 3, 2),                          # 27 values: rank 13
    "one_pixel": _normal_edge(1, 1, 3),
    "a_nan_difference": _normal_edge(3, 5, 4, (7, NAN)),         # the median is nan
    "an_inf_difference": _normal_edge(3, 5, 5, (7, INF)),        # inf sorts as a value: the median is finite
    "mostly_inf": _normal_edge(1, 1, 6, (1, INF)),               # 3 values, rank 1 ...
}
NORMAL_EDGES["mostly_inf"][0].reshape(-1)[2] = INF               # ... and two of them inf: the median IS inf
