"""Inputs of the point-cloud export tests (test_export_reference.py, test_gpu_export.py) and of the fixture's generator
(golden/make_reference_export_golden.py): one recipe, so that the GPU tests run on frames of the kind the reference's outputs were
recorded on; the NumPy restatement of the sampler's keyed bijection; the error bounds of the back-projection.

The depth image is a tilted wall with a nearer box in front of it, a narrow bump and a small hole of zero depth (no Gaussian
composited there), quantised to multiples of 2^-10 so that a fixture holds it as uint16.  The inverse-depth Laplacian is then a few
1e-4 on the wall (quantisation noise), a third of a unit across the box's outline and around 1e6 at the hole: no threshold decision
at 0.004 or 0.01 lies within the rounding envelope, which the generator and the tests CHECK (``flagged_edge_decisions``) rather than
assume.  Colours are 8-bit, the surface-normal image holds multiples of 1 / 256 with a one-pixel border of exactly 0.5 — the zero
normals of the depth -> normal stencil's border."""
import math

import numpy as np
import torch

U24 = 2.0 ** -24
DEPTH_GRID = 1024.0
NORMAL_GRID = 256.0

FIXTURE_FRAMES = ((45, 70), (33, 130), (64, 64))                      # H, W
EDGE_SETTINGS = ((0.004, 10), (0.01, 3), (0.004, 0), (0.004, 1))      # threshold, dilation iterations
SAMPLES = 500                                                         # samples_per_frame of the fixture's draws
PICK_SEED = 20240                                                     # torch.manual_seed before the reference's randperm


def depth_image(H, W):
    """float32 [H,W], multiples of 2^-10."""
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    d = 3.0 + 0.011 * xx + 0.007 * yy                                            # the wall
    bx, by = 0.62 * W, 0.36 * H
    d = d - 0.45 * torch.exp(-((xx - bx) ** 2 + (yy - by) ** 2) / (2 * 1.6 ** 2))   # the bump
    y0, y1, x0, x1 = int(0.5 * H), int(0.5 * H) + int(0.4 * H), int(0.15 * W), int(0.15 * W) + int(0.42 * W)
    d[y0:y1, x0:x1] = 1.5 + 0.004 * xx[y0:y1, x0:x1]                              # the box
    d = torch.round(d * DEPTH_GRID) / DEPTH_GRID
    d[2:4, W - 7:W - 4] = 0.0                                                     # the hole
    return d.float()


def frame_inputs(H, W):
    """dict: depth float32 [H,W,1], rgb float32 [H,W,3] (k / 255), surface_normal float32 [H,W,3] (k / 256, border 0.5), mask bool
    [H,W,1], and their integer forms for a fixture."""
    g = torch.Generator().manual_seed(7919 * H + W)
    depth = depth_image(H, W)
    rgb_u8 = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.int64).to(torch.uint8)
    n = torch.nn.functional.normalize(torch.tensor([0.2, -0.3, 0.9]) + 0.35 * torch.randn(H, W, 3, generator=g), dim=-1)
    normal_q = torch.round((n + 1) / 2 * NORMAL_GRID).to(torch.int16)
    normal_q[0], normal_q[-1], normal_q[:, 0], normal_q[:, -1] = 128, 128, 128, 128
    mask = torch.rand(H, W, generator=g) > 0.15
    mask[H // 3:H // 3 + 5, W // 2:W // 2 + 9] = False
    return unpack_inputs(torch.round(depth * DEPTH_GRID).to(torch.int32), rgb_u8, normal_q, mask)


def unpack_inputs(depth_q, rgb_u8, normal_q, mask):
    H, W = depth_q.shape
    return dict(depth_q=depth_q, rgb_u8=rgb_u8, normal_q=normal_q,
                depth=(depth_q.float() / DEPTH_GRID).reshape(H, W, 1), rgb=rgb_u8.float() / 255.0,
                surface_normal=normal_q.float() / NORMAL_GRID, mask=mask.reshape(H, W, 1))


def camera(H, W):
    """(camera_to_worlds float32 [1,3,4] in nerfstudio's convention, fx, fy, cx, cy): a generic rotation, fx != fy, an off-centre
    principal point."""
    a, b, c = 0.4, -0.7, 0.25
    Rx = torch.tensor([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]], dtype=torch.float64)
    Ry = torch.tensor([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]], dtype=torch.float64)
    Rz = torch.tensor([[math.cos(c), -math.sin(c), 0], [math.sin(c), math.cos(c), 0], [0, 0, 1]], dtype=torch.float64)
    c2w = torch.cat([Rz @ Ry @ Rx, torch.tensor([[0.8], [-1.3], [2.1]], dtype=torch.float64)], dim=1)
    return c2w.float()[None], 61.5, 58.25, W / 2 + 0.75, H / 2 - 0.5


class Cam:
    """The fields of ``model.Camera`` that the export reads."""

    def __init__(self, c2w, fx, fy, cx, cy, W, H):
        self.camera_to_worlds, self.fx, self.fy, self.cx, self.cy, self.width, self.height = c2w, fx, fy, cx, cy, W, H


class Box:
    """nerfstudio's OrientedBox attributes."""

    def __init__(self, R, T, S):
        self.R, self.T, self.S = R, T, S


# ---- decisions that fp32 rounding may turn ---------------------------------------------------------------------------------------------


def _taps(r):
    p = torch.nn.functional.pad(r, (1, 1, 1, 1))
    H, W = r.shape
    return [p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1))]


def flagged_edge_decisions(depth, threshold):
    """bool [H,W]: the decisions ``lap > threshold`` of a float32 [H,W] depth image within 16 u sum|taps| of the threshold, the Laplacian
    evaluated in float64 on the reciprocals rounded to float32 (what every fp32 side starts from).  Four additions and the product by
    4 are at most 4 u sum|taps| apart between any two orders of summation; 16 u is four times that."""
    assert depth.dtype == torch.float32 and depth.dim() == 2
    r = (1.0 / (depth + 1e-6)).double()
    t = _taps(r)
    lap = t[0] + t[1] + t[2] + t[3] - 4 * r
    mag = t[0].abs() + t[1].abs() + t[2].abs() + t[3].abs() + 4 * r.abs()
    return ~((lap - threshold).abs() > 16 * U24 * mag)                 # a nan Laplacian (inf - inf) counts as flagged


def chebyshev_dilate(edge, itr):
    """bool [H,W] NumPy: an edge within Chebyshev distance ``itr``, by 2 itr + 1 shifted ORs per axis."""
    e = np.asarray(edge, dtype=bool)
    H, W = e.shape
    rows = np.zeros_like(e)
    for s in range(-itr, itr + 1):
        lo, hi = max(0, s), min(W, W + s)
        if lo < hi:
            rows[:, lo:hi] |= e[:, lo - s:hi - s]
    out = np.zeros_like(e)
    for s in range(-itr, itr + 1):
        lo, hi = max(0, s), min(H, H + s)
        if lo < hi:
            out[lo:hi] |= rows[lo - s:hi - s]
    return out


# ---- the sampler's keyed bijection (include/dnsplat.h), restated in NumPy ------------------------------------------------------------

_M32 = np.uint64(0xFFFFFFFF)
ROUNDS = 4


def mix32(x):
    x = np.asarray(x, dtype=np.uint64) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    return x ^ (x >> np.uint64(16))


def permutation(t, n, seed, rounds=ROUNDS):
    """pi(t) for an array of t < n: the balanced Feistel network on 2 ceil(ceil(log2 n) / 2) bits (at least 2) with cycle walking."""
    bits = int(n - 1).bit_length() if n > 1 else 0
    half = max(1, (bits + 1) // 2)
    mask = np.uint64((1 << half) - 1)
    seed &= 2 ** 64 - 1
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    keys = [mix32(lo ^ mix32((hi + np.uint64(0x9E3779B9) * np.uint64(r + 1)) & _M32)) for r in range(rounds)]
    x = np.array(t, dtype=np.uint64).reshape(-1)
    assert x.size == 0 or int(x.max()) < n
    todo = np.ones(x.shape, dtype=bool)
    while todo.any():
        L, R = x[todo] >> np.uint64(half), x[todo] & mask
        for r in range(rounds):
            L, R = R, L ^ (mix32(R ^ keys[r]) & mask)
        x[todo] = (L << np.uint64(half)) | R
        todo = x >= n
    return x.astype(np.int64)


def sample(valid_flat, k, seed):
    """(indices int64 [m], n, m) the sampler must return for a flat bool validity array."""
    compact = np.flatnonzero(np.asarray(valid_flat).reshape(-1))
    n = int(compact.size)
    m = min(k, n)
    if n <= k:
        return compact.astype(np.int64), n, m
    return compact[permutation(np.arange(k), n, seed)].astype(np.int64), n, m


# ---- error bounds of the back-projection (fp64 yardstick in, per-component bounds out) -------------------------------------------------


def point_bound(depth, c2w_cv, fx, fy, cx, cy, W, indices):
    """8 u (sum_i |p_i| |A_ij| + |t_j|) per component, float64 [m,3]: 2 roundings in p, 3 products, 3 additions."""
    d = depth.reshape(-1).double()[indices]
    u = (indices % W).double() + 0.5
    v = torch.div(indices, W, rounding_mode="floor").double() + 0.5
    p = torch.stack([(u - cx) * d / fx, (v - cy) * d / fy, d], dim=-1)
    A = torch.linalg.inv(c2w_cv[:3, :3].double())
    return 8 * U24 * (p.abs() @ A.abs() + c2w_cv[:3, 3].double().abs())


def normal_bound(normals64, c2w_cv):
    """16 u sum_j |R_ij| |n_j| per component for unit normals [m,3] in the world frame: 13 roundings counted on the path (2 s - 1: 1,
    the squared norm: 5, the root: 1, the quotient: 1, the product with R: 5).  |n_j| is taken in the camera frame: R^T n."""
    R = c2w_cv[:3, :3].double()
    cam = normals64.double() @ R                                       # rows R^T n
    return 16 * U24 * (cam.abs() @ R.abs().T)


# ---- the fixture tests/golden/reference_export.npz -------------------------------------------------------------------------------------


def bits(g, key, shape):
    return torch.from_numpy(np.unpackbits(g[key])[:int(np.prod(shape))].reshape(shape).astype(bool))


def fixture_frame(g, H, W):
    pre = f"f{H}x{W}_"
    f = unpack_inputs(torch.from_numpy(g[pre + "depth_q"].astype(np.int32)), torch.from_numpy(g[pre + "rgb_u8"]),
                      torch.from_numpy(g[pre + "normal_q"]), bits(g, pre + "mask", (H, W)))
    f.update(c2w_gl=torch.from_numpy(g[pre + "c2w_gl"]), c2w_cv=torch.from_numpy(g[pre + "c2w_cv"]),
             intr=tuple(float(x) for x in g[pre + "intr"]), pre=pre)
    return f
