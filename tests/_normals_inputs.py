"""Inputs of the normal-estimation tests (test_normals_reference.py, test_gpu_normals.py): the smallest clouds at which a part of
csrc/normals.hip can go wrong, each a deterministic function of its name.  The restatement's result for a case is computed once per
process and shared.

The clouds of ``cluster_cloud`` are sized from the kernel's buffer (``torch_normals.buffer_capacity``): ``model_selections`` restates
the index's cell assignment and the kernel's append-or-select rule in Python and asserts HERE that a query's accepted candidates fill
the buffer exactly, overflow it once, or overflow it several times."""
import functools

import numpy as np
import torch

WAVE = 64


def shell(seed: int, n: int, sigma: float = 0.01) -> torch.Tensor:
    """float32 [n,3]: a unit sphere's shell of thickness sigma; tie-free with probability one"""
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(n, 3, dtype=torch.float64, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    return (d * (1 + sigma * torch.randn(n, 1, dtype=torch.float64, generator=g))).float()


def blob(seed: int, n: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, dtype=torch.float64, generator=g).float()


def lattice(side: int = 7, seed: int = 31) -> torch.Tensor:
    """the integer lattice [0, side)^3 in a seeded order: every d² is an integer, and the K-th place falls inside a group of equal d²"""
    k = torch.arange(side)
    pts = torch.stack(torch.meshgrid(k, k, k, indexing="ij"), dim=-1).reshape(-1, 3).float()
    return pts[torch.randperm(pts.shape[0], generator=torch.Generator().manual_seed(seed))]


def quarter_lattice(side: int = 7, seed: int = 32) -> torch.Tensor:
    """spacing 0.25, exact in float32: with radius 0.5 the six neighbours two steps along an axis lie at EXACTLY d² = radius²"""
    return lattice(side, seed) * 0.25


def tilted_plane(seed: int, n: int, a: float = 0.5, b: float = 0.25) -> torch.Tensor:
    """z = a x + b y with x, y multiples of 2^-10 in [-1, 1): every coordinate is exact in float32, the points lie ON the plane"""
    g = torch.Generator().manual_seed(seed)
    xy = torch.randint(-1024, 1024, (n, 2), generator=g).double() / 1024
    return torch.cat([xy, (a * xy[:, :1] + b * xy[:, 1:])], dim=1).float()


def flat(seed: int, n: int) -> torch.Tensor:
    """all z equal 0: an index axis without extent, and a normal of exactly (0, 0, 1)"""
    c = blob(seed, n)
    c[:, 2] = 0.0
    return c


def line(seed: int, n: int) -> torch.Tensor:
    """on the x axis: two index axes without extent; every covariance has rank one"""
    c = blob(seed, n)
    c[:, 1:] = 0.0
    return c


def far_point(seed: int, n: int) -> torch.Tensor:
    """a blob and one point far away: its rings grow to the whole grid"""
    return torch.cat([blob(seed, n) * 0.2, torch.tensor([[40.0, 40.0, 40.0]])])


def with_nan(seed: int, n: int) -> torch.Tensor:
    c = shell(seed, n)
    c[7, 1] = float("nan")
    c[n - 50, 0] = float("nan")
    return c


def hybrid_cloud() -> torch.Tensor:
    """a dense shell, a sparse blob around it and a few far points: with radius 0.3 and knn 30 some rows keep fewer than 3, some
    between 3 and 29, some all 30"""
    g = torch.Generator().manual_seed(44)
    far = (torch.rand(40, 3, dtype=torch.float64, generator=g) - 0.5) * 8
    return torch.cat([shell(41, 1500), blob(42, 400) * 0.6, far.float()])


HYBRID_RADIUS, HYBRID_KNN = 0.3, 30


# ---- clouds sized from the buffer -----------------------------------------------------------------------------------------------------

def grid_dim(N: int) -> int:
    """df_grid_dim: about two points per cell"""
    g = int(round((N / 2.0) ** (1.0 / 3.0)))
    while (g + 1) ** 3 * 2 <= N:
        g += 1
    while g > 1 and g ** 3 * 2 > N:
        g -= 1
    return min(max(g, 1), 128)


def cells(points: torch.Tensor) -> np.ndarray:
    """the cell of every point, int64 [N,3]: df_header_kernel and df_axis_cell in float32"""
    p = points.numpy().astype(np.float32)
    G = grid_dim(p.shape[0])
    lo, hi = p.min(axis=0), p.max(axis=0)
    ext = (hi - lo).astype(np.float32)
    assert (ext > 0).all()
    inv = (np.float32(G) / ext).astype(np.float32)
    t = ((p - lo).astype(np.float32) * inv).astype(np.float32)
    return np.where(t >= 0, np.minimum(t, np.float32(G - 1)).astype(np.int64), 0)


def cluster_cloud(m: int) -> torch.Tensor:
    """the 8 corners of [-1, 1]^3, then m points on a segment a hundredth of a cell long in the middle of one cell, their distance to
    the LAST point falling with the index: to that query every candidate of its own cell beats all that came before"""
    N = 8 + m
    G = grid_dim(N)
    w = 2.0 / G
    centre = -1.0 + (G // 2 + 0.5) * w
    k = torch.tensor([-1.0, 1.0])
    corners = torch.stack(torch.meshgrid(k, k, k, indexing="ij"), dim=-1).reshape(-1, 3)
    step = 0.01 * w / m
    seg = torch.full((m, 3), centre, dtype=torch.float64)
    seg[:, 0] += step * torch.arange(m - 1, -1, -1, dtype=torch.float64)
    return torch.cat([corners, seg.float()])


def model_selections(points: torch.Tensor, knn: int, query: int):
    """(selections inside ring 0, the fullest the buffer got) for ``query``, whose cell must hold the cluster and nothing else: the
    kernel reads a cell's points in ascending index, 64 at a time, appends those below the threshold and, when a batch would not fit
    into the 2 KP entries, keeps the K lowest first."""
    from dn_splatter_amd import torch_normals as tn
    from dn_splatter_amd.torch_geometry import squared_distance

    cap, K = tn.buffer_capacity(knn), min(knn, points.shape[0])
    c = cells(points)
    mine = np.flatnonzero((c == c[query]).all(axis=1))
    assert len(mine) == points.shape[0] - 8 and mine[0] == 8, "the cluster shares one cell and the corners lie elsewhere"
    d2 = squared_distance(points[query].double()[None], points[mine].double()).tolist()
    held, thr, selections, fullest = [], (float("inf"), -1), 0, 0
    for base in range(0, len(mine), WAVE):
        batch = [(d2[j], int(mine[j])) for j in range(base, min(base + WAVE, len(mine)))]
        accepted = [e for e in batch if e < thr]
        if accepted and len(held) + len(accepted) > cap:
            held = sorted(held)[:K]
            thr = held[K - 1]
            selections += 1
            accepted = [e for e in accepted if e < thr]
        held += accepted
        fullest = max(fullest, len(held))
        assert len(held) <= cap
    return selections, fullest


def model_most_selections(points: torch.Tensor, knn: int) -> int:
    """The most selections any query of the cloud runs, by the kernel's rule restated for EVERY query: the cells of ring r around the
    query's cell in the order z, y, then the row's run of cells (a row of a cube face is one run, an inner row its two end cells), a
    run's points in ascending cell and index, 64 at a time; a batch that would not fit is preceded by a selection, a ring that leaves
    K or more entries ends with one, and so does a search that found fewer than K.  The outside-the-cube bound is left out: it only
    ends a search after which nothing could be accepted."""
    from dn_splatter_amd import torch_normals as tn
    from dn_splatter_amd.torch_geometry import squared_distance

    N = points.shape[0]
    cap, K = tn.buffer_capacity(knn), min(knn, N)
    c = cells(points)
    G = grid_dim(N)
    p64 = points.double()
    d2 = squared_distance(p64[:, None, :], p64[None, :, :]).tolist()
    occupied = {}
    for i in range(N):
        occupied.setdefault(tuple(int(v) for v in c[i]), []).append(i)
    most = 0
    for q in range(N):
        cx, cy, cz = (int(v) for v in c[q])
        runs = {}
        for (x, y, z), members in occupied.items():
            r = max(abs(x - cx), abs(y - cy), abs(z - cz))
            face = abs(z - cz) == r or abs(y - cy) == r
            seg = 0 if face or x == cx - r else 1
            runs.setdefault((r, z, y, seg), []).append((x, members))
        held, thr, selections, dirty = [], (float("inf"), -1), 0, False
        keys = sorted(runs)
        for r in range(G):
            for key in [k for k in keys if k[0] == r]:
                run = [i for _, members in sorted(runs[key]) for i in members]
                for base in range(0, len(run), WAVE):
                    accepted = [e for e in ((d2[q][i], i) for i in run[base:base + WAVE]) if e < thr]
                    if not accepted:
                        continue
                    if len(held) + len(accepted) > cap:
                        held = sorted(held)[:K]
                        thr = held[K - 1] if len(held) >= K else thr
                        selections += 1
                        dirty = False
                        accepted = [e for e in accepted if e < thr]
                    held += accepted
                    dirty = dirty or bool(accepted)
                    assert len(held) <= cap
            if dirty and len(held) >= K:
                held = sorted(held)[:K]
                thr = held[K - 1]
                selections += 1
                dirty = False
        most = max(most, selections + (1 if dirty else 0))
    return most


CLUSTER_KNN = (40, 200)                                    # buffers of 128 and of 512 entries


@functools.lru_cache(maxsize=None)
def cluster_case(knn: int, kind: str):
    """(cloud, the selections inside ring 0 of the last point's query, the most selections of any query): 'exact' fills the buffer to its last entry, 'once' needs one
    selection for the one candidate more, 'often' needs one for every batch behind the first buffer."""
    from dn_splatter_amd import torch_normals as tn

    cap = tn.buffer_capacity(knn)
    m = {"exact": cap, "once": cap + 1, "often": 3 * cap}[kind]
    points = cluster_cloud(m)
    selections, fullest = model_selections(points, knn, points.shape[0] - 1)
    if kind == "exact":
        assert (selections, fullest) == (0, cap)
    elif kind == "once":
        assert selections == 1 and fullest == cap
    else:
        assert selections >= 3 and fullest > cap - WAVE
    return points, selections, model_most_selections(points, knn)


# ---- named clouds and their expected results ----------------------------------------------------------------------------------------------

def _identical() -> torch.Tensor:
    return torch.tensor([[0.25, -1.5, 3.0]]).repeat(300, 1)


def _collinear() -> torch.Tensor:
    return torch.tensor([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0], [2.0, 4.0, 6.0]])


CLOUDS = {
    "n1": lambda: blob(50, 1), "n2": lambda: blob(50, 2), "n3": lambda: blob(50, 3), "n4": lambda: blob(50, 4),
    "collinear": _collinear, "identical": _identical,
    "base": lambda: shell(51, 3000, 0.02),
    "n40": lambda: shell(52, 40), "n41": lambda: shell(52, 41), "n257": lambda: shell(53, 257),
    "lattice": lattice, "quarter_lattice": quarter_lattice,
    "flat": lambda: flat(54, 500), "line": lambda: line(55, 300),
    "far_point": lambda: far_point(56, 1000), "with_nan": lambda: with_nan(57, 400),
    "hybrid": hybrid_cloud, "tilted": lambda: tilted_plane(58, 600),
}
BASE_KNN = (3, 32, 33, 64, 65, 200, 256)                   # the wave width, the three buffer sizes, the maximum


@functools.lru_cache(maxsize=None)
def cloud(name) -> torch.Tensor:
    if isinstance(name, tuple):                              # ("cluster", knn, kind)
        return cluster_case(name[1], name[2])[0]
    return CLOUDS[name]()


@functools.lru_cache(maxsize=None)
def expected(name, knn: int, radius=None, orient_toward=None):
    """The restatement's (normals, covariance, neighbors, count) on the CPU."""
    from dn_splatter_amd import torch_normals as tn

    return tn.estimate_normals(cloud(name), knn=knn, radius=radius, orient_toward=orient_toward)


# ---- the depth frame ----------------------------------------------------------------------------------------------------------------------

FRAME = dict(H=24, W=32, fx=30.0, fy=31.0, cx=15.5, cy=12.25)


def frame_pose() -> np.ndarray:
    """an OpenCV camera-to-world that is not axis-aligned, 4x4 float64"""
    a, b = 0.4, -0.3
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    c2w = np.eye(4)
    c2w[:3, :3] = Rz @ Rx
    c2w[:3, 3] = (0.3, -0.2, 1.1)
    return c2w


FRAME_PLANE = (np.array([0.2, -0.1, -1.0]) / np.linalg.norm([0.2, -0.1, -1.0]), 2.0)     # n . x = -2 in the camera: z about 2


def frame_depth() -> torch.Tensor:
    """float32 [H,W]: the depth of the camera-space plane FRAME_PLANE along every pixel's ray, a block of pixels without depth"""
    H, W = FRAME["H"], FRAME["W"]
    n, d = FRAME_PLANE
    u = (np.arange(W) + 0.5 - FRAME["cx"]) / FRAME["fx"]
    v = (np.arange(H) + 0.5 - FRAME["cy"]) / FRAME["fy"]
    uu, vv = np.meshgrid(u, v, indexing="xy")
    z = -d / (n[0] * uu + n[1] * vv + n[2])
    z[5:11, 8:19] = 0.0
    return torch.from_numpy(z.astype(np.float32))
