"""Inputs of the point-cloud filter tests (test_cloud_filter_reference.py, test_gpu_cloud_filter.py): the thin shell with far outliers
the outlier rule is about, and the small clouds at which a part of the kernels can go wrong.  Every cloud is a deterministic function
of its name; the restatement's result for a case is computed once per process and shared."""
import functools

import torch


def cloud(seed: int, n_shell: int, n_out: int) -> torch.Tensor:
    """float32 [n_shell + n_out, 3]: a unit sphere's shell of thickness 0.01 (sigma), then uniform outliers in the cube of side 6."""
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(n_shell, 3, dtype=torch.float64, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    r = 1 + 0.01 * torch.randn(n_shell, 1, dtype=torch.float64, generator=g)
    out = (torch.rand(n_out, 3, dtype=torch.float64, generator=g) - 0.5) * 6
    return torch.cat([d * r, out]).float()


# the clouds of the issue's tables: (seed, n_shell, n_out) -> (kept, outliers removed)
SHELLS = {(0, 4096, 64): (4097, 63), (1, 300, 8): (300, 8), (2, 20000, 200): (20011, 189)}
SHELL0_THRESHOLD = 0.5167772208584265                      # cloud(0, 4096, 64), nb_neighbors = 20, std_ratio = 2
SHELL0_VOXELS = {0.05: (3127, 5), 0.5: (138, 119), 10.0: (7, 4134)}          # voxel_size -> (voxels, the largest voxel's points)


def _duplicates() -> torch.Tensor:
    """a shell, then 25 copies of one point beside it: their 20 nearest are copies, avg = 0, and they are removed"""
    return torch.cat([cloud(3, 500, 4), torch.tensor([[1.5, 0.25, -0.5]]).repeat(25, 1)])


def _pairs() -> torch.Tensor:
    """every point twice, the copies far apart in index: ranks 0 and 1 tie at d² = 0 and the index breaks the tie"""
    c = cloud(4, 200, 3)
    return torch.cat([c, c])


def _planar() -> torch.Tensor:
    """all z equal: the grid is one cell thick along z"""
    c = cloud(5, 400, 6)
    c[:, 2] = 0.25
    return c


def _with_nan() -> torch.Tensor:
    """two rows with a nan coordinate: avg = -1, left out of n_valid, nobody's neighbour"""
    c = cloud(6, 300, 5)
    c[7, 1] = float("nan")
    c[250, 0] = float("nan")
    return c


OUTLIER_CLOUDS = {
    "n1": lambda: cloud(7, 1, 0), "n2": lambda: cloud(7, 2, 0), "n19": lambda: cloud(7, 17, 2), "n20": lambda: cloud(7, 18, 2),
    "n21": lambda: cloud(7, 19, 2),
    "n257": lambda: cloud(8, 250, 7),                       # a second workgroup
    "n66000": lambda: cloud(9, 65400, 600),                 # 258 partials: a second trip of the partial fold
    "duplicates": _duplicates, "pairs": _pairs, "planar": _planar, "with_nan": _with_nan,
}
# (cloud, nb_neighbors, std_ratio): every size at 20 / 2.0, the neighbour counts and the other ratio on one workgroup and a bit
OUTLIER_CASES = [(name, 20, 2.0) for name in OUTLIER_CLOUDS] + [("n257", 1, 2.0), ("n257", 2, 2.0), ("n257", 32, 2.0), ("n257", 20, 0.5),
                                                                ("pairs", 2, 2.0), ("n21", 32, 0.5)]


@functools.lru_cache(maxsize=None)
def outlier_cloud(name: str) -> torch.Tensor:
    if isinstance(name, tuple):
        return cloud(*name)
    return OUTLIER_CLOUDS[name]()


@functools.lru_cache(maxsize=None)
def expected_avg(name, nb_neighbors: int, device: str = "cpu") -> torch.Tensor:
    """The restatement's avg (float64 [N], CPU); the search's additions and multiplications run on ``device``."""
    from dn_splatter_amd import torch_cloud_filter as tcf

    return tcf.neighbor_mean(outlier_cloud(name).to(device), nb_neighbors)


def lattice_cloud() -> torch.Tensor:
    """coordinates that are exact multiples of voxel_size = 0.25, negative ones included, each lattice point thrice with a small
    offset pattern that keeps two of them ON a voxel boundary: the floor decisions"""
    g = torch.Generator().manual_seed(11)
    k = torch.randint(-9, 10, (400, 3), generator=g).double()
    base = k * 0.25
    return torch.cat([base, base + 0.125, base.flip(0) - 0.125]).float()


VOXEL_CASES = {
    "n1": (lambda: cloud(12, 1, 0), 0.1),
    "one_voxel": (lambda: cloud(13, 4900, 100), 100.0),     # N = 5000: every point in one voxel, the contended row
    "own_voxel": (lambda: cloud(14, 3000, 0), 1e-5),        # every point its own voxel: V = N
    "n66000": (lambda: cloud(9, 65400, 600), 0.05),
    "lattice": (lattice_cloud, 0.25),
    "shell_0.05": (lambda: cloud(0, 4096, 64), 0.05), "shell_0.5": (lambda: cloud(0, 4096, 64), 0.5),
    "shell_10": (lambda: cloud(0, 4096, 64), 10.0),
}


@functools.lru_cache(maxsize=None)
def voxel_case(name: str):
    make, voxel_size = VOXEL_CASES[name]
    return make(), voxel_size


def attributes(points: torch.Tensor, seed: int = 21):
    """(normals, colors) float32 [N,3]: unit vectors and values in [0, 1)"""
    g = torch.Generator().manual_seed(seed)
    n = torch.randn(points.shape[0], 3, dtype=torch.float64, generator=g)
    n = n / n.norm(dim=-1, keepdim=True)
    return n.float(), torch.rand(points.shape[0], 3, generator=g)
