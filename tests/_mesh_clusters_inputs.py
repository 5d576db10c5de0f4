"""Inputs shared by tests/test_mesh_clusters_reference.py (CPU) and tests/test_gpu_mesh_clusters.py: meshes as (name, triangles int32
[T,3] numpy, n_vertices), each the smallest at which some part of csrc/meshclusters.hip can go wrong, and the restatement's answer per
input, computed once and shared.  Everything is deterministic; nothing here touches a GPU."""
import functools

import numpy as np

# ----------------------------------------------------------------------------------------------- the sphere lattice
SPHERE_R = 33
SPHERE_SIZES = (356, 260, 200, 152, 92, 68, 32, 8)         # 8 clusters of each
SPHERE_V, SPHERE_T, SPHERE_CLUSTERS = 4800, 9344, 64
# (keep_largest, min_triangles) -> (threshold, clusters kept, triangles kept); None where the issue states no figure
SPHERE_FILTERS = {(50, 50): (50, 48, 9024), (50, 8): (32, 56, 9280), (10, 1): (260, 16, 4928), (100, 50): (50, 48, None),
                  (1, 1): (None, 8, None), (64, 1): (None, 64, None)}


def sphere_volume() -> np.ndarray:
    """float32 [33,33,33]: the minimum over 64 spheres of (distance to the centre - radius); centres (4 + 8a + .25, 4 + 8b + .25,
    4 + 8c + .25) for a, b, c in 0..3, sphere i (c fastest) of radius 0.6 + 0.35 (i % 8)."""
    x = np.stack(np.meshgrid(*[np.arange(SPHERE_R, dtype=np.float64)] * 3, indexing="ij"), axis=-1)
    field = np.full((SPHERE_R,) * 3, np.inf)
    i = 0
    for a in range(4):
        for b in range(4):
            for c in range(4):
                centre = np.array([4 + 8 * a + 0.25, 4 + 8 * b + 0.25, 4 + 8 * c + 0.25])
                field = np.minimum(field, np.linalg.norm(x - centre, axis=-1) - (0.6 + 0.35 * (i % 8)))
                i += 1
    return field.astype(np.float32)


@functools.lru_cache(maxsize=None)
def sphere_mesh():
    """(vertices float32 [4800,3], triangles int32 [9344,3]) of torch_marching at level 0."""
    from dn_splatter_amd import torch_marching

    vertices, triangles = torch_marching.marching_cubes(sphere_volume(), 0.0)
    return np.ascontiguousarray(vertices), np.ascontiguousarray(triangles.astype(np.int32))


def permutation(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).permutation(n)


# ----------------------------------------------------------------------------------------------- the small shapes
STRIP_T = (1, 2, 255, 256, 257, 4097)
STRIP_ORDERS = ("natural", "reversed", "shuffled")


def strip(T: int, order: str):
    """Triangle i = (i, i + 1, i + 2): one cluster, union chains as long as the mesh."""
    i = np.arange(T, dtype=np.int32)
    t = np.stack([i, i + 1, i + 2], axis=1)
    if order == "reversed":
        t = t[::-1]
    elif order == "shuffled":
        t = t[permutation(T, 1000 + T)]
    return t.copy(), T + 2                                  # a copy: a reversed view of one row still counts as contiguous


def bow_tie():
    """Two fans of 5 triangles that meet in vertex 0 and nothing else: two clusters."""
    left = [(0, 1 + j, 2 + j) for j in range(5)]
    right = [(0, 7 + j, 8 + j) for j in range(5)]
    return np.array(left + right, dtype=np.int32), 13


def non_manifold():
    """67 triangles (0, 1, 2 + j) on one edge: more than a wave contends for one table slot and one root."""
    return np.array([(0, 1, 2 + j) for j in range(67)], dtype=np.int32), 69


def duplicates():
    """(a, b, c), (c, b, a) and (a, b, c) again: one cluster of size 3."""
    return np.array([(3, 1, 2), (2, 1, 3), (3, 1, 2)], dtype=np.int32), 4


DEGENERATE_V = 9


def degenerate():
    """A small valid mesh — a fan 0-1-2-3-4 around vertex 0 and a lone triangle (5, 6, 8) — with (5, 5, 6), which joins the lone
    triangle through its one real edge {5, 6}, (7, 7, 7), a cluster of its own with no edge at all, and the invalid rows (7, 8, 99)
    and (-1, 0, 1) mixed in.  V = 9."""
    return np.array([(0, 1, 2), (5, 5, 6), (-1, 0, 1), (0, 2, 3), (7, 7, 7), (5, 6, 8), (7, 8, 99), (0, 3, 4)], dtype=np.int32), DEGENERATE_V


def dense_soup():
    """V = 64, T = 5000 random triples: few distinct edges, each held by many triangles."""
    return np.random.default_rng(11).integers(0, 64, (5000, 3)).astype(np.int32), 64


def sparse_soup():
    """V = 200 000, T = 70 000 random triples: about T clusters of size 1, the table near its worst-case load, the numbering scan and the
    selection over tens of thousands of clusters."""
    return np.random.default_rng(12).integers(0, 200_000, (70_000, 3)).astype(np.int32), 200_000


def sphere_case():
    return sphere_mesh()[1], SPHERE_V


def sphere_permuted_case():
    t = sphere_mesh()[1]
    return np.ascontiguousarray(t[permutation(t.shape[0], 5)]), SPHERE_V


CASES = {"sphere": sphere_case, "sphere_permuted": sphere_permuted_case, "bow_tie": bow_tie, "non_manifold": non_manifold,
         "duplicates": duplicates, "degenerate": degenerate, "dense_soup": dense_soup, "sparse_soup": sparse_soup}
for _T in STRIP_T:
    for _order in STRIP_ORDERS:
        CASES[f"strip_{_T}_{_order}"] = functools.partial(strip, _T, _order)
CASE_NAMES = tuple(CASES)

# the filters each case is cut with: the reference's, one where keep_largest decides, one that keeps everything valid
FILTERS = {"sphere": tuple(SPHERE_FILTERS), "sphere_permuted": ((50, 50), (50, 8)), "sparse_soup": ((50, 1), (50, 2)),
           "dense_soup": ((50, 50), (1, 1), (2, 2)), "degenerate": ((50, 50), (1, 1), (2, 2), (3, 1)), "bow_tie": ((1, 1), (2, 5), (1, 6)),
           "non_manifold": ((50, 50), (1, 100)), "duplicates": ((1, 1), (1, 4))}
for _T in STRIP_T:
    for _order in STRIP_ORDERS:
        FILTERS[f"strip_{_T}_{_order}"] = ((50, 50), (1, 1)) if _order == "natural" else ((1, 1),)


@functools.lru_cache(maxsize=None)
def case(name: str):
    """(triangles int32 [T,3] numpy, n_vertices)."""
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected_clusters(name: str):
    """The restatement's (labels int32 [T], sizes int32 [n_clusters]) for a case, computed once."""
    from dn_splatter_amd import torch_mesh_clusters

    triangles, V = case(name)
    return torch_mesh_clusters.cluster_connected_triangles(triangles, V)


@functools.lru_cache(maxsize=None)
def expected_filter(name: str, keep_largest: int, min_triangles: int):
    """The restatement's (threshold, keep bool [T], vertex_index int32 [V'], triangles int32 [T',3]) for a case, from the shared labels."""
    from dn_splatter_amd import torch_mesh_clusters

    triangles, V = case(name)
    return torch_mesh_clusters.filter_triangles(triangles, V, keep_largest, min_triangles, clusters=expected_clusters(name))
