"""torch_cloud_filter, the restatement the cloud-filter kernels are held to, against independent code: its outlier rule against scipy's
cKDTree.query on the float64 copy of the cloud plus the formulas of include/dnsplat.h written in numpy, its voxel rule against numpy's
unique / add.at float64 mean.  No GPU.

The kept sets must be EQUAL: on these clouds the nearest avg lies 4.5 % (cloud 0), 23 % (cloud 1) and 11 % (cloud 2) from the threshold,
which no reordered fold can bridge, so no point is left out of the comparison.  The fixed-point voxel mean lies within
voxel_size * 2^-30 of the float64 mean per component: each term rounds at 2^-31 of a voxel (2^-32 per point at the most, and so for their
mean), `ref` carries up to half an ulp at the 2^21 extent limit (2^-32 of a voxel), and the last two operations round once each; the
attribute means lie within 2^-30."""
import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import _cloud_filter_inputs as inputs


@pytest.fixture(scope="module")
def tcf(dns):
    from dn_splatter_amd import torch_cloud_filter

    return torch_cloud_filter


def numpy_outlier_rule(points: torch.Tensor, nb_neighbors: int, std_ratio: float):
    p = points.double().numpy()
    K = min(nb_neighbors, len(p))
    d, _ = cKDTree(p).query(p, k=K)
    avg = d.reshape(len(p), K).sum(axis=1) / K
    n_valid = len(p)
    mean = avg[avg > 0].sum() / n_valid
    std = np.sqrt(((avg[avg > 0] - mean) ** 2).sum() / (n_valid - 1))
    threshold = mean + std_ratio * std
    return avg, mean, std, threshold, np.nonzero((avg > 0) & (avg < threshold))[0]


@pytest.mark.parametrize("key", sorted(inputs.SHELLS))
def test_outlier_rule_equals_scipy_and_numpy(tcf, key):
    points = inputs.outlier_cloud(key)
    n_shell = key[1]
    kept, removed = inputs.SHELLS[key]
    ind, stats = tcf.remove_statistical_outlier(points, 20, 2.0)
    assert torch.equal(stats["avg"], inputs.expected_avg(key, 20))
    avg, mean, std, threshold, want = numpy_outlier_rule(points, 20, 2.0)
    N = points.shape[0]
    # the tree sums its K distances in another order than ascending rank: K roundings of 2^-53 relative
    assert np.abs(stats["avg"].numpy() - avg).max() <= 20 * 2.0 ** -53 * avg.max()
    for name, value in (("mean", mean), ("std", std), ("threshold", threshold)):
        assert abs(float(stats[name]) - value) <= N * 2.0 ** -52 * abs(value), name
    assert int(stats["n_valid"]) == N and int(stats["n_kept"]) == ind.numel()
    assert np.array_equal(ind.numpy(), want)                                      # EQUAL: nothing is near the threshold
    assert ind.numel() == kept and int((ind >= n_shell).sum()) == points.shape[0] - n_shell - removed
    assert int((ind < n_shell).sum()) == n_shell - (N - kept - removed)          # and the shell points the table says
    margin = np.abs(avg[avg > 0] - threshold).min() / threshold
    assert margin > 0.04, margin
    if key == (0, 4096, 64):
        assert abs(float(stats["threshold"]) - inputs.SHELL0_THRESHOLD) <= N * 2.0 ** -52 * inputs.SHELL0_THRESHOLD


def test_outlier_rule_small_and_degenerate_clouds(tcf):
    one = inputs.outlier_cloud("n1")
    ind, stats = tcf.remove_statistical_outlier(one)
    assert ind.numel() == 0 and stats["avg"].tolist() == [0.0] and int(stats["n_valid"]) == 1 and float(stats["threshold"]) == 0.0
    ind, stats = tcf.remove_statistical_outlier(inputs.outlier_cloud("n257"), nb_neighbors=1)
    assert ind.numel() == 0 and not stats["avg"].any()                           # K = 1: the point itself, avg = 0, nothing kept
    c = inputs.outlier_cloud("with_nan")
    ind, stats = tcf.remove_statistical_outlier(c)
    bad = ~torch.isfinite(c).all(dim=-1)
    assert int(bad.sum()) == 2 and stats["avg"][bad].tolist() == [-1.0, -1.0] and int(stats["n_valid"]) == c.shape[0] - 2
    assert not bad[ind].any()
    good = c[~bad]
    avg = numpy_outlier_rule(good, 20, 2.0)[0]                                    # the nan rows are nobody's neighbours
    assert np.abs(stats["avg"][~bad].numpy() - avg).max() <= 20 * 2.0 ** -53 * avg.max()
    d = inputs.outlier_cloud("duplicates")
    ind, stats = tcf.remove_statistical_outlier(d)
    assert not stats["avg"][-25:].any() and int(ind.max()) < d.shape[0] - 25     # 25 copies: 20 neighbours at distance 0, removed
    for bad_k in (0, 33, -1):
        with pytest.raises(ValueError, match="nb_neighbors"):
            tcf.neighbor_mean(one, bad_k)


def test_ranking_breaks_distance_ties_by_index(tcf):
    c = inputs.outlier_cloud("pairs")
    n = c.shape[0] // 2
    d2 = tcf.neighbor_d2(c, 3)
    assert not d2[:, :2].any() and bool((d2[:, 2] > 0).all())                     # itself and its copy, then a true neighbour
    assert torch.equal(d2[:n], d2[n:])


def numpy_voxel_rule(points: torch.Tensor, voxel_size: float, *attrs):
    p = points.double().numpy()
    lo = p.min(axis=0) - voxel_size / 2
    idx = np.floor((p - lo) / voxel_size).astype(np.int64)
    key = idx[:, 0] | (idx[:, 1] << 21) | (idx[:, 2] << 42)
    uniq, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    order = np.argsort(first)                                                     # first appearance
    number = np.empty_like(order)
    number[order] = np.arange(len(order))
    voxel_of = number[inverse.reshape(-1)]
    counts = np.bincount(voxel_of)
    means = []
    for a in (p,) + tuple(x.double().numpy() for x in attrs):
        s = np.zeros((len(uniq), 3))
        np.add.at(s, voxel_of, a)
        means.append(s / counts[:, None])
    return voxel_of, counts, means


@pytest.mark.parametrize("voxel_size", sorted(inputs.SHELL0_VOXELS))
def test_voxel_rule_equals_the_float64_mean(tcf, voxel_size):
    points = inputs.outlier_cloud((0, 4096, 64))
    normals, colors = inputs.attributes(points)
    got_p, got_n, got_c, voxel_of, counts = tcf.voxel_down_sample(points, voxel_size, normals, colors, return_trace=True)
    want_of, want_counts, (want_p, want_n, want_c) = numpy_voxel_rule(points, voxel_size, normals, colors)
    V, largest = inputs.SHELL0_VOXELS[voxel_size]
    assert got_p.shape == (V, 3) and int(counts.max()) == largest
    assert voxel_of.dtype == torch.int32 and counts.dtype == torch.int32 and got_p.dtype == got_n.dtype == got_c.dtype == torch.float64
    assert np.array_equal(voxel_of.numpy(), want_of) and np.array_equal(counts.numpy(), want_counts)
    first = [int((voxel_of == v).nonzero()[0]) for v in range(V)]
    assert first == sorted(first)                                                 # numbered in order of first appearance
    assert np.abs(got_p.numpy() - want_p).max() <= voxel_size * 2.0 ** -30
    assert np.abs(got_n.numpy() - want_n).max() <= 2.0 ** -30 and np.abs(got_c.numpy() - want_c).max() <= 2.0 ** -30
    only_p = tcf.voxel_down_sample(points, voxel_size)
    assert only_p[1] is None and only_p[2] is None and torch.equal(only_p[0], got_p)


def test_voxel_rule_floor_decisions_on_lattice_coordinates(tcf):
    points, voxel_size = inputs.voxel_case("lattice")
    got_p, _, _, voxel_of, counts = tcf.voxel_down_sample(points, voxel_size, return_trace=True)
    want_of, want_counts, (want_p,) = numpy_voxel_rule(points, voxel_size)
    assert np.array_equal(voxel_of.numpy(), want_of) and np.array_equal(counts.numpy(), want_counts)
    assert np.abs(got_p.numpy() - want_p).max() <= voxel_size * 2.0 ** -30


def test_voxel_rule_refuses_what_the_kernel_refuses(tcf):
    points = inputs.outlier_cloud("n257")
    normals, colors = inputs.attributes(points)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="voxel_size"):
            tcf.voxel_down_sample(points, bad)
    with_nan = points.clone()
    with_nan[5, 2] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        tcf.voxel_down_sample(with_nan, 0.1)
    with pytest.raises(ValueError, match="2\\^21"):
        tcf.voxel_down_sample(points, 1e-7)                                       # the shell alone spans 2e7 voxels
    big = colors.clone()
    big[3, 0] = 2.5
    with pytest.raises(ValueError, match="beyond 2"):
        tcf.voxel_down_sample(points, 0.1, normals, big)
    nan_normals = normals.clone()
    nan_normals[0, 0] = float("nan")
    with pytest.raises(ValueError, match="beyond 2"):
        tcf.voxel_down_sample(points, 0.1, nan_normals)
