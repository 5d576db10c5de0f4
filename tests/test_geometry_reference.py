"""The PyTorch restatement of the geometry scores (dn_splatter_amd/torch_geometry.py) against THE REFERENCE's own outputs
(tests/golden/reference_geometry.npz, written by tests/golden/make_reference_geometry_golden.py from dn_splatter/metrics.py and
dn_splatter/eval/eval_mesh_vis_cull.py), and the mesh sampler's restatement on three small meshes.  CPU only.

Tolerances.  Nearest indices: equal on every row.  Distances: 4 x 2^-52 relative — scipy sums the three squares without FMA, df_search
(and the restatement) with two, which is one rounding of d² apart, plus one of the square root, with a margin of 2.  Means and the
percentile: 1e-12 relative — at most 2^12 terms of 2^-53 each, with margin.  The reference's fp32 shares: 2^-23 relative of count / n.
The fixture is only a yardstick while no reference distance sits on the threshold and no row's best two candidates tie: both are asserted
below on the reference data itself, at 1e-9.
"""
import os

import numpy as np
import pytest
import torch

import _geometry_inputs as inputs

HERE = os.path.dirname(os.path.abspath(__file__))
REL_D = 4 * 2.0 ** -52
REL_MEAN = 1e-12
REL_F32 = 2.0 ** -23


@pytest.fixture(scope="module")
def tg():
    from dn_splatter_amd import torch_geometry

    return torch_geometry


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "reference_geometry.npz")))


@pytest.fixture(scope="module")
def clouds(golden):
    return {k: torch.from_numpy(golden[k]) for k in ("src", "src_normals", "tgt", "tgt_normals")}


@pytest.fixture(scope="module")
def directions(tg, clouds):
    """The restatement's two directions, computed once: "acc" = source to target, "comp" = target to source."""
    c = clouds
    return {"acc": tg.cloud_distances(c["src"], c["tgt"], c["src_normals"], c["tgt_normals"]),
            "comp": tg.cloud_distances(c["tgt"], c["src"], c["tgt_normals"], c["src_normals"])}


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def test_fixture_holds_the_inputs_and_is_well_separated(golden):
    tgt, _ = inputs.target()
    src, _ = inputs.source()
    assert np.array_equal(golden["tgt"], tgt) and np.array_equal(golden["src"], src)
    assert golden["tgt"].dtype == np.float32 and golden["tgt"].shape == (inputs.N_TARGET, 3) and golden["src"].shape == (inputs.N_SOURCE, 3)
    assert (golden["src"][:inputs.FAR, 0] > inputs.BOX[0] + 2.9).all(), "the far points are outside the box"
    for name in ("acc", "comp"):
        d, second = golden[name + "_dist"], golden[name + "_second"]
        assert np.abs(d - 0.05).min() > 1e-9, "a reference distance sits on the threshold"
        assert ((second - d) / second).min() > 1e-9, "a row's best two candidates tie"
    share = (golden["acc_dist"] <= 0.05).mean()
    assert 0.2 < share < 0.8 and golden["pd_acc"] > 0.05, "the threshold and the percentile do not separate"


def test_fma_is_exact():
    """The emulated fused multiply-add against exact rational arithmetic, on products that cancel against the addend."""
    from fractions import Fraction

    from dn_splatter_amd.torch_geometry import fma

    rng = np.random.default_rng(0)
    n = 3000
    a = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)
    b = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)
    c = -a * b * (1 + rng.standard_normal(n) * 1e-10 * rng.integers(0, 2, n)) + rng.standard_normal(n) * 10.0 ** rng.integers(-20, 8, n) * rng.integers(0, 2, n)
    d = rng.standard_normal(n).astype(np.float32).astype(np.float64) - rng.standard_normal(n).astype(np.float32).astype(np.float64)
    A, B, C = np.concatenate([a, d]), np.concatenate([b, d]), np.concatenate([c, np.abs(rng.standard_normal(n))])
    got = fma(torch.from_numpy(A), torch.from_numpy(B), torch.from_numpy(C)).numpy()
    want = np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(A, B, C)])
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", ["acc", "comp"])
def test_nearest_neighbours_and_distances(golden, directions, name):
    got = directions[name]
    assert np.array_equal(got["idx"].numpy(), golden[name + "_idx"].astype(np.int64))
    d, want = torch.sqrt(got["dist2"]).numpy(), golden[name + "_dist"]
    assert (np.abs(d - want) <= REL_D * want).all(), np.max(np.abs(d - want) / want)
    dot, want_dot = got["absdot"].numpy(), golden[name + "_dot"]
    # four divisions-by-norm and a three-term dot: the operands are <= 1, 8 roundings of 2^-53 absolute
    assert (np.abs(dot - want_dot) <= 8 * 2.0 ** -53).all()


@pytest.mark.parametrize("name", ["acc", "comp"])
def test_scalars_of_a_direction(tg, golden, directions, name):
    s, c = directions[name]["scalars"], directions[name]["counts"]
    g, ci = tg.GEOM_INDEX, tg.COUNT_INDEX
    d = golden[name + "_dist"]
    assert rel(s[g["mean_d"]], d.mean()) <= REL_MEAN
    assert rel(s[g["mean_d2"]], (d ** 2).mean()) <= REL_MEAN
    assert rel(s[g["mean_absdot"]], golden[name + "_dot"].mean()) <= REL_MEAN
    assert int(c[ci["n"]]) == len(d) and int(c[ci["n_nonfinite"]]) == 0
    assert int(c[ci["n_lt"]]) == int((d < 0.05).sum()) and int(c[ci["n_le"]]) == int((d <= 0.05).sum())
    assert float(s[g["share_lt"]]) == int((d < 0.05).sum()) / len(d)
    assert rel(s[g["min_d"]], d.min()) <= REL_D and rel(s[g["max_d"]], d.max()) <= REL_D


def test_percentiles_against_numpy(tg, golden, clouds):
    for q, want in zip(golden["percentiles"], golden["accuracy"]):
        got = tg.calculate_accuracy(clouds["src"], clouds["tgt"], percentile=float(q))
        assert rel(got, want) <= REL_MEAN, (q, float(got), want)


def test_pd_metrics(tg, golden, clouds):
    assert rel(tg.calculate_accuracy(clouds["src"], clouds["tgt"]), golden["pd_acc"]) <= REL_MEAN
    got = tg.calculate_completeness(clouds["src"], clouds["tgt"])
    assert rel(got, golden["pd_comp"]) <= REL_MEAN and rel(got, golden["completeness"]) <= REL_MEAN


def test_compute_metrics(tg, golden, clouds, directions):
    c = clouds
    got = tg.cloud_metrics(c["src"], c["src_normals"], c["tgt"], c["tgt_normals"])
    want = dict(zip(golden["mesh_keys"].tolist(), golden["mesh_values"].tolist()))
    assert set(want) == {"Acc", "Comp", "C-L1", "NC", "F-score"} and set(got) == set(tg.METRIC_KEYS)
    for k in ("Acc", "Comp", "C-L1", "NC"):
        assert rel(got[k], want[k]) <= REL_MEAN, k
    # the reference's shares are fp32 means of 0 / 1 values
    assert rel(golden["mesh_precision"], got["precision"]) <= REL_F32 and rel(golden["mesh_recall"], got["recall"]) <= REL_F32
    assert rel(want["F-score"], got["F-score"]) <= 4 * REL_F32            # 2 P R / (P + R) of two fp32 shares
    d_acc, d_comp = golden["acc_dist"], golden["comp_dist"]
    assert rel(got["C-L2"], 0.5 * ((d_comp ** 2).mean() + (d_acc ** 2).mean())) <= REL_MEAN
    same = tg.metrics_from_directions(directions["comp"]["scalars"], directions["acc"]["scalars"])
    assert all(torch.equal(same[k], got[k]) for k in got)


def test_f_score_is_nan_without_any_point_within_the_threshold(tg):
    a = torch.zeros(3, 3)
    b = torch.ones(2, 3)
    m = tg.cloud_metrics(a, None, b, None, threshold=0.05)
    assert float(m["precision"]) == 0.0 and float(m["recall"]) == 0.0 and np.isnan(float(m["F-score"])) and np.isnan(float(m["NC"]))


def test_ties_and_non_finite_rows(tg):
    tgt = torch.tensor([[1.0, 0, 0], [0, 0, 0], [1.0, 0, 0], [0, 0, 0]])
    src = torch.tensor([[0.9, 0, 0], [float("nan"), 0, 0], [0.1, 0, 0], [0, float("inf"), 0]])
    out = tg.cloud_distances(src, tgt)
    assert out["idx"].tolist() == [0, -1, 1, -1]
    assert int(out["counts"][tg.COUNT_INDEX["n_nonfinite"]]) == 2
    assert torch.isnan(out["scalars"][:4]).tolist() == [True, True, True, True]


def test_struct_layouts_and_constants_match_the_c_compiler(tg, tmp_path):
    """sizeof / offsetof of the two argument structs as gcc sees the header == the ctypes mirrors; the DNSPLAT_GEOM_* indices == the
    restatement's tables."""
    import ctypes
    import subprocess

    from dn_splatter_amd import _lib

    header = os.path.join(os.path.dirname(HERE), "include", "dnsplat.h")
    structs = {"dnsplat_cloud_distances_args": _lib.CloudDistancesArgs, "dnsplat_mesh_sample_args": _lib.MeshSampleArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', 'int main(void){']
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    for k in tg.GEOM_KEYS:
        lines.append(f'printf("{k} %d\\n", DNSPLAT_GEOM_{k.upper()});')
    for k in tg.COUNT_KEYS:
        lines.append(f'printf("{k} %d\\n", DNSPLAT_GEOM_{k.upper()});')
    lines.append('printf("COUNT %d\\nCOUNTS %d\\n", DNSPLAT_GEOM_COUNT, DNSPLAT_GEOM_COUNTS);')
    lines.append('return 0;}')
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f"{cname}.{f}"
    assert {k: int(got[k]) for k in tg.GEOM_KEYS} == tg.GEOM_INDEX and {k: int(got[k]) for k in tg.COUNT_KEYS} == tg.COUNT_INDEX
    assert int(got["COUNT"]) == tg.GEOM_COUNT and int(got["COUNTS"]) == tg.GEOM_COUNTS


# ---- the mesh sampler ----------------------------------------------------------------------------------------------------------------

MESHES ={"tetrahedron": inputs.tetrahedron, "square": inputs.square_with_degenerate, "grid": inputs.grid_mesh}
S = 1 << 16


@pytest.fixture(scope="module")
def sampled(tg):
    out = {}
    for name, make in MESHES.items():
        v, t = (torch.from_numpy(x) for x in make())
        areas, normals = tg.mesh_areas(v, t)
        out[name] = (v, t, areas, normals, tg.sample_mesh_surface(v, t, count=S, seed=3))
    return out


@pytest.mark.parametrize("name", list(MESHES))
def test_samples_lie_in_their_triangles(tg, sampled, name):
    v, t, areas, normals, (points, point_normals, faces) = sampled[name]
    assert points.dtype == torch.float32 and points.shape == (S, 3) and faces.shape == (S,)
    assert int(faces.min()) >= 0 and int(faces.max()) < t.shape[0]
    bary = tg.barycentrics(points, v, t, faces)
    # the point is three fp32 roundings of a combination of coordinates below 2.5: 1e-6 of slack on the unit interval
    assert float(bary.min()) >= -1e-6 and float(bary.max()) <= 1 + 1e-6
    assert torch.equal(point_normals, normals[faces])
    assert float(areas[faces].min()) > 0.0, "a zero-area face was drawn"


def test_areas_and_normals(tg, sampled):
    v, t, areas, normals, _ = sampled["tetrahedron"]
    assert torch.equal(areas[:3], torch.tensor([0.75, 1.0, 1.5], dtype=torch.float64))
    assert abs(float(areas[3]) - 0.5 * np.sqrt(3.0 ** 2 + 2.0 ** 2 + 1.5 ** 2)) < 1e-15
    assert torch.equal(normals[0], torch.tensor([0.0, 0.0, -1.0]))
    _, _, areas, normals, _ = sampled["square"]
    assert areas.tolist() == [0.5, 0.0, 0.5] and normals[1].tolist() == [0.0, 0.0, 0.0]


def test_degenerate_and_out_of_range_faces_are_never_drawn(tg, sampled):
    assert not bool((sampled["square"][4][2] == 1).any())
    v, t = (torch.from_numpy(x) for x in inputs.grid_mesh())
    t = t.clone()
    t[7] = torch.tensor([3, 10 ** 6, 4], dtype=torch.int32)
    t[100] = torch.tensor([-1, 2, 4], dtype=torch.int32)
    areas, _ = tg.mesh_areas(v, t)
    assert float(areas[7]) == 0.0 and float(areas[100]) == 0.0
    points, _, faces = tg.sample_mesh_surface(v, t, count=S, seed=1)
    assert not bool(((faces == 7) | (faces == 100)).any()) and bool(torch.isfinite(points).all())


def test_equal_seeds_give_equal_bytes_and_different_seeds_differ(tg, sampled):
    v, t, _, _, (points, normals, faces) = sampled["grid"]
    again = tg.sample_mesh_surface(v, t, count=S, seed=3)
    assert torch.equal(again[0].view(torch.int32), points.view(torch.int32)) and torch.equal(again[2], faces)
    other = tg.sample_mesh_surface(v, t, count=S, seed=4)
    assert not torch.equal(other[2], faces) and not torch.equal(other[0], points)
    wide = tg.sample_mesh_surface(v, t, count=S, seed=3 + (1 << 32))
    assert not torch.equal(wide[2], faces), "the upper half of the seed is ignored"


@pytest.mark.parametrize("name", list(MESHES))
def test_face_counts_follow_the_areas(sampled, name):
    """Every face's count over 2^16 samples within 6 sigma of the binomial expectation S area_f / area; none exempt."""
    _, t, areas, _, (_, _, faces) = sampled[name]
    p = (areas / areas.sum()).numpy()
    counts = np.bincount(faces.numpy(), minlength=t.shape[0])
    sigma = np.sqrt(S * p * (1 - p))
    assert (np.abs(counts - S * p) <= 6 * sigma).all(), np.max(np.abs(counts - S * p) / np.maximum(sigma, 1e-300))


def test_count_from_the_area(tg):
    v, t = (torch.from_numpy(x) for x in inputs.square_with_degenerate())
    points, _, _ = tg.sample_mesh_surface(v, t, samples_per_area=1e3)
    assert points.shape[0] == 1000


# ---- the builders of tests/test_gpu_geometry_edges.py ----------------------------------------------------------------------------------
# What the GPU cases rest on is proven here from the restatement, without a GPU: the lattice's d² patterns, where sorted neighbours
# split, which sources sit on the threshold, and what the restatement makes of the sampler's edge meshes.

ROUND_BITS = inputs.ROUND_BITS
LATTICE_CASES = {"plain": dict(m=4097, seed=71), "mixed": dict(m=4097, seed=72, a_values=(0, 1, 2, 4096), far=5),
                 "wide": dict(m=65537, seed=73, a_values=tuple(range(8)), n_j=64, n_i=64)}


@pytest.mark.parametrize("name", list(LATTICE_CASES))
def test_distance_lattice_patterns_are_exact(tg, name):
    src, tgt, patterns, triples = inputs.distance_lattice(**LATTICE_CASES[name])
    m = LATTICE_CASES[name]["m"]
    assert src.dtype == np.float32 and src.shape == (m, 3) and tgt.shape == (3, 3) and patterns.shape == (m,)
    d2 = tg.squared_distance(torch.from_numpy(src), torch.from_numpy(tgt[0]))
    assert np.array_equal(d2.numpy().view(np.int64), patterns), "the integer derivation of the pattern is not the restatement's d²"
    idx, near = tg.nearest(torch.from_numpy(tgt), torch.from_numpy(src))
    assert not bool(idx.any()), "the origin is not every source's nearest target"
    assert np.array_equal(near.numpy().view(np.int64), patterns)


def test_distance_lattice_drives_the_late_rounds():
    _, _, patterns, triples = inputs.distance_lattice(**LATTICE_CASES["plain"])
    assert len(set((patterns >> 20).tolist())) == 1, "the plain lattice differs above bit 20"
    assert len(set(patterns.tolist())) == 1024 >= 900
    a, j, i = triples.T
    assert not a.any() and np.array_equal(patterns, inputs.LATTICE_ONE | ((j * j) << 10) | (i * i))
    assert np.bincount(np.unique(patterns, return_counts=True)[1])[2:].sum() > 900, "fewer than 900 values are drawn more than once"
    srt = np.sort(patterns)
    rounds = {inputs.split_round(p, q, ROUND_BITS) for p, q in zip(srt[:-1], srt[1:])}
    assert rounds == {4, 5, 6}, rounds                                 # 6: equal neighbours


def test_mixed_lattice_splits_in_every_round():
    _, _, patterns, triples = inputs.distance_lattice(**LATTICE_CASES["mixed"])
    srt = np.sort(patterns)
    rounds = {inputs.split_round(p, q, ROUND_BITS) for p, q in zip(srt[:-1], srt[1:])}
    assert rounds == {0, 1, 2, 3, 4, 5, 6}, rounds
    assert (triples[:5] == -1).all() and (srt[-5:] == np.sort(patterns[:5])).all(), "the far sources are not the five largest"
    assert inputs.split_round(srt[-6], srt[-5], ROUND_BITS) == 0
    one = inputs.LATTICE_ONE
    assert inputs.split_round(one, one, ROUND_BITS) == 6 and inputs.split_round(one, one + 1, ROUND_BITS) == 5
    assert [inputs.split_round(one, one ^ (1 << b), ROUND_BITS) for b in (9, 10, 19, 20, 30, 31, 41, 42, 52, 53)] == [5, 4, 4, 3, 3, 2, 2, 1, 1, 0]


def test_lattice_sources_on_the_threshold():
    """d = sqrt(d²) is exactly 1 for the triples (0, 0, 0) and (0, 0, 1) — sqrt(1 + 2^-52) rounds to 1 — and above 1 for every other."""
    _, _, patterns, triples = inputs.distance_lattice(**LATTICE_CASES["plain"])
    d = np.sqrt(patterns.view(np.float64))
    on = (triples[:, 0] == 0) & (triples[:, 1] == 0) & (triples[:, 2] <= 1)
    assert np.array_equal(d <= 1.0, on) and not (d < 1.0).any()
    assert int((triples == 0).all(axis=1).sum()) >= 1 and int(on.sum()) > int((triples == 0).all(axis=1).sum())


def test_rank_percentile_lands_between_two_ranks():
    for n in (2, 513, 4097, 65537):
        for k in (0, n // 3, n - 2):
            h = (n - 1) * (inputs.rank_percentile(k, n) / 100.0)
            assert int(np.floor(h)) == k and 0.25 < h - k < 0.75


def test_sampler_edge_meshes(tg):
    v, t = (torch.from_numpy(x) for x in inputs.collinear_mesh())
    areas, normals = tg.mesh_areas(v, t)
    assert areas.tolist() == [0.0, 0.0, 0.0] and not bool(normals.any())
    cdf = torch.cumsum(areas, 0)
    for last in (0.0, float("nan"), float("inf"), -1.0):
        c = cdf.clone()
        c[-1] = last
        points, point_normals, faces = tg.mesh_sample(65, 9, c, v, t, normals)
        assert bool((faces == -1).all()) and bool(torch.isnan(points).all()) and not bool(point_normals.any())
    v, t = (torch.from_numpy(x) for x in inputs.square_between_degenerates())
    areas, normals = tg.mesh_areas(v, t)
    assert areas.tolist() == [0.0, 0.0, 0.5, 0.0, 0.5, 0.0, 0.0]
    _, _, faces = tg.sample_mesh_surface(v, t, count=70_000, seed=9)
    counts = np.bincount(faces.numpy(), minlength=7)
    assert counts[[0, 1, 3, 5, 6]].sum() == 0 and abs(counts[2] - 35_000) <= 6 * np.sqrt(70_000 * 0.25)
    v, t = (torch.from_numpy(x) for x in inputs.one_triangle())
    points, _, faces = tg.sample_mesh_surface(v, t, count=257, seed=9)
    assert not bool(faces.any())
    bary = tg.barycentrics(points, v, t, faces)
    assert float(bary.min()) >= -1e-6 and float(bary.max()) <= 1 + 1e-6
