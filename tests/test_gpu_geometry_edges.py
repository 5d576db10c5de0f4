"""The geometry scores (csrc/geometry.hip) past the sizes and inputs of tests/test_gpu_geometry.py: every round of the radix selection with
work to do, the finish kernel's fold past one trip, a distance equal to the threshold, non-finite target rows, and the sampler's edge
meshes.  The reference is the PyTorch restatement (dn_splatter_amd/torch_geometry.py) in float64 on the device, through
``test_gpu_geometry.compare``: idx, d² and both order statistics bit for bit, the counts equal.

The selection cases rest on ``_geometry_inputs.distance_lattice``, whose d² patterns are integers known on the host
(tests/test_geometry_reference.py proves them from the restatement without a GPU): thousands of values that share their top 44 bits, so
that the last two rounds see full bins, ties and a remaining rank above 0, and chosen ranks whose two order statistics part in a named
round.  Every case asserts from the constants below that it lies past its edge; ``test_constants_are_the_kernels`` reads them out of the
source.

One new tolerance, for the means past one fold trip, derived from the code and not from a run.  A term of a sum passes through at most
depth = 2 (log2 64 + 2) + ceil(n_part / 256) additions: the wave butterfly and the four-wave tail of gm_search_kernel, the strided loop
of gm_finish_kernel, its butterfly and its tail.  All terms are non-negative, so the kernel's sum is within depth x 2^-53 relative of the
exact one; 2 units for the division and the rounding of ``math.fsum``, 2 for a device sqrt that may differ from the host's in the last
place: (depth + 4) x 2^-53 against fsum over the kernel's own per-point outputs.  Every other comparison is exact or a bound
test_gpu_geometry.py states."""
import math
import os
import re

import numpy as np
import pytest
import torch

import _geometry_inputs as inputs
from test_gpu_geometry import DEV, bits, compare, dev

pytestmark = pytest.mark.gpu

GM_THREADS = 256                # source points per partial; partials per trip of the finish kernel's fold
GM_HPER = 8                     # d² values per thread of a histogram round
GM_HSPAN = GM_THREADS * GM_HPER
GM_ROUNDS = 6
GM_BINS = 2048
GM_BITS = (11, 11, 11, 11, 10, 10)
WAVE = 64

M_ROUNDS = 2 * GM_HSPAN + 1     # two full histogram blocks and a block of one element
LATTICES = {"plain": dict(m=M_ROUNDS, seed=71), "mixed": dict(m=M_ROUNDS, seed=72, a_values=(0, 1, 2, 4096), far=5)}
WIDE = dict(seed=73, a_values=tuple(range(8)), n_j=64, n_i=64)


@pytest.fixture(scope="module")
def geo():
    from dn_splatter_amd import geometry

    return geometry


@pytest.fixture(scope="module")
def tg():
    from dn_splatter_amd import torch_geometry

    return torch_geometry


@pytest.fixture(scope="module")
def lattices():
    """name -> (src, tgt on the device, the host's patterns of d², the integer triples); built once."""
    out = {}
    for name, kw in LATTICES.items():
        src, tgt, patterns, triples = inputs.distance_lattice(**kw)
        out[name] = dev(src, tgt) + (patterns, triples)
    return out


def pattern(x: float) -> int:
    return int(np.float64(x).view(np.int64))


def ceil_div(a: int, b: int) -> int:
    return (a + b - 1) // b


def test_constants_are_the_kernels(geo):
    """The constants the cases below reason from are the ones geometry.hip compiles."""
    text = open(os.path.join(os.path.dirname(os.path.abspath(geo.__file__)), "csrc", "geometry.hip")).read()

    def rhs(name):
        found = re.search(r"constexpr int\s+" + name + r"\b\s*=\s*([^;\n/]+)", text)
        assert found, name
        return found.group(1).strip()

    assert int(rhs("GM_THREADS")) == GM_THREADS and int(rhs("GM_HPER")) == GM_HPER and int(rhs("GM_ROUNDS")) == GM_ROUNDS
    assert int(rhs("GM_BINS")) == GM_BINS and rhs("GM_HSPAN") == "GM_THREADS * GM_HPER"
    found = re.search(r"constexpr int gm_bits\(int round\)\s*\{\s*return round < (\d+) \? (\d+) : (\d+);\s*\}", text)
    assert found, "gm_bits"
    wide_rounds, wide, narrow = (int(x) for x in found.groups())
    assert tuple(wide if r < wide_rounds else narrow for r in range(GM_ROUNDS)) == GM_BITS
    assert sum(GM_BITS) == 64 and 1 << max(GM_BITS) == GM_BINS
    common = open(os.path.join(os.path.dirname(os.path.abspath(geo.__file__)), "csrc", "splat_common.h")).read()
    assert int(re.search(r"#define DNS_WAVE\s+(\d+)", common).group(1)) == WAVE and "GM_WAVES = GM_THREADS / DNS_WAVE" in text
    assert inputs.ROUND_BITS == GM_BITS, "the CPU proofs of the lattice (tests/test_geometry_reference.py) use other rounds"


# ---- 1. every round of the selection -----------------------------------------------------------------------------------------------------

def neighbours_that_split_in(srt, split: int) -> int:
    """A rank k, searched from the middle, whose sorted neighbours k and k + 1 part in round ``split`` (GM_ROUNDS: they are equal)."""
    n = len(srt)
    for step in range(n - 1):
        k = (n // 2 + step) % (n - 1)
        if inputs.split_round(srt[k], srt[k + 1], GM_BITS) == split:
            return k
    raise AssertionError(f"no sorted neighbours part in round {split}")


@pytest.mark.parametrize("data,split", [("plain", 6), ("plain", 5), ("plain", 4), ("mixed", 3), ("mixed", 2), ("mixed", 1), ("mixed", 0)])
def test_two_ranks_that_part_in_a_named_round(geo, tg, lattices, data, split):
    """The two order statistics share every bin before round ``split`` and part in it: 6 is situation (i) of equal values, 5 two round-5
    bins of one round-4 bin, 4 two round-4 bins, 3 to 1 the rounds that ``a`` moves, 0 the far sources.  The ranks are chosen on the host
    from the builder's integer patterns; the kernel's two order statistics are those patterns."""
    src, tgt, patterns, _ = lattices[data]
    M = len(patterns)
    assert M == 2 * GM_HSPAN + 1 and ceil_div(M, GM_HSPAN) == 3
    srt = np.sort(patterns)
    k = neighbours_that_split_in(srt, split)
    q = inputs.rank_percentile(k, M)
    h = (M - 1) * (q / 100.0)
    assert math.floor(h) == k and 0.0 < h - k < 1.0, "the weight is 0: the second rank would not matter"
    lo, hi = int(srt[k]), int(srt[k + 1])
    assert inputs.split_round(lo, hi, GM_BITS) == split and (lo == hi) == (split == GM_ROUNDS)
    if split >= 4:
        assert lo >> 20 == hi >> 20 == inputs.LATTICE_ONE >> 20, "the ranks part before round 4"
        assert k > int(np.searchsorted(srt, lo)) or split < GM_ROUNDS, "the remaining rank inside the last bin is 0"
    if split == 0:
        assert k == M - 1 - LATTICES[data]["far"], "the rank does not straddle the far sources"
    got = geo.cloud_distances(src, tgt, percentile=q)
    compare(tg, got, tg.cloud_distances(src, tgt, percentile=q), normals=False)
    assert np.array_equal(bits(got.dist2).cpu().numpy(), patterns), "d² is not the pattern the lattice was built for"
    assert (pattern(got.order_lo_d2), pattern(got.order_hi_d2)) == (lo, hi)


@pytest.mark.parametrize("data", list(LATTICES))
@pytest.mark.parametrize("q", [0.0, 100.0])
def test_first_and_last_rank_among_ties(geo, tg, lattices, data, q):
    src, tgt, patterns, _ = lattices[data]
    got = geo.cloud_distances(src, tgt, percentile=q)
    compare(tg, got, tg.cloud_distances(src, tgt, percentile=q), normals=False)
    srt = np.sort(patterns)
    want = (int(srt[0]), int(srt[1])) if q == 0.0 else (int(srt[-1]), int(srt[-1]))     # ranks 0 and 1 (weight 0); n - 1 twice
    assert (pattern(got.order_lo_d2), pattern(got.order_hi_d2)) == want
    assert got.percentile == (got.min_d if q == 0.0 else got.max_d)


@pytest.mark.parametrize("q", [0.0, 37.5, 90.0, 100.0])
def test_every_source_identical(geo, tg, q):
    """One bin takes every count in every round, and the remaining rank stays k0 until the last."""
    M = M_ROUNDS
    src, tgt = dev(np.tile(np.array([[1.0, 0.0, 0.0]], dtype=np.float32), (M, 1)), inputs.LATTICE_TARGET)
    assert math.floor((M - 1) * (q / 100.0)) == {0.0: 0, 37.5: 1536, 90.0: 3686, 100.0: M - 1}[q]
    got = geo.cloud_distances(src, tgt, percentile=q, threshold=1.0)
    compare(tg, got, tg.cloud_distances(src, tgt, percentile=q, threshold=1.0), normals=False)
    assert (pattern(got.order_lo_d2), pattern(got.order_hi_d2)) == (inputs.LATTICE_ONE, inputs.LATTICE_ONE)
    assert got.percentile == 1.0 and got.mean_d == 1.0 and got.mean_d2 == 1.0 and got.min_d == 1.0 and got.max_d == 1.0
    assert (got.n, got.n_lt, got.n_le, got.n_nonfinite) == (M, 0, M, 0)


def test_a_distance_equal_to_the_threshold(geo, tg, lattices):
    """threshold = 1.0 against sources at d = 1.0 exactly: they count in n_le and not in n_lt.  d = sqrt(d²) is 1.0 for the triples
    (0, 0, 0) — d² = 1 — and (0, 0, 1), whose d² = 1 + 2^-52 has the square root 1 + 2^-53 - ..., which rounds to 1; every other source
    is farther.  Both sets are counted on the host from the builder's integers (tests/test_geometry_reference.py proves the rule)."""
    src, tgt, patterns, triples = lattices["plain"]
    M = len(patterns)
    exact = int((triples == 0).all(axis=1).sum())
    on = int(((triples[:, 0] == 0) & (triples[:, 1] == 0) & (triples[:, 2] <= 1)).sum())
    assert exact >= 1 and on > exact and on == int((np.sqrt(patterns.view(np.float64)) <= 1.0).sum())
    got = geo.cloud_distances(src, tgt, threshold=1.0)
    compare(tg, got, tg.cloud_distances(src, tgt, threshold=1.0), normals=False)
    assert (got.n, got.n_lt, got.n_le, got.n_nonfinite) == (M, 0, on, 0)
    assert got.share_lt == 0.0 and got.share_le == on / M
    assert float(geo.calculate_completeness(tgt, src, threshold=1.0)) == 0.0
    # one ulp to either side of the threshold moves both counts as the comparison says
    below, above = float(np.nextafter(1.0, 0.0)), float(np.nextafter(1.0, 2.0))
    under, over = geo.cloud_distances(src, tgt, threshold=below), geo.cloud_distances(src, tgt, threshold=above)
    assert (under.n_lt, under.n_le) == (0, 0)
    nxt = int((np.sqrt(patterns.view(np.float64)) <= above).sum())
    assert (over.n_lt, over.n_le) == (on, nxt)


def test_a_nan_source_row_among_ties(geo, tg, lattices):
    """The nan pattern sorts above every d²: a rank below M - n_nonfinite finds what it finds without the row, the last rank finds nan."""
    clean, tgt, patterns, _ = lattices["plain"]
    M, row = len(patterns), 1234
    src = clean.clone()
    src[row, 1] = float("nan")
    keep = np.arange(M) != row
    srt = np.sort(patterns[keep])
    k = neighbours_that_split_in(srt, 5)
    cases = {"below": (inputs.rank_percentile(k, M), int(srt[k]), int(srt[k + 1])),
             "straddling": (inputs.rank_percentile(M - 2, M), int(srt[-1]), None), "last": (100.0, None, None)}
    assert k + 1 < M - 1 and math.floor((M - 1) * (cases["straddling"][0] / 100.0)) == M - 2
    for name, (q, lo, hi) in cases.items():
        got = geo.cloud_distances(src, tgt, percentile=q, threshold=1.0)
        want = tg.cloud_distances(src, tgt, percentile=q, threshold=1.0)
        assert torch.equal(got.idx.long(), want["idx"]) and int(got.idx[row]) == -1 and int(got.idx.abs().sum()) == 1
        assert np.array_equal(bits(got.dist2).cpu().numpy()[keep], patterns[keep]) and bool(torch.isnan(got.dist2[row]))
        assert torch.equal(got.counts, want["counts"]) and got.n_nonfinite == 1 and got.n == M
        gs, ws = got.scalars.tolist(), want["scalars"].tolist()
        for key in ("order_lo_d2", "order_hi_d2"):
            g, w = gs[tg.GEOM_INDEX[key]], ws[tg.GEOM_INDEX[key]]
            assert pattern(g) == pattern(w) or (math.isnan(g) and math.isnan(w)), (name, key)
        assert (math.isnan(got.order_lo_d2) if lo is None else pattern(got.order_lo_d2) == lo), name
        assert (math.isnan(got.order_hi_d2) if hi is None else pattern(got.order_hi_d2) == hi), name
        for key in ("mean_d", "mean_d2", "percentile", "min_d", "max_d", "mean_absdot"):
            assert math.isnan(getattr(got, key)), (name, key)
        assert got.share_le == ws[tg.GEOM_INDEX["share_le"]] and got.n_le == int((np.sqrt(patterns[keep].view(np.float64)) <= 1.0).sum())


# ---- 2. the fold past one trip -----------------------------------------------------------------------------------------------------------

def fold_bound(M: int) -> float:
    n_part = ceil_div(M, GM_THREADS)
    depth = 2 * (int(math.log2(WAVE)) + 2) + ceil_div(n_part, GM_THREADS)
    return (depth + 4) * 2.0 ** -53


def fold_inputs(data: str, M: int):
    if data == "room":
        (tgt, tgt_n), (src, src_n) = inputs.target(1000), inputs.source(M, seed=50)
        return src, tgt, src_n, tgt_n, None
    src, tgt, patterns, _ = inputs.distance_lattice(M, **WIDE)
    rng = np.random.default_rng(74)
    return src, tgt, rng.standard_normal((M, 3)).astype(np.float32), rng.standard_normal((3, 3)).astype(np.float32), patterns


@pytest.mark.parametrize("M", [GM_THREADS * GM_THREADS, GM_THREADS * GM_THREADS + 1])
@pytest.mark.parametrize("data", ["room", "lattice"])
def test_fold_trips(geo, tg, data, M):
    """M = 65537 is 257 partials: thread 0 of the finish kernel makes a second trip, and the histogram rounds run 33 blocks.  M = 65536
    is the one-trip control.  The exact outputs against the restatement, the means against an exactly rounded sum of the kernel's own
    per-point outputs at the bound derived in this file's docstring.  Observed on the MI355X, error / bound: 0 for ten of the twelve means
    (equal to the exactly rounded sum), 0.06 for mean_d of the room at 65536, 0.05 for mean_absdot of the lattice at 65536."""
    n_part = ceil_div(M, GM_THREADS)
    trips = ceil_div(n_part, GM_THREADS)
    assert (n_part, trips, ceil_div(M, GM_HSPAN)) == ((257, 2, 33) if M > GM_THREADS * GM_THREADS else (256, 1, 32))
    bound = fold_bound(M)
    assert bound == (16 + trips + 4) * 2.0 ** -53
    src_h, tgt_h, src_nh, tgt_nh, patterns = fold_inputs(data, M)
    src, tgt, src_n, tgt_n = dev(src_h, tgt_h, src_nh, tgt_nh)
    got = geo.cloud_distances(src, tgt, src_n, tgt_n, threshold=1.0 if data == "lattice" else 0.05)
    want = tg.cloud_distances(src, tgt, src_n, tgt_n, threshold=1.0 if data == "lattice" else 0.05)
    compare(tg, got, want, means=False)
    if patterns is not None:
        assert np.array_equal(bits(got.dist2).cpu().numpy(), patterns)
        srt = np.sort(patterns)
        k = math.floor((M - 1) * 0.9)
        assert (pattern(got.order_lo_d2), pattern(got.order_hi_d2)) == (int(srt[k]), int(srt[k + 1]))
        assert got.n_le == int((np.sqrt(patterns.view(np.float64)) <= 1.0).sum()) > 0 and got.n_lt == 0
    else:
        assert 0 < got.n_le < M
    d2 = got.dist2.cpu().numpy()
    sums = {"mean_d2": d2, "mean_d": np.sqrt(d2), "mean_absdot": got.absdot.cpu().numpy()}
    for key, terms in sums.items():
        assert terms.shape == (M,) and (terms >= 0.0).all()
        exact = math.fsum(terms.tolist()) / M
        err = abs(getattr(got, key) - exact) / exact
        print(f"fold {data} M={M} {key}: {getattr(got, key)!r} exact {exact!r} error / bound = {err / bound:.4f}")
        assert err <= bound, (key, err / bound)


# ---- 3. non-finite targets -----------------------------------------------------------------------------------------------------------

def assert_no_comparable_target(tg, got, want, M):
    assert torch.equal(got.idx.long(), want["idx"]) and bool((got.idx == -1).all())
    assert bool(torch.isnan(got.dist2).all()) and bool(torch.isnan(want["dist2"]).all()) and bool(torch.isnan(got.absdot).all())
    assert torch.equal(got.counts, want["counts"]) and (got.n, got.n_lt, got.n_le, got.n_nonfinite) == (M, 0, 0, M)
    for key in ("mean_d", "mean_d2", "mean_absdot", "percentile", "min_d", "max_d", "order_lo_d2", "order_hi_d2"):
        assert math.isnan(getattr(got, key)) and math.isnan(float(want["scalars"][tg.GEOM_INDEX[key]])), key
    assert got.share_lt == 0.0 and got.share_le == 0.0


def test_nan_target_rows_are_nobodys_neighbour(geo, tg):
    tgt_h, tgt_nh = inputs.target(1000)
    tgt_h = tgt_h.copy()
    rows = [3, 500, 999]
    for c, r in enumerate(rows):
        tgt_h[r, c] = np.nan
    tgt, tgt_n = dev(tgt_h, tgt_nh)
    src, src_n = dev(*inputs.source(513))
    got = geo.cloud_distances(src, tgt, src_n, tgt_n)
    compare(tg, got, tg.cloud_distances(src, tgt, src_n, tgt_n))
    assert not bool(torch.isin(got.idx, torch.tensor(rows, dtype=torch.int32, device=DEV)).any()) and int(got.idx.min()) >= 0
    assert got.n_nonfinite == 0


@pytest.mark.parametrize("bad", ["nan_spread", "nan_one_axis", "inf_spread", "inf_one_axis", "mixed"])
def test_no_target_can_be_compared_with(geo, tg, bad):
    """N = 17 target rows, each with a nan or an inf coordinate: include/dnsplat.h gives every source row idx = -1, d² = nan and a count
    in N_NONFINITE.  An inf target has d² = inf to every source, which df_search keeps (inf, i) < (inf, 0x7fffffff); gm_search_kernel
    does not take it for a neighbour."""
    tgt_h, tgt_nh = inputs.target(17)
    tgt_h = tgt_h.copy()
    r = np.arange(17)
    if bad == "nan_spread":
        tgt_h[r, r % 3] = np.nan
    elif bad == "nan_one_axis":
        tgt_h[:, 0] = np.nan
    elif bad == "inf_spread":
        tgt_h[r, r % 3] = np.where(r % 2 == 0, np.inf, -np.inf)
    elif bad == "inf_one_axis":
        tgt_h[:, 2] = np.inf
    else:
        tgt_h[r, r % 3] = np.where(r % 2 == 0, np.inf, np.nan)
    assert not np.isfinite(tgt_h).all(axis=1).any()
    tgt, tgt_n = dev(tgt_h, tgt_nh)
    src, src_n = dev(*inputs.source(65))
    got = geo.cloud_distances(src, tgt, src_n, tgt_n)
    assert_no_comparable_target(tg, got, tg.cloud_distances(src, tgt, src_n, tgt_n), 65)


def test_finite_targets_win_over_inf_rows(geo, tg):
    tgt_h, tgt_nh = inputs.target(1000)
    tgt_h = tgt_h.copy()
    tgt_h[3, 0], tgt_h[500, 0], tgt_h[999, 0], tgt_h[999, 1] = np.inf, -np.inf, np.inf, np.nan
    tgt, tgt_n = dev(tgt_h, tgt_nh)
    src, src_n = dev(*inputs.source(513))
    got = geo.cloud_distances(src, tgt, src_n, tgt_n)
    compare(tg, got, tg.cloud_distances(src, tgt, src_n, tgt_n))
    assert not bool(torch.isin(got.idx, torch.tensor([3, 500, 999], dtype=torch.int32, device=DEV)).any()) and int(got.idx.min()) >= 0
    assert got.n_nonfinite == 0 and bool(torch.isfinite(got.dist2).all())


# ---- 4. the sampler's edges ----------------------------------------------------------------------------------------------------------

def sample_both(geo, tg, S, seed, cdf, v, t, normals):
    points, point_normals, faces = geo.mesh_sample(S, seed, cdf, v, t, normals)
    want_p, want_n, want_f = tg.mesh_sample(S, seed, cdf, v, t, normals)
    assert faces.dtype == torch.int32 and torch.equal(faces.long(), want_f)
    assert torch.equal(bits(points), bits(want_p)) and torch.equal(bits(point_normals), bits(want_n))
    return points, point_normals, faces


def assert_nothing_drawn(points, point_normals, faces):
    assert bool((faces == -1).all()) and bool(torch.isnan(points).all()) and not bool(point_normals.any())


def test_a_mesh_without_area(geo, tg):
    v, t = dev(*inputs.collinear_mesh())
    areas, normals = geo.mesh_areas(v, t)
    assert t.shape[0] == 3 and areas.tolist() == [0.0, 0.0, 0.0] and not bool(normals.any())
    cdf = torch.cumsum(areas, dim=0)
    assert_nothing_drawn(*sample_both(geo, tg, 65, 9, cdf, v, t, normals))
    with pytest.raises(ValueError):
        geo.sample_mesh_surface(v, t, count=None)
    assert_nothing_drawn(*geo.sample_mesh_surface(v, t, count=65))


def test_zero_area_faces_at_both_ends_of_the_cdf(geo, tg):
    v, t = dev(*inputs.square_between_degenerates())
    areas, normals = geo.mesh_areas(v, t)
    assert areas.tolist() == [0.0, 0.0, 0.5, 0.0, 0.5, 0.0, 0.0]
    cdf = torch.cumsum(areas, dim=0)
    assert cdf.tolist() == [0.0, 0.0, 0.5, 0.5, 1.0, 1.0, 1.0]
    S = 70_000
    points, _, faces = sample_both(geo, tg, S, 9, cdf, v, t, normals)
    counts = np.bincount(faces.cpu().numpy(), minlength=7)
    assert counts[[0, 1, 3, 5, 6]].sum() == 0 and counts[2] + counts[4] == S, "a face without area was drawn"
    p = 0.5
    assert (np.abs(counts[[2, 4]] - S * p) <= 6 * np.sqrt(S * p * (1 - p))).all()
    bary = tg.barycentrics(points, v, t, faces.long())
    assert float(bary.min()) >= -1e-6 and float(bary.max()) <= 1 + 1e-6


def test_a_single_face(geo, tg):
    """T = 1: the binary search starts with lo == hi."""
    v, t = dev(*inputs.one_triangle())
    areas, normals = geo.mesh_areas(v, t)
    assert t.shape[0] == 1 and float(areas[0]) > 0.0
    S = GM_THREADS + 1
    points, point_normals, faces = sample_both(geo, tg, S, 9, torch.cumsum(areas, dim=0), v, t, normals)
    assert not bool(faces.any()) and torch.equal(point_normals, normals.expand(S, 3))
    bary = tg.barycentrics(points, v, t, faces.long())
    assert float(bary.min()) >= -1e-6 and float(bary.max()) <= 1 + 1e-6


@pytest.mark.parametrize("last", [float("nan"), float("inf"), float("-inf"), -1.0, 0.0])
def test_a_cdf_without_a_positive_finite_total(geo, tg, last):
    v, t = dev(*inputs.square_between_degenerates())
    areas, normals = geo.mesh_areas(v, t)
    cdf = torch.cumsum(areas, dim=0)
    cdf[-1] = last
    got = sample_both(geo, tg, 65, 9, cdf, v, t, normals)
    assert_nothing_drawn(*got)
    zero = geo.mesh_sample(65, 9, torch.zeros_like(cdf), v, t, normals)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got, zero))
