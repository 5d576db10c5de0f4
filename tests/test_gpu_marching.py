"""Marching cubes on the MI355X (csrc/marching.hip) against the numpy restatement (dn_splatter_amd/torch_marching.py).  Every comparison
is EXACT: counts equal, triangles as integers, vertices as fp32 bit patterns.  The output is a canonical function of the volume — no
atomics, IEEE division, no contraction — so there is no tolerance to choose; the one bound in this file is the float64 world mapping's
(4 x 2^-53 x radius: three double roundings), in the last test.

Shapes: a word of 64 flat lattice points is the kernels' unit; the pass over the volume gives a wave 4 words, the other kernels 16
consecutive words (64 a workgroup); a scan block is 1024 words.  (2,2,2) is below one word, (5,6,7) and (3,2,9) end inside a word with
rows that straddle lanes, (65,3,2) = 7 and (2,2,129) = 9 words end inside a wave's run and put row, plane and word boundaries in every
relative position, (17,9,33) = 79 words is one workgroup and a ragged second one, 64³ is 4096 words = 4 scan blocks, 70³ is 5360 words
with a ragged last block."""
import os

import numpy as np
import pytest
import torch

import _density_inputs as density_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(2, 2, 2), (5, 6, 7), (3, 2, 9), (17, 9, 33), (65, 3, 2), (2, 2, 129), (64, 64, 64)]


@pytest.fixture(scope="module")
def mc():
    from dn_splatter_amd import marching

    return marching


@pytest.fixture(scope="module")
def tm():
    from dn_splatter_amd import torch_marching

    return torch_marching


def noise(shape, seed=0):
    return np.random.default_rng(seed + sum(shape)).random(shape, dtype=np.float32)


def smooth(shape):
    """A sphere centred off the lattice points, radius 0.3 of the longest axis + 0.4: crosses edges of every shape above."""
    s = np.asarray(shape, dtype=np.float64) - 1
    x = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), axis=-1)
    return (0.3 * s.max() + 0.4 - np.linalg.norm(x - (0.37 * s + 0.0131), axis=-1)).astype(np.float32)


def same_bits(got: torch.Tensor, want: np.ndarray) -> bool:
    got = got.cpu().numpy()
    return got.dtype == want.dtype and got.shape == want.shape and bool((got.view(np.int32) == want.view(np.int32)).all())


def check(mc, tm, vol: np.ndarray, level: float):
    """The device's mesh of ``vol`` equals the restatement's, bit for bit.  Returns the restatement's (vertices, triangles)."""
    want_v, want_t = tm.marching_cubes(vol, level)
    got_v, got_t = mc.marching_cubes(torch.from_numpy(vol).to(DEV), level)
    assert got_v.dtype == torch.float32 and got_t.dtype == torch.int32 and got_v.is_cuda and got_t.is_cuda
    assert (got_v.shape[0], got_t.shape[0]) == (len(want_v), len(want_t))
    assert same_bits(got_t, want_t)
    assert same_bits(got_v, want_v)
    return want_v, want_t


def test_all_256_single_cells(mc, tm):
    for case in range(256):
        vol = np.array([1.0 if (case >> c) & 1 else -1.0 for c in range(8)], dtype=np.float32)
        vol = np.ascontiguousarray(vol.reshape(2, 2, 2).transpose(2, 1, 0))         # corner c sits at (c & 1, c >> 1 & 1, c >> 2 & 1)
        _, t = check(mc, tm, vol, 0.0)
        assert len(t) == int(tm.case_table()[1][case])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("field", ["noise", "smooth"])
def test_shapes_that_straddle_the_groupings(mc, tm, shape, field):
    vol, level = (noise(shape), 0.5) if field == "noise" else (smooth(shape), 0.0)
    v, t = check(mc, tm, vol, level)
    assert len(v) > 0 and len(t) > 0


def test_scan_carries_across_blocks(mc, tm):
    """70^3 = 5360 words: six scan blocks of 1024 words, the last one ragged; sphere plus noise puts vertices in every one of them."""
    shape = (70, 70, 70)
    assert mc.scratch_bytes(shape) > 0 and (70 ** 3 + 63) // 64 > 4096
    vol = (0.01 * smooth(shape) + (noise(shape, 3) - 0.5)).astype(np.float32)
    v, t = check(mc, tm, vol, 0.0)
    owner = np.floor(v.astype(np.float64))
    blocks = ((owner[:, 0] * 70 + owner[:, 1]) * 70 + owner[:, 2]) // (64 * 1024)
    assert set(blocks.astype(int).tolist()) >= set(range(6))


def test_empty_surfaces(mc, tm):
    for vol in (np.ones((9, 8, 7), np.float32), np.zeros((9, 8, 7), np.float32), np.full((9, 8, 7), np.nan, np.float32)):
        v, t = check(mc, tm, vol, 0.5)
        assert len(v) == 0 and len(t) == 0
    for shape in ((1, 9, 9), (9, 1, 9), (9, 9, 1), (1, 1, 1), (1, 1, 70)):
        v, t = check(mc, tm, noise(shape), 0.5)
        assert len(v) == 0 and len(t) == 0


def test_non_finite_values_and_the_exporters_fill(mc, tm):
    vol = noise((13, 11, 17), 7)
    rng = np.random.default_rng(11)
    for value in (np.nan, np.inf, -np.inf, -1e6):
        idx = tuple(rng.integers(0, n, 40) for n in vol.shape)
        vol[idx] = value
    vol[4:7, 3:6, 8:12] = -1e6                              # a block outside the crop box
    vol[6, 5, 10], vol[6, 5, 11], vol[6, 6, 10] = np.inf, -np.inf, np.nan      # non-finite neighbours of each other
    v, _ = check(mc, tm, vol, 0.5)
    assert bool(np.isnan(v).any())


def test_values_equal_to_the_level_give_the_same_degenerate_triangles(mc, tm):
    vol = noise((12, 10, 14), 9)
    vol[np.random.default_rng(2).random(vol.shape) < 0.2] = 0.5
    v, t = check(mc, tm, vol, 0.5)
    p = v[t]
    assert bool((np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1) == 0).any())
    check(mc, tm, (vol > 0.5).astype(np.float32), 0.0)      # only 0 (the level) and 1: every t is 0 or 1, every vertex a lattice point


@pytest.mark.parametrize("short", ["triangles", "vertices"])
def test_capacity_below_the_count(mc, tm, short):
    vol = noise((17, 9, 33))
    want_v, want_t = tm.marching_cubes(vol, 0.5)
    V, T = len(want_v), len(want_t)
    cap_v, cap_t = (V, T - 1) if short == "triangles" else (V - 1, T)
    guard = 16
    vertices = torch.full((V + guard, 3), -777.0, dtype=torch.float32, device=DEV)
    triangles = torch.full((T + guard, 3), -7, dtype=torch.int32, device=DEV)
    count = mc.mc_count(torch.from_numpy(vol).to(DEV), 0.5)
    status = mc.mc_emit(count, vertices, triangles, cap_v=cap_v, cap_t=cap_t)
    assert status.dtype == torch.int32 and status.tolist() == [mc.STATUS_TRIANGLES if short == "triangles" else mc.STATUS_VERTICES]
    assert count.counts.tolist() == [V, T]                  # the counts stay valid
    assert same_bits(vertices[:cap_v], want_v[:cap_v]) and same_bits(triangles[:cap_t], want_t[:cap_t])
    assert bool((vertices[cap_v:] == -777.0).all()) and bool((triangles[cap_t:] == -7).all())
    # the same scratch again with room for everything: status back to 0
    status = mc.mc_emit(count, vertices, triangles, cap_v=V, cap_t=T)
    assert status.tolist() == [0] and same_bits(vertices[:V], want_v) and same_bits(triangles[:T], want_t)
    assert bool((vertices[V:] == -777.0).all()) and bool((triangles[T:] == -7).all())


def test_capacity_mode_reads_nothing_and_reports(mc, tm):
    vol = smooth((17, 9, 33))
    want_v, want_t = tm.marching_cubes(vol, 0.0)
    V, T = len(want_v), len(want_t)
    out = mc.marching_cubes(torch.from_numpy(vol).to(DEV), 0.0, capacity=(V + 5, T + 3))
    assert tuple(out.vertices.shape) == (V + 5, 3) and tuple(out.triangles.shape) == (T + 3, 3)
    assert out.counts.tolist() == [V, T] and out.status.tolist() == [0]
    assert same_bits(out.vertices[:V], want_v) and same_bits(out.triangles[:T], want_t)
    out = mc.marching_cubes(torch.from_numpy(vol).to(DEV), 0.0, capacity=(0, 0))
    assert out.counts.tolist() == [V, T] and out.status.tolist() == [mc.STATUS_VERTICES | mc.STATUS_TRIANGLES]


def test_equal_inputs_give_equal_bytes(mc):
    vol = torch.from_numpy(smooth((64, 64, 64)) + 2.0 * (noise((64, 64, 64), 1) - 0.5)).to(DEV)
    v0, t0 = mc.marching_cubes(vol, 0.0)
    v1, t1 = mc.marching_cubes(vol.clone(), 0.0)
    assert v0.shape[0] > 10_000
    assert torch.equal(v0.view(torch.int32), v1.view(torch.int32)) and torch.equal(t0, t1)


def test_mcubes_call_shape_and_cpu_refusal(mc, tm, dns):
    vol = smooth((12, 13, 14))
    want_v, want_t = tm.mcubes_marching_cubes(vol, 0.0)
    for volume in (vol, torch.from_numpy(vol), torch.from_numpy(vol).to(DEV)):
        vertices, triangles = mc.mcubes_marching_cubes(volume, 0.0)
        assert isinstance(vertices, np.ndarray) and vertices.dtype == np.float64 and isinstance(triangles, np.ndarray) and triangles.dtype == np.int64
        assert np.array_equal(vertices, want_v) and np.array_equal(triangles, want_t)
    with pytest.raises(dns.DnsplatError, match="no CPU fallback"):
        mc.marching_cubes(torch.from_numpy(vol), 0.0)


@pytest.mark.parametrize("crop", [False, True])
def test_mesh_equals_the_composition(mc, tm, dns, crop):
    """marching_cubes_mesh on the density tests' fixture == density_volume -> restatement -> mapping -> closest."""
    _, t = density_inputs.load_golden(os.path.join(HERE, "golden", density_inputs.GOLDEN))
    t = {k: v.to(DEV) for k, v in t.items()}
    field = dns.GaussianDensityField(t["means"], t["scales"], t["quats"], t["opacities"])
    colors = torch.rand(field.N, 3, generator=torch.Generator().manual_seed(4)).to(DEV)
    R, radius = 24, density_inputs.VOLUME_RADIUS
    box = density_inputs.crop_box(DEV) if crop else None
    world, triangles, vertex_colors = mc.marching_cubes_mesh(field, R, radius, level=0.5, crop_box=box, colors=colors)

    volume = dns.density_volume(field, R, radius, box)
    want_v, want_t = tm.marching_cubes(volume.cpu().numpy(), 0.5)
    X = (torch.linspace(-1, 1, R, device=DEV) * radius).cpu()
    want_world = tm.world_mapping(want_v, X, X, X)
    want_colors = colors[field.closest(torch.from_numpy(want_world).float().to(DEV))[:, 0]]
    assert len(want_v) > 1000 and world.dtype == torch.float64 and world.is_cuda and triangles.is_cuda and vertex_colors.is_cuda
    assert same_bits(triangles, want_t)
    assert tuple(world.shape) == want_world.shape
    err = float(np.abs(world.cpu().numpy() - want_world).max())
    print(f"world mapping: worst difference {err:.3e} (bound {4 * 2.0 ** -53 * radius:.3e})")
    assert err <= 4 * 2.0 ** -53 * radius
    assert torch.equal(vertex_colors, want_colors)
    assert mc.marching_cubes_mesh(field, R, radius, level=0.5, crop_box=box)[2] is None
