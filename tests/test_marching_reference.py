"""Marching cubes without a GPU: the generated case table, the numpy restatement (dn_splatter_amd/torch_marching.py, the yardstick of
tests/test_gpu_marching.py) on fields whose surface is known, the world mapping of export_mesh.py:789-795, the layout of
``dnsplat_mc_args`` and the host-side argument checks of the three entry points.

Nothing is pinned to ``mcubes``: it is a third-party library, absent here, with a table and a vertex order of its own.  What is checked
is the contract of include/dnsplat.h from first principles: vertices are exactly the sign-changing lattice edges, the oriented surface
is closed, it has the topology of the field, and it faces out of the dense region."""
import ctypes
import os
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "dnsplat.h")
TABLE = os.path.join(ROOT, "dn-splatter_amd", "csrc", "mc_table.h")
HISTOGRAM = {0: 2, 1: 16, 2: 50, 3: 80, 4: 76, 5: 32}


@pytest.fixture(scope="module")
def gen():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_mc_table

    return gen_mc_table


@pytest.fixture(scope="module")
def tm():
    from dn_splatter_amd import torch_marching

    return torch_marching


# ------------------------------------------------------------------------------------------------ the table


def test_regenerating_the_table_gives_the_committed_bytes(gen):
    assert gen.render().encode() == open(TABLE, "rb").read()


def test_table_counts(gen, tm):
    tab = gen.table()
    assert sum(len(t) for t in tab) == 820 and max(len(t) for t in tab) == 5
    assert dict(Counter(len(t) for t in tab)) == HISTOGRAM
    assert tab[0] == [] and tab[255] == []
    owner, ntri, tri = tm.case_table()                      # what the restatement parses from the header is the generator's table
    assert owner.tolist() == [[*d, a] for d, a in gen.EDGES]
    for c in range(256):
        flat = [e for t in tab[c] for e in t]
        assert ntri[c] == len(tab[c]) and tri[c].tolist() == flat + [-1] * (15 - len(flat))


def test_every_triangle_uses_crossing_edges_of_its_case(gen):
    for c in range(256):
        crossing = set()
        for e, (d, a) in enumerate(gen.EDGES):
            lo = d[0] | d[1] << 1 | d[2] << 2
            hi = lo | (1 << a)
            if ((c >> lo) & 1) != ((c >> hi) & 1):
                crossing.add(e)
        used = {e for t in gen.triangles(c) for e in t}
        assert used == crossing, c                          # every crossing edge carries a vertex of some triangle, and no other edge does
        for t in gen.triangles(c):
            assert len(set(t)) == 3


def test_complement_reverses_the_loops_only_without_an_ambiguous_face(gen):
    def canon(loop):
        i = loop.index(min(loop))
        return tuple(loop[i:] + loop[:i])

    n_ambiguous = 0
    for c in range(256):
        mine = sorted(canon(l) for l in gen.loops(c))
        mirrored = sorted(canon(l[::-1]) for l in gen.loops(255 - c))
        if gen.ambiguous_faces(c):
            n_ambiguous += 1
            assert mine != mirrored, c                      # the face rule separates the ABOVE corners in both: other segments
        else:
            assert mine == mirrored, c
    assert 0 < n_ambiguous < 256


def test_single_corner_cases_face_away_from_the_corner(gen):
    """Orientation from first principles: with one corner above, the triangle's right-hand normal points away from it."""
    for corner in range(8):
        (tri,) = gen.triangles(1 << corner)
        pts = []
        for e in tri:
            d, a = gen.EDGES[e]
            p = np.array(d, dtype=float)
            p[a] += 0.5
            pts.append(p)
        n = np.cross(pts[1] - pts[0], pts[2] - pts[0])
        assert n @ (np.mean(pts, axis=0) - np.array(gen.corner_offset(corner), dtype=float)) > 0


# ------------------------------------------------------------------------------------------------ smooth fields

R_SMOOTH = 24
CENTRE = np.array([11.3, 11.6, 11.45])


def _grid(shape):
    return np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij"), axis=-1)


def _sphere(x):
    d = x - CENTRE
    r = np.linalg.norm(d, axis=-1)
    return 8.2 - r, -d / r[..., None]


def _torus(x, R=6.7, r=2.9):
    d = x - CENTRE
    rho = np.hypot(d[..., 0], d[..., 1])
    q = np.sqrt((rho - R) ** 2 + d[..., 2] ** 2)
    grad = np.stack([(rho - R) * d[..., 0] / rho, (rho - R) * d[..., 1] / rho, d[..., 2]], axis=-1) / q[..., None]
    return r - q, -grad


def directed_edges(triangles):
    t = np.asarray(triangles, dtype=np.int64)
    return Counter(zip(np.concatenate([t[:, 0], t[:, 1], t[:, 2]]).tolist(), np.concatenate([t[:, 1], t[:, 2], t[:, 0]]).tolist()))


def count_sign_changes(vol, level):
    above = vol > np.float32(level)
    return int((above[:-1] != above[1:]).sum() + (above[:, :-1] != above[:, 1:]).sum() + (above[:, :, :-1] != above[:, :, 1:]).sum())


@pytest.mark.parametrize("field,euler", [(_sphere, 2), (_torus, 0)])
def test_smooth_surfaces_are_closed_manifolds_facing_out(tm, field, euler):
    vol = field(_grid((R_SMOOTH,) * 3))[0].astype(np.float32)
    assert not bool((vol == 0).any())
    vertices, triangles = tm.marching_cubes(vol, 0.0)
    assert vertices.dtype == np.float32 and triangles.dtype == np.int32
    V, T = len(vertices), len(triangles)
    assert V == count_sign_changes(vol, 0.0) and V > 500
    edges = directed_edges(triangles)
    assert set(edges.values()) == {1}
    assert all((b, a) in edges for a, b in edges)           # two-manifold: every directed edge once, its reverse once
    assert V - len(edges) // 2 + T == euler
    p = vertices.astype(np.float64)[triangles]
    normal = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    gradient = field(p.mean(axis=1))[1]
    assert bool((np.einsum("ij,ij->i", normal, gradient) < 0).all())


# ------------------------------------------------------------------------------------------------ noise


@pytest.mark.parametrize("shape", [(9, 9, 9), (5, 6, 7), (3, 2, 9)])
def test_noise_surfaces_are_closed_chains(tm, shape):
    """Balance, not strict two-manifoldness: on noise a fan diagonal can coincide with a neighbouring cell's, so a directed edge may be
    used twice — but as often in one direction as in the other, unless both ends lie on the lattice boundary, where the surface ends."""
    vol = np.random.default_rng(sum(shape)).random(shape, dtype=np.float32)
    vertices, triangles = tm.marching_cubes(vol, 0.5)
    assert len(vertices) == count_sign_changes(vol, 0.5) and len(triangles) > 0
    assert triangles.min() >= 0 and triangles.max() < len(vertices)
    on_boundary = ((vertices == 0) | (vertices == np.asarray(shape, dtype=np.float32) - 1)).any(axis=1)
    edges = directed_edges(triangles)
    interior = 0
    for (a, b), n in edges.items():
        if on_boundary[a] and on_boundary[b]:
            continue
        interior += 1
        assert edges.get((b, a), 0) == n, (a, b)
    assert interior > 0


def test_degenerate_and_non_finite_values(tm):
    vol = np.random.default_rng(5).random((6, 5, 7), dtype=np.float32)
    vol[2, 2, 3] = 0.5                                      # equal to the level: not above, t = 0 or 1 on its edges
    vol[1, 1, 1], vol[3, 3, 3], vol[4, 1, 5], vol[0, 0, 0] = np.nan, np.inf, -np.inf, -1e6
    vertices, triangles = tm.marching_cubes(vol, 0.5)
    assert len(vertices) == count_sign_changes(vol, 0.5)
    nan = np.isnan(vertices)
    assert nan.any() and bool((vertices.view(np.int32)[nan] == 0x7FC00000).all())
    p = vertices[triangles]
    area = np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    assert bool((area == 0).any())                          # the zero-area triangles at the corner equal to the level are kept
    assert tm.marching_cubes(np.zeros((4, 1, 4), np.float32), 0.5)[0].shape == (0, 3)
    v0, t0 = tm.marching_cubes(np.ones((4, 4, 4), np.float32), 0.5)
    assert v0.shape == (0, 3) and t0.shape == (0, 3) and t0.dtype == np.int32


# ------------------------------------------------------------------------------------------------ mapping, call shape


def test_world_mapping_is_the_references_expression(tm):
    R, radius = 24, 3.7
    X = torch.linspace(-1, 1, R) * radius
    vol = _sphere(_grid((R,) * 3))[0].astype(np.float32)
    vertices, _ = tm.mcubes_marching_cubes(vol, 0.0)
    X_np = Y_np = Z_np = X.cpu().numpy()
    v_x = vertices[:, 0] / (R - 1)                          # export_mesh.py:789-795
    v_y = vertices[:, 1] / (R - 1)
    v_z = vertices[:, 2] / (R - 1)
    world_x = X_np[0] + v_x * (X_np[-1] - X_np[0])
    world_y = Y_np[0] + v_y * (Y_np[-1] - Y_np[0])
    world_z = Z_np[0] + v_z * (Z_np[-1] - Z_np[0])
    want = np.stack([world_x, world_y, world_z], axis=-1)
    got = tm.world_mapping(vertices, X, X, X)
    assert got.dtype == np.float64 and want.dtype == np.float64
    assert float(np.abs(got - want).max()) <= 4 * 2.0 ** -53 * radius
    assert float(np.abs(got).max()) <= radius


def test_mcubes_call_shape(tm):
    vol = _sphere(_grid((12, 13, 14)) * 2.0)[0].astype(np.float32)
    for volume in (vol, torch.from_numpy(vol)):
        vertices, triangles = tm.mcubes_marching_cubes(volume, 0.0)
        assert isinstance(vertices, np.ndarray) and vertices.dtype == np.float64 and vertices.ndim == 2 and vertices.shape[1] == 3
        assert isinstance(triangles, np.ndarray) and triangles.dtype == np.int64 and triangles.ndim == 2 and triangles.shape[1] == 3
        assert len(vertices) > 0 and triangles.max() == len(vertices) - 1


def test_product_refuses_cpu_tensors(dns):
    with pytest.raises(dns.DnsplatError, match="no CPU fallback"):
        dns.marching_cubes(torch.zeros(4, 4, 4), 0.5)
    assert dns.marching.marching_cubes is dns.marching_cubes and callable(dns.marching_cubes_mesh) and callable(dns.mcubes_marching_cubes)


# ------------------------------------------------------------------------------------------------ the C boundary


def test_host_rejections_touch_no_gpu(dns):
    from dn_splatter_amd import _lib

    L = dns.load_library()
    buf = (ctypes.c_float * 16)()                           # never dereferenced: every call below returns before a launch
    p = ctypes.cast(buf, ctypes.c_void_p)

    def args(nx, ny, nz, volume=p, scratch=p, counts=p):
        a = _lib.McArgs()
        a.volume, a.nx, a.ny, a.nz, a.level = volume, nx, ny, nz, 0.5
        a.scratch, a.scratch_bytes, a.counts = scratch, 1 << 62, counts
        a.cap_v = a.cap_t = 4
        a.vertices = a.triangles = a.status = p
        return a

    for fn in (L.dnsplat_mc_count, L.dnsplat_mc_emit):
        assert fn(None, None) == -1
        assert fn(ctypes.byref(args(1291, 1291, 1291)), None) == -1             # 1291^3 >= 2^31
        assert fn(ctypes.byref(args(1 << 16, 1 << 15, 1)), None) == -1          # exactly 2^31
        assert fn(ctypes.byref(args(8, 8, 8, volume=None)), None) == -1
        assert fn(ctypes.byref(args(-2, 8, 8)), None) == -1
        assert fn(ctypes.byref(args(8, 8, -1)), None) == -1
        assert fn(ctypes.byref(args(8, 0, 8)), None) == -1
        assert fn(ctypes.byref(args(8, 8, 8, counts=None)), None) == -1
        assert fn(ctypes.byref(args(8, 8, 8, scratch=None)), None) == -1
        short = args(8, 8, 8)
        short.scratch_bytes = L.dnsplat_mc_scratch_bytes(8, 8, 8) - 1
        assert fn(ctypes.byref(short), None) == -2
    bad = args(8, 8, 8)
    bad.cap_t = -1
    assert L.dnsplat_mc_emit(ctypes.byref(bad), None) == -1
    bad = args(8, 8, 8)
    bad.status = None
    assert L.dnsplat_mc_emit(ctypes.byref(bad), None) == -1


def test_scratch_bytes(dns):
    L = dns.load_library()
    for shape in ((0, 4, 4), (4, -1, 4), (1291, 1291, 1291), (1 << 16, 1 << 15, 1), (2 ** 31 - 1, 2, 1)):
        assert L.dnsplat_mc_scratch_bytes(*shape) == 0, shape
    sizes = [L.dnsplat_mc_scratch_bytes(r, r, r) for r in (1, 2, 3, 4, 5, 17, 64, 65, 70, 256, 512, 1290)]
    assert sizes[0] > 0 and sizes == sorted(sizes)
    assert L.dnsplat_mc_scratch_bytes(512, 512, 512) >= 512 ** 3 // 64 * 24    # three crossing masks per word of 64 points at the least
    assert L.dnsplat_mc_scratch_bytes(512, 512, 512) <= 512 ** 3               # a quarter of the volume's own bytes at the most
    assert L.dnsplat_mc_scratch_bytes(5, 6, 7) == L.dnsplat_mc_scratch_bytes(7, 5, 6)


def test_struct_layout_matches_the_c_compiler(dns, tmp_path):
    """sizeof / offsetof of dnsplat_mc_args as gcc sees the header == the ctypes mirror (the method of tests/test_abi.py)."""
    from dn_splatter_amd import _lib

    cname, cls = "dnsplat_mc_args", _lib.McArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){', f'printf("{cname} %zu\\n", sizeof({cname}));']
    for fname, _ in cls._fields_:
        lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got[cname]) == ctypes.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, fname
