"""csrc/meshclusters.hip against its CPU restatement (dn_splatter_amd/torch_mesh_clusters.py): every comparison is integer equality,
there is no tolerance anywhere, and every call's status word must be 0.  The inputs (tests/_mesh_clusters_inputs.py) are the smallest at
which a part of the kernels can go wrong: chains as long as the mesh in three row orders, sizes around one workgroup, an edge of 67
triangles, duplicate and degenerate and invalid rows, a soup with few edges and one with the table at its worst-case load and tens of
thousands of clusters for the numbering scan and the selection."""
import ctypes
import os

import pytest
import torch

import _mesh_clusters_inputs as inputs
import _tsdf_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -777


@pytest.fixture(scope="module")
def mcl():
    from dn_splatter_amd import mesh_clusters

    return mesh_clusters


def run_clusters(mcl, name):
    triangles, V = inputs.case(name)
    return mcl.cluster_buffers(torch.from_numpy(triangles).to(DEV), V)


def run_filter(name, buffers, keep_largest, min_triangles, cap_v=None, cap_t=None, emits=1):
    """dnsplat_mesh_filter_count and `emits` times dnsplat_mesh_filter_emit through the op layer, with sentinel-filled output buffers of
    cap_v / cap_t rows (None: the restatement's counts).  Returns (threshold, counts, [(vertex_index, triangles, status), ...])."""
    from dn_splatter_amd import _lib
    from dn_splatter_amd._ops import _mesh_filter_args, _stream

    triangles, V = inputs.case(name)
    tri = torch.from_numpy(triangles).to(DEV)
    T = tri.shape[0]
    L = _lib.lib()
    scratch = torch.empty((L.dnsplat_mesh_filter_scratch_bytes(V, T) + 7) // 8, dtype=torch.int64, device=DEV)
    threshold = torch.full((1,), SENTINEL, dtype=torch.int32, device=DEV)
    counts = torch.full((2,), SENTINEL, dtype=torch.int64, device=DEV)
    a = _mesh_filter_args(V, tri, buffers.labels, buffers.sizes, buffers.counts, keep_largest, min_triangles, scratch, threshold, counts)
    _lib.run("dnsplat_mesh_filter_count", L.dnsplat_mesh_filter_count, ctypes.byref(a), _stream())
    _, _, want_index, want_triangles = inputs.expected_filter(name, keep_largest, min_triangles)
    cap_v = want_index.shape[0] if cap_v is None else cap_v
    cap_t = want_triangles.shape[0] if cap_t is None else cap_t
    out = []
    for _ in range(emits):
        vertex_index = torch.full((cap_v + 3,), SENTINEL, dtype=torch.int32, device=DEV)
        out_triangles = torch.full((cap_t + 2, 3), SENTINEL, dtype=torch.int32, device=DEV)
        status = torch.full((1,), SENTINEL, dtype=torch.int32, device=DEV)
        a = _mesh_filter_args(V, tri, buffers.labels, buffers.sizes, buffers.counts, keep_largest, min_triangles, scratch, threshold, counts,
                              vertex_index[:cap_v], out_triangles[:cap_t], status)
        _lib.run("dnsplat_mesh_filter_emit", L.dnsplat_mesh_filter_emit, ctypes.byref(a), _stream())
        out.append((vertex_index.cpu(), out_triangles.cpu(), int(status.item())))
    return int(threshold.item()), counts.tolist(), out


@pytest.mark.parametrize("name", inputs.CASE_NAMES)
def test_clusters_and_filter_equal_the_restatement(mcl, name):
    triangles, V = inputs.case(name)
    T = triangles.shape[0]
    want_labels, want_sizes = inputs.expected_clusters(name)
    n = want_sizes.shape[0]
    b = run_clusters(mcl, name)
    assert b.status.tolist() == [0]
    assert b.counts.tolist() == [n, int((want_labels >= 0).sum())]
    assert torch.equal(b.labels.cpu(), want_labels)
    sizes = b.sizes.cpu()
    assert sizes.shape == (T,) and torch.equal(sizes[:n], want_sizes) and not sizes[n:].any()
    for keep_largest, min_triangles in inputs.FILTERS[name]:
        want_threshold, want_keep, want_index, want_triangles = inputs.expected_filter(name, keep_largest, min_triangles)
        threshold, counts, [(vertex_index, out, status)] = run_filter(name, b, keep_largest, min_triangles)
        where = (name, keep_largest, min_triangles)
        assert threshold == want_threshold, where
        assert counts == [want_index.shape[0], want_triangles.shape[0]], where
        assert status == 0, where
        nv, nt = counts
        assert torch.equal(vertex_index[:nv], want_index) and torch.equal(out[:nt], want_triangles), where
        assert bool((vertex_index[nv:] == SENTINEL).all()) and bool((out[nt:] == SENTINEL).all()), where      # nothing past the counts
    assert b.status.tolist() == [0]


def test_sphere_filter_counts_on_the_device(mcl):
    b = run_clusters(mcl, "sphere")
    labels = inputs.expected_clusters("sphere")[0]
    triangles = torch.from_numpy(inputs.case("sphere")[0])
    for filt, (want_threshold, want_clusters, want_triangles) in inputs.SPHERE_FILTERS.items():
        threshold, (nv, nt), [(vertex_index, out, status)] = run_filter("sphere", b, *filt)
        assert status == 0
        if want_threshold is not None:
            assert threshold == want_threshold
        if want_triangles is not None:
            assert nt == want_triangles
        keep = inputs.expected_filter("sphere", *filt)[1]
        assert len(set(labels[keep].tolist())) == want_clusters
        assert torch.equal(vertex_index[:nv][out[:nt].long()], triangles[keep])       # the kept rows, in their order, through the remap


def test_the_same_set_of_triangles_survives_a_permutation_of_the_rows(mcl):
    perm = torch.from_numpy(inputs.permutation(inputs.SPHERE_T, 5))
    plain, permuted = torch.from_numpy(inputs.case("sphere")[0]), torch.from_numpy(inputs.case("sphere_permuted")[0])
    for name, tri in (("sphere", plain), ("sphere_permuted", permuted)):
        b = run_clusters(mcl, name)
        _, (nv, nt), [(vertex_index, out, status)] = run_filter(name, b, 50, 8)
        assert status == 0 and b.status.tolist() == [0]
        rows = vertex_index[:nv][out[:nt].long()]
        keep = inputs.expected_filter("sphere", 50, 8)[1]
        want = plain[keep] if name == "sphere" else plain[perm][keep[perm]]
        assert torch.equal(rows, want)


@pytest.mark.parametrize("short", ["vertices", "triangles", "both", "zero"])
def test_capacity_below_the_count(mcl, short):
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dnsplat.h")).read()
    bit = {k: int(text.split(f"#define DNSPLAT_MESH_FILTER_STATUS_{k} ")[1].split()[0]) for k in ("VERTICES", "TRIANGLES")}
    b = run_clusters(mcl, "sphere")
    _, _, want_index, want_triangles = inputs.expected_filter("sphere", 50, 50)
    V1, T1 = want_index.shape[0], want_triangles.shape[0]
    cap_v = {"vertices": V1 - 300, "both": 257, "zero": 0}.get(short, V1)
    cap_t = {"triangles": T1 - 1, "both": 255, "zero": 0}.get(short, T1)
    threshold, counts, emitted = run_filter("sphere", b, 50, 50, cap_v=cap_v, cap_t=cap_t, emits=2)
    assert threshold == 50 and counts == [V1, T1]                                # the counts are the mesh's, not the buffers'
    want_status = (bit["VERTICES"] if cap_v < V1 else 0) | (bit["TRIANGLES"] if cap_t < T1 else 0)
    for vertex_index, out, status in emitted:                                    # a second emit after one count: the same bytes
        assert status == want_status and status != 0
        assert torch.equal(vertex_index[:cap_v], want_index[:cap_v]) and bool((vertex_index[cap_v:] == SENTINEL).all())
        # a triangle row within the capacity names its vertices by their new ids even where those lie past cap_v
        assert torch.equal(out[:cap_t], want_triangles[:cap_t]) and bool((out[cap_t:] == SENTINEL).all())
    assert torch.equal(emitted[0][0], emitted[1][0]) and torch.equal(emitted[0][1], emitted[1][1])


def test_two_runs_give_the_same_bytes(mcl):
    """The order in which the atomics land differs from run to run; the output does not."""
    first, second = run_clusters(mcl, "dense_soup"), run_clusters(mcl, "dense_soup")
    assert torch.equal(first.labels, second.labels) and torch.equal(first.sizes, second.sizes) and torch.equal(first.counts, second.counts)
    assert first.status.tolist() == [0] and second.status.tolist() == [0]


def test_cluster_connected_triangles_reads_the_count_once(mcl, dns):
    triangles, V = inputs.case("degenerate")
    labels, sizes = dns.cluster_connected_triangles(torch.from_numpy(triangles).to(DEV).long(), V)      # any integer dtype
    want_labels, want_sizes = inputs.expected_clusters("degenerate")
    assert labels.is_cuda and labels.dtype == torch.int32 and sizes.dtype == torch.int32
    assert torch.equal(labels.cpu(), want_labels) and torch.equal(sizes.cpu(), want_sizes)
    assert labels.tolist() == [0, 1, -1, 0, 2, 1, -1, 0] and sizes.tolist() == [3, 2, 1]


def test_filter_small_clusters_gathers_every_per_vertex_tensor(mcl, dns):
    from dn_splatter_amd import torch_mesh_clusters as ref

    vertices, triangles = inputs.sphere_mesh()
    world = torch.from_numpy(vertices).double() * 0.01 - 0.5                     # float64 world positions
    colours = torch.rand(vertices.shape[0], 3, generator=torch.Generator().manual_seed(3))
    lattice = torch.from_numpy(vertices)
    mesh = (world, torch.from_numpy(triangles), colours, None, lattice)
    want = ref.filter_small_clusters(mesh, 50, 8, return_index=True)
    got = dns.filter_small_clusters(tuple(None if x is None else x.to(DEV) for x in mesh), 50, 8, return_index=True)
    assert len(got) == len(want) == 6 and got[3] is None
    for g, w in zip(got, want):
        if w is not None:
            assert g.is_cuda and g.dtype == w.dtype and torch.equal(g.cpu(), w)
    out_vertices, out_triangles = got[0], got[1].cpu()
    assert out_triangles.shape == (9280, 3)
    assert int(out_triangles.min()) == 0 and int(out_triangles.max()) == out_vertices.shape[0] - 1          # no index out of range
    assert torch.equal(torch.unique(out_triangles), torch.arange(out_vertices.shape[0], dtype=torch.int32))  # no unreferenced vertex
    assert len(dns.filter_small_clusters((world.to(DEV), torch.from_numpy(triangles).to(DEV)))) == 2       # the tuple shape it was given
    # a filter that keeps nothing: empty tensors of the same dtypes
    triangles, V = inputs.case("sparse_soup")
    points = torch.zeros(V, 3, dtype=torch.float64, device=DEV)
    v0, t0, index = dns.filter_small_clusters((points, torch.from_numpy(triangles).to(DEV)), 50, 2, return_index=True)
    assert v0.shape == (0, 3) and v0.dtype == torch.float64 and t0.shape == (0, 3) and t0.dtype == torch.int32 and index.shape == (0,)


# ----------------------------------------------------------------------------------------------- behind the TSDF extraction
@pytest.fixture(scope="module")
def volume_with_floaters():
    """The sphere scene of tests/_tsdf_inputs.py fused on the device, plus five 3 x 3 x 3 islands of weight 1 whose centre voxel alone is
    inside: an octahedron of 8 triangles each, far from the sphere's surface."""
    from dn_splatter_amd import tsdf

    s = _tsdf_inputs.sphere_scene()
    vol = tsdf.TSDFVolume(s["origin"], s["voxel"], s["dims"], device=DEV)
    vol.integrate(s["depth"].to(DEV), s["rgb"].to(DEV), s["poses"], s["K"])
    for i, j, k in ((3, 3, 3), (3, 40, 5), (42, 4, 41), (24, 24, 24), (41, 41, 3)):      # corners of the box, and the sphere's centre
        assert not vol.weight[i - 1:i + 2, j - 1:j + 2, k - 1:k + 2].any()
        vol.weight[i - 1:i + 2, j - 1:j + 2, k - 1:k + 2] = 1.0
        vol.tsdf[i - 1:i + 2, j - 1:j + 2, k - 1:k + 2] = 1.0
        vol.tsdf[i, j, k] = -0.5
        vol.color[i - 1:i + 2, j - 1:j + 2, k - 1:k + 2] = 40.0 * (1 + i % 5)
    return s, vol


def test_extract_mesh_without_the_argument_is_what_it_was(volume_with_floaters):
    from dn_splatter_amd import torch_tsdf

    s, vol = volume_with_floaters
    want_v, want_t, want_c = torch_tsdf.extract_mesh(vol.tsdf.cpu(), vol.weight.cpu(), vol.color.cpu(), s["origin"], s["voxel"])
    for got in (vol.extract_mesh(), vol.extract_mesh(filter_clusters=None)):
        vertices, triangles, colours = got
        assert vertices.dtype == torch.float64 and torch.equal(vertices.cpu().view(torch.int64), torch.as_tensor(want_v).view(torch.int64))
        assert triangles.dtype == torch.int32 and torch.equal(triangles.cpu(), torch.as_tensor(want_t))
        assert torch.equal(colours.cpu().view(torch.int32), torch.as_tensor(want_c).view(torch.int32))


@pytest.mark.parametrize("filt", [(50, 50), True, (1, 1), (3, 9), (6, 1)])
def test_extract_mesh_with_the_filter_is_the_extraction_then_the_filter(dns, mcl, volume_with_floaters, filt):
    from dn_splatter_amd import torch_mesh_clusters as ref

    s, vol = volume_with_floaters
    raw = vol.extract_mesh()
    labels, sizes = dns.cluster_connected_triangles(raw[1], raw[0].shape[0])
    assert sorted(sizes.tolist())[:5] == [8] * 5 and sizes.shape[0] >= 6         # the floaters exist
    pair = (50, 50) if filt is True else filt
    got = vol.extract_mesh(filter_clusters=filt)
    chained = dns.filter_small_clusters(raw, *pair)
    want = ref.filter_small_clusters(tuple(x.cpu() for x in raw), *pair)
    assert len(got) == 3
    for g, c, w in zip(got, chained, want):
        assert g.dtype == w.dtype and torch.equal(g, c) and torch.equal(g.cpu(), w)
    n_clusters = sizes.shape[0]
    threshold = ref.size_threshold(sizes.cpu(), *pair)
    assert got[1].shape[0] == int(sizes[sizes >= threshold].sum())
    if pair in ((50, 50), (3, 9)):
        assert 0 < got[1].shape[0] == raw[1].shape[0] - 40                       # the five octahedra are gone, nothing else
    if pair == (6, 1) and n_clusters == 6:
        assert got[1].shape[0] == raw[1].shape[0]
    with pytest.raises(ValueError, match="capacity"):
        vol.extract_mesh(capacity=(10, 10), filter_clusters=filt)
