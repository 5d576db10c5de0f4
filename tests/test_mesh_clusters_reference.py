"""torch_mesh_clusters, the CPU restatement the cluster kernels are held to, against an independent statement of the same definition:
scipy's connected_components over triangle-triangle pairs from an edge sort (the restatement itself uses no graph library), the counts
the issue lists for the sphere lattice, and the literal expression of the reference's text (export_mesh.py:1029-1033)."""
import numpy as np
import pytest
import torch

import _mesh_clusters_inputs as inputs


def scipy_clusters(triangles: np.ndarray, n_vertices: int):
    """(labels int32 [T], sizes int32 [n_clusters]): components of the graph whose nodes are the valid triangles and whose links join
    the triangles of every undirected edge, renumbered by lowest triangle."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    t = triangles.astype(np.int64)
    T = t.shape[0]
    valid = ((t >= 0) & (t < n_vertices)).all(axis=1)
    tri = np.repeat(np.arange(T), 3)
    ends = np.stack([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]], axis=1).reshape(-1, 2)
    use = np.repeat(valid, 3) & (ends[:, 0] != ends[:, 1])
    tri, ends = tri[use], np.sort(ends[use], axis=1)
    key = ends[:, 0] * np.int64(n_vertices) + ends[:, 1]
    order = np.argsort(key, kind="stable")
    key, tri = key[order], tri[order]
    same = key[1:] == key[:-1]                                                    # neighbours in the sort that hold one edge
    graph = coo_matrix((np.ones(int(same.sum()), dtype=np.int8), (tri[:-1][same], tri[1:][same])), shape=(T, T))
    _, comp = connected_components(graph, directed=False)
    labels = np.full(T, -1, dtype=np.int32)
    ids = np.flatnonzero(valid)
    _, first, inverse = np.unique(comp[ids], return_index=True, return_inverse=True)   # first: the lowest valid triangle of each component
    rank = np.argsort(np.argsort(first))                                          # components in ascending order of that triangle
    labels[ids] = rank[inverse].astype(np.int32)
    return labels, np.bincount(labels[ids], minlength=0).astype(np.int32)


def test_the_sphere_lattice_is_the_one_the_counts_were_worked_out_for():
    vertices, triangles = inputs.sphere_mesh()
    assert vertices.shape == (inputs.SPHERE_V, 3) and triangles.shape == (inputs.SPHERE_T, 3)
    labels, sizes = inputs.expected_clusters("sphere")
    assert sizes.shape[0] == inputs.SPHERE_CLUSTERS
    assert sorted(sizes.tolist(), reverse=True) == [s for s in inputs.SPHERE_SIZES for _ in range(8)]
    assert int(labels.min()) == 0 and int(sizes.sum()) == inputs.SPHERE_T


@pytest.mark.parametrize("name", inputs.CASE_NAMES)
def test_restatement_equals_scipy(name):
    triangles, V = inputs.case(name)
    labels, sizes = inputs.expected_clusters(name)
    want_labels, want_sizes = scipy_clusters(triangles, V)
    assert labels.dtype == torch.int32 and sizes.dtype == torch.int32
    assert np.array_equal(labels.numpy(), want_labels)
    assert np.array_equal(sizes.numpy(), want_sizes)


@pytest.mark.parametrize("filt", list(inputs.SPHERE_FILTERS))
def test_sphere_filter_counts(filt):
    want_threshold, want_clusters, want_triangles = inputs.SPHERE_FILTERS[filt]
    labels, sizes = inputs.expected_clusters("sphere")
    threshold, keep, vertex_index, out = inputs.expected_filter("sphere", *filt)
    if want_threshold is not None:
        assert threshold == want_threshold
    assert len(set(labels[keep].tolist())) == want_clusters
    if want_triangles is not None:
        assert int(keep.sum()) == want_triangles == out.shape[0]
    # ties at the threshold are all kept, nothing below it is
    assert bool((sizes[labels[keep].long()] >= threshold).all()) and bool((sizes[labels[~keep].long()] < threshold).all())
    # no unreferenced vertex, no index out of range
    assert torch.equal(torch.unique(out.reshape(-1)).to(torch.int32), torch.arange(vertex_index.shape[0], dtype=torch.int32))
    triangles = torch.from_numpy(inputs.case("sphere")[0])
    assert torch.equal(vertex_index[out.long()], triangles[keep])


def test_permuting_the_rows_keeps_the_same_set_of_triangles():
    perm = inputs.permutation(inputs.SPHERE_T, 5)
    for filt in inputs.FILTERS["sphere_permuted"]:
        keep = inputs.expected_filter("sphere", *filt)[1].numpy()
        keep_permuted = inputs.expected_filter("sphere_permuted", *filt)[1].numpy()
        assert np.array_equal(keep_permuted, keep[perm])


def test_strips_are_one_cluster_labelled_zero():
    for T in inputs.STRIP_T:
        for order in inputs.STRIP_ORDERS:
            labels, sizes = inputs.expected_clusters(f"strip_{T}_{order}")
            assert sizes.tolist() == [T] and not labels.any()


def test_small_shapes():
    labels, sizes = inputs.expected_clusters("bow_tie")
    assert labels.tolist() == [0] * 5 + [1] * 5 and sizes.tolist() == [5, 5]      # a shared vertex alone does not connect
    labels, sizes = inputs.expected_clusters("non_manifold")
    assert sizes.tolist() == [67] and not labels.any()
    labels, sizes = inputs.expected_clusters("duplicates")
    assert sizes.tolist() == [3] and not labels.any()


def test_degenerate_and_invalid_rows():
    triangles, V = inputs.case("degenerate")
    labels, sizes = inputs.expected_clusters("degenerate")
    #                         fan  (5,5,6)  invalid  fan  (7,7,7)  (5,6,8)  invalid  fan
    assert labels.tolist() == [0, 1, -1, 0, 2, 1, -1, 0]
    assert sizes.tolist() == [3, 2, 1]                                            # the degenerate rows count
    threshold, keep, vertex_index, out = inputs.expected_filter("degenerate", 50, 1)
    assert threshold == 1                                                         # 3 clusters < 50: min_triangles, no IndexError
    assert keep.tolist() == [True, False, False, True, False, True, False, True]  # degenerate and invalid rows are never emitted
    assert vertex_index.tolist() == [0, 1, 2, 3, 4, 5, 6, 8]                      # 7: only (7,7,7) and an invalid row referenced it
    threshold, keep, _, _ = inputs.expected_filter("degenerate", 2, 2)
    assert threshold == 2 and keep.tolist() == [True, False, False, True, False, True, False, True]   # (5,6,8): its cluster has size 2
    threshold, keep, _, _ = inputs.expected_filter("degenerate", 1, 1)
    assert threshold == 3 and keep.tolist() == [True, False, False, True, False, False, False, True]


@pytest.mark.parametrize("name", [n for n in inputs.CASE_NAMES if not n.startswith("strip")])
def test_the_reference_expression_agrees_where_it_is_defined(name):
    """export_mesh.py:1029-1033, literally, on the restatement's labels: n = max(np.sort(sizes)[-50], 50); remove sizes[labels] < n."""
    labels, sizes = (x.numpy() for x in inputs.expected_clusters(name))
    triangles, V = inputs.case(name)
    if sizes.shape[0] < 50:
        with pytest.raises(IndexError):
            np.sort(sizes)[-50]
        assert inputs.expected_filter(name, 50, 50)[0] == 50
        return
    n = max(np.sort(sizes)[-50], 50)
    valid = labels >= 0
    remove = np.ones(labels.shape[0], dtype=bool)
    remove[valid] = sizes[labels[valid]] < n
    t = triangles.astype(np.int64)
    distinct = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])    # remove_degenerate_triangles
    threshold, keep, _, _ = inputs.expected_filter(name, 50, 50)
    assert threshold == n
    assert np.array_equal(keep.numpy(), ~remove & distinct)


def test_filter_small_clusters_gathers_every_per_vertex_tensor():
    from dn_splatter_amd import torch_mesh_clusters as ref

    vertices, triangles = inputs.sphere_mesh()
    world = torch.from_numpy(vertices).double() * 0.01 - 0.5
    colours = torch.rand(vertices.shape[0], 3, generator=torch.Generator().manual_seed(3))
    out = ref.filter_small_clusters((world, torch.from_numpy(triangles), None, colours), 50, 50, return_index=True)
    assert len(out) == 5 and out[2] is None
    _, _, vertex_index, want = inputs.expected_filter("sphere", 50, 50)
    assert torch.equal(out[4], vertex_index) and torch.equal(out[1], want)
    assert torch.equal(out[0], world[vertex_index.long()]) and torch.equal(out[3], colours[vertex_index.long()])
    with pytest.raises(ValueError):
        ref.size_threshold([1, 2], 0, 1)
