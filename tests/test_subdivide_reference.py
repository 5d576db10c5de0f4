"""The subdivision's restatement (``dn_splatter_amd.torch_subdivide``) on the CPU: against an independent numpy statement written the
way trimesh's text reads (``_subdivide_inputs.numpy_subdivide_to_size``, midpoints numbered by ``np.unique``), against invariants that
need no restatement (every edge short enough, the area kept, every child in its parent's plane), and at its edges.  trimesh is not
at hand: the rule is this project's definition, parity unpinned against it."""
import math

import numpy as np
import pytest
import torch

import _subdivide_inputs as inputs


@pytest.fixture(scope="module")
def ts():
    from dn_splatter_amd import torch_subdivide

    return torch_subdivide


@pytest.fixture(scope="module")
def results(ts):
    """name -> (mesh, (vertices, triangles, face_index) of the restatement, its rounds): computed once, never changed."""
    out = {}
    for name, (mesh, max_edge, _, _, _) in inputs.CASES.items():
        v, f = mesh()
        rounds = []
        out[name] = ((v, f), ts.subdivide_to_size(v, f, max_edge, return_index=True, rounds=rounds), rounds)
    return out


def soup_of(vertices, triangles):
    return np.asarray(vertices)[np.asarray(triangles).astype(np.int64)]


def lengths(tri):
    """[T,3] by the stated formula, in numpy."""
    d = np.roll(tri, -1, axis=1) - tri
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def areas(tri):
    return 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)


# ---- an independent statement --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(inputs.CASES))
def test_restatement_equals_the_numpy_statement_and_the_measured_counts(ts, results, name):
    mesh, max_edge, want_rounds, want_v, want_t = inputs.CASES[name]
    (v, f), (gv, gt, gi), rounds = results[name]
    nv, nf, ni, nrounds = inputs.numpy_subdivide_to_size(v, f, max_edge)
    assert gv.dtype == torch.float64 and gt.dtype == torch.int32 and gi.dtype == torch.int32
    assert rounds == nrounds and len(rounds) == inputs.ROUNDS[name]
    if want_rounds is not None:
        assert rounds == want_rounds
    assert (gv.shape[0], gt.shape[0]) == (nv.shape[0], nf.shape[0]) == (want_v, want_t)
    if name in inputs.LAST_ROUND_TRIANGLES:
        assert rounds[-1][0] == inputs.LAST_ROUND_TRIANGLES[name] and rounds[-1][1] == 0
    if name == "box_0.8":
        assert (768, 256) in [(r[0], r[1]) for r in rounds]                     # one block of long triangles among three
    assert np.array_equal(gi.numpy(), ni)
    assert np.array_equal(soup_of(gv, gt), nv[nf])
    sv, st, si = ts.subdivide_to_size(v, f, max_edge, return_index=True, midpoint_order="sorted")
    assert sv.shape == gv.shape and torch.equal(si, gi)
    assert np.array_equal(soup_of(sv, st), soup_of(gv, gt))
    if name != "box_3.0":                                                        # the numbering itself does differ
        assert not torch.equal(st, gt)


def test_soup_has_what_it_is_there_for():
    v, f = inputs.soup()
    assert v.dtype == np.float32 and v.shape == (400, 3) and f.shape == (900, 3)
    assert ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).any()
    edges = np.sort(f[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), axis=1)
    assert len(np.unique(edges, axis=0)) < len(edges)                            # shared edges


# ---- invariants that need no restatement ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(inputs.CASES))
def test_every_edge_is_short_and_the_area_is_kept(results, name):
    max_edge = inputs.CASES[name][1]
    (v, f), (gv, gt, gi), _ = results[name]
    tri = soup_of(gv, gt)
    assert lengths(tri).max() <= max_edge
    before, after = math.fsum(areas(soup_of(v.astype(np.float64), f))), math.fsum(areas(tri))
    assert abs(after - before) <= 1e-12 * before
    assert 0 <= int(gi.min()) and int(gi.max()) < f.shape[0]
    assert int(gt.min()) == 0 and int(gt.max()) == gv.shape[0] - 1               # every vertex referenced, nothing beyond


@pytest.mark.parametrize("name", [n for n in sorted(inputs.CASES) if n.startswith("box")])
def test_box_children_lie_in_the_plane_of_their_parent(results, name):
    (v, f), (gv, gt, gi), _ = results[name]
    parent = soup_of(v.astype(np.float64), f)[gi.numpy()]                        # [T',3,3]
    normal = np.cross(parent[:, 1] - parent[:, 0], parent[:, 2] - parent[:, 0])
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    centroid = soup_of(gv, gt).mean(axis=1)
    off = np.abs(((centroid - parent[:, 0]) * normal).sum(axis=1))
    assert off.max() <= 16 * np.finfo(np.float64).eps * 5.0                      # axis-aligned faces of a box of side <= 5
    # and inside the parent: barycentric coordinates of the centroid, in the parent's two edge vectors
    e1, e2, w = parent[:, 1] - parent[:, 0], parent[:, 2] - parent[:, 0], centroid - parent[:, 0]
    d11, d12, d22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    b1, b2 = (w * e1).sum(1), (w * e2).sum(1)
    det = d11 * d22 - d12 * d12
    s, t = (d22 * b1 - d12 * b2) / det, (d11 * b2 - d12 * b1) / det
    assert s.min() > 0 and t.min() > 0 and (s + t).max() < 1


# ---- edge cases ----------------------------------------------------------------------------------------------------------------------

def strictness_triangle():
    v = np.array([[0.1, 0.2, 0.3], [0.7, 0.9, 0.4], [0.2, 0.8, 1.1]])
    f = np.array([[0, 1, 2]])
    return v, f, float(lengths(v[f]).max())


def test_the_comparison_is_strict(ts):
    v, f, longest = strictness_triangle()
    gv, gt, gi = ts.subdivide_to_size(v, f, longest, return_index=True)
    assert np.array_equal(gv.numpy(), v) and np.array_equal(gt.numpy(), f) and gi.tolist() == [0]
    gv, gt, gi = ts.subdivide_to_size(v, f, np.nextafter(longest, 0.0), return_index=True)
    assert gt.shape[0] == 4 and gv.shape[0] == 6 and gi.tolist() == [0, 0, 0, 0]
    assert gt.tolist() == [[0, 3, 5], [3, 1, 4], [5, 4, 2], [3, 4, 5]]
    assert np.array_equal(gv.numpy()[3:], np.stack([(v[0] + v[1]) / 2, (v[1] + v[2]) / 2, (v[2] + v[0]) / 2]))


def test_max_iter(ts):
    v, f = inputs.box_room()
    with pytest.raises(ValueError, match="max_iter exceeded"):
        ts.subdivide_to_size(v, f, 0.8, max_iter=2)
    with pytest.raises(ValueError, match="max_iter exceeded"):
        ts.subdivide_to_size(v, f, 0.8, max_iter=3)                              # four rounds split; the fifth only emits
    assert ts.subdivide_to_size(v, f, 0.8, max_iter=4)[1].shape[0] == 1536
    gv, gt = ts.subdivide_to_size(v, f, 10.0, max_iter=0)                        # nothing long: round 0 is the end
    assert np.array_equal(gv.numpy(), v.astype(np.float64)) and np.array_equal(gt.numpy(), f)


def test_nothing_long_returns_the_referenced_vertices_in_order(ts):
    v = np.array([[0, 0, 0], [9, 9, 9], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)      # vertex 1 is referenced by nothing
    f = np.array([[4, 3, 2], [0, 2, 3]])
    gv, gt, gi = ts.subdivide_to_size(v, f, 2.0, return_index=True)
    assert np.array_equal(gv.numpy(), v[[0, 2, 3, 4]].astype(np.float64))
    assert gt.tolist() == [[3, 2, 1], [0, 1, 2]] and gi.tolist() == [0, 1]


def test_an_empty_mesh_gives_empty_tensors(ts):
    gv, gt, gi = ts.subdivide_to_size(np.zeros((3, 3)), np.zeros((0, 3), dtype=np.int64), 1.0, return_index=True)
    assert gv.shape == (0, 3) and gt.shape == (0, 3) and gi.shape == (0,)
    assert gv.dtype == torch.float64 and gt.dtype == torch.int32 and gi.dtype == torch.int32


def test_a_nan_coordinate_makes_no_triangle_long(ts):
    v = np.array([[0, 0, 0], [100, np.nan, 0], [np.nan, 100, 0], [0, 0, 50]], dtype=np.float64)
    f = np.array([[0, 1, 2], [2, 3, 2]])                                         # every edge of both has a nan length
    gv, gt = ts.subdivide_to_size(v, f, 1.0, max_iter=0)
    assert gt.tolist() == f.tolist() and np.array_equal(gv.numpy(), v, equal_nan=True)


def test_bad_arguments(ts):
    v, f = inputs.box_room()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_edge"):
            ts.subdivide_to_size(v, f, bad)
    with pytest.raises(ValueError, match="max_iter"):
        ts.subdivide_to_size(v, f, 1.0, max_iter=-1)
    with pytest.raises(ValueError, match="outside"):
        ts.subdivide_to_size(v, np.array([[0, 1, 8]]), 1.0)
    with pytest.raises(ValueError, match="midpoint_order"):
        ts.subdivide_to_size(v, f, 1.0, midpoint_order="hash")
