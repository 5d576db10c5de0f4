"""The subdivision of long triangles on the GPU (csrc/subdivide.hip through dn_splatter_amd.subdivide) against its CPU restatement
(dn_splatter_amd.torch_subdivide) with exact equality — float64 vertices bit for bit, triangles and face_index — on the five inputs of
_subdivide_inputs (a round of one block of long triangles among three, last rounds of exactly one and of four trips of the block-count
scan, a soup with shared edges and repeated vertices), at its edges, and through ``cull_mesh(subdivide=True)``."""
import numpy as np
import pytest
import torch

import _mesh_cull_inputs as cull_inputs
import _subdivide_inputs as inputs

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def sd():
    from dn_splatter_amd import subdivide

    return subdivide


@pytest.fixture(scope="module")
def ts():
    from dn_splatter_amd import torch_subdivide

    return torch_subdivide


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.is_cuda and g.dtype == w.dtype and g.shape == w.shape
        assert torch.equal(g.cpu(), w)


# ---- against the restatement ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(inputs.CASES))
def test_equals_the_restatement(sd, ts, name):
    mesh, max_edge, want_rounds, want_v, want_t = inputs.CASES[name]
    v, f = mesh()
    cpu_rounds, gpu_rounds = [], []
    want = ts.subdivide_to_size(v, f, max_edge, return_index=True, rounds=cpu_rounds)
    got = sd.subdivide_to_size(dev(v), dev(f), max_edge, return_index=True, rounds=gpu_rounds)
    assert gpu_rounds == cpu_rounds and len(gpu_rounds) == inputs.ROUNDS[name]
    if want_rounds is not None:
        assert gpu_rounds == want_rounds
    assert (got[0].shape[0], got[1].shape[0]) == (want_v, want_t)
    assert got[0].dtype == torch.float64 and got[1].dtype == torch.int32 and got[2].dtype == torch.int32
    same(got, want)
    if name in ("box_0.8", "soup_0.12"):
        # float32 and float64 input of the same values: equal bytes; and a second run: equal bytes
        same(sd.subdivide_to_size(dev(v.astype(np.float64)), dev(f.astype(np.int64)), max_edge, return_index=True), want)
        same(sd.subdivide_to_size(dev(v), dev(f), max_edge, return_index=True), want)
        same(sd.subdivide_mesh((dev(v), dev(f), None), max_edge), want[:2])


def test_two_runs_of_the_largest_case_give_equal_bytes(sd):
    v, f = inputs.box_room()
    a = sd.subdivide_to_size(dev(v), dev(f), 0.05, return_index=True)
    b = sd.subdivide_to_size(dev(v), dev(f), 0.05, return_index=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---- edge cases on the device ----------------------------------------------------------------------------------------------------------

def test_the_comparison_is_strict(sd, ts):
    v = np.array([[0.1, 0.2, 0.3], [0.7, 0.9, 0.4], [0.2, 0.8, 1.1]])
    f = np.array([[0, 1, 2]], dtype=np.int32)
    longest = float(ts.edge_lengths(torch.from_numpy(v), torch.from_numpy(f)).max())
    got = sd.subdivide_to_size(dev(v), dev(f), longest, return_index=True)
    same(got, ts.subdivide_to_size(v, f, longest, return_index=True))
    assert got[1].shape[0] == 1 and torch.equal(got[0].cpu(), torch.from_numpy(v))
    below = float(np.nextafter(longest, 0.0))
    got = sd.subdivide_to_size(dev(v), dev(f), below, return_index=True)
    same(got, ts.subdivide_to_size(v, f, below, return_index=True))
    assert got[1].shape[0] == 4 and got[0].shape[0] == 6


def test_nothing_long_drops_the_unreferenced_vertex(sd, ts):
    v = np.array([[0, 0, 0], [9, 9, 9], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
    f = np.array([[4, 3, 2], [0, 2, 3]], dtype=np.int32)
    got = sd.subdivide_to_size(dev(v), dev(f), 2.0, max_iter=0, return_index=True)
    same(got, ts.subdivide_to_size(v, f, 2.0, max_iter=0, return_index=True))
    assert got[0].shape[0] == 4 and got[1].tolist() == [[3, 2, 1], [0, 1, 2]]


def test_a_nan_coordinate_makes_no_triangle_long(sd, ts):
    v = np.array([[0, 0, 0], [100, np.nan, 0], [np.nan, 100, 0], [0, 0, 50]], dtype=np.float64)
    f = np.array([[0, 1, 2], [2, 3, 2]], dtype=np.int32)
    got = sd.subdivide_to_size(dev(v), dev(f), 1.0, max_iter=0)
    assert got[1].tolist() == f.tolist()
    assert torch.equal(got[0].cpu().view(torch.int64), torch.from_numpy(v).view(torch.int64))


def test_an_empty_mesh_gives_empty_tensors(sd):
    got = sd.subdivide_to_size(torch.zeros(3, 3, device=DEV), torch.zeros(0, 3, dtype=torch.int32, device=DEV), 1.0, return_index=True)
    assert [tuple(g.shape) for g in got] == [(0, 3), (0, 3), (0,)] and all(g.is_cuda for g in got)
    assert [g.dtype for g in got] == [torch.float64, torch.int32, torch.int32]


def test_max_iter_exceeded_raises_and_the_next_call_works(sd, ts):
    v, f = inputs.box_room()
    with pytest.raises(ValueError, match="max_iter exceeded"):
        sd.subdivide_to_size(dev(v), dev(f), 0.8, max_iter=2)
    same(sd.subdivide_to_size(dev(v), dev(f), 0.8, max_iter=4), ts.subdivide_to_size(v, f, 0.8, max_iter=4))


def test_an_index_equal_to_v_raises(sd, ts):
    v, f = inputs.box_room()
    f = f.copy()
    f[5, 1] = v.shape[0]
    with pytest.raises(ValueError, match="outside"):
        sd.subdivide_to_size(dev(v), dev(f), 3.0)
    f[5, 1] = -1
    with pytest.raises(ValueError, match="outside"):
        sd.subdivide_to_size(dev(v), dev(f), 3.0)
    v, f = inputs.box_room()
    same(sd.subdivide_to_size(dev(v), dev(f), 3.0), ts.subdivide_to_size(v, f, 3.0))


# ---- through the cull ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=["box", "fitted"])
def box_scene(request):
    """The box room as it is — the poses of _mesh_cull_inputs see it partly from outside — and fitted around them (they stand in a
    room [-2, 2] x [-1, 1] x [-2, 2])."""
    v, f = inputs.box_room()
    if request.param == "fitted":
        v = (v - np.array([2.5, 2.0, 1.5], dtype=np.float32)) * np.array([0.8, 0.5, 4.0 / 3.0], dtype=np.float32)
    return v.astype(np.float32), f, cull_inputs.room_poses(), cull_inputs.K, cull_inputs.HEIGHT, cull_inputs.WIDTH


def test_cull_mesh_with_subdivide_equals_the_restatement_and_the_chain_by_hand(sd, box_scene):
    from dn_splatter_amd import mesh_cull, torch_mesh_cull

    v, f, poses, K, H, W = box_scene
    mesh = (dev(v), dev(f))
    kw = dict(subdivide=True, max_edge=0.2)
    got = mesh_cull.cull_mesh(mesh, poses, K, H, W, **kw)
    want = torch_mesh_cull.cull_mesh((torch.from_numpy(v), torch.from_numpy(f)), poses, K, H, W, **kw)
    fine = sd.subdivide_mesh(mesh, 0.2)
    assert 0 < want[1].shape[0] < fine[1].shape[0]                               # the cull cuts, and not everything
    assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1].to(torch.int32))
    rendered = mesh_cull.render_mesh_depth(mesh[0], mesh[1], poses, K, H, W)     # of the ORIGINAL mesh
    obs, invalid = mesh_cull.vertex_visibility(fine[0], poses, K, H, W, rendered, None, False, True)
    hand = mesh_cull.cut_mesh(fine[0], fine[1], obs, invalid)
    assert torch.equal(got[0], hand[0]) and torch.equal(got[1], hand[1])
    coarse = mesh_cull.cull_mesh(mesh, poses, K, H, W)                           # without it, whole wall triangles stay or go
    assert coarse[1].shape[0] != got[1].shape[0]


def test_cull_mesh_without_subdivide_is_the_call_without_the_keyword(box_scene):
    from dn_splatter_amd import mesh_cull

    v, f, poses, K, H, W = box_scene
    mesh = (dev(v), dev(f))
    a = mesh_cull.cull_mesh(mesh, poses, K, H, W, subdivide=False)
    b = mesh_cull.cull_mesh(mesh, poses, K, H, W)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    room_v, room_f = cull_inputs.room()
    mesh = (dev(room_v), dev(room_f))
    a = mesh_cull.cull_mesh(mesh, poses, K, H, W, subdivide=False, max_edge=0.001, max_iter=0)
    b = mesh_cull.cull_mesh(mesh, poses, K, H, W)
    assert a[0].shape[0] > 0 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
