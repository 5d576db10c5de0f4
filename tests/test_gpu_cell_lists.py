"""The fused path's tile lists per CELL of several tiles (dnsplat_bin_cells / dnsplat_raster_cells, DNSPLAT_BIN_CELL).

A cell list is the depth-ordered union of the tight per-tile lists of the cell's tiles; every 16x8 half tile of the cell takes it in
batches of 64, culls what cannot reach its own pixels and walks the rest.  So for every cell shape the images are the per-tile
(1x1) images bit for bit, the gradients stay inside the allowance the parity suite holds the per-tile path to, and everything
``last_info`` says about tile lists is what 1x1 says.  Small frames: a few thousand anisotropic Gaussians, tile grids that are no
multiple of any cell."""
import contextlib

import pytest
import torch

from _scenes import assert_close, assert_equal_int

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = ("1x1", "2x1", "1x2", "2x2", "4x2")
KEYS = ("rgb", "depth", "normal", "accumulation")


@contextlib.contextmanager
def cell(shape):
    from dn_splatter_amd import _ops

    prev = dict(_ops.BIN_CELL)
    _ops.set_bin_cell(shape)
    try:
        yield
    finally:
        _ops.BIN_CELL.update(prev)


def _params(N, seed, sh_rest_std=0.1):
    """Raw parameters of N anisotropic Gaussians with spread opacities (the parity suite's recipe), on the CPU."""
    from dn_splatter_amd import synthetic

    gp = synthetic.make_gauss_params(N, sh_rest_std=sh_rest_std, seed=seed)
    g = torch.Generator().manual_seed(seed + 77)
    gp["scales"] = gp["scales"].detach() + torch.randn(N, 3, generator=g) * 0.6
    gp["opacities"] = gp["opacities"].detach() + torch.randn(N, 1, generator=g) * 2.0
    return {k: v.detach() for k, v in gp.items()}


def _frame(dns, gp, cam, shape, cot=None):
    """One fused get_outputs (+ backward over ``cot``) with the given cell shape: (images, gradients, renderer)."""
    p = {k: v.detach().to(DEV).clone().requires_grad_(k != "normals") for k, v in gp.items()}
    with cell(shape):
        m = dns.DNSplatterRenderer(p, fused=True)
        out = m.get_outputs(cam.to(DEV))
        assert m.last_info["tight_tiles"] and m.last_info["cell_shape"] == tuple(int(x) for x in shape.split("x"))
        if cot is not None:
            torch.autograd.backward([out[k] for k in KEYS], [c.to(DEV) for c in cot])
        torch.cuda.synchronize()
    return {k: out[k].detach().clone() for k in KEYS}, {k: v.grad.clone() for k, v in p.items() if v.grad is not None}, m


# ---- odd cell edges ------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("W,H,N,focal", [(72, 40, 3000, 55.0),      # 5 x 3 tiles: odd on both axes, the last column is 8 pixels wide
                                         (16, 16, 1500, 14.0)])     # one tile in a cell that is otherwise outside the image
def test_images_equal_the_per_tile_images_for_every_cell_shape(dns, W, H, N, focal):
    from dn_splatter_amd import synthetic

    gp = _params(N, seed=41)
    cam = synthetic.orbit_camera(2, width=W, height=H, focal=focal)
    ref, _, m1 = _frame(dns, gp, cam, "1x1")
    n1 = int(m1.last_info["n_isects"])
    assert n1 > 0 and int(m1.last_info["n_cell_pairs"]) == n1
    for shape in SHAPES[1:]:
        out, _, m = _frame(dns, gp, cam, shape)
        for k in KEYS:
            assert torch.equal(out[k], ref[k]), f"{W}x{H}, cells {shape}: {k} differs from the per-tile image"
        nc = int(m.last_info["n_cell_pairs"])
        print(f"[cells] {W}x{H} cells {shape}: {nc} cell pairs for {n1} tile pairs")
        assert int(m.last_info["n_isects"]) == n1 and 0 < nc <= n1


# ---- several batches and buckets: gradients against the oracle ------------------------------------------------------------------


@pytest.fixture(scope="module")
def dense(dns, orc):
    """A frame whose lists run over several 64-entry batches and 128-splat buckets, its oracle side computed ONCE (the reference
    sequence in fp32 and fp64, test_gpu_parity._mirror_pair) and the cotangents that pair was run with."""
    from dn_splatter_amd import _ops, synthetic
    from test_gpu_parity import OUT_KEYS, _mirror_pair
    from _scenes import zero_borderline

    assert OUT_KEYS == KEYS
    gp = _params(6000, seed=23)
    cam = synthetic.orbit_camera(3, width=88, height=72, focal=70.0)       # 6 x 5 tiles
    prev = _ops.DETERMINISTIC["on"]
    dns.set_deterministic(True)
    try:
        with cell("2x2"):
            hip, ora, keep = _mirror_pair(dns, orc, gp, cam, dict(fused=True), cot_seed=6, what="cell lists, dense frame")
    finally:
        dns.set_deterministic(prev)
    gen = torch.Generator().manual_seed(6)         # _mirror_pair's cotangents, drawn again
    cot = [zero_borderline(torch.rand(ora[0][k].shape, generator=gen) * 2 - 1, keep) for k in KEYS]
    return dict(gp=gp, cam=cam, hip=hip, ora=ora, keep=keep, cot=cot)


@pytest.mark.usefixtures("hip_deterministic")
def test_gradients_stay_inside_the_oracle_allowance_for_every_cell_shape(dns, dense):
    from test_gpu_parity import _check_mirror

    ref = None
    for shape in SHAPES:
        out, grads, m = _frame(dns, dense["gp"], dense["cam"], shape, dense["cot"])
        p = {k: torch.zeros(0) for k in dense["gp"]}
        hip = (out, {k: _WithGrad(grads.get(k)) for k in p}, m)
        _check_mirror(hip, dense["ora"], dense["keep"], f"cells {shape}", ints=False)
        if ref is None:
            ref = out
        for k in KEYS:
            assert torch.equal(out[k], ref[k]), (shape, k)
        b = m.last_info["_cell_lists"]
        n = b.n_isects
        lens = (b.tile_ends.long() - b.tile_offsets[:-1].long()).clamp_min(0)
        if shape == "1x1":
            # the shape of the work, from the busiest tile's list: how many of its entries reach alpha >= 1/255 at some pixel centre of
            # the tile's upper half — those every cull keeps (a lower bound of what that half tile keeps), more than one bucket of 128
            info = m.last_info
            t = int(lens.argmax())
            ids = b.flatten_ids[int(b.tile_offsets[t]):int(b.tile_ends[t])].long()
            xy, con = info["means2d"].detach().reshape(-1, 2)[ids].double(), info["conics"].detach().reshape(-1, 3)[ids].double()
            op = torch.sigmoid(dense["gp"]["opacities"].to(DEV).double()).reshape(-1)[ids]
            tx, ty = t % info["tile_width"], t // info["tile_width"]
            px = (tx * 16 + torch.arange(16, device=DEV).double() + 0.5).repeat(8)
            py = (ty * 16 + torch.arange(8, device=DEV).double() + 0.5).repeat_interleave(16)
            dx, dy = px[None] - xy[:, :1], py[None] - xy[:, 1:]
            sig = 0.5 * (con[:, :1] * dx * dx + con[:, 2:] * dy * dy) + con[:, 1:2] * dx * dy
            kept = int(((op[:, None] * torch.exp(-sig)) >= 1.0 / 255 + 1e-9).any(1).sum())
            print(f"[cells] dense frame: the busiest tile lists {ids.numel()} Gaussians, its upper half keeps at least {kept}")
            assert kept > 128
        print(f"[cells] dense frame, cells {shape}: {n} list entries, longest list {int(lens.max())}")
        assert int(lens.max()) > 64
    # two runs of one shape: the same bits (deterministic mode)
    o1, g1, _ = _frame(dns, dense["gp"], dense["cam"], "2x2", dense["cot"])
    o2, g2, _ = _frame(dns, dense["gp"], dense["cam"], "2x2", dense["cot"])
    for k in g1:
        assert torch.equal(g1[k], g2[k]), "two runs of 2x2 cells differ in grad " + k


class _WithGrad:
    """What _check_mirror reads of a parameter: its ``.grad``."""

    def __init__(self, grad):
        self.grad = grad


# ---- plane indexing -------------------------------------------------------------------------------------------------------------


@pytest.mark.usefixtures("hip_deterministic")
def test_backward_through_the_forward_masks_agrees_with_the_one_that_culls_itself(dns, dense):
    """2x2 cells: eight planes of keep masks.  The backward that takes the forward's ballots and the instantiation that runs the
    rectangle test again take the same decisions, so they add the same rows (deterministic mode: in the same order) — equal up to
    what two differently scheduled instantiations of one sum may differ by, the 1e-5 of the tensor's scale the suite allows two
    evaluation orders of one frame (deferred vs sync, tight vs gsplat boxes).  A half tile reading another plane's words would drop or
    add whole splats."""
    from dn_splatter_amd import _ops

    res = {}
    prev = _ops.KEEP_MASKS
    try:
        for masks in (True, False):
            _ops.KEEP_MASKS = masks
            res[masks] = _frame(dns, dense["gp"], dense["cam"], "2x2", dense["cot"])
    finally:
        _ops.KEEP_MASKS = prev
    assert res[True][2].last_info["_cell_lists"].keep is not None and res[False][2].last_info["_cell_lists"].keep is None
    for k in KEYS:
        assert torch.equal(res[True][0][k], res[False][0][k]), k
    for k in res[True][1]:
        assert_close(res[True][1][k], res[False][1][k], "2x2 cells, masks vs re-derived cull: grad " + k, tol=1e-5)


# ---- the list contract ----------------------------------------------------------------------------------------------------------


def _lists(info):
    """(flatten_ids, offsets incl. the end) of ``last_info``, on the CPU."""
    fid = info["flatten_ids"].cpu().long()
    offs = torch.cat([info["isect_offsets"].reshape(-1).cpu().long(), torch.tensor([fid.numel()])])
    return fid, offs


def _check_contract(info1, info, shape, orc_lists=None):
    """``info`` (cells ``shape``) against ``info1`` (1x1) of the same frame(s)."""
    cw, ch = (int(x) for x in shape.split("x"))
    C, th, tw = info1["isect_offsets"].shape
    fid1, offs1 = _lists(info1)
    # what last_info says about tile lists is what 1x1 says
    fid, offs = _lists(info)
    assert int(info["n_isects"]) == int(info1["n_isects"]) == fid1.numel()
    assert_equal_int(fid, fid1, f"cells {shape}: last_info flatten_ids")
    assert_equal_int(offs, offs1, f"cells {shape}: last_info isect_offsets")
    # the kernels' own lists: per cell, the depth-ordered union of the cell's tile lists, every Gaussian once
    b = info["_cell_lists"]
    assert (b.list_width, b.list_height) == (-(-tw // cw), -(-th // ch))
    n = b.n_isects
    assert n == int(info["n_cell_pairs"])
    cfid = b.flatten_ids[:n].cpu().long()
    starts, ends = b.tile_offsets[:-1].cpu().long(), b.tile_ends.cpu().long()
    depths = info["depths"].reshape(-1).cpu()
    empty = 0
    pos = 0
    for c in range(C):
        for cy in range(b.list_height):
            for cx in range(b.list_width):
                parts = []
                for ty in range(cy * ch, min((cy + 1) * ch, th)):
                    for tx in range(cx * cw, min((cx + 1) * cw, tw)):
                        t = (c * th + ty) * tw + tx
                        parts.append(fid1[offs1[t]:offs1[t + 1]])
                ids = torch.unique(torch.cat(parts))                       # ascending entry index
                # depth order, ties by entry index: the order every tile list has (a stable sort of the index-sorted entries)
                want = ids[torch.sort(depths[ids].view(torch.int32), stable=True).indices]
                l = (c * b.list_height + cy) * b.list_width + cx
                got = cfid[starts[l]:ends[l]] if ends[l] > starts[l] else cfid[:0]
                assert_equal_int(got, want, f"cells {shape}: list of cell ({cx}, {cy}) of camera {c}")
                if want.numel():
                    assert int(starts[l]) == pos, f"cells {shape}: the lists are not stored back to back in cell order"
                pos += want.numel()
                empty += want.numel() == 0
    assert pos == n
    return empty


def test_cell_lists_are_the_depth_ordered_unions_of_the_tile_lists(dns, orc):
    """Two cameras in one batch and a frame with empty cells; the per-tile lists are the oracle's in order, with pairs left out."""
    from dn_splatter_amd import synthetic

    N, W, H = 2500, 104, 56                                               # 7 x 4 tiles
    gp = _params(N, seed=57)
    cams = [synthetic.orbit_camera(i, width=W, height=H, focal=120.0).to(DEV) for i in (1, 4)]
    # a second scene pushed into the image's left half: whole cells stay empty
    gq = {k: v.clone() for k, v in gp.items()}
    gq["scales"] = gq["scales"] - 1.2
    cam_side = synthetic.orbit_camera(1, width=W, height=H, focal=30.0)     # the whole cloud a quarter of the image wide
    cam_side.cx = float(cam_side.cx) - 0.4 * W

    def batch(params, cameras, shape):
        p = {k: v.to(DEV) for k, v in params.items()}
        with cell(shape):
            m = dns.DNSplatterRenderer(p, fused=True)
            outs = m.get_outputs_batch(cameras)
            torch.cuda.synchronize()
        return outs, m.last_info

    for what, params, cameras in (("two cameras", gp, cams), ("empty cells", gq, [cam_side.to(DEV)])):
        outs1, info1 = batch(params, cameras, "1x1")
        # the per-tile tight lists against the oracle's lists of the kernel's own projection: the same tiles in the same order, pairs left out
        fid1, offs1 = _lists(info1)
        C = len(cameras)
        for c in range(C):
            with torch.no_grad():
                _t, isect_ids, fid_o = orc.isect_tiles(info1["means2d"][c].detach().cpu(), info1["radii"][c].cpu(), info1["depths"][c].detach().cpu(),
                                                      16, info1["tile_width"], info1["tile_height"])
            tile_o = (isect_ids >> 32).long()
            T = info1["tile_width"] * info1["tile_height"]
            lo, hi = int(offs1[c * T]), int(offs1[(c + 1) * T])
            tile_g = torch.searchsorted(offs1, torch.arange(lo, hi), right=True) - 1 - c * T
            key_g, key_o = tile_g * N + (fid1[lo:hi] - c * N), tile_o * N + fid_o.long()
            assert torch.equal(key_o[torch.isin(key_o, key_g)], key_g), f"{what}: the 1x1 lists are not an order-preserving sub-list of the oracle's"
        empties = []
        for shape in SHAPES[1:]:
            outs, info = batch(params, cameras, shape)
            for o, o1 in zip(outs, outs1):
                for k in KEYS:
                    assert torch.equal(o[k], o1[k]), (what, shape, k)
            empties.append(_check_contract(info1, info, shape))
        print(f"[cells] {what}: empty cells per shape {dict(zip(SHAPES[1:], empties))}")
        if what == "empty cells":
            assert min(empties) > 0
