"""The bin policies ("capacity", "deferred", "static" / graph.GraphedStep) over list cells.

A frame binned per cell keeps TWO capacities per frame size — ``capacity_hint`` in (tile, Gaussian) pairs and ``cell_hint`` in (cell,
Gaussian) pairs, with ``n_max`` / ``n_max_cells`` and ``static_cap`` / ``static_cap_cells`` under "static" — and its count arrives as two
words.  The policy tests of test_gpu_parity.py run below BIN_CELL_MIN_TILES and never touch the second set; here the same frames
(320 x 240 / 20 000 Gaussians, 256 x 192 / 30 000) are forced onto 2x2 cells.  Deterministic mode throughout: the lists of every policy
are those of "sync", so images AND gradients are compared with torch.equal."""
import pytest
import torch

from _scenes import assert_equal_int

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip_deterministic")]
DEV = "cuda:0"
KEYS = ("rgb", "depth", "normal", "accumulation")
CELLS = (1, 1)                                   # the shifts of 2x2 cells: what the keys of the cell records end in


@pytest.fixture(autouse=True)
def two_by_two(dns):
    """2x2 cells at every frame size for the test; cell shape, bin policy and capacity guesses are what they were afterwards."""
    from dn_splatter_amd import _ops

    prev = dict(_ops.BIN_CELL), _ops.BIN_POLICY["mode"]
    hints = dict(_ops.BUFFERS.capacity_hint), dict(_ops.BUFFERS.cell_hint)
    _ops.set_bin_cell("2x2")
    yield
    _ops.BIN_CELL.update(prev[0])
    _ops.set_bin_policy(prev[1])
    for d, old in zip((_ops.BUFFERS.capacity_hint, _ops.BUFFERS.cell_hint), hints):
        d.clear()
        d.update(old)


class _Scene:
    """20 000 Gaussians seen at 320 x 240 (300 tiles, 150 cells): frames with a backward over fixed cotangents under a given policy."""

    def __init__(self, dns, seed, view=2):
        from dn_splatter_amd import synthetic

        self.dns = dns
        self.gp = synthetic.make_gauss_params(20_000, sh_rest_std=0.1, seed=seed, device=DEV)
        self.cam = synthetic.orbit_camera(view, width=320, height=240, focal=200.0).to(DEV)
        gen = torch.Generator(device=DEV).manual_seed(3)
        self.cot = [torch.rand((240, 320, c), device=DEV, generator=gen) * 2 - 1 for c in (3, 1, 3, 1)]
        self.key = (torch.device(DEV), 20_000, 320, 240)

    def frame(self, policy):
        self.dns.set_bin_policy(policy)
        for v in self.gp.values():
            v.grad = None
        r = self.dns.DNSplatterRenderer(self.gp, fused=True)
        out = r.get_outputs(self.cam)
        assert r.last_info["cell_shape"] == (2, 2) and r.last_info["_cell_lists"].cells == CELLS
        torch.autograd.backward([out[k] for k in KEYS], self.cot)
        torch.cuda.synchronize()
        return ({k: out[k].detach().clone() for k in KEYS}, {k: v.grad.clone() for k, v in self.gp.items() if v.grad is not None}, r)


def _lists(r):
    info = r.last_info
    return dict(n_isects=int(info["n_isects"]), n_cell_pairs=int(info["n_cell_pairs"]), flatten_ids=info["flatten_ids"].clone(),
                isect_offsets=info["isect_offsets"].clone(), cell_ids=info["_cell_lists"].flatten_ids[:int(info["n_cell_pairs"])].clone())


def _assert_same_frame(got, want, what):
    (o, g, r), (o0, g0, l0) = got, want
    for k in KEYS:
        assert torch.equal(o[k], o0[k]), f"{what}: {k}"
    assert set(g) == set(g0)
    for k in g0:
        assert torch.equal(g[k], g0[k]), f"{what}: grad {k}"
    l = _lists(r)
    assert (l["n_isects"], l["n_cell_pairs"]) == (l0["n_isects"], l0["n_cell_pairs"]), what
    for k in ("flatten_ids", "isect_offsets", "cell_ids"):
        assert_equal_int(l[k], l0[k], f"{what}: {k}")


def _emit_counter(monkeypatch):
    """Counts the emit + tile sort launches of the cell lists (the per-tile face a test reads sorts its own lists, without cells)."""
    from dn_splatter_amd import _lib

    calls = []
    real = _lib.run

    def spy(name, fn, *args):
        if name == "dnsplat_bin_emit_sort" and fn is _lib.lib().dnsplat_bin_emit_sort_cells:
            calls.append(name)
        return real(name, fn, *args)

    monkeypatch.setattr(_lib, "run", spy)
    return calls


def test_capacity_policy_reruns_when_either_guess_is_short(dns, monkeypatch):
    from dn_splatter_amd import _ops

    sc = _Scene(dns, seed=15)
    hints, cell_hints = _ops.BUFFERS.capacity_hint, _ops.BUFFERS.cell_hint
    key, ckey = sc.key, sc.key + CELLS
    o0, g0, r0 = sc.frame("sync")
    want = (o0, g0, _lists(r0))
    n_tile, n_cell = want[2]["n_isects"], want[2]["n_cell_pairs"]
    print(f"[cells] capacity: {n_cell} cell pairs for {n_tile} tile pairs; guesses {cell_hints[ckey]} / {hints[key]}")
    assert 1000 < n_cell < n_tile and hints[key] >= n_tile and cell_hints[ckey] >= n_cell
    calls = _emit_counter(monkeypatch)
    for what, plant in (("short cell guess", lambda: cell_hints.__setitem__(ckey, 1000)),
                        ("short tile guess, the cell guess fits", lambda: hints.__setitem__(key, 1000)),
                        ("both guesses fit", lambda: None)):
        plant()
        fits = what == "both guesses fit"
        assert fits or _ops._capacity_guess(key, CELLS) == 1000
        del calls[:]
        got = sc.frame("capacity")
        print(f"[cells] capacity, {what}: {len(calls)} emit launches, lists of {got[2].last_info['_cell_lists'].flatten_ids.numel()} entries")
        assert len(calls) == (1 if fits else 2), what
        cap = got[2].last_info["_cell_lists"].flatten_ids.numel()
        assert cap == n_cell if not fits else cap >= n_cell, f"{what}: the re-run takes the exact size"
        _assert_same_frame(got, want, "capacity, " + what)
        assert hints[key] >= n_tile and cell_hints[ckey] >= n_cell, what


def test_deferred_policy_raises_on_a_short_cell_guess_and_the_repeated_step_fits(dns):
    from dn_splatter_amd import _lib, _ops

    sc = _Scene(dns, seed=4)
    cell_hints = _ops.BUFFERS.cell_hint
    ckey = sc.key + CELLS
    o0, g0, r0 = sc.frame("sync")
    want = (o0, g0, _lists(r0))
    n_tile, n_cell = want[2]["n_isects"], want[2]["n_cell_pairs"]
    got = sc.frame("deferred")
    b = got[2].last_info["_cell_lists"]
    assert b.pending is not None or b._n is not None
    _assert_same_frame(got, want, "deferred")
    cell_hints[ckey] = 1000                                               # far below the real count; the per-tile guess fits
    with pytest.raises(_lib.DnsplatError, match="exceed the capacity"):
        sc.frame("deferred")
        _ops.verify_pending_counts(torch.device(DEV), block=True)
    print(f"[cells] deferred: {n_cell} cell pairs against a guess of 1000 raised; the guess is {cell_hints[ckey]} now")
    assert cell_hints[ckey] >= n_cell and _ops.BUFFERS.capacity_hint[sc.key] >= n_tile
    dns.set_bin_policy("deferred")
    for v in sc.gp.values():
        v.grad = None
    r = dns.DNSplatterRenderer(sc.gp, fused=True)
    out = r.get_outputs(sc.cam)
    b = r.last_info["_cell_lists"]
    pending = b.pending
    assert pending is not None and pending.cells == CELLS and pending.capacity == cell_hints[ckey], "the repeated step is deferred again"
    # the per-tile count is the second word of the frame's pending slot: reading it is what waits, and nothing else is asked
    assert int(r.last_info["n_isects"]) == n_tile == pending.n_tile == int(pending.slot[1]) and pending.n == n_cell == int(pending.slot[0])
    assert b.pending is None and b._n_tile == n_tile
    torch.autograd.backward([out[k] for k in KEYS], sc.cot)
    torch.cuda.synchronize()
    _ops.verify_pending_counts(torch.device(DEV), block=True)
    _assert_same_frame(({k: out[k].detach() for k in KEYS}, {k: v.grad for k, v in sc.gp.items() if v.grad is not None}, r), want,
                       "deferred, the repeated step")


def _cell_records(stream):
    from dn_splatter_amd import _ops

    skey = (torch.device(DEV), stream.cuda_stream)
    return [k for d in (_ops.BUFFERS.n_max_cells, _ops.BUFFERS.static_cap_cells) for k in d if k[:2] == skey]


def test_graphed_step_over_cells_replays_equal_eager_frames(dns):
    from dn_splatter_amd import dp, synthetic
    from dn_splatter_amd.graph import GraphedStep

    sc = _Scene(dns, seed=6, view=1)
    poses = [synthetic.orbit_camera(i, width=320, height=240, focal=200.0).to(DEV) for i in (1, 3)]
    ref = []
    for c in poses:
        sc.cam.camera_to_worlds.copy_(c.camera_to_worlds)
        o, g, r = sc.frame("sync")
        ref.append((o, g, int(r.last_info["n_cell_pairs"]), int(r.last_info["n_isects"])))
        r.forget()
    sc.cam.camera_to_worlds.copy_(poses[0].camera_to_worlds)
    r = dns.DNSplatterRenderer(sc.gp, fused=True)

    def compute():
        out = r.get_outputs(sc.cam)
        torch.autograd.backward([out[k] for k in KEYS], sc.cot)
        return out

    for v in sc.gp.values():
        v.grad = None
    step = GraphedStep(compute, params={k: sc.gp[k] for k in dp.GRAD_KEYS})
    try:
        recs = _cell_records(step.stream)
        assert len(recs) == 2 and all(k[2:] == sc.key + CELLS for k in recs), recs
        for i in (0, 1, 0):
            sc.cam.camera_to_worlds.copy_(poses[i].camera_to_worlds)          # a new pose, in place
            out = step()
            torch.cuda.synchronize()
            b = r.last_info["_cell_lists"]
            assert b.cells == CELLS and int(b._n_dev.item()) == ref[i][2] and int(b._n_tile_dev.item()) == ref[i][3]
            for k in KEYS:
                assert torch.equal(out[k], ref[i][0][k]), (i, k)
            for k, g in ref[i][1].items():
                assert torch.equal(sc.gp[k].grad, g), f"graph replay, pose {i}: grad {k}"
        step.check()
        from dn_splatter_amd import _ops

        skey = (torch.device(DEV), step.stream.cuda_stream)
        n_max = int(_ops.BUFFERS.n_max_cells[skey + sc.key + CELLS].item())
        cap = _ops.BUFFERS.static_cap_cells[skey + sc.key + CELLS]
        print(f"[cells] static: running maximum {n_max} cell pairs in buffers of {cap}; per tile {int(_ops.BUFFERS.n_max[skey + sc.key].item())} "
              f"in {_ops.BUFFERS.static_cap[skey + sc.key]}")
        assert n_max == max(ref[0][2], ref[1][2]) <= cap and int(_ops.BUFFERS.n_max[skey + sc.key].item()) == max(ref[0][3], ref[1][3])
    finally:
        stream = step.stream
        step.close()
    assert _cell_records(stream) == []


@pytest.mark.filterwarnings("ignore:The AccumulateGrad node's stream does not match")       # the re-capture runs on a new side stream by design
def test_graphed_step_cell_overflow_is_reported_and_a_recapture_fits(dns):
    """The near pose of test_gpu_parity.test_graphed_step_overflow_is_reported_and_a_recapture_fits against a pose far outside the cloud:
    the near pose needs more CELL pairs than the buffers captured at the far pose hold."""
    from dn_splatter_amd import _lib, _ops, dp, synthetic
    from dn_splatter_amd.graph import GraphedStep

    N, W, H = 30_000, 256, 192
    gp = synthetic.make_gauss_params(N, sh_rest_std=0.1, seed=11, device=DEV)
    far = synthetic.orbit_camera(0, width=W, height=H, focal=60.0).to(DEV)
    # three times as far out as that test's far pose: there a Gaussian sits in 1.8 cells on average (55 085 cell pairs against the near
    # pose's 69 065) and 1.25 x that + 4096 would hold the near pose — cell pairs grow far less with the footprint than tile pairs do
    far.camera_to_worlds[..., :3, 3] *= 3.0
    near = synthetic.orbit_camera(0, width=W, height=H, focal=60.0).to(DEV)
    near.camera_to_worlds[..., :3, 3] *= 0.35
    cam = synthetic.orbit_camera(0, width=W, height=H, focal=60.0).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(3)
    cot = [torch.rand((H, W, c), device=DEV, generator=gen) * 2 - 1 for c in (3, 1, 3, 1)]
    r = dns.DNSplatterRenderer(gp, fused=True)

    def compute():
        out = r.get_outputs(cam)
        torch.autograd.backward([out[k] for k in KEYS], cot)
        return out

    def count(c):
        dns.set_bin_policy("sync")
        r.forget()
        with torch.no_grad():
            r.get_outputs(c)
        n = int(r.last_info["n_cell_pairs"]), int(r.last_info["n_isects"])
        assert r.last_info["cell_shape"] == (2, 2)
        r.forget()
        return n

    hkey = (torch.device(DEV), N, W, H)
    (c_far, t_far), (c_near, t_near) = count(far), count(near)
    print(f"[cells] far / near pose: {c_far} / {c_near} cell pairs, {t_far} / {t_near} tile pairs")
    assert c_near > 1.25 * c_far + 4096 and c_far < t_far and c_near < t_near, "the near pose does not outgrow the far pose's cell buffers"
    _ops.BUFFERS.capacity_hint.pop(hkey, None)                                   # the guesses of the two counting frames
    _ops.BUFFERS.cell_hint.pop(hkey + CELLS, None)
    cam.camera_to_worlds.copy_(far.camera_to_worlds)
    for v in gp.values():
        v.grad = None
    step = GraphedStep(compute, params={k: gp[k] for k in dp.GRAD_KEYS})
    step2 = None
    try:
        step(); step.check()
        captured = _ops.BUFFERS.cell_hint[hkey + CELLS]
        assert c_far <= captured < c_near
        cam.camera_to_worlds.copy_(near.camera_to_worlds)
        step()
        with pytest.raises(_lib.DnsplatError, match="more than the captured buffers hold"):
            step.check()
        print(f"[cells] static overflow: captured for {captured} cell pairs, the guess is {_ops.BUFFERS.cell_hint[hkey + CELLS]} now")
        assert _ops.BUFFERS.cell_hint[hkey + CELLS] >= c_near and _ops.BUFFERS.capacity_hint[hkey] >= t_near
        first = step.stream
        step2 = step.recapture()                                                     # warm-up at the near pose, enlarged buffers
        assert step.graphs == [] and step2.graphs and _cell_records(first) == []
        step2()
        step2.check()
        torch.cuda.synchronize()
        b = r.last_info["_cell_lists"]
        assert int(b._n_dev.item()) == c_near and int(b._n_tile_dev.item()) == t_near and b.flatten_ids.numel() >= c_near
        assert len(_cell_records(step2.stream)) == 2
    finally:
        for s in (step, step2):
            if s is not None:
                s.close()
    assert _cell_records(step.stream) == [] and _cell_records(step2.stream) == []


def test_cells_are_taken_from_1024_tiles_on(dns):
    """Left to itself the fused path takes 2x2 cells from BIN_CELL_MIN_TILES tiles per image on; the images are those of one list per
    tile either way."""
    from dn_splatter_amd import _ops, synthetic

    assert _ops.BIN_CELL_MIN_TILES == 1024
    gp = synthetic.make_gauss_params(20_000, sh_rest_std=0.1, seed=9, device=DEV)
    dns.set_bin_policy("sync")
    for W, H, tiles, shape in ((512, 512, 1024, (2, 2)), (496, 512, 992, (1, 1))):
        cam = synthetic.orbit_camera(1, width=W, height=H, focal=300.0).to(DEV)
        res = {}
        for forced in (None, "1x1"):
            _ops.set_bin_cell(forced)
            r = dns.DNSplatterRenderer(gp, fused=True)
            with torch.no_grad():
                out = r.get_outputs(cam)
            info = r.last_info
            assert info["tile_width"] * info["tile_height"] == tiles
            res[forced] = ({k: out[k].clone() for k in KEYS}, info["cell_shape"], int(info["n_cell_pairs"]), int(info["n_isects"]))
        print(f"[cells] {W} x {H} ({tiles} tiles), unforced: cells {res[None][1]}, {res[None][2]} list entries for {res[None][3]} tile pairs")
        assert res[None][1] == shape and res["1x1"][1] == (1, 1)
        assert res[None][3] == res["1x1"][3] == res["1x1"][2] > 0
        assert (res[None][2] < res[None][3]) if shape == (2, 2) else (res[None][2] == res[None][3])
        for k in KEYS:
            assert torch.equal(res[None][0][k], res["1x1"][0][k]), (W, H, k)
