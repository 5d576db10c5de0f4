"""The CELLS instantiations of the compositing kernels (csrc/raster_fwd.hip, csrc/raster_bwd.hip: one list per cell of several tiles) at
the batch, bucket and fold edges test_gpu_raster_edges.py holds the per-tile instantiations to.

The edge frames of that file go through ``_ops.rasterize_dn(..., tight=True, tile_boxes=<gsplat's boxes of the frame>)`` under every
cell shape of BIN_CELL_SHAPES, keep masks on and off, both saturation twins, default and deterministic mode — and so do their
cell-interleaved variants (edge_frame(cell=); the frame of capped alphas with the clamping loop only), in which the depths of the tiles of a cell alternate: a half tile then meets keep-mask
words that are 0 inside its walk, fills its buckets from many sparse batches and reads ``last_ids`` as positions in a list that is
mostly someone else's (tests/test_edge_scenes.py asserts those regimes on the CPU; the cases here print them).

Asserted: the kernels' lists are the restatement's cell lists (_cell_binning_ref.py) and the per-tile face of the frame is the oracle's
lists; images and all five gradient tensors are bit-equal to the 1x1 run of the same frame in the same mode (every contributing splat
reaches one pixel, so a record receives at most two non-zero rows and their sum does not depend on order); and every run matches the
oracle through the parent file's checks."""
import functools

import pytest
import torch

from _scenes import EDGE_SMALL, assert_equal_int, edge_cameras, edge_cell_lists, edge_frame, edge_lists, edge_main_cases, edge_model, \
    edge_tile_boxes, regime_line
from test_gpu_raster_edges import (DEV, GRAD_KEYS, INTR, _check_binning, _check_grads, _check_images, _cot_fused, _exact_oracle,  # noqa: F401
                                   _grads, _leaves, _oracle_fused_frame, _same, _stacked)

pytestmark = pytest.mark.gpu
SHAPES = ("2x1", "1x2", "2x2", "4x2")
IMAGES = ("rgb", "depth", "normal", "accumulation")
# (keep masks, deterministic mode, saturation flag): the clamp-free twin runs only in the default mode
COMBOS = [(masks, det, sat) for masks in (True, False) for det, sat in ((False, 0), (False, 1), (True, 1))]
# name: (edge_frame arguments, the cell shape whose model is printed; None: every shape, the frame is small)
FRAMES = {
    "main": (dict(), ()),
    "main over 2x1 cells": (dict(interleave=True, cell=(2, 1)), ("2x1",)),
    "main over 1x2 cells": (dict(interleave=True, cell=(1, 2)), ("1x2",)),
    "main over 2x2 cells": (dict(interleave=True, cell=(2, 2)), ("2x2",)),
    "main over 4x2 cells": (dict(interleave=True, cell=(4, 2)), ("4x2",)),
    "height40": (dict(), None),
    "height44": (dict(), None),
    "height40 over 2x2 cells": (dict(cell=(2, 2)), None),
    "height40 over 4x2 cells": (dict(cell=(4, 2)), None),
    "height44 over 2x2 cells": (dict(cell=(2, 2)), None),
    "height44 over 4x2 cells": (dict(cell=(4, 2)), None),
    "cap": (dict(), ("2x2",)),
    "cap over 2x2 cells": (dict(interleave=True, cell=(2, 2)), ("2x2",)),
    "deep": (dict(), None),
    "deep over 2x2 cells": (dict(interleave=True, cell=(2, 2)), None),
}


@pytest.fixture(autouse=True)
def _globals_restored(dns):
    """The cell shape, the keep-mask switch, the bin policy, the deterministic mode and the capacity guesses are what they were."""
    from dn_splatter_amd import _ops

    prev = dict(_ops.BIN_CELL), _ops.KEEP_MASKS, _ops.BIN_POLICY["mode"], _ops.DETERMINISTIC["on"]
    hints = dict(_ops.BUFFERS.capacity_hint), dict(_ops.BUFFERS.cell_hint)
    _ops.set_bin_policy("sync")
    yield
    _ops.BIN_CELL.update(prev[0])
    _ops.KEEP_MASKS = prev[1]
    _ops.set_bin_policy(prev[2])
    _ops.set_deterministic(prev[3])
    for d, old in zip((_ops.BUFFERS.capacity_hint, _ops.BUFFERS.cell_hint), hints):
        d.clear()
        d.update(old)


@functools.lru_cache(maxsize=None)
def _cframe(name):
    """(frame, the oracle's per-tile lists) of FRAMES[name]."""
    from oracle import oracle as orc

    kw = FRAMES[name][0]
    base = name.split(",")[0].split(" over ")[0]
    if base == "main":
        s = edge_frame(edge_main_cases(), 256, 256, **kw)
    else:
        W, H, cases, kw0 = EDGE_SMALL[base]
        s = edge_frame(cases, W, H, **dict(kw0, **kw))
    return s, edge_lists(orc, s)


@functools.lru_cache(maxsize=None)
def _coracle(name, seed=2):
    from oracle import oracle as orc

    s, (offs, fid) = _cframe(name)
    cot = _cot_fused(s, seed)
    return (cot,) + _oracle_fused_frame(orc, s, offs, fid, cot, s["background8"][:3])


def _shifts(shape):
    from dn_splatter_amd import _ops

    return _ops.BIN_CELL_SHAPES[shape]


def _hip_fused_cells(frames, lists, cots, shape, masks, det, sat, check_lists, bg_rgb=None):
    """test_gpu_raster_edges._hip_fused over the frames' gsplat boxes with one list per cell of ``shape``.  ``check_lists``: the kernels'
    lists against the restatement's cell lists and the frame's per-tile face against the oracle's lists.
    -> per camera ((rgb, depth, normal, accumulation), grads), figures of the lists"""
    from dn_splatter_amd import _ops

    assert _ops.SATURATION_FLAG
    _ops.set_bin_cell(shape)
    _ops.set_deterministic(det)
    _ops.KEEP_MASKS = masks
    s0 = frames[0]
    sx, sy = _shifts(shape)
    lv = [_leaves(s, s["colors8"][:, :7]) for s in frames]
    splats = torch.cat([_ops._PackFn.apply(l["xys"], l["conics"], l["opacities"], l["colors"]) for l in lv])
    m2d = torch.stack([l["xys"].detach() for l in lv]).clone().requires_grad_(True)
    holder = {"saturation_flag": torch.tensor([sat], dtype=torch.int32, device=DEV)}
    boxes = torch.stack([edge_tile_boxes(s) for s in frames]).to(DEV).contiguous()
    outs = _ops.rasterize_dn(m2d, splats, *_stacked(frames), background_rgb=(s0["background8"][:3] if bg_rgb is None else bg_rgb).to(DEV),
                             width=s0["W"], height=s0["H"], intrinsics=[INTR] * len(frames), absgrad=True, holder=holder, tight=True,
                             tile_boxes=boxes)[:4]
    assert bool(holder["saturation_flag"].item() == sat)
    b = holder["binning"]
    assert (b.keep is not None) == masks
    fig = dict(pairs=b.n_isects, tile_pairs=b.n_tile_pairs, lists=b.list_width * b.list_height * len(frames))
    if shape == "1x1":
        assert b.cells is None and "tile_lists" not in holder
        if check_lists:
            _check_binning(b, frames, lists)
    else:
        assert b.cells == (sx, sy) and (b.list_width, b.list_height) == (-(-s0["tw"] >> sx), -(-s0["th"] >> sy))
        assert b.tile_boxes is boxes and 0 < b.n_isects <= b.n_tile_pairs == sum(l[1].numel() for l in lists)
        if check_lists:
            coffs, cfid = edge_cell_lists(frames, sx, sy)
            assert b.n_isects == cfid.numel()
            assert_equal_int(b.flatten_ids[:b.n_isects].cpu().long(), cfid, f"cells {shape}: flatten_ids")
            assert_equal_int(b.filled_offsets().cpu().long(), coffs, f"cells {shape}: offsets")
            lens = coffs[1:] - coffs[:-1]
            starts, ends = b.tile_offsets[:-1].cpu().long(), b.tile_ends.cpu().long()
            assert_equal_int((ends - starts).clamp_min(0), lens, f"cells {shape}: list lengths")
            assert_equal_int(starts[lens > 0], coffs[:-1][lens > 0], f"cells {shape}: list starts")
            fig["longest"] = int(lens.max())
            _check_binning(holder["tile_lists"], frames, lists)       # the per-tile face: the oracle's lists
    torch.autograd.backward(list(outs), [torch.stack([c[i] for c in cots]).to(DEV) for i in range(4)])
    torch.cuda.synchronize()
    return [(tuple(o[c].detach().cpu() for o in outs), _grads(m2d, lv[c], c)) for c in range(len(frames))], fig


_BASE = {}


def _baseline(key, frames, lists, cots, combo, bg_rgb=None):
    """The 1x1 run (the per-tile instantiations over the same boxes) of a frame in one combination, computed once."""
    k = (key,) + combo
    if k not in _BASE:
        _BASE[k] = _hip_fused_cells(frames, lists, cots, "1x1", *combo, check_lists=combo[1:] == (False, 1), bg_rgb=bg_rgb)[0]
    return _BASE[k]


def _name(shape, combo):
    masks, det, sat = combo
    return f"cells {shape}, keep masks {'on' if masks else 'off'}, {'deterministic' if det else 'default'} mode, saturation flag {sat}"


def _print_cell_regimes(s, c, n_cam, coffs, cfid, shape, what):
    """The cell model of camera ``c``'s case half tiles, printed; returns it by (tile, half)."""
    sx, sy = _shifts(shape)
    n_cells = (coffs.numel() - 1) // n_cam
    model = edge_model(s, coffs[c * n_cells:(c + 1) * n_cells + 1], cfid - c * s["N"], cells=(sx, sy))
    by = {(r["tile"], r["half"]): r for r in model}
    for t, h, n, stop in s["cases"]:
        r = by.get((t, h))
        if r is None:
            assert n == 0
            continue
        assert r["kept"] == n, f"tile {t} half {h}: {r['kept']} kept entries, the recipe has {n}"
        print(regime_line(r, f"{what}, cells {shape}: {n} x {stop}: "))
    return by


def _assert_regime(name, shape, by, s):
    """The regime the case is named for, from the model of the lists the kernels walk."""
    live = [r for r in by.values() if r["queue"] > 0]
    if "over" in name and name.endswith(shape + " cells") and name.startswith("main"):
        # a 2x1 cell holds ONE case tile and the padding tile in front of it, whose entries lie behind the case's: its half tiles meet
        # the culled entries between their own (a bucket from more than two batches), no batch that is all someone else's
        most = 2 if shape == "2x1" else 4
        assert shape == "2x1" or any(r["foreign_gap"] for r in live), "no all-foreign batch inside a walk"
        assert any(tk == 128 and nb > most for r in live for tk, nb in zip(r["takes_masks"], r["batches_masks"])), \
            f"no bucket from > {most} batches"
        assert {r["fold"] for r in live} == {1, 2, 4} and any(r["stop_ends_batch"] for r in by.values())
    if name.startswith("height"):
        # cells whose lower tiles lie partly (or, for the half tiles below the image, wholly) outside the image
        sy = _shifts(shape)[1]
        assert s["th"] % (1 << sy) != 0 or sy == 0
        low = by[(9, 1)]
        assert low["kept"] == 97 and (low["contrib"] == 0 and low["hi"] == -1 if s["H"] == 40 else 0 < low["contrib"] < 97)
    if name.startswith("deep"):
        assert by[(3, 1)]["queue"] == 20001 and len(by[(3, 1)]["takes_masks"]) > 150


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", sorted(FRAMES))
def test_cell_kernels_equal_the_per_tile_kernels_and_the_oracle(orc, name, shape):
    s, (offs, fid) = _cframe(name)
    cot, imgs_o, g_o, A, S, _g64 = _coracle(name)
    modelled = FRAMES[name][1]
    by = None
    if modelled is None or shape in modelled:
        coffs, cfid = edge_cell_lists([s], *_shifts(shape))
        by = _print_cell_regimes(s, 0, 1, coffs, cfid, shape, name)
        _assert_regime(name, shape, by, s)
    # capped alphas: the projection would have raised the saturation flag, so the clamp-free twin (flag 0) is not a valid run of that frame
    combos = [c for c in COMBOS if c[2] == 1 or not name.startswith("cap")]
    for combo in combos:
        masks, det, sat = combo
        (i1, g1), = _baseline(name, [s], [(offs, fid)], [cot], combo)
        ((imgs, g),), fig = _hip_fused_cells([s], [(offs, fid)], [cot], shape, *combo, check_lists=combo == combos[0])
        what = f"{name}, {_name(shape, combo)}"
        if combo == combos[0]:
            print(f"[raster] {name}, cells {shape}: {fig['pairs']} cell pairs for {fig['tile_pairs']} tile pairs in {fig['lists']} lists, "
                  f"longest {fig['longest']}")
            assert fig["pairs"] < fig["tile_pairs"] or not name.startswith("main")
        for a, b, nm in zip(imgs, i1, IMAGES):
            _same(a, b, f"{what} vs 1x1: {nm}")
        for k in GRAD_KEYS:
            _same(g[k], g1[k], f"{what} vs 1x1: grad {k}")
        _check_images(imgs, imgs_o, what, IMAGES)
        _check_grads(g, g_o, A, S, s, what, det, epilogue=True)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("interleaved", [False, True])
def test_camera_batch_over_cells(orc, shape, interleaved):
    """Three cameras in one launch: lists, keep-mask words and planes at non-zero camera offsets, counted in cells."""
    frames = edge_cameras(**(dict(cell=(2, 2)) if interleaved else {}))
    lists = [edge_lists(orc, s) for s in frames]
    key = f"cameras{' over 2x2 cells' if interleaved else ''}"
    bg = frames[0]["background8"][:3]
    cots = [_cot_fused(s, 10 + c) for c, s in enumerate(frames)]
    coffs, cfid = edge_cell_lists(frames, *_shifts(shape))
    gaps = 0
    for c, s in enumerate(frames):
        by = _print_cell_regimes(s, c, len(frames), coffs, cfid, shape, f"{key}, camera {c}")
        gaps += sum(r["foreign_gap"] for r in by.values())
        if c:
            assert min(r["rs"] for r in by.values()) > 0
    if interleaved and shape == "2x2":
        assert gaps > 0, "no all-foreign batch inside a walk"
    oracle = [_oracle_fused_frame(orc, s, *lists[c], cots[c], bg) for c, s in enumerate(frames)]
    for combo in COMBOS:
        det = combo[1]
        base = _baseline(key, frames, lists, cots, combo, bg_rgb=bg)
        batch, fig = _hip_fused_cells(frames, lists, cots, shape, *combo, check_lists=combo == COMBOS[0], bg_rgb=bg)
        if combo == COMBOS[0]:
            print(f"[raster] {key}, cells {shape}: {fig['pairs']} cell pairs for {fig['tile_pairs']} tile pairs in {fig['lists']} lists")
            assert fig["pairs"] < fig["tile_pairs"]
        for c, s in enumerate(frames):
            what = f"{key}, camera {c}, {_name(shape, combo)}"
            for a, b, nm in zip(batch[c][0], base[c][0], IMAGES):
                _same(a, b, f"{what} vs 1x1: {nm}")
            for k in GRAD_KEYS:
                _same(batch[c][1][k], base[c][1][k], f"{what} vs 1x1: grad {k}")
            imgs_o, go, A, S, _ = oracle[c]
            _check_images(batch[c][0], imgs_o, what, IMAGES)
            _check_grads(batch[c][1], go, A, S, s, what, det, epilogue=True)
