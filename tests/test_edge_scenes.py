"""The edge scenes of tests/test_gpu_raster_edges.py, checked on the CPU: the oracle's lists have the structure every recipe asks for,
and the float64 model of the compositing kernels (tests/_scenes.py edge_model) puts every case where the recipe says — counts, stop
indices, the backward's bound `hi`, bucket sizes, folds and queue carries — so that the GPU file really walks those edges."""
import pytest
import torch

from _scenes import (EDGE_BOUNDARY_STOPS, EDGE_COUNTS, EDGE_OFFSETS, EDGE_SMALL, allstop_groups, edge_cameras, edge_cell_lists, edge_frame,
                     edge_lists, edge_main_cases, edge_model)


def _by_half(model):
    return {(r["tile"], r["half"]): r for r in model}


def _expected_stops(n, stop, cap):
    """{pixel: list index of the entry that stops it}: a stack's fourth entry (cap: its second)."""
    k = 1 if cap else 3
    if stop == "early" and n >= 5:
        return {5: 1 + k}
    if stop == "boundary":
        return {3 + 9 * (s // 64): s - 3 + k for s in EDGE_BOUNDARY_STOPS if s < n}
    if stop == "allstop" and n >= 8:
        return {(j * 37) % 128: 4 * j + k for j in range(allstop_groups(n))}
    return {}


def _check_cases(s, offs, fid, model, cap=False):
    by = _by_half(model)
    flat = offs.reshape(-1).long()
    first_id = 0                  # the case entries have consecutive ids, case after case
    for k, (t, h, n, stop) in enumerate(s["cases"]):
        first_id += s["cases"][k - 1][2] if k else 0
        r = by.get((t, h))
        if r is None:
            assert n == 0, (t, h)
            continue
        assert r["kept"] == n, f"tile {t} half {h}: {r['kept']} kept entries, the recipe has {n}"
        other = by.get((t, 1 - h))
        assert other is None or other["kept"] == 0, f"tile {t}: the recipe of one half reaches the other"
        inside = s["H"] >= 16 * (t // s["tw"]) + 8 * h + 8
        if inside:
            assert r["contrib"] == n
            # entries of the neighbours whose boxes reach this tile (culled here) may come first
            li = fid[int(flat[t]):int(flat[t]) + r["L"]].long()
            pre = int(torch.nonzero(li == first_id)[0]) if n else 0
            # with interleaving, a culled entry sits in front of every second case entry
            exp = {p: pre + i + (i // 2 if s["interleave"] else 0) for p, i in _expected_stops(n, stop, cap).items()}
            assert r["stop"] == exp, (t, h, n, stop, r["stop"], exp)
        if stop == "allstop" and n >= 8 and inside:
            last = max(_expected_stops(n, stop, cap).values())       # recipe index of the entry that stops the last pixel
            assert r["hi"] == max(r["stop"].values()) - 1 and r["queue"] == last and r["kept_above_hi"] == n - last
        elif inside:
            assert r["queue"] == n - r["kept_above_hi"] and (r["kept_above_hi"] == 0 or stop == "boundary")
        assert r["queue"] + r["kept_above_hi"] == r["kept"]


@pytest.mark.parametrize("interleave,phase", [(False, 0), (True, 0), (False, 1), (True, 2)])
def test_main_edge_frame_has_the_recipe_structure(orc, interleave, phase):
    s = edge_frame(edge_main_cases(), 256, 256, interleave=interleave, phase=phase)
    offs, fid = edge_lists(orc, s)
    model = edge_model(s, offs, fid)
    _check_cases(s, offs, fid, model)
    by = _by_half(model)
    flat = offs.reshape(-1).long()
    for k, (t, h, n, stop) in enumerate(s["cases"]):
        assert int(flat[t]) % 64 == EDGE_OFFSETS[(k + phase) % 3], f"tile {t}: range_start % 64"
    # every list is in recipe order: the case entries of a half tile appear in their id order
    ids = [fid[int(flat[t]):int(flat[t + 1])].long() for t, _h, _n, _s in s["cases"]]
    for (t, h, n, stop), li in zip(s["cases"], ids):
        own = li[li < s["n_case"]]
        own = own[s["xys"][own, 0].floor().long() // 16 == t % s["tw"]]
        own = own[(s["xys"][own, 1].floor().long() // 16) == t // s["tw"]]
        assert own.numel() == n and bool((own[1:] > own[:-1]).all())
        assert (interleave and n > 0) == bool((s["kind"][li.long()] == 1).any())
    # the regimes the GPU file relies on
    never = [by[(t, h)] for t, h, n, stop in s["cases"] if stop == "never" and n > 0]
    last_takes = {[x for x in r["takes_masks"] if x > 0][-1] for r in never}
    assert last_takes == {n % 128 or 128 for n in EDGE_COUNTS if n > 0}
    assert {1, 32, 33, 64, 65, 127, 128} <= last_takes
    folds = {r["fold"] for r in model if r["queue"] > 0}
    assert folds == {1, 2, 4}
    assert any(max(r["carries_masks"] or [0]) > 0 for r in model) and any(max(r["carries_scan"] or [0]) > 0 for r in model)
    # `hi` inside a 64-entry batch with kept entries above it in the same batch: the keep-mask clip (m &= (2 << top) - 1) bites
    assert any(r["kept_above_hi"] > 0 and (r["hi"] + 1) % 64 != 0 for r in model)
    # hi in a later bucket than the last index of most pixels
    assert any(r["n_stopped"] and max(r["stop"].values()) < 128 <= r["hi"] for r in model)
    # no decision of the frame is borderline for the oracle either
    border = torch.zeros(256, 256, dtype=torch.uint8)
    flip = torch.zeros(256, 256)
    orc.rasterize_fwd(s["xys"], s["conics"], s["colors8"][:, :4], s["opacities"], s["background8"][:4], 256, 256, 16, offs, fid,
                      border, flip)
    assert int(border.sum()) == 0


def test_interleaving_and_shifting_keep_the_contributing_entries(orc):
    """The identity frames of the GPU file differ only in culled entries and padding: same ids, same kept entries, same stops."""
    base = edge_frame(edge_main_cases(), 256, 256)
    for kw in (dict(interleave=True), dict(phase=1), dict(interleave=True, phase=2)):
        s = edge_frame(edge_main_cases(), 256, 256, **kw)
        assert s["n_case"] == base["n_case"]
        for k in ("xys", "conics", "opacities", "depths", "radii"):
            assert torch.equal(s[k][:s["n_case"]], base[k][:base["n_case"]])
        assert torch.equal(s["colors8"][:s["n_case"]], base["colors8"][:base["n_case"]])
        assert bool((s["opacities"][s["n_case"]:] < 1.0 / 255.0).all())


@pytest.mark.parametrize("name", sorted(EDGE_SMALL))
def test_small_edge_frames(orc, name):
    W, H, cases, kw = EDGE_SMALL[name]
    s = edge_frame(cases, W, H, **kw)
    offs, fid = edge_lists(orc, s)
    model = edge_model(s, offs, fid)
    _check_cases(s, offs, fid, model, cap=kw.get("cap", False))
    by = _by_half(model)
    if name == "height40":
        assert by[(9, 1)]["kept"] == 97 and by[(9, 1)]["contrib"] == 0 and by[(9, 1)]["hi"] == -1
    if name == "height44":
        assert 0 < by[(9, 1)]["contrib"] < 97
    if name == "deep":
        assert by[(3, 1)]["L"] >= 20_000 and by[(3, 1)]["queue"] == 20001 and len(by[(3, 1)]["takes_masks"]) > 150
    if name == "cap":
        assert bool((s["opacities"] > 0.999).any())


def test_camera_batch_frames_end_on_a_batch_boundary(orc):
    frames = edge_cameras()
    assert len({s["N"] for s in frames}) == 1
    for s in frames:
        offs, fid = edge_lists(orc, s)
        assert fid.numel() % 64 == 0
        last = int(offs.reshape(-1)[-1])
        assert last < fid.numel(), "the last tile's list is not empty"
        _check_cases(s, offs, fid, edge_model(s, offs, fid))


# ---- the same frames when the lists are kept per cell of several tiles (tests/test_gpu_raster_cell_edges.py) ---------------------------


def _cell_models(orc, frames, sx, sy):
    """Per camera: (per-tile model, cell model) by (tile, half); asserts that every half tile keeps, blends and stops on the same
    entries whether it walks its tile's list or its cell's."""
    coffs, cfid = edge_cell_lists(frames, sx, sy)
    n_cells = (coffs.numel() - 1) // len(frames)
    out = []
    for c, s in enumerate(frames):
        offs, fid = edge_lists(orc, s)
        per_tile = _by_half(edge_model(s, offs, fid))
        per_cell = _by_half(edge_model(s, coffs[c * n_cells:(c + 1) * n_cells + 1], cfid - c * s["N"], cells=(sx, sy)))
        assert set(per_tile) == set(per_cell)
        for key, r in per_tile.items():
            q = per_cell[key]
            assert q["kept_ids"] == r["kept_ids"] and q["contrib_ids"] == r["contrib_ids"] and q["stop_ids"] == r["stop_ids"], key
            assert (q["kept"], q["contrib"], q["n_stopped"], q["n_blending"]) == (r["kept"], r["contrib"], r["n_stopped"], r["n_blending"])
            assert q["L"] >= r["L"] and q["list"] == (key[0] // s["tw"] >> sy) * ((s["tw"] + (1 << sx) - 1) >> sx) + (key[0] % s["tw"] >> sx)
        out.append((per_tile, per_cell))
    return out


def _assert_cell_regimes(models, what):
    """What sets the CELLS kernels apart from their parents, each reached by at least one half tile."""
    rs = [r for _t, per_cell in models for r in per_cell.values()]
    live = [r for r in rs if r["queue"] > 0]
    print(f"[raster] {what}: {len(live)} half tiles with work; all-foreign batch inside the walk: {sum(r['foreign_gap'] for r in live)}; "
          f"most batches per full bucket: {max([b for r in live for tk, b in zip(r['takes_masks'], r['batches_masks']) if tk == 128] or [0])}")
    assert any(r["foreign_gap"] for r in live), what + ": no half tile has an all-foreign batch between two batches it keeps entries of"
    assert any(tk == 128 and b > 4 for r in live for tk, b in zip(r["takes_masks"], r["batches_masks"])), \
        what + ": no 128-entry bucket is filled from more than four batches"
    assert {r["fold"] for r in live} == {1, 2, 4}, what
    assert any(max(r["carries_masks"] or [0]) > 0 for r in rs) and any(max(r["carries_scan"] or [0]) > 0 for r in rs), what
    assert any(r["kept_above_hi"] > 0 for r in rs), what
    assert any(r["stop_ends_batch"] for r in rs), what + ": no stop whose entry is the last of a batch of the cell list"


@pytest.mark.parametrize("cw,ch", [(2, 2), (4, 2)])
def test_cell_interleaved_main_frame_reaches_the_cell_regimes(orc, cw, ch):
    sx, sy = cw.bit_length() - 1, ch.bit_length() - 1
    plain = edge_frame(edge_main_cases(), 256, 256, interleave=True)
    s = edge_frame(edge_main_cases(), 256, 256, interleave=True, cell=(cw, ch))
    # the same records but for the depths, every list as long as it was, every tile's own entries in the recipe's order
    for k in ("xys", "conics", "opacities", "radii", "tiles", "kind", "colors8"):
        assert torch.equal(s[k], plain[k]), k
    assert s["fill"] == plain["fill"] and not torch.equal(s["depths"], plain["depths"])
    assert bool((s["depths"] == s["depths"].double().float()).all()) and float(s["depths"].max()) < 2 ** 24
    assert s["depths"].unique().numel() == s["N"]
    offs, fid = edge_lists(orc, s)
    offs0, fid0 = edge_lists(orc, plain)
    assert torch.equal(offs, offs0)
    m0 = _by_half(edge_model(plain, offs0, fid0))
    (per_tile, per_cell), = _cell_models(orc, [s], sx, sy)
    for key, r in m0.items():
        assert per_tile[key]["kept_ids"] == r["kept_ids"] and per_tile[key]["stop_ids"] == r["stop_ids"], key
    _assert_cell_regimes([(per_tile, per_cell)], f"main frame interleaved over {cw}x{ch} cells")
    # the frame as it was, under the same cells: the control — a half tile's entries are one contiguous run of its cell's list
    (_pt, pc0), = _cell_models(orc, [plain], sx, sy)
    assert not any(r["foreign_gap"] for r in pc0.values())


def test_cell_interleaved_camera_batch(orc):
    frames = edge_cameras(cell=(2, 2))
    assert len({s["N"] for s in frames}) == 1
    models = _cell_models(orc, frames, 1, 1)
    _assert_cell_regimes(models, "three cameras interleaved over 2x2 cells")
    assert any(r["rs"] > 0 and r["tile"] < 16 for r in models[2][1].values()), "the last camera's lists start inside the batch"
