"""The numpy restatement of the cell binning (_cell_binning_ref.cell_lists, what test_gpu_cell_binning.py holds the kernels to) against
the contract test_gpu_cell_lists._check_contract states, entry by entry: a cell's list is the depth-ordered union of the per-tile
lists of its tiles, every entry once, ties by entry index, the lists back to back in (camera, cell row, cell column) order."""
import numpy as np
import pytest

import _cell_binning_ref as ref

SHIFTS = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 1), (3, 0), (0, 4), (4, 4)]


def _entries(seed, E, tw, th, sx, sy, levels=None):
    rng = np.random.default_rng(seed)
    boxes, radii, depths = ref.random_entries(rng, E, tw, th, max_w=max(1, tw), max_h=max(1, th), depth_levels=levels)
    edge = ref.edge_entries(tw, th, sx, sy)
    ex = ref.pack_boxes(*(np.array([r[i] for r in edge]) for i in range(4)), tw)
    k = min(len(edge), E)
    boxes[:k] = ex[:k]
    radii[:k] = 1
    return boxes, radii, depths


@pytest.mark.parametrize("sx,sy", SHIFTS)
@pytest.mark.parametrize("tw,th,C", [(1, 1, 1), (5, 3, 1), (7, 4, 2), (1, 9, 3), (9, 1, 1), (33, 18, 1)])
def test_restatement_is_the_union_of_the_per_tile_lists(sx, sy, tw, th, C):
    E = 40 * C
    boxes, radii, depths = _entries(sx * 16 + sy + tw, E, tw, th, sx, sy, levels=5 if tw == 7 else None)
    got = ref.cell_lists(boxes, radii, depths, tw, th, C, sx, sy)
    want, n_tile = ref.brute_force_lists(boxes, radii, depths, tw, th, C, sx, sy)
    assert got["n_tile_pairs"] == n_tile
    assert got["n_isects"] == sum(len(v) for v in want.values()) == len(got["flatten_ids"])
    assert got["lists"].tolist() == sorted(want)
    pos = 0
    for l, s, e in zip(got["lists"].tolist(), got["starts"].tolist(), got["ends"].tolist()):
        assert s == pos, "the lists are not stored back to back in list order"
        assert got["flatten_ids"][s:e].tolist() == want[l], (l, sx, sy)
        pos = e
    assert pos == got["n_isects"]
    # gsplat's offsets: an empty list carries the offset of the next non-empty one
    offs = got["offsets"]
    assert offs[0] == 0 and offs[-1] == pos and (np.diff(offs) >= 0).all()
    assert offs[got["lists"]].tolist() == got["starts"].tolist()
    if sx == sy == 0:
        assert got["n_isects"] == n_tile


def test_culled_and_hollow_entries_are_not_listed():
    tw, th = 6, 5
    boxes = ref.pack_boxes([0, 1, 2, 0], [0, 1, 2, 0], [2, 2, 0, 3], [2, 2, 0, 3], tw)
    radii = np.array([1, 0, 1, 1], dtype=np.int32)
    depths = np.array([2.0, 1.0, 0.5, 2.0], dtype=np.float32)
    got = ref.cell_lists(boxes, radii, depths, tw, th, 1, 1, 1)
    # entry 1 is culled, entry 2 has an empty box; 0 and 3 tie in depth: index order
    assert got["flatten_ids"].tolist() == [0, 3, 3, 3, 3]
    assert got["lists"].tolist() == [0, 1, 3, 4]
    assert got["n_tile_pairs"] == 4 + 9 and got["n_isects"] == 1 + 4


def test_regime_restates_the_route_of_the_tile_sort():
    f = ref.regime(512, 6, 1, 1, 1, 10)
    assert (f["lw"], f["lh"], f["cells"], f["passes"], f["dbits"], f["key"], f["exact"]) == (256, 3, 768, 2, [5, 5], 16, True)
    assert not ref.regime(513, 6, 1, 1, 1, 10)["exact"]
    f = ref.regime(512, 514, 1, 1, 1, 10)
    assert (f["cells"], f["dbits"], f["key"], f["exact"]) == (65792, [6, 6, 5], 32, False)
    f = ref.regime(8192, 8192, 1, 2, 1, 10)
    assert (f["cells"], f["bits"], f["dbits"]) == (1 << 23, 23, [8, 8, 7])
    for cells, d in [(2, 1), (3, 2), (5, 3), (129, 8), (255, 8), (256, 8)]:
        f = ref.regime(cells, 1, 1, 0, 0, 1)
        assert f["passes"] == 1 and f["dbits"] == [d]
    assert ref.regime(257, 1, 1, 0, 0, 1)["passes"] == 2
