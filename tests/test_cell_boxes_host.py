"""csrc/bin_ranges.h dns_cell_box — the tile box of a Gaussian coarsened to the list cells of the fused path (dnsplat_bin_cells) — as a
stand-alone host program (tools/cell_box_host_check.cpp: its own main, no Python in the process) against a brute-force enumeration
of tiles -> cells; and the pair-count table of the issue's cell shapes from tools/cell_pairs.py on a small scene."""
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cell_box_matches_the_enumeration_of_tiles(tmp_path):
    exe = tmp_path / "cell_box_host_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "dn-splatter_amd", "csrc"),
                    os.path.join(ROOT, "tools", "cell_box_host_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr


def test_cell_pair_counts_of_the_table_script():
    """tools/cell_pairs.py counts (cell, Gaussian) pairs from tile boxes as dns_cell_box does: against the enumeration, on random boxes."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import cell_pairs

    g = torch.Generator().manual_seed(2)
    tw, th, n = 13, 7, 500
    x0 = torch.randint(0, tw, (n,), generator=g)
    y0 = torch.randint(0, th, (n,), generator=g)
    x1 = torch.minimum(x0 + torch.randint(0, 6, (n,), generator=g), torch.tensor(tw))      # some boxes empty
    y1 = torch.minimum(y0 + torch.randint(0, 5, (n,), generator=g), torch.tensor(th))
    for cw, ch in cell_pairs.SHAPES:
        pairs, lists = cell_pairs.count(x0, y0, x1, y1, tw, th, cw, ch)
        want = 0
        for i in range(n):
            want += len({(y // ch, x // cw) for y in range(int(y0[i]), int(y1[i])) for x in range(int(x0[i]), int(x1[i]))})
        assert pairs == want and lists == -(-tw // cw) * -(-th // ch), (cw, ch)
