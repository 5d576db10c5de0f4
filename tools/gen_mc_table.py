#!/usr/bin/env python3
"""Generates dn-splatter_amd/csrc/mc_table.h, the marching-cubes case table, by tracing contours on the six faces of the cube.

Conventions (the ones csrc/marching.hip and torch_marching.py read from the header):
  corner c       sits at offset (di, dj, dk) = (c & 1, (c >> 1) & 1, (c >> 2) & 1) from the cell's lowest lattice point; bit c of a case
                 is set iff that corner is above the level.
  edge e         the twelve (owner corner, axis) pairs in ascending (flat index of the owner, axis) order, the owner being the end with
                 the lower index — the order in which the lattice numbers its vertices, so a lower edge id is a lower vertex id.
  face rule      seen from outside the cube, walk a face counter-clockwise.  A face edge is LEAVING if it goes from an above corner to
                 a below one, ENTERING if from below to above.  Every leaving edge is joined to the entering edge of the same run of
                 above corners; on an ambiguous face (two diagonal above corners) that gives two segments that each cut off one above
                 corner.  The rule reads the face's four signs only, so both cells that share a face draw the same segments.
  loops          a crossing cube edge is leaving on one of its two faces and entering on the other, so the segments leaving -> entering
                 form a permutation of the crossing edges: directed loops.  Loops are listed by their lowest edge id and each is
                 fan-triangulated from that edge.  Walked this way the above side is on the left and the right-hand normal points
                 towards increasing value, so every triangle (l0, l_i, l_i+1) is written reversed, (l0, l_i+1, l_i): normals point
                 out of the dense region.

Usage: python tools/gen_mc_table.py            writes the header
       python tools/gen_mc_table.py --stdout   prints it"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "dn-splatter_amd", "csrc", "mc_table.h")
MAX_TRI = 5


def corner_offset(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def _edges():
    found = []
    for c in range(8):
        d = corner_offset(c)
        for a in range(3):
            if d[a] == 0:
                found.append((d[0] * 4 + d[1] * 2 + d[2], a, d))
    found.sort()
    return [(d, a) for _, a, d in found]


EDGES = _edges()                                            # edge id -> ((di, dj, dk) of the owner, axis)
_EDGE_ID = {e: i for i, e in enumerate(EDGES)}


def edge_between(c0, c1):
    d0, d1 = corner_offset(c0), corner_offset(c1)
    diff = [a for a in range(3) if d0[a] != d1[a]]
    assert len(diff) == 1
    return _EDGE_ID[(min(d0, d1), diff[0])]


def _corner(d):
    return d[0] | d[1] << 1 | d[2] << 2


def _faces():
    """Six faces as four corners each, counter-clockwise seen from outside."""
    faces = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for side in (0, 1):
            ring = []
            for ub, uc in ((0, 0), (1, 0), (1, 1), (0, 1)):      # counter-clockwise seen from +a (b to the right, c up)
                d = [0, 0, 0]
                d[a], d[b], d[c] = side, ub, uc
                ring.append(_corner(d))
            if side == 0:
                ring.reverse()
            p = [corner_offset(x) for x in ring]
            u = [p[1][k] - p[0][k] for k in range(3)]
            v = [p[2][k] - p[1][k] for k in range(3)]
            n = [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
            assert n[a] == (1 if side else -1) and n[b] == 0 and n[c] == 0, "face not counter-clockwise from outside"
            faces.append(tuple(ring))
    return faces


FACES = _faces()


def ambiguous_faces(case):
    """The faces of `case` with exactly two above corners, diagonal to each other."""
    out = []
    for f, ring in enumerate(FACES):
        s = [(case >> c) & 1 for c in ring]
        if s == [1, 0, 1, 0] or s == [0, 1, 0, 1]:
            out.append(f)
    return out


def segments(case):
    """{leaving edge: entering edge} over the six faces."""
    nxt = {}
    for ring in FACES:
        s = [(case >> c) & 1 for c in ring]
        for q in range(4):
            if s[q] and not s[(q + 1) % 4]:                      # ring[q] -> ring[q + 1] leaves; walk back over the run of above corners
                r = q
                while s[(r - 1) % 4]:
                    r = (r - 1) % 4
                    assert r != q
                leaving = edge_between(ring[q], ring[(q + 1) % 4])
                entering = edge_between(ring[(r - 1) % 4], ring[r])
                assert leaving not in nxt
                nxt[leaving] = entering
    return nxt


def loops(case):
    """The directed loops of `case`, each rotated to start at its lowest edge id, listed by that edge."""
    nxt = segments(case)
    crossing = sorted(e for e, (d, a) in enumerate(EDGES)
                      if ((case >> _corner(d)) & 1) != ((case >> _corner(tuple(d[k] + (k == a) for k in range(3)))) & 1))
    assert sorted(nxt) == crossing and sorted(nxt.values()) == crossing, case
    out, seen = [], set()
    for e in crossing:
        if e in seen:
            continue
        loop = [e]
        seen.add(e)
        while nxt[loop[-1]] != e:
            loop.append(nxt[loop[-1]])
            seen.add(loop[-1])
        assert len(loop) >= 3
        out.append(loop)
    return out


def triangles(case):
    tris = []
    for loop in loops(case):
        for i in range(1, len(loop) - 1):
            tris.append((loop[0], loop[i + 1], loop[i]))
    return tris


def table():
    return [triangles(c) for c in range(256)]


def render():
    tab = table()
    assert max(len(t) for t in tab) <= MAX_TRI
    lines = [
        "// mc_table.h — the marching-cubes case table.  GENERATED by tools/gen_mc_table.py (face-contour tracing); do not edit:",
        "// tests/test_marching_reference.py regenerates it and compares the bytes.",
        "//   corner c of a cell sits at (di, dj, dk) = (c & 1, (c >> 1) & 1, (c >> 2) & 1); bit c of a case: that corner is above the level.",
        "//   MC_EDGE_OWNER[e] = {di, dj, dk, axis}: edge e runs from that corner along `axis`; ascending e is ascending vertex id.",
        "//   MC_NTRI[case]: triangles of the case; MC_TRI[case][3 t + c]: edge of corner c of triangle t, -1 behind the last one.",
        "#ifndef DNSPLAT_MC_TABLE_H",
        "#define DNSPLAT_MC_TABLE_H",
        "#define MC_MAX_TRI %d" % MAX_TRI,
        "#define MC_TABLE_TRIANGLES %d" % sum(len(t) for t in tab),
        "#ifndef MC_TABLE_QUALIFIER",
        "#define MC_TABLE_QUALIFIER static const",
        "#endif",
        "MC_TABLE_QUALIFIER signed char MC_EDGE_OWNER[12][4] = {",
    ]
    for d, a in EDGES:
        lines.append("    {%d, %d, %d, %d}," % (d[0], d[1], d[2], a))
    lines.append("};")
    lines.append("MC_TABLE_QUALIFIER unsigned char MC_NTRI[256] = {")
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(tab[c])) for c in range(r, r + 32)) + ",")
    lines.append("};")
    lines.append("MC_TABLE_QUALIFIER signed char MC_TRI[256][16] = {")
    for c in range(256):
        flat = [e for t in tab[c] for e in t]
        flat += [-1] * (16 - len(flat))
        lines.append("    {" + ", ".join("%2d" % e for e in flat) + "},  // %3d" % c)
    lines.append("};")
    lines.append("#endif")
    return "\n".join(lines) + "\n"


def main(argv):
    text = render()
    if "--stdout" in argv:
        sys.stdout.write(text)
    else:
        with open(HEADER, "w") as f:
            f.write(text)
        print("wrote", HEADER)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
