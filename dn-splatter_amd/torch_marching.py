"""Marching cubes — the CPU restatement of ``csrc/marching.hip`` in numpy, from the generated case table ``csrc/mc_table.h``
(tools/gen_mc_table.py), and the world mapping of the reference's ``MarchingCubesMesh`` (dn_splatter/export_mesh.py:789-795).  No HIP.
It is the yardstick the kernels are held to with exact equality, so the contract is stated here in full:

  * a lattice point is ABOVE iff ``v > level`` in float32 (NaN is not above);
  * one vertex per lattice edge whose two ends differ in that test.  The edge from point p along axis a belongs to p; vertices are
    numbered in ascending (flat index of p, a).  Position, float32, lattice coordinates: ``t = (level - v(p)) / (v(p + e_a) - v(p))``,
    component a is ``float(p_a) + t``, the others are the integers; every operation rounded once, no contraction.  A non-finite ``t``
    is written as the arithmetic gives it, except that a NaN is written as the one quiet NaN 0x7FC00000: IEEE 754 leaves sign and
    payload of a generated NaN to the platform, and the output is meant to be one function of the volume on all of them;
  * triangles are int32 vertex ids; cells in ascending flat index of their lowest corner, within a cell in the table's order; the
    right-hand normal points towards decreasing value;
  * a corner equal to ``level`` gives ``t`` = 0 or 1 and zero-area triangles.  They are kept, as any table-driven extractor keeps them.

With ``observed`` (a boolean lattice; for a TSDF volume ``weight > min_weight`` in float32) the extraction covers only what was seen,
Open3D's rule for such a volume: an edge owns a vertex iff both its ends are observed and differ in the test, a cell has its table
case iff all eight corners are observed (else none), numbering and order as above.  The value of an unobserved point never reaches
a result.  Every triangle's vertices exist; at the rim of the observed region a vertex may be referenced by no triangle and stays.
"""
from __future__ import annotations

import os
import re

import numpy as np
import torch

_TABLE = None
CANONICAL_NAN = 0x7FC00000
MAX_POINTS = 2 ** 31            # Rx Ry Rz must stay below it


def case_table():
    """(owner [12,4] int64: di, dj, dk, axis of every edge; ntri [256] int64; tri [256,15] int64, -1 behind the last triangle), parsed
    from the header the kernels compile."""
    global _TABLE
    if _TABLE is None:
        text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "mc_table.h")).read()
        text = re.sub(r"//[^\n]*", "", text)

        def numbers(name):
            body = re.search(name + r"(?:\[\d+\])+\s*=\s*\{(.*?)\};", text, re.S).group(1)
            return np.array([int(x) for x in re.findall(r"-?\d+", body)], dtype=np.int64)

        owner = numbers("MC_EDGE_OWNER").reshape(12, 4)
        ntri = numbers("MC_NTRI")
        tri = numbers("MC_TRI").reshape(256, 16)[:, :15]
        assert ntri.shape == (256,) and int(ntri.sum()) == int(re.search(r"MC_TABLE_TRIANGLES (\d+)", text).group(1))
        _TABLE = (owner, ntri, tri)
    return _TABLE


def _volume(volume) -> np.ndarray:
    if torch.is_tensor(volume):
        volume = volume.detach().cpu().numpy()
    volume = np.ascontiguousarray(volume, dtype=np.float32)
    if volume.ndim != 3:
        raise ValueError(f"volume must be [Rx,Ry,Rz], got {volume.shape}")
    if volume.size >= MAX_POINTS:
        raise ValueError(f"a lattice of {volume.shape} has 2^31 points or more")
    return volume


def _observed(observed, shape) -> np.ndarray:
    if torch.is_tensor(observed):
        observed = observed.detach().cpu().numpy()
    observed = np.asarray(observed)
    if observed.dtype != np.bool_ or observed.shape != shape:
        raise ValueError(f"observed must be a boolean lattice of shape {shape}, got {observed.dtype} {observed.shape}")
    return observed


def marching_cubes(volume, level, observed=None):
    """(vertices float32 [V,3] in lattice coordinates, triangles int32 [T,3]) as numpy arrays; ``observed``: see the module docstring."""
    v = _volume(volume)
    level = np.float32(level)
    Rx, Ry, Rz = v.shape
    n = v.size
    owner, ntri, tri = case_table()
    if min(Rx, Ry, Rz) < 2:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    above = v > level
    if observed is not None:
        seen = _observed(observed, v.shape)
        above = above & seen
    strides = (Ry * Rz, Rz, 1)
    cross = np.zeros((Rx, Ry, Rz, 3), dtype=bool)
    cross[:-1, :, :, 0] = above[:-1] != above[1:]
    cross[:, :-1, :, 1] = above[:, :-1] != above[:, 1:]
    cross[:, :, :-1, 2] = above[:, :, :-1] != above[:, :, 1:]
    if observed is not None:
        cross[:-1, :, :, 0] &= seen[:-1] & seen[1:]
        cross[:, :-1, :, 1] &= seen[:, :-1] & seen[:, 1:]
        cross[:, :, :-1, 2] &= seen[:, :, :-1] & seen[:, :, 1:]
    keys = np.flatnonzero(cross.reshape(-1))                # ascending (flat index of p, axis)
    p, a = keys // 3, keys % 3
    V = keys.size
    flat = v.reshape(-1)
    v0 = flat[p]
    v1 = flat[p + np.asarray(strides, dtype=np.int64)[a]]
    with np.errstate(all="ignore"):
        t = (level - v0) / (v1 - v0)
        ijk = np.stack([p // (Ry * Rz), (p // Rz) % Ry, p % Rz], axis=1)
        vertices = ijk.astype(np.float32)
        rows = np.arange(V)
        vertices[rows, a] = vertices[rows, a] + t
    assert vertices.dtype == np.float32 and t.dtype == np.float32
    bits = vertices.view(np.int32)
    bits[np.isnan(vertices)] = CANONICAL_NAN
    vid = np.full(n * 3, -1, dtype=np.int64)
    vid[keys] = np.arange(V)

    case = np.zeros((Rx - 1, Ry - 1, Rz - 1), dtype=np.int64)
    for c in range(8):
        di, dj, dk = c & 1, (c >> 1) & 1, (c >> 2) & 1
        case |= above[di:Rx - 1 + di, dj:Ry - 1 + dj, dk:Rz - 1 + dk].astype(np.int64) << c
    if observed is not None:
        for c in range(8):                                  # a cell with an unobserved corner has no case
            di, dj, dk = c & 1, (c >> 1) & 1, (c >> 2) & 1
            case[~seen[di:Rx - 1 + di, dj:Ry - 1 + dj, dk:Rz - 1 + dk]] = 0
    ii, jj, kk = np.nonzero(ntri[case] > 0)                 # C order: ascending flat index of the lowest corner
    cells = (ii * Ry + jj) * Rz + kk
    cc = case[ii, jj, kk]
    edges = tri[cc]                                         # [cells, 15]
    live = edges >= 0
    e = np.where(live, edges, 0)
    corner = cells[:, None] + owner[e, 0] * strides[0] + owner[e, 1] * strides[1] + owner[e, 2]
    ids = vid[corner * 3 + owner[e, 3]]
    assert bool((ids[live] >= 0).all()), "the table names an edge that does not cross"
    triangles = ids[live].reshape(-1, 3).astype(np.int32)
    return vertices, triangles


def world_mapping(vertices, X, Y, Z):
    """export_mesh.py:789-795 on lattice-coordinate ``vertices`` [V,3]: ``X[0] + (v / (R - 1)) * (X[-1] - X[0])`` per axis, in float64
    with the span formed in the axes' own precision first, as the reference's numpy expression evaluates it.  numpy in, numpy out."""
    vertices = np.asarray(vertices, dtype=np.float64)
    out = np.empty((vertices.shape[0], 3), dtype=np.float64)
    for a, axis in enumerate((X, Y, Z)):
        axis = axis.detach().cpu().numpy() if torch.is_tensor(axis) else np.asarray(axis)
        out[:, a] = axis[0] + (vertices[:, a] / (axis.shape[0] - 1)) * (axis[-1] - axis[0])
    return out


def mcubes_marching_cubes(volume, level):
    """The call shape of ``mcubes.marching_cubes`` (export_mesh.py:778): float64 [V,3] and int64 [T,3] numpy arrays."""
    vertices, triangles = marching_cubes(volume, level)
    return vertices.astype(np.float64), triangles.astype(np.int64)
