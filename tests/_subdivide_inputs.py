"""Inputs of the subdivision tests, in numpy: the box room, the random soup, the five (input, max_edge) cases with the round counts
measured with the numpy statement below, and that statement itself — ``subdivide_to_size`` written the way trimesh's text reads
(``remesh.subdivide`` on the long faces, midpoints numbered by ``np.unique`` over the sorted edge rows), sharing no line with
``dn_splatter_amd.torch_subdivide``."""
import numpy as np


def box_room():
    """(vertices float32 [8,3], triangles int32 [12,3]): the box [0,5] x [0,4] x [0,3], vertices numbered with z fastest, six quads of
    two triangles."""
    vertices = np.array([(x, y, z) for x in (0.0, 5.0) for y in (0.0, 4.0) for z in (0.0, 3.0)], dtype=np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    triangles = np.array([t for (i, j, k, l) in quads for t in ((i, j, k), (i, k, l))], dtype=np.int32)
    return vertices, triangles


def soup():
    """(vertices float32 [400,3], triangles int32 [900,3]): uniform points in the unit cube and triangles of random indices, with
    edges many triangles share and at least one triangle with a repeated vertex (the first seed from 0 up that has one)."""
    for seed in range(64):
        rng = np.random.default_rng(seed)
        vertices = rng.uniform(size=(400, 3)).astype(np.float32)
        triangles = rng.integers(0, 400, size=(900, 3)).astype(np.int32)
        t = triangles
        if ((t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2])).any():
            return vertices, triangles
    raise AssertionError("no seed gives a triangle with a repeated vertex")


# name -> (mesh, max_edge, the per-round (triangles, long, current vertices, done vertices) where the issue lists them, V', T')
CASES = {
    "box_3.0": (box_room, 3.0, [(12, 12, 8, 0), (48, 16, 26, 24), (64, 0, 58, 50)], 74, 96),
    "box_0.8": (box_room, 0.8, None, 866, 1536),
    "box_0.05": (box_room, 0.05, None, 198146, 393216),
    "box_0.025": (box_room, 0.025, None, 789506, 1572864),
    "soup_0.12": (soup, 0.12, [(900, 900, 400, 0), (3600, 3600, 3049, 0), (14400, 13792, 11037, 533), (55168, 17856, 36701, 24701),
                               (71424, 0, 66785, 42088)], 67322, 109344),
}
# what the cases are there for: the number of rounds, and a round of a given size
ROUNDS = {"box_3.0": 3, "box_0.8": 5, "box_0.05": 9, "box_0.025": 10, "soup_0.12": 5}
LAST_ROUND_TRIANGLES = {"box_0.8": 1024, "box_0.05": 262144, "box_0.025": 1048576}


def numpy_subdivide_to_size(vertices, faces, max_edge, max_iter=10):
    """trimesh's text: per round, the faces with an edge over max_edge are subdivided (each edge's midpoint once, by np.unique over
    the sorted edge rows; four children per face), the others are "done" with their referenced vertices.  Returns (vertices float64,
    faces int64, face_index int64, rounds)."""
    current_v, current_f = np.asarray(vertices, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    current_i = np.arange(len(current_f))
    done_v, done_f, done_i, rounds, emitted = [], [], [], [], 0
    for i in range(max_iter + 1):
        tri = current_v[current_f]
        d = np.roll(tri, -1, axis=1) - tri
        length = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        too_long = (length > max_edge).any(axis=1)
        ok = current_f[~too_long]
        referenced = np.unique(ok)
        renumber = np.full(len(current_v), -1)
        renumber[referenced] = np.arange(len(referenced))
        done_v.append(current_v[referenced])
        done_f.append(renumber[ok] + emitted)
        done_i.append(current_i[~too_long])
        emitted += len(referenced)
        rounds.append((len(current_f), int(too_long.sum()), len(current_v), len(referenced)))
        if not too_long.any():
            break
        if i == max_iter:
            raise ValueError("max_iter exceeded")
        f = current_f[too_long]
        edges = np.sort(f[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), axis=1)
        unique, inverse = np.unique(edges, axis=0, return_inverse=True)
        mid = current_v[unique].mean(axis=1)
        m = inverse.reshape(-1, 3) + len(current_v)
        current_f = np.column_stack([f[:, 0], m[:, 0], m[:, 2], m[:, 0], f[:, 1], m[:, 1], m[:, 2], m[:, 1], f[:, 2],
                                     m[:, 0], m[:, 1], m[:, 2]]).reshape(-1, 3)
        current_i = np.repeat(current_i[too_long], 4)
        current_v = np.vstack([current_v, mid])
    return np.vstack(done_v), np.vstack(done_f), np.concatenate(done_i), rounds
