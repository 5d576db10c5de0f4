"""Inputs of the mesh visibility culling tests, in numpy: the room of the golden fixture (tests/golden/reference_mesh_cull.npz), random
triangle scenes for the depth render, OpenGL look-at poses, and an independent per-pixel ray / triangle intersection in float64
(Moeller and Trumbore, "Fast, minimum storage ray/triangle intersection", 1997) that shares no formula with the package's edge
functions.  Every coordinate is an fp32 value."""
import numpy as np

HEIGHT, WIDTH = 36, 48
K = np.array([[30.0, 0.0, 24.0], [0.0, 30.0, 18.0], [0.0, 0.0, 1.0]], dtype=np.float32)


def _grid(origin, du, dv, nu, nv):
    """(vertices, triangles) of a planar patch: (nu + 1) x (nv + 1) points origin + i du + j dv, two triangles per cell."""
    i, j = np.meshgrid(np.arange(nu + 1), np.arange(nv + 1), indexing="ij")
    pts = np.asarray(origin)[None] + i.reshape(-1, 1) * np.asarray(du)[None] + j.reshape(-1, 1) * np.asarray(dv)[None]
    tri = []
    for a in range(nu):
        for b in range(nv):
            p = a * (nv + 1) + b
            tri += [[p, p + nv + 1, p + 1], [p + 1, p + nv + 1, p + nv + 2]]
    return pts, np.asarray(tri)


def room():
    """A closed room [-2, 2] x [-1, 1] x [-2, 2] (y up) with an inner wall at x = 0.3125 from the back wall to z = 0.5: what lies behind
    the wall is hidden from cameras on the other side.  (vertices float32 [V,3], triangles int32 [T,3]); the faces share no vertices."""
    s = 0.5
    parts = [
        _grid((-2, -1, -2), (s, 0, 0), (0, 0, s), 8, 8),          # floor
        _grid((-2, 1, -2), (s, 0, 0), (0, 0, s), 8, 8),           # ceiling
        _grid((-2, -1, -2), (s, 0, 0), (0, s, 0), 8, 4),          # back wall z = -2
        _grid((-2, -1, 2), (s, 0, 0), (0, s, 0), 8, 4),           # front wall z = 2
        _grid((-2, -1, -2), (0, 0, s), (0, s, 0), 8, 4),          # x = -2
        _grid((2, -1, -2), (0, 0, s), (0, s, 0), 8, 4),           # x = 2
        _grid((0.3125, -1, -2), (0, 0, s), (0, s, 0), 5, 4),      # the inner wall
    ]
    vertices, triangles, base = [], [], 0
    for v, t in parts:
        vertices.append(v)
        triangles.append(t + base)
        base += len(v)
    return np.concatenate(vertices).astype(np.float32), np.concatenate(triangles).astype(np.int32)


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """A camera-to-world matrix in the OpenGL convention (x right, y up, the camera looks down -z), float64 [4,4]."""
    eye, target, up = (np.asarray(a, dtype=np.float64) for a in (eye, target, up))
    back = eye - target
    back /= np.linalg.norm(back)
    right = np.cross(up, back)
    right /= np.linalg.norm(right)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, np.cross(back, right), back, eye
    return c2w


def room_poses():
    """8 poses on the near side of the inner wall, at irrational-looking positions so that no vertex projects onto a pixel boundary."""
    eyes = [(-1.37, 0.11, 1.23), (-1.52, -0.23, 0.41), (-0.83, 0.17, 1.61), (-1.11, 0.05, -0.57),
            (-0.41, -0.13, 1.37), (-1.71, 0.21, -1.29), (1.13, 0.07, 1.31), (-0.67, -0.31, 0.77)]
    targets = [(0.3, -0.3, -1.7), (0.3, -0.1, -1.3), (-0.4, -0.4, -1.9), (0.2, -0.2, -1.9),
               (0.3, -0.3, -0.9), (-0.9, -0.6, -1.9), (-1.8, -0.1, -0.2), (0.3, -0.2, -1.9)]
    return np.stack([look_at(e, t) for e, t in zip(eyes, targets)])


def random_scene(n_triangles, seed, crossing=True):
    """(vertices float32 [3 n,3], triangles int32 [n,3], one OpenGL pose): triangles of mixed size in front of the camera, about a
    third of them (with ``crossing``) with a vertex behind it, so that they cross z = 0."""
    rng = np.random.default_rng(seed)
    centre = np.stack([rng.uniform(-3, 3, n_triangles), rng.uniform(-2, 2, n_triangles), rng.uniform(-8, -0.5, n_triangles)], axis=1)
    size = rng.choice([0.05, 0.4, 2.5], size=(n_triangles, 1, 1), p=[0.4, 0.4, 0.2])
    if n_triangles == 1:                                                          # a lone triangle is a large one near the axis
        size[:] = 2.5
        centre[:, :2] *= 0.2
    v = centre[:, None, :] + rng.uniform(-1, 1, (n_triangles, 3, 3)) * size
    if crossing:
        behind = rng.random(n_triangles) < 0.33
        v[behind, 0, 2] = rng.uniform(0.2, 3.0, int(behind.sum()))
    pose = look_at((0.13, -0.07, 0.21), (0.3, 0.1, -5.0))
    return v.reshape(-1, 3).astype(np.float32), np.arange(3 * n_triangles, dtype=np.int32).reshape(-1, 3), pose[None]


def opencv_view(pose):
    """(R, t) float64 of the OpenCV world-to-camera transform of one OpenGL camera-to-world pose, by numpy's general inverse."""
    c2w = np.array(pose, dtype=np.float64)
    c2w[:3, 1] *= -1
    c2w[:3, 2] *= -1
    w2c = np.linalg.inv(c2w)
    return w2c[:3, :3], w2c[:3, 3]


def moller_trumbore_depth(vertices, triangles, pose, K, height, width, znear=0.01, zfar=10.0):
    """float64 [H,W] (inf where nothing is hit) and the boolean coverage: per pixel the smallest z of the intersections of the ray
    o + s d, o = 0, d = ((u + 0.5 - cx) / fx, (v + 0.5 - cy) / fy, 1), with the triangles in camera space; barycentric test, both
    windings, z = s in [znear, zfar]."""
    R, t = opencv_view(pose)
    p = vertices.astype(np.float64)[triangles] @ R.T + t                          # [T,3,3]
    K = np.asarray(K, dtype=np.float64)
    u, v = np.meshgrid(np.arange(width) + 0.5, np.arange(height) + 0.5, indexing="xy")
    d = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones_like(u)], axis=-1)     # [H,W,3]
    best = np.full((height, width), np.inf)
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    for i in range(len(p)):
        h = np.cross(d, e2[i])
        a = h @ e1[i]
        with np.errstate(divide="ignore", invalid="ignore"):
            f = 1.0 / a
            s = -p[i, 0]
            bu = f * (h @ s)
            q = np.cross(s, e1[i])
            bv = f * (d @ q)
            z = f * (q @ e2[i])
        hit = (a != 0) & (bu >= 0) & (bv >= 0) & (bu + bv <= 1) & (z >= znear) & (z <= zfar)
        best = np.where(hit & (z < best), z, best)
    return best, np.isfinite(best)
