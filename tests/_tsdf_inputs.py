"""Inputs shared by tests/test_tsdf_reference.py (CPU) and tests/test_gpu_tsdf.py: the sphere scene of the issue, orbit poses with a
camera inside the volume and one looking away, smooth depth frames with patches of 0, NaN and beyond depth_trunc, weight lattices for the
observed marching cubes.  Everything is deterministic and small; nothing here touches a GPU."""
import numpy as np
import torch

SHAPES = [(5, 6, 7), (3, 2, 9), (65, 3, 2), (2, 2, 129), (17, 9, 33), (64, 64, 64)]


def look_at(eye, target=(0.0, 0.0, 0.0)) -> np.ndarray:
    """Camera-to-world [4,4] in the OpenGL convention (the camera looks down its -z) at ``eye``, looking at ``target``."""
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    z = eye - target
    z = z / np.linalg.norm(z)
    up = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    x = np.cross(up, z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    P = np.eye(4)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = x, y, z, eye
    return P


def intrinsics(width: int, height: int, focal: float) -> np.ndarray:
    return np.array([[focal, 0.0, width / 2.0], [0.0, focal, height / 2.0], [0.0, 0.0, 1.0]])


# ----------------------------------------------------------------------------------------------- the sphere scene
SPHERE_RADIUS, SPHERE_N, SPHERE_IMAGE, SPHERE_FOCAL, SPHERE_DISTANCE = 0.3, 48, 64, 60.0, 2.0


def sphere_scene(seed: int = 0):
    """A sphere of radius 0.3 at the origin in a 48^3 volume of voxel 1 / 48 over [-0.5, 0.5)^3, six axis-aligned cameras at distance 2,
    analytic z-depth at 64 x 64 with the pixel centres at the integers (pixel_offset 0.5), colours random.  dict of the arguments."""
    W = H = SPHERE_IMAGE
    K = intrinsics(W, H, SPHERE_FOCAL)
    D = SPHERE_DISTANCE
    poses = np.stack([look_at(e) for e in [(D, 0, 0), (-D, 0, 0), (0, D, 0), (0, -D, 0), (0, 0, D), (0, 0, -D)]])
    dx, dy = np.meshgrid((np.arange(W) - K[0, 2]) / K[0, 0], (np.arange(H) - K[1, 2]) / K[1, 1])
    norm = np.sqrt(dx * dx + dy * dy + 1.0)
    cos = 1.0 / norm                                        # the ray's z component; the centre is at (0, 0, D) in every camera
    b = cos * D
    disc = b * b - (D * D - SPHERE_RADIUS ** 2)
    t = np.where(disc > 0, b - np.sqrt(np.maximum(disc, 0.0)), 0.0)
    depth = torch.from_numpy(np.stack([(t * cos).astype(np.float32)] * 6))
    rgb = torch.rand(6, H, W, 3, generator=torch.Generator().manual_seed(seed))
    return {"dims": (SPHERE_N,) * 3, "voxel": 1.0 / SPHERE_N, "origin": (-0.5, -0.5, -0.5), "K": K, "poses": poses, "depth": depth,
            "rgb": rgb, "height": H, "width": W}


# ----------------------------------------------------------------------------------------------- frames for the integration tests
DEPTH_TRUNC, SDF_TRUNC = 3.0, 0.1


def volume_frame(shape):
    """(origin, voxel) of a volume of ``shape`` centred on the origin whose longest axis spans 1."""
    voxel = 1.0 / max(shape)
    return tuple(-0.5 * voxel * (n - 1) for n in shape), voxel


def orbit_poses(C: int) -> np.ndarray:
    """C poses: a small orbit at radius 1.4 around the volume; pose 1 is inside the volume, pose 2 looks away from it."""
    poses = []
    for c in range(C):
        a = 2.0 * np.pi * c / 17.0 + 0.3
        eye = (1.4 * np.cos(a), 1.4 * np.sin(a), 0.35 * np.sin(3.0 * a))
        if c == 1:
            poses.append(look_at((0.03, -0.02, 0.01), (0.5, 0.4, 0.1)))
        elif c == 2:
            poses.append(look_at(eye, tuple(2.0 * e for e in eye)))
        else:
            poses.append(look_at(eye, (0.02, -0.03, 0.01)))
    return np.stack(poses)


def frames(C: int, height: int, width: int, seed: int = 0):
    """(depth float32 [C,H,W], rgb float32 [C,H,W,3]): depth smooth around the orbit's distance — surfaces inside, in front of and behind
    the volume — with patches of 0, NaN, -1 and 5 > DEPTH_TRUNC; rgb spills outside [0, 1] and holds a NaN."""
    g = torch.Generator().manual_seed(seed + 100 * C + width)
    v, u = torch.meshgrid(torch.arange(height, dtype=torch.float32), torch.arange(width, dtype=torch.float32), indexing="ij")
    depth = torch.stack([1.4 + 0.45 * torch.sin(0.21 * u + 0.5 * c) * torch.cos(0.17 * v - 0.3 * c) for c in range(C)])
    depth[0, : height // 2, : width // 2] *= 0.05          # a near surface: the camera inside the volume sees some too
    if C > 1:
        depth[1] *= 0.2
    for c in range(C):
        y, x = (5 * c + 3) % (height - 6), (7 * c + 2) % (width - 6)
        depth[c, y:y + 4, x:x + 3] = 0.0
        depth[c, (y + 9) % (height - 4):(y + 9) % (height - 4) + 3, x:x + 4] = float("nan")
        depth[c, y:y + 2, (x + 11) % (width - 4):(x + 11) % (width - 4) + 3] = 5.0
        depth[c, (y + 15) % (height - 2), x] = -1.0
    rgb = torch.rand(C, height, width, 3, generator=g) * 1.2 - 0.1
    rgb[0, 1, 1, 0] = float("nan")
    return depth.contiguous(), rgb.contiguous()


# ----------------------------------------------------------------------------------------------- lattices for the observed extraction
def noise(shape, seed=0):
    return np.random.default_rng(seed + sum(shape)).random(shape, dtype=np.float32)


def smooth(shape):
    """A sphere centred off the lattice points, radius 0.3 of the longest axis + 0.4: crosses edges of every shape above."""
    s = np.asarray(shape, dtype=np.float64) - 1
    x = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), axis=-1)
    return (0.3 * s.max() + 0.4 - np.linalg.norm(x - (0.37 * s + 0.0131), axis=-1)).astype(np.float32)


def weights(shape, unobserved: float, min_weight: float, seed: int = 0) -> np.ndarray:
    """float32 weights of which a share ``unobserved`` is not > min_weight — among them min_weight itself, a NaN and a negative value —
    and the rest is, the smallest float32 above min_weight included."""
    rng = np.random.default_rng(seed + 7 * sum(shape))
    m = np.float32(min_weight)
    low = np.array([m, np.nan, m - np.float32(1.0), -np.inf], dtype=np.float32)
    high = np.array([np.nextafter(m, np.float32(np.inf)), m + np.float32(1.0), 100.0, np.inf], dtype=np.float32)
    hidden = rng.random(shape) < unobserved
    return np.where(hidden, low[rng.integers(0, 4, shape)], high[rng.integers(0, 4, shape)]).astype(np.float32)


def observed(weight: np.ndarray, min_weight: float) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return weight > np.float32(min_weight)


def boundary_edges(triangles: np.ndarray) -> int:
    """The number of undirected edges that lie in exactly one triangle."""
    t = np.asarray(triangles, dtype=np.int64)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    _, count = np.unique(e, axis=0, return_counts=True)
    return int((count == 1).sum())
