"""Golden vectors of the mesh visibility culling, produced by THE REFERENCE's own code: ``cull_from_one_pose`` and
``get_grid_culling_pattern`` of dn_splatter/eval/eval_mesh_vis_cull.py, whose module imports (open3d, trimesh, pyrender, cv2, tyro, ...)
cannot be satisfied here: the two function definitions are cut out of the file with ``ast`` and executed as they stand, with numpy,
``deepcopy`` and an identity ``tqdm`` in their namespace.

Nothing of the reference is copied: only inputs (the room and the poses of tests/_mesh_cull_inputs.py, the depth maps the PyTorch
restatement renders of it, a sensor depth with a missing patch) and the reference's OUTPUTS for the flag combinations
(remove_missing_depth, remove_occlusion) = (T,T), (T,F), (F,T) are stored (tests/golden/reference_mesh_cull.npz).

The maker asserts what keeps the fixture decisive: no vertex lies within 1e-9 of any comparison the votes take (the four frustum
bounds, pz > 0, the depth test with its sum formed in float32 as numpy forms it and in float64, the truncation of px and py), so every
float64 restatement takes the same decisions; ``obs > 3`` holds for some vertices and not for others; the cut keeps some triangles
and drops some as unobserved and some as invalid.

    python tests/golden/make_reference_mesh_cull_golden.py     # needs the reference checkout; rewrites reference_mesh_cull.npz
"""
import ast
import os
import sys
from copy import deepcopy

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_reference_golden import REF  # noqa: E402

import _mesh_cull_inputs as inputs  # noqa: E402

FLAGS = {"tt": (True, True), "tf": (True, False), "ft": (False, True)}        # (remove_missing_depth, remove_occlusion)
MARGIN = 1e-9


def load_cull():
    path = os.path.join(REF, "dn_splatter/eval/eval_mesh_vis_cull.py")
    tree = ast.parse(open(path).read())
    wanted = ("cull_from_one_pose", "get_grid_culling_pattern")
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in wanted]
    assert sorted(n.name for n in body) == sorted(wanted)
    ns = {"np": np, "deepcopy": deepcopy, "tqdm": lambda it, **kw: it}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns


def margins(points, poses, K, H, W, rendered):
    """The smallest distance of any vertex, under any pose, to a comparison of cull_from_one_pose."""
    worst = np.inf
    for pose, depth in zip(poses, rendered):
        R, t = inputs.opencv_view(pose)
        uvz = (K.astype(np.float64) @ (R @ points.T + t[:, None])).T
        pz = uvz[:, 2] + 1e-8
        px, py = uvz[:, 0] / pz, uvz[:, 1] / pz
        inside = (0 <= px) & (px <= W - 1) & (0 <= py) & (py <= H - 1) & (pz > 0)
        frustum = np.min(np.abs(np.stack([px, px - (W - 1), py, py - (H - 1), pz])), axis=0)
        worst = min(worst, frustum.min())
        u, v = px[inside].astype(np.int32), py[inside].astype(np.int32)
        worst = min(worst, np.abs(px[inside] - np.round(px[inside])).min(), np.abs(py[inside] - np.round(py[inside])).min())
        limit32 = (depth[v, u] + np.float32(0.02)).astype(np.float64)
        limit64 = depth[v, u].astype(np.float64) + 0.02
        assert np.array_equal(pz[inside] < limit32, pz[inside] < limit64)
        worst = min(worst, np.abs(pz[inside] - limit32).min(), np.abs(pz[inside] - limit64).min())
    return worst


def cut_masks(triangles, obs, invalid):
    """:251-260 in numpy: (observed, invalid, kept) per triangle."""
    o, i = obs[triangles], invalid[triangles]
    observed = (o > 3).any(axis=1)
    bad = (i > 0.7 * o).all(axis=1)
    return observed, bad, observed & ~bad


def main(path=os.path.join(HERE, "reference_mesh_cull.npz")):
    from dn_splatter_amd import torch_mesh_cull as tmc

    ns = load_cull()
    vertices, triangles = inputs.room()
    poses, K, H, W = inputs.room_poses(), inputs.K, inputs.HEIGHT, inputs.WIDTH
    rendered = tmc.render_mesh_depth(torch.from_numpy(vertices), torch.from_numpy(triangles), poses, K, H, W).numpy()
    assert rendered.dtype == np.float32 and (rendered > 0).mean() > 0.99, "a closed room is hit everywhere"
    depth_gt = rendered.copy()
    depth_gt[:, :14, :] = 0.0                                                    # the sensor saw nothing in the upper rows
    depth_gt[:, 20:30, 30:44] = 0.0

    points = vertices.astype(np.float64)
    worst = margins(points, poses, K, H, W, rendered)
    print(f"{len(vertices)} vertices, {len(triangles)} triangles, {len(poses)} poses; nearest comparison {worst:.3e}")
    assert worst > MARGIN

    save = {"vertices": vertices, "triangles": triangles, "poses": poses, "K": K, "height": np.int32(H), "width": np.int32(W),
            "rendered_depth": rendered, "depth_gt": depth_gt}
    for name, (missing, occlusion) in FLAGS.items():
        obs, invalid = ns["get_grid_culling_pattern"](points, [p for p in poses], H, W, K, rendered_depth_list=[d for d in rendered],
                                                       depth_gt_list=[d for d in depth_gt], remove_missing_depth=missing,
                                                       remove_occlusion=occlusion)
        assert np.array_equal(obs, np.round(obs)) and np.array_equal(invalid, np.round(invalid))
        save["obs_" + name], save["invalid_" + name] = obs.astype(np.int32), invalid.astype(np.int32)
        observed, bad, kept = cut_masks(triangles, obs, invalid)
        print(f"{name}: obs > 3 for {int((obs > 3).sum())} of {len(obs)} vertices; {int(kept.sum())} triangles kept, "
              f"{int((~observed).sum())} unobserved, {int((observed & bad).sum())} invalid")
        assert 0 < (obs > 3).sum() < len(obs)
        assert kept.any() and (~observed).any()
        if missing:
            assert (observed & bad).any()
    np.savez_compressed(path, **save)
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
