"""Golden vectors of the depth-to-normal step, produced by THE REFERENCE's own code: ``get_camera_coords``, ``backproject`` and
``compute_angle_between_normals`` of dn_splatter/scripts/depth_to_normal.py, whose module imports (open3d, cv2, tyro, natsort, ...)
cannot be satisfied here: the three function definitions, and the statements of ``DepthToNormal.main``'s frame loop that turn the
monocular map into the world (from the assignment of ``w2c`` to the re-encoded ``mono_normal``, :197-206), are cut out of the file with
``ast`` and executed as they stand, with numpy and their inputs in their namespace.

Nothing of the reference is copied: only inputs (the small seeded frame and the pose of tests/_normals_inputs.py, a seeded field of unit
normals standing in for the estimated ones, a seeded 8-bit monocular normal map) and the reference's OUTPUTS are stored
(tests/golden/reference_depth_normals.npz): the world points and pixel coordinates of ``backproject``, and the angles of
``compute_angle_between_normals`` between the two ``(n + 1) / 2``-encoded maps with the 10-degree mask of :208-209.

``estimate_normals`` itself cannot be pinned: Open3D is absent.

    python tests/golden/make_reference_depth_normals_golden.py     # needs the reference checkout; rewrites reference_depth_normals.npz
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_reference_golden import REF  # noqa: E402

import _normals_inputs as inputs  # noqa: E402

H, W = 12, 16
INTRINSICS = dict(fx=15.0, fy=15.5, cx=7.75, cy=6.125)


def load_functions():
    path = os.path.join(REF, "dn_splatter/scripts/depth_to_normal.py")
    tree = ast.parse(open(path).read())
    wanted = ("get_camera_coords", "backproject", "compute_angle_between_normals")
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in wanted]
    assert sorted(n.name for n in body) == sorted(wanted)
    ns = {"np": np}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    # the frame loop of DepthToNormal.main: the statements from `w2c = ...` up to the next assignment of `mono_normal`
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "DepthToNormal")
    main_fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "main")
    loop = next(n for n in main_fn.body if isinstance(n, ast.For))

    def assigns(node, name):
        return isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name) and node.targets[0].id == name

    first = next(k for k, n in enumerate(loop.body) if assigns(n, "w2c"))
    last = next(k for k, n in enumerate(loop.body) if k > first and assigns(n, "mono_normal"))
    ns["mono_to_world"] = compile(ast.Module(body=loop.body[first:last + 1], type_ignores=[]), path, "exec")
    return ns


def mono_in_world(ns, mono_image, pose):
    """the reference's statements on (mono_normal in [0, 1], c2w_ref, h, w): the re-encoded monocular normals in the world"""
    frame = {"np": np, "mono_normal": mono_image / 255.0, "c2w_ref": pose, "h": mono_image.shape[0], "w": mono_image.shape[1]}
    exec(ns["mono_to_world"], frame)
    return frame["mono_normal"]


def main(path=os.path.join(HERE, "reference_depth_normals.npz")):
    ns = load_functions()
    rng = np.random.default_rng(71)
    c2w = inputs.frame_pose()
    depth = (1.5 + rng.random((H, W))).astype(np.float32)
    depth[3:5, 4:9] = 0.0                                                        # pixels without depth: the reference keeps them
    means3d, image_coords = ns["backproject"](depths=depth, img_size=(W, H), c2w=c2w, **INTRINSICS)
    assert means3d.shape == (H * W, 3) and means3d.dtype == np.float64 and image_coords.dtype == np.float32

    normals = rng.normal(size=(H, W, 3))
    normals /= np.linalg.norm(normals, axis=2, keepdims=True)
    mono_image = rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)
    mono_image[(mono_image == 128).all(axis=2)] = 129                            # no zero vector after the decoding below
    encoded = (normals + 1) / 2                                                  # :183
    mono_world = mono_in_world(ns, mono_image, c2w)
    degrees = ns["compute_angle_between_normals"](encoded, mono_world)
    mask = degrees > 10
    near = np.abs(degrees - 10).min()
    print(f"{H}x{W} frame; {int(mask.sum())} of {mask.size} pixels beyond 10 degrees; the nearest angle to the threshold is {near:.3e} away")
    assert 0 < mask.sum() < mask.size and near > 1e-6
    np.savez_compressed(path, depth=depth, c2w=c2w, height=np.int32(H), width=np.int32(W),
                        intrinsics=np.array([INTRINSICS[k] for k in ("fx", "fy", "cx", "cy")]),
                        means3d=means3d, image_coords=image_coords, normals=normals, mono_image=mono_image, degrees=degrees, mask=mask)
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
