"""Golden vectors of the point-cloud export, produced by THE REFERENCE's own code: ``find_depth_edges`` and
``pick_indices_at_random`` (dn_splatter/export_mesh.py:50-90) loaded from their text with ``extract_function`` — the module itself
cannot be imported, it pulls in open3d and tyro — ``get_colored_points_from_depth`` from utils/camera_utils.py loaded by path, and the
normal-map transform of ``DepthAndNormalMapsPoisson.main`` (:408-428), which is inline there, executed from its text as
``regularization_case`` executes get_loss_dict.  Nothing of the reference is copied: only inputs (tests/_export_inputs.py) and the
reference's OUTPUTS are stored (tests/golden/reference_export.npz).

    python tests/golden/make_reference_export_golden.py     # needs the reference checkout; rewrites reference_export.npz
"""
import ast
import os
import sys
import textwrap

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_reference_golden import REF, _load, extract_function, extract_method  # noqa: E402

import _export_inputs as inputs  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from dn_splatter_amd import torch_export as te  # noqa: E402

EXPORT_MESH = os.path.join(REF, "dn_splatter/export_mesh.py")


def reference_functions():
    ns = dict(torch=torch, F=F)
    for name in ("find_depth_edges", "pick_indices_at_random"):
        exec(compile(textwrap.dedent(extract_function(EXPORT_MESH, name)), f"export_mesh.py::{name}", "exec"), ns)
    return ns["find_depth_edges"], ns["pick_indices_at_random"]


def normal_map_transform():
    """The statements under ``if self.normal_method == "normal_maps":`` of DepthAndNormalMapsPoisson.main as a function of
    (outputs, c2w, indices) returning ``normal_map``."""
    text = extract_method(EXPORT_MESH, "DepthAndNormalMapsPoisson", "main")
    for node in ast.walk(ast.parse(text)):
        if isinstance(node, ast.If) and ast.unparse(node.test) == "self.normal_method == 'normal_maps'":
            body = "\n".join(ast.unparse(stmt) for stmt in node.body)
            code = compile(body, "export_mesh.py::DepthAndNormalMapsPoisson.main[normal_maps]", "exec")

            def run(outputs, c2w, indices):
                ns = dict(torch=torch, outputs=outputs, c2w=c2w, indices=indices)
                exec(code, ns)
                return ns["normal_map"]

            return run
    raise KeyError("the normal_maps branch was not found")


def main(path=os.path.join(HERE, "reference_export.npz")):
    find_depth_edges, pick_indices_at_random = reference_functions()
    cu = _load("dn_splatter.utils.camera_utils", "dn_splatter/utils/camera_utils.py")
    normals_of = normal_map_transform()
    save = {}
    for H, W in inputs.FIXTURE_FRAMES:
        pre = f"f{H}x{W}_"
        f = inputs.frame_inputs(H, W)
        c2w_gl, fx, fy, cx, cy = inputs.camera(H, W)
        c2w_cv = te.export_c2w(c2w_gl)                                  # export_mesh.py:370-375
        depth = f["depth"]
        save.update({pre + "depth_q": f["depth_q"].numpy().astype(np.uint16), pre + "rgb_u8": f["rgb_u8"].numpy(),
                     pre + "normal_q": f["normal_q"].numpy(), pre + "mask": np.packbits(f["mask"].numpy()),
                     pre + "c2w_gl": c2w_gl.numpy(), pre + "c2w_cv": c2w_cv.numpy(),
                     pre + "intr": np.array([fx, fy, cx, cy], dtype=np.float64)})
        valid = {}
        for thr, itr in inputs.EDGE_SETTINGS:
            # the recipe's conditions: no decision within the rounding envelope (the allowed number is 0), and the reference's
            # fp32 map is the fp64 restatement's
            n_flagged = int(inputs.flagged_edge_decisions(depth[..., 0], thr).sum())
            assert n_flagged == 0, (H, W, thr, n_flagged)
            edges = find_depth_edges(depth, threshold=thr, dilation_itr=itr)
            assert edges.shape == (H, W, 1) and edges.dtype == torch.float32
            assert torch.equal(edges.double(), te.find_depth_edges(depth.double(), thr, itr)), "fp32 map differs from the fp64 restatement"
            v = edges < 0.2
            valid[(thr, itr)] = v
            save[pre + f"valid_t{thr}_i{itr}"] = np.packbits(v.numpy())
            raw = int((te.depth_laplacian(depth[..., 0]) > thr).sum())
            print(f"{H}x{W} threshold {thr} itr {itr}: {raw} raw edge pixels, valid share {float(v.float().mean()):.3f}")
        outputs = {"rgb": f["rgb"], "normal": f["surface_normal"], "surface_normal": f["surface_normal"]}
        for tag, vmask in (("depth", depth), ("edges", valid[(0.004, 10)])):
            torch.manual_seed(inputs.PICK_SEED)
            indices = pick_indices_at_random(vmask, inputs.SAMPLES)
            assert indices.dtype == torch.int64 and len(indices) == inputs.SAMPLES < int(torch.count_nonzero(vmask))
            save[pre + f"pick_{tag}"] = indices.numpy().astype(np.int32)
            normals = normals_of(outputs, c2w_cv, indices)
            for mtag, mask in (("", None), ("_masked", f["mask"])):
                d = depth.clone()
                if mask is not None:
                    d[~mask] = 0                                        # export_mesh.py:395-396
                xyz, rgb = cu.get_colored_points_from_depth(depths=d, rgbs=outputs["rgb"], fx=fx, fy=fy, cx=cx, cy=cy, img_size=(W, H),
                                                            c2w=c2w_cv, mask=indices)
                assert torch.equal(rgb, f["rgb"].view(-1, 3)[indices])
                save[pre + f"points_{tag}{mtag}"] = xyz.numpy()
            save[pre + f"normals_{tag}"] = normals.numpy()
        # everything the loop keeps when fewer pixels are valid than asked for: ascending order
        few = pick_indices_at_random(valid[(0.004, 10)], H * W)
        assert torch.equal(few, torch.nonzero(valid[(0.004, 10)].ravel()).ravel())
        # the tsdf exporter's call (:868-880): all pixels, no index tensor
        xyz, rgb = cu.get_colored_points_from_depth(depths=depth, rgbs=outputs["rgb"], fx=fx, fy=fy, cx=cx, cy=cy, img_size=(W, H), c2w=c2w_cv)
        assert torch.equal(rgb, f["rgb"].view(-1, 3))
        save[pre + "points_all"] = xyz.numpy()
    np.savez_compressed(path, **save)
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
