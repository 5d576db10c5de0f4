"""Golden vectors of the geometry scores, produced by THE REFERENCE's own code:

  * ``calculate_accuracy``, ``calculate_completeness`` and ``PDMetrics`` of dn_splatter/metrics.py, loaded by path with the torchmetrics
    stand-in of make_reference_metrics_golden.py;
  * ``compute_metrics``, ``distance_p2p`` and ``get_threshold_percentage`` of dn_splatter/eval/eval_mesh_vis_cull.py, whose module imports
    (open3d, trimesh, pyrender, cv2, tyro, ...) cannot be satisfied here: the three function definitions are cut out of the file with
    ``ast`` and executed as they stand, with numpy and scipy's cKDTree in their namespace, a no-op ``get_colored_pcd`` and stand-in mesh
    objects that supply ``.area``, ``.sample(count, return_index=True)`` and ``.face_normals`` from PRE-DRAWN samples (one "face" per
    sample), so that what runs behind the sampling is the reference's own arithmetic.

Nothing of the reference is copied: only inputs (tests/_geometry_inputs.py, fp32 values) and the reference's OUTPUTS are stored
(tests/golden/reference_geometry.npz).

    python tests/golden/make_reference_geometry_golden.py     # needs the reference checkout; rewrites reference_geometry.npz
"""
import ast
import os
import sys
import types

import numpy as np
from scipy.spatial import cKDTree

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_reference_golden import REF  # noqa: E402
from make_reference_metrics_golden import load_metrics  # noqa: E402

import _geometry_inputs as inputs  # noqa: E402

PERCENTILES = (0.0, 50.0, 90.0, 100.0)


def load_mesh_eval():
    """{name: function} of the three functions, executed from the reference's text; ``recorded`` collects what get_threshold_percentage
    returned (compute_metrics folds precision and recall into F and does not return them)."""
    path = os.path.join(REF, "dn_splatter/eval/eval_mesh_vis_cull.py")
    tree = ast.parse(open(path).read())
    wanted = ("get_threshold_percentage", "distance_p2p", "compute_metrics")
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in wanted]
    assert sorted(n.name for n in body) == sorted(wanted)
    ns = {"np": np, "cKDTree": cKDTree, "get_colored_pcd": lambda pcd, metric: None}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    recorded = []
    inner = ns["get_threshold_percentage"]

    def recording(dist, thresholds):
        out = inner(dist, thresholds)
        recorded.append(out)
        return out

    ns["get_threshold_percentage"] = recording
    return ns, recorded


class SampledMesh:
    """What compute_metrics touches of a trimesh: ``area`` such that int(area * 1e4) is the number of pre-drawn samples, ``sample`` that
    hands them out with their indices, ``face_normals`` with one row per sample."""

    def __init__(self, points, normals):
        self.points, self.face_normals = points.astype(np.float64), normals.astype(np.float64)
        self.area = (len(points) + 0.5) / 1e4

    def sample(self, count, return_index=False):
        assert count == len(self.points) and return_index
        return self.points, np.arange(count)


def main(path=os.path.join(HERE, "reference_geometry.npz")):
    ref = load_metrics()
    ns, recorded = load_mesh_eval()
    tgt, tgt_n = inputs.target()
    src, src_n = inputs.source()
    save = {"tgt": tgt, "tgt_normals": tgt_n, "src": src, "src_normals": src_n, "percentiles": np.array(PERCENTILES)}

    # the two directions of distance_p2p: "acc" = source (the prediction) to target, "comp" = target to source
    for name, (a, an, b, bn) in {"acc": (src, src_n, tgt, tgt_n), "comp": (tgt, tgt_n, src, src_n)}.items():
        dist, dot = ns["distance_p2p"](a.astype(np.float64), an.astype(np.float64), b.astype(np.float64), bn.astype(np.float64))
        two, idx = cKDTree(b.astype(np.float64)).query(a.astype(np.float64), k=2)
        assert np.array_equal(two[:, 0], dist)
        save[name + "_dist"], save[name + "_dot"], save[name + "_idx"], save[name + "_second"] = dist, dot, idx[:, 0].astype(np.int32), two[:, 1]
        near = np.abs(dist - 0.05).min()
        gap = ((two[:, 1] - two[:, 0]) / two[:, 1]).min()
        print(f"{name}: {len(dist)} rows, nearest distance to the threshold {near:.3e}, smallest relative gap of the best two {gap:.3e}")
        assert near > 1e-9 and gap > 1e-9

    rst = ns["compute_metrics"](SampledMesh(src, src_n), SampledMesh(tgt, tgt_n))
    recall, precision = recorded                                        # compute_metrics asks for recall first (:354), then precision
    save["mesh_keys"] = np.array(list(rst.keys()))
    save["mesh_values"] = np.array([float(rst[k]) for k in rst], dtype=np.float64)
    save["mesh_precision"], save["mesh_recall"] = np.float32(precision[0]), np.float32(recall[0])
    print({k: float(v) for k, v in rst.items()}, "precision", precision[0], "recall", recall[0])

    pd = ref.PDMetrics()
    acc, comp = pd(types.SimpleNamespace(points=src.astype(np.float64)), types.SimpleNamespace(points=tgt.astype(np.float64)))
    save["pd_acc"], save["pd_comp"] = np.float64(acc), np.float64(comp)
    save["accuracy"] = np.array([ref.calculate_accuracy(src.astype(np.float64), tgt.astype(np.float64), percentile=q) for q in PERCENTILES])
    save["completeness"] = np.float64(ref.calculate_completeness(src.astype(np.float64), tgt.astype(np.float64), threshold=0.05))
    print(f"PDMetrics acc {acc:.6f} comp {comp:.4f}; share <= 0.05 {float(precision[0]):.3f}")
    assert 0.2 < float(precision[0]) < 0.8 and 0.05 < acc, "the threshold and the percentile do not separate"
    np.savez_compressed(path, **save)
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
