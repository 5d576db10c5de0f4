"""Golden vectors of the evaluation metrics, produced by THE REFERENCE's own code: DepthMetrics, NormalMetrics and mean_angular_error of
dn_splatter/metrics.py, loaded by path as make_reference_golden.py loads the other modules.  The file imports torchmetrics at its top
(for RGBMetrics, which is not used here): that import is satisfied with an empty stand-in, so the psnr formula is NOT pinned by this
fixture.  Nothing of the reference is copied: only inputs (tests/_metrics_inputs.py, quantised) and the reference's OUTPUTS are stored
(tests/golden/reference_metrics.npz).

    python tests/golden/make_reference_metrics_golden.py     # needs the reference checkout; rewrites reference_metrics.npz
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_reference_golden import _load  # noqa: E402

import _metrics_inputs as inputs  # noqa: E402


def load_metrics():
    for name in ("torchmetrics", "torchmetrics.image", "torchmetrics.image.lpip"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchmetrics.image"].PeakSignalNoiseRatio = object
    sys.modules["torchmetrics.image"].StructuralSimilarityIndexMeasure = object
    sys.modules["torchmetrics.image.lpip"].LearnedPerceptualImagePatchSimilarity = object
    return _load("dn_splatter_metrics_by_path", "dn_splatter/metrics.py")


def _np(ts):
    return np.array([float(t) for t in ts], dtype=np.float32)


def main(path=os.path.join(HERE, "reference_metrics.npz")):
    ref = load_metrics()
    depth_metrics, normal_metrics = ref.DepthMetrics(), ref.NormalMetrics()
    assert depth_metrics.tolerance == inputs.TOLERANCE
    save = {"tolerance": np.float64(depth_metrics.tolerance)}
    for (H, W), seed in zip(inputs.FIXTURE_FRAMES, (0, 1)):
        f = inputs.frame(H, W, seed)
        pre = f"f{H}x{W}_"
        save[pre + "depth_q"] = torch.round(f["depth"] * inputs.DEPTH_GRID).to(torch.int32).numpy().astype(np.uint16)
        save[pre + "gt_depth_q"] = torch.round(f["gt_depth"] * inputs.DEPTH_GRID).to(torch.int32).numpy().astype(np.uint16)
        save[pre + "normal_q"] = torch.round(f["normal"] * inputs.GRID).to(torch.int32).numpy().astype(np.uint16)
        save[pre + "gt_normal_u8"] = f["gt_normal_u8"].numpy()
        back = inputs.fixture_frame({k: v for k, v in save.items()}, H, W)
        assert all(torch.equal(back[k], f[k]) for k in back), "the stored integers do not give the inputs back"
        # as the model calls them (dn_model.py:882-884, :907-910)
        d = depth_metrics(f["depth"].permute(2, 0, 1), f["gt_depth"].permute(2, 0, 1))
        n = normal_metrics(f["normal"].permute(2, 0, 1).unsqueeze(0), f["gt_normal"].permute(2, 0, 1).unsqueeze(0))
        angle = ref.mean_angular_error(f["normal"].permute(2, 0, 1).unsqueeze(0), f["gt_normal"].permute(2, 0, 1).unsqueeze(0))
        save[pre + "depth"], save[pre + "normal"], save[pre + "angle"] = _np(d), _np(n), angle.numpy().astype(np.float32)
        print(f"{H}x{W}: depth {_np(d)}  normal {_np(n)}")
        assert 0.2 < float(d[4]) < float(d[5]) < float(d[6]) < 1.0, "the thresholds do not separate"
    for name, (pred, gt) in inputs.DEPTH_EDGES.items():
        save["edge_depth_" + name] = _np(depth_metrics(pred, gt))
        print(f"depth edge {name}: {save['edge_depth_' + name]}")
    for name, (pred, gt) in inputs.NORMAL_EDGES.items():
        save["edge_normal_" + name] = _np(normal_metrics(pred, gt))
        print(f"normal edge {name}: {save['edge_normal_' + name]}")
    np.savez_compressed(path, **save)
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
