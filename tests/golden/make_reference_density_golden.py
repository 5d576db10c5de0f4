"""Golden vectors of the Gaussian density field, produced by THE REFERENCE's own code: ``knn_sk`` of dn_splatter/utils/knn.py loaded
by path (sklearn on the CPU), ``DNSplatterModel.get_density`` and ``get_density_grad`` (dn_model.py:1077-1135, :1449-1494) executed from
their text on a stub that carries the parameters — with ``scale_rot_to_inv_cov3d`` from the same file's text and gsplat's
``quat_to_rotmat`` by its published formula, as make_reference_golden.py supplies it — and the lattice statements of
``MarchingCubesMesh.main`` (export_mesh.py:740-773) executed from their text.  ``get_closest_gaussians`` itself moves its arguments to
"cuda"; the stub's calls ``knn_sk(x=means, y=samples, k=16)`` as it does, without the move.  nerfstudio's ``OrientedBox.within`` is not
at hand: the crop box is ``torch_export.within`` ("parity unpinned", as in the export fixture).  Nothing of the reference is copied: only
inputs (tests/_density_inputs.py) and the reference's OUTPUTS are stored (tests/golden/reference_density.npz).

    python tests/golden/make_reference_density_golden.py     # needs the reference checkout and sklearn; rewrites reference_density.npz
"""
import ast
import os
import sys
import textwrap
import types
from typing import Optional

import numpy as np
import torch
from torch import Tensor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_reference_golden import REF, _load, extract_function, extract_method, quat_to_rotmat_published  # noqa: E402

import _density_inputs as inputs  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from dn_splatter_amd import torch_density as td  # noqa: E402
from dn_splatter_amd import torch_export as te  # noqa: E402

DN_MODEL = os.path.join(REF, "dn_splatter/dn_model.py")
EXPORT_MESH = os.path.join(REF, "dn_splatter/export_mesh.py")


def reference_model(t):
    """A stub with the parameters and the reference's two methods, compiled from their text."""
    knn_sk = _load("dn_splatter.utils.knn", "dn_splatter/utils/knn.py").knn_sk
    ns = dict(torch=torch, Tensor=Tensor, Optional=Optional, quat_to_rotmat=quat_to_rotmat_published)
    exec(compile(extract_function(DN_MODEL, "scale_rot_to_inv_cov3d"), "dn_model.py::scale_rot_to_inv_cov3d", "exec"), ns)
    for name in ("get_density", "get_density_grad"):
        exec(compile(textwrap.dedent(extract_method(DN_MODEL, "DNSplatterModel", name)), f"dn_model.py::{name}", "exec"), ns)

    class Stub:
        device = torch.device("cpu")

        def get_closest_gaussians(self, samples):
            return knn_sk(x=self.means, y=samples, k=16)             # dn_model.py:1070-1074 without the move to "cuda"

    stub = Stub()
    for k in ("means", "scales", "quats", "opacities"):
        setattr(stub, k, t[k])
    stub.get_density = types.MethodType(ns["get_density"], stub)
    stub.get_density_grad = types.MethodType(ns["get_density_grad"], stub)
    return stub, knn_sk


def lattice_statements():
    """The statements of MarchingCubesMesh.main from ``X = torch.linspace(...)`` to the -1e6 fill, as a function of
    (self, radius, crop_box, model) returning ``densities``."""
    tree = ast.parse(textwrap.dedent(extract_method(EXPORT_MESH, "MarchingCubesMesh", "main")))
    for node in ast.walk(tree):
        if isinstance(node, ast.With):
            names = [ast.unparse(s.targets[0]) if isinstance(s, ast.Assign) else "" for s in node.body]
            if "X" in names:
                first = names.index("X")
                last = max(i for i, s in enumerate(node.body) if isinstance(s, ast.If) and "-1000000.0" in ast.unparse(s))
                code = compile("\n".join(ast.unparse(s) for s in node.body[first:last + 1]), "export_mesh.py::MarchingCubesMesh.main[lattice]", "exec")

                def run(self, radius, crop_box, model):
                    ns = dict(torch=torch, self=self, radius=radius, crop_box=crop_box, model=model,
                              CONSOLE=types.SimpleNamespace(print=lambda *a, **k: None))
                    exec(code, ns)
                    return ns["densities"]

                return run
    raise KeyError("the lattice statements were not found")


def main(path=os.path.join(HERE, inputs.GOLDEN)):
    t = inputs.field_inputs()
    means, samples = t["means"], t["samples"]
    model, knn_sk = reference_model(t)

    # the recipe's conditions (the allowed count of each is 0)
    gap = inputs.smallest_rank_gap(means, samples)
    assert gap >= inputs.GAP, f"two consecutive ranks are {gap:.3e} apart (relative)"
    assert torch.unique(means, dim=0).shape[0] == means.shape[0], "duplicate means"

    closest = knn_sk(x=means, y=samples, k=16)
    assert closest.dtype == torch.int64 and tuple(closest.shape) == (inputs.M_FIX, 16)
    assert torch.equal(closest, td.knn(means, samples, 16, skip=1)), "knn_sk differs from the stable fp64 ranking"
    for n, m in ((1000, 1000), (18, 65)):                             # sklearn's other code paths (brute force below its leaf size)
        u = inputs.field_inputs(n, m, seed=inputs.SEED + n)
        assert torch.equal(knn_sk(x=u["means"], y=u["samples"], k=16), td.knn(u["means"], u["samples"], 16, skip=1)), (n, m)

    with torch.no_grad():
        dens = model.get_density(samples)
        dens_given = model.get_density(samples, closest_gaussians=closest)
        assert torch.equal(dens, dens_given)
        grads = {nc: model.get_density_grad(samples, num_closest_gaussians=nc) for nc in (None, 1, 5)}
    t64 = {k: v.double() for k, v in t.items()}
    sum64 = td.density_sum(t64["means"], t64["scales"], t64["quats"], t64["opacities"], t64["samples"], closest)
    flag = (sum64 - 1.0).abs() <= inputs.SWITCH_ENVELOPE
    side32 = td.density_sum(t["means"], t["scales"], t["quats"], t["opacities"], samples, closest) >= 1.0
    assert torch.equal(side32[~flag], (sum64 >= 1.0)[~flag]), "an unflagged density took the other side of the switch in fp32"

    # e_ref: the reference's own fp32 outputs against the fp64 restatement
    d64 = td.density(t64["means"], t64["scales"], t64["quats"], t64["opacities"], t64["samples"], closest)
    e_d = ((dens.double() - d64).abs() / d64.clamp_min(1e-4))[~flag].max()
    e_n = max(float((grads[nc].double() - td.density_grad(t64["means"], t64["scales"], t64["quats"], t64["samples"], nc, closest)).abs().max())
              for nc in grads)
    print(f"N = {inputs.N_FIX}, M = {inputs.M_FIX}: smallest rank gap {gap:.3e}; {int(flag.sum())} samples flagged at the switch; "
          f"{int((sum64 >= 1).sum())} densities above it, {int((dens <= 1e-4).sum())} at the floor")
    print(f"e_ref: density {float(e_d):.3e} (relative to max(value, 1e-4)), normals {e_n:.3e} (component-wise)")

    box = inputs.crop_box()
    box.within = types.MethodType(lambda self, pts: te.within(self, pts), box)
    exporter = types.SimpleNamespace(resolution=inputs.VOLUME_R, batch_size=1000)
    run = lattice_statements()
    with torch.no_grad():
        vol = run(exporter, inputs.VOLUME_RADIUS, None, model)
        vol_crop = run(exporter, inputs.VOLUME_RADIUS, box, model)
    assert tuple(vol.shape) == (inputs.VOLUME_R,) * 3 and 0 < int((vol_crop == -1e6).sum()) < vol.numel()

    save = {k: v.numpy() for k, v in t.items()}
    save.update(closest=closest.numpy().astype(np.uint16), density=dens.numpy(), switch_flag=np.packbits(flag.numpy()),
                e_ref=np.array([float(e_d), e_n]), volume=vol.numpy(), volume_crop=vol_crop.numpy(),
                volume_spec=np.array([inputs.VOLUME_R, inputs.VOLUME_RADIUS], dtype=np.float64))
    for nc, gr in grads.items():
        save[f"grad_{nc or 'all'}"] = gr.numpy()
    np.savez_compressed(path, **save)
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
