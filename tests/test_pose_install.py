"""install(): with a camera optimiser the projection takes the optimised pose, the normal frame the raw camera (dn_model.py:475 vs
:551, :560); with the optimiser off the two are one tensor and nothing is passed.  No GPU: the fused pass is replaced by a recorder."""
import types

import torch

from test_install import _fixture, _model_class


def test_install_hands_the_optimised_pose_to_the_projection_and_the_raw_one_to_the_normals(dns, monkeypatch):
    from dn_splatter_amd import fused

    g, params, cam = _fixture()
    N, W, H = int(g["N"]), int(g["W"]), int(g["H"])
    calls = {}

    def render_dn_outputs(means, quats, scales, opacities, features_dc, features_rest, c2w, fx, fy, cx, cy, width, height, sh_degree,
                          background_rgb, normal_camera_to_world="absent", **kw):
        calls.update(c2w=c2w, normal=normal_camera_to_world)
        img = lambda c: torch.zeros(height, width, c)                          # noqa: E731
        out = {"rgb": img(3) + c2w.sum(), "depth": img(1), "normal": img(3), "surface_normal": img(3), "accumulation": img(1)}
        info = {"means2d": means[None, :, :2] * 1.0, "radii": torch.ones(1, N, dtype=torch.int32), "depths": torch.ones(1, N),
                "conics": torch.ones(1, N, 3), "tiles_per_gauss": torch.ones(1, N, dtype=torch.int32), "normals_world": torch.zeros(N, 3)}
        return out, info

    monkeypatch.setattr(fused, "render_dn_outputs", render_dn_outputs)
    Model = _model_class()
    dns.install(Model)
    try:
        m = Model(params, step=int(g["step"]))
        m.get_outputs(cam)                                                     # optimiser "off": apply_to_camera returns the raw tensor
        assert torch.equal(calls["c2w"], cam.camera_to_worlds[0]) and calls["normal"] is None
        leaf = (cam.camera_to_worlds + 0.01).detach().requires_grad_(True)     # stand-in optimiser: a [1,3,4] leaf
        m.camera_optimizer = types.SimpleNamespace(apply_to_camera=lambda c: leaf)
        out = m.get_outputs(cam)
        assert torch.equal(calls["c2w"], leaf[0]) and calls["c2w"].requires_grad
        assert torch.equal(calls["normal"], cam.camera_to_worlds[0]) and not calls["normal"].requires_grad
        out["rgb"].sum().backward()
        assert leaf.grad is not None and leaf.grad.shape == (1, 3, 4)          # the pose is part of the graph install() builds
        m.training = False                                                     # evaluation: the raw pose for both (dn_model.py:424)
        m.get_outputs(cam)
        assert torch.equal(calls["c2w"], cam.camera_to_worlds[0]) and calls["normal"] is None
    finally:
        dns.uninstall(Model)
