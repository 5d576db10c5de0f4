"""Golden vectors of the level-set ray search, produced by THE REFERENCE's own code: ``DNSplatterModel.compute_level_surface_points``
(dn_model.py:1206-1447) executed from its text on a stub that carries the parameters, with ``knn_sk`` of dn_splatter/utils/knn.py
(sklearn on the CPU) and ``get_colored_points_from_depth`` of utils/camera_utils.py loaded by path, ``scale_rot_to_inv_cov3d`` and
``invert_quaternion`` from the same file's text, gsplat's ``quat_to_rotmat`` by its published formula (as make_reference_golden.py
supplies it), a ``get_outputs`` that returns the fixture's depth and rgb, and a stand-in for ``random`` whose ``sample(range, k)``
returns the first k of the range in order: with ``num_samples`` above the pixel count the golden holds EVERY hit in raster order.
The method's frame is read when it returns (``sys.setprofile``) for the reference's own float32 ``densities`` and ``points_range``, from
which the rays it hit, their first sample above each level and its ``intersection_t`` follow by its own statements (checked against the
frame's values for the last level).  Nothing of the reference is copied: only inputs
(tests/_levelset_inputs.py) and the reference's OUTPUTS are stored (tests/golden/reference_levelset.npz).

    python tests/golden/make_reference_levelset_golden.py     # needs the reference checkout and sklearn; rewrites the npz
"""
import os
import sys
import textwrap
import types
from typing import Literal, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_reference_golden import REF, StubCameras, _load, extract_function, extract_method, load_reference, quat_to_rotmat_published  # noqa: E402

import _levelset_inputs as inputs  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from dn_splatter_amd import torch_export as te  # noqa: E402
from dn_splatter_amd import torch_levelset as tl  # noqa: E402

DN_MODEL = os.path.join(REF, "dn_splatter/dn_model.py")
NAME = "compute_level_surface_points"


class InOrder:
    """``random`` for the method: the first k of the population, in order."""

    @staticmethod
    def sample(population, k):
        return list(population)[:k]


def reference_model(gp, fr):
    cam_utils, _, _ = load_reference()
    knn_sk = _load("dn_splatter.utils.knn", "dn_splatter/utils/knn.py").knn_sk
    ns = dict(torch=torch, Tensor=Tensor, Optional=Optional, Tuple=Tuple, Literal=Literal, Cameras=object, random=InOrder, knn_sk=knn_sk,
              get_colored_points_from_depth=cam_utils.get_colored_points_from_depth, quat_to_rotmat=quat_to_rotmat_published)
    for fn in ("scale_rot_to_inv_cov3d", "invert_quaternion"):
        exec(compile(extract_function(DN_MODEL, fn), f"dn_model.py::{fn}", "exec"), ns)
    exec(compile(textwrap.dedent(extract_method(DN_MODEL, "DNSplatterModel", NAME)), f"dn_model.py::{NAME}", "exec"), ns)

    class Stub:
        device = torch.device("cpu")

        def get_outputs(self, camera):
            return {"depth": fr["depth"].clone(), "rgb": fr["rgb"].clone()}

    stub = Stub()
    for k, v in gp.items():
        setattr(stub, k, v)
    setattr(stub, NAME, types.MethodType(ns[NAME], stub))
    return stub


def run_reference(model, camera, mask, mode):
    """(all_outputs, the method's own float32 densities [n,21]) for one normal mode."""
    seen = {}

    def profile(f, event, arg):
        if event == "return" and f.f_code.co_name == NAME:
            seen.update(densities=f.f_locals["densities"].clone(), empty=f.f_locals["empty_pixels"].clone(),
                        first=f.f_locals["first_point_above_level"].clone(), ranges=f.f_locals["points_range"][..., 0].clone(),
                        t=f.f_locals["intersection_t"].clone())

    sys.setprofile(profile)
    try:
        with torch.no_grad():
            out = getattr(model, NAME)(camera, 10 ** 9, mask=mask, surface_levels=inputs.LEVELS, return_normal=mode)
    finally:
        sys.setprofile(None)
    return out, seen


def main(path=os.path.join(HERE, inputs.GOLDEN)):
    gp, fr, cam = inputs.scene()
    H, W = inputs.H_FIX, inputs.W_FIX
    P = H * W
    camera = StubCameras(cam.camera_to_worlds, cam.fx, cam.fy, cam.cx, cam.cy, W, H)
    model = reference_model(gp, fr)
    ref, seen = run_reference(model, camera, fr["mask"], "closest_gaussian")
    ref_an, seen_an = run_reference(model, camera, fr["mask"], "analytical")
    assert torch.equal(seen["densities"], seen_an["densities"])
    ref_D = seen["densities"]

    args = (fr["depth"], cam.camera_to_worlds, cam.fx, cam.fy, cam.cx, cam.cy, W, H, fr["mask"], inputs.LEVELS)
    g64 = {k: v.double() for k, v in gp.items()}
    r64 = tl.level_rays(g64["means"], g64["scales"], g64["quats"], g64["opacities"], *args)
    r32 = tl.level_rays(gp["means"], gp["scales"], gp["quats"], gp["opacities"], *args)
    part = r64["part"]
    n = int(part.sum())
    assert tuple(ref_D.shape) == (n, tl.RANGE_POINTS), (ref_D.shape, n)

    # the recipe's conditions
    d, p32 = tl.world_points(*args[:-1])
    cam_utils = sys.modules["dn_splatter.utils.camera_utils"]
    own, _ = cam_utils.get_colored_points_from_depth(depths=fr["depth"], rgbs=fr["rgb"], fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy,
                                                     img_size=(W, H), c2w=te.export_c2w(cam.camera_to_worlds.reshape(3, 4)))
    assert torch.equal(own[part], p32[part]), "the back-projected points differ from torch_export's"
    gap = inputs.smallest_rank_gap(gp["means"], p32[part], inputs.RANKS)
    assert gap >= inputs.GAP, f"two consecutive ranks are {gap:.3e} apart (relative)"
    knn_sk = sys.modules["dn_splatter.utils.knn"].knn_sk
    assert torch.equal(knn_sk(gp["means"], p32[part], 16), r64["closest"][part]), "knn_sk differs from the stable fp64 ranking"
    neg, zero, masked = int((fr["depth"] < 0).sum()), int((fr["depth"] == 0).sum()), int((~fr["mask"]).sum())
    assert neg > 0 and zero > 0 and masked > 0 and bool((gp["opacities"] > 0).any()) and bool((gp["opacities"] < 0).any())

    L32 = [torch.tensor(L, dtype=torch.float32) for L in inputs.LEVELS]
    e_t, e_n, shares = 0.0, 0.0, []
    save = {}
    for l, level in enumerate(inputs.LEVELS):
        # the reference's own two comparisons on its own densities (dn_model.py:1353-1357)
        under, above = ref_D - L32[l] < 0, ref_D - L32[l] > 0
        first_ref = above.max(dim=-1).indices
        empty_ref = ~under[:, 0] | (first_ref == 0)
        if l == len(inputs.LEVELS) - 1:
            assert torch.equal(empty_ref, seen["empty"]) and torch.equal(first_ref, seen["first"][:, 0])
        hits = int((~empty_ref).sum())
        for mode, out in (("closest", ref), ("analytical", ref_an)):
            assert tuple(out[level]["points"].shape) == (hits, 3), (level, mode)
        flag = inputs.flagged(r64, l)[part]
        share = float(flag.sum()) / n
        shares.append(share)
        empty64, first64 = r64["empty"][l][part], r64["first_above"][l][part]
        ok = ~flag
        assert share <= inputs.MAX_FLAGGED, f"level {level}: {share:.3%} of the rays are flagged"
        assert torch.equal(empty_ref[ok], empty64[ok]) and torch.equal((first_ref * ~empty_ref)[ok], first64[ok]), \
            f"level {level}: an unflagged ray decided otherwise in the reference's fp32"
        assert torch.equal(r32["empty"][l][part][ok], empty64[ok]) and torch.equal(r32["first_above"][l][part][ok], first64[ok])
        hit_share, empty_share, distinct = float((~empty64).sum()) / n, float(empty64.sum()) / n, int(torch.unique(first64[~empty64]).numel())
        assert hit_share >= 0.25 and empty_share >= 0.10 and distinct >= 10, (level, hit_share, empty_share, distinct)

        # e_ref on the unflagged hits: rows of the reference's outputs are its hits in raster order
        both = ok & ~empty_ref & ~empty64
        rows = (torch.cumsum(~empty_ref, 0) - 1)[both]
        full = torch.nonzero(part).reshape(-1)[both]
        a = first_ref[~empty_ref][:, None]                                                     # dn_model.py:1364-1380 on its own tensors
        Dh, Th = ref_D[~empty_ref], seen["ranges"][~empty_ref]
        Da, Db, Ta, Tb = Dh.gather(1, a)[:, 0], Dh.gather(1, a - 1)[:, 0], Th.gather(1, a)[:, 0], Th.gather(1, a - 1)[:, 0]
        t_hits = (level - Db) / (Da - Db) * (Ta - Tb) + Tb
        if l == len(inputs.LEVELS) - 1:
            assert torch.equal(t_hits, seen["t"])
        e_t = max(e_t, float(((t_hits[rows].double() - r64["t"][l][full]).abs() / (r64["kappa"][l][full] * r64["dT"][l][full])).max()))
        save[f"ref_t_L{l}"] = t_hits.numpy()
        e_n = max(e_n, float((ref_an[level]["normals"][rows].double() - r64["normals"][l][full]).abs().max()))
        assert torch.equal(ref[level]["colors"], fr["rgb"].reshape(-1, 3)[torch.nonzero(part).reshape(-1)[~empty_ref]])
        assert torch.equal(ref[level]["normals"], gp["normals"][r64["closest"][part][~empty_ref][:, 0]])
        print(f"level {level}: {hits} hits of {n} rays ({hit_share:.1%}), {empty_share:.1%} empty, {distinct} distinct first_above, "
              f"{int(flag.sum())} flagged ({share:.3%})")
        for mode, out in (("closest", ref), ("analytical", ref_an)):
            for k in ("points", "normals", "colors"):
                if not (k == "colors" or (mode == "analytical" and k == "points")):        # colours are the frame's; points repeat
                    save[f"ref_{mode}_L{l}_{k}"] = out[level][k].numpy()
        assert torch.equal(ref[level]["points"], ref_an[level]["points"]) and torch.equal(ref[level]["colors"], ref_an[level]["colors"])
    e_d = float(((ref_D.double() - r64["densities"][part]).abs() / r64["densities"][part].clamp_min(1e-4)).max())
    print(f"{n} of {P} pixels take part ({zero} zero, {neg} negative, {masked} masked); smallest rank gap {gap:.3e}")
    print(f"e_ref: t {e_t:.3e} (of kappa dT), analytical normals {e_n:.3e} (component-wise); densities {e_d:.3e} (relative to max(value, 1e-4))")
    print("flagged shares:", ", ".join(f"{s:.5f}" for s in shares))

    save.update({k: v.numpy() for k, v in gp.items()})
    save.update(size=np.array([H, W]), depth=fr["depth"].numpy().reshape(H, W), rgb_u8=torch.round(fr["rgb"] * 255).to(torch.uint8).numpy(),
                mask=np.packbits(fr["mask"].numpy().reshape(-1)), ref_densities=ref_D.numpy(), e_ref=np.array([e_t, e_n, e_d]),
                flagged_share=np.array(shares))
    np.savez_compressed(path, **save)
    print(path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
