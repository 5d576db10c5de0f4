"""The level-set ray search against vectors produced by THE REFERENCE's own code (tests/golden/make_reference_levelset_golden.py:
``DNSplatterModel.compute_level_surface_points`` executed from its text on the recipe of _levelset_inputs.py): the PyTorch restatement
of torch_levelset — the fp64 yardstick of tests/test_gpu_levelset.py and the CPU path of ``install_level_sets`` — the layout of the two
new argument structs and the argument checks of the entry points.

Tolerances.  The generator printed, for 3600 Gaussians and a 48 x 40 frame of which 1652 pixels take part,
    e_ref: t 2.527e-06 (of kappa dT), analytical normals 4.720e-06 (component-wise); densities 1.258e-05 (relative to max(value, 1e-4))
    flagged shares: 0.00061, 0.00000, 0.00000
— the error of the reference's own fp32 outputs against the fp64 restatement on the unflagged hits (_levelset_inputs.E_REF_T /
E_REF_NORMAL).  t is measured in units of kappa (T_a - T_{a-1}), kappa = (|D_a| + |D_{a-1}| + L) / |D_a - D_{a-1}| the condition
number of the interpolation.  The fp32 restatement is held to 1 x e_ref plus its own distance from the fp64 one."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import _levelset_inputs as inputs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "dnsplat.h")
NL = len(inputs.LEVELS)


@pytest.fixture(scope="module")
def gold():
    return inputs.load_golden(os.path.join(HERE, "golden", inputs.GOLDEN))


@pytest.fixture(scope="module")
def rays(gold):
    """The restatement on the fixture in float64 and float32, once."""
    from dn_splatter_amd import torch_levelset as tl

    _, gp, fr, cam = gold
    args = (fr["depth"], cam.camera_to_worlds, cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height, fr["mask"], inputs.LEVELS)
    g64 = {k: v.double() for k, v in gp.items()}
    return (tl.level_rays(g64["means"], g64["scales"], g64["quats"], g64["opacities"], *args),
            tl.level_rays(gp["means"], gp["scales"], gp["quats"], gp["opacities"], *args))


def test_the_fixture_is_the_recipe(gold):
    g, gp, fr, cam = gold
    fresh_gp, fresh_fr, _ = inputs.scene()
    for k, v in fresh_gp.items():
        assert torch.equal(v, gp[k]), k
    for k, v in fresh_fr.items():
        assert torch.equal(v, fr[k]), k
    assert (cam.height, cam.width) == (inputs.H_FIX, inputs.W_FIX)
    assert bool((fr["depth"] == 0).any()) and bool((fr["depth"] < 0).any()) and not bool(fr["mask"].all())
    assert bool((gp["opacities"] > 0).any()) and bool((gp["opacities"] < 0).any())


def test_range_table_is_torchs_linspace():
    from dn_splatter_amd import torch_levelset as tl

    r = tl.range_table()
    assert r.dtype == torch.float32 and torch.equal(r, torch.linspace(-3, 3, 21)) and float(r[0]) == -3.0 and float(r[20]) == 3.0


def test_the_recipes_conditions_hold(gold, rays):
    """What the generator asserted, again from the file: rank gaps, the shares of hits and empties, the flagged shares, and that no
    unflagged ray decided otherwise in the reference's fp32."""
    g, gp, fr, cam = gold
    r64, _ = rays
    part = r64["part"]
    n = int(part.sum())
    assert g["ref_densities"].shape == (n, 21)
    assert inputs.smallest_rank_gap(gp["means"], r64["points"][part].float(), inputs.RANKS) >= inputs.GAP
    for l in range(NL):
        empty_ref, first_ref = inputs.reference_decisions(g, l)
        flag = inputs.flagged(r64, l)[part]
        share = float(flag.sum()) / n
        print(f"level {inputs.LEVELS[l]}: {int((~empty_ref).sum())} hits, {int(flag.sum())} flagged ({share:.5f})")
        assert share <= inputs.MAX_FLAGGED and abs(share - inputs.FLAGGED_SHARE[l]) < 1e-5 and abs(share - float(g["flagged_share"][l])) < 1e-9
        ok = ~flag
        empty64, first64 = r64["empty"][l][part], r64["first_above"][l][part]
        assert torch.equal(empty_ref[ok], empty64[ok]) and torch.equal(first_ref[ok], first64[ok])
        assert float((~empty64).sum()) / n >= 0.25 and float(empty64.sum()) / n >= 0.10
        assert torch.unique(first64[~empty64]).numel() >= 10


def _hits(g, r64, l):
    """(rows of the reference's outputs, pixels) of the unflagged rays that both the reference and the fp64 restatement hit."""
    part = r64["part"]
    empty_ref, _ = inputs.reference_decisions(g, l)
    both = ~inputs.flagged(r64, l)[part] & ~empty_ref & ~r64["empty"][l][part]
    return (torch.cumsum(~empty_ref, 0) - 1)[both], torch.nonzero(part).reshape(-1)[both]


def test_e_ref_is_what_the_header_states(gold, rays):
    g, gp, fr, cam = gold
    r64, _ = rays
    e_t = e_n = 0.0
    for l in range(NL):
        rows, pix = _hits(g, r64, l)
        t_ref = torch.from_numpy(g[f"ref_t_L{l}"])[rows].double()
        e_t = max(e_t, float(((t_ref - r64["t"][l][pix]).abs() / (r64["kappa"][l][pix] * r64["dT"][l][pix])).max()))
        e_n = max(e_n, float((inputs.ref_level(g, l, "analytical")[1][rows].double() - r64["normals"][l][pix]).abs().max()))
    e_d = float(((torch.from_numpy(g["ref_densities"]).double() - r64["densities"][r64["part"]]).abs()
                 / r64["densities"][r64["part"]].clamp_min(1e-4)).max())
    print(f"e_ref t {e_t:.3e} normals {e_n:.3e} densities {e_d:.3e}; file {g['e_ref']}")
    assert e_t <= inputs.E_REF_T * 1.001 and e_n <= inputs.E_REF_NORMAL * 1.001 and e_d <= inputs.E_REF_DENSITY * 1.001
    assert g["e_ref"][0] <= inputs.E_REF_T * 1.001 and g["e_ref"][1] <= inputs.E_REF_NORMAL * 1.001
    assert inputs.TOL_T == 4 * inputs.E_REF_T and inputs.TOL_NORMAL == 4 * inputs.E_REF_NORMAL


def test_fp32_restatement_reproduces_the_references_hits(gold, rays):
    g, gp, fr, cam = gold
    r64, r32 = rays
    part = r64["part"]
    assert torch.equal(r32["part"], part) and torch.equal(r32["closest"], r64["closest"])
    for l in range(NL):
        empty_ref, first_ref = inputs.reference_decisions(g, l)
        ok = ~inputs.flagged(r64, l)[part]
        assert torch.equal(r32["empty"][l][part][ok], empty_ref[ok]) and torch.equal(r32["first_above"][l][part][ok], first_ref[ok])
        rows, pix = _hits(g, r64, l)
        pts_ref, nrm_closest = inputs.ref_level(g, l, "closest")
        _, nrm_an = inputs.ref_level(g, l, "analytical")
        if bool(ok.all()):                                                                              # the same rays: the same colours, bit for bit
            assert torch.equal(torch.nonzero(part).reshape(-1)[~empty_ref], torch.nonzero(~r32["empty"][l]).reshape(-1))
        assert torch.equal(nrm_closest[rows], gp["normals"][r32["closest"][pix, 0]])                      # bit-equal
        scale = r64["kappa"][l][pix] * r64["dT"][l][pix]
        own = (r32["t"][l][pix].double() - r64["t"][l][pix]).abs()
        err = (r32["t"][l][pix].double() - torch.from_numpy(g[f"ref_t_L{l}"])[rows].double()).abs()
        print(f"level {inputs.LEVELS[l]}: t restatement vs reference, worst {float((err / scale).max()):.3e} of kappa dT")
        assert bool((err <= inputs.E_REF_T * scale + own).all())
        own_n = (r32["normals"][l][pix].double() - r64["normals"][l][pix]).abs()
        assert bool(((r32["normals"][l][pix] - nrm_an[rows]).abs().double() <= inputs.E_REF_NORMAL + own_n).all())
        # the point through t: one fp32 rounding of the point's magnitude on top
        x = r64["points"][pix] + torch.from_numpy(g[f"ref_t_L{l}"])[rows].double()[:, None] * r64["dir"][pix]
        assert bool(((pts_ref[rows].double() - x).abs() <= 2.0 ** -22 * pts_ref[rows].double().abs().max(dim=-1, keepdim=True).values).all())


class _Model:
    """What install_level_sets reads from a model."""

    def __init__(self, gp, fr):
        for k, v in gp.items():
            setattr(self, k, v)
        self._fr = fr

    def get_outputs(self, camera):
        return {"depth": self._fr["depth"], "rgb": self._fr["rgb"]}


def test_install_level_sets_cpu_path_returns_the_references_shape(dns, gold, rays):
    g, gp, fr, cam = gold
    r64, r32 = rays
    model = _Model(gp, fr)
    assert dns.install_level_sets(model) == ["compute_level_surface_points"]
    out = model.compute_level_surface_points(cam, 10 ** 9, mask=fr["mask"], return_normal="analytical")
    assert list(out.keys()) == list(inputs.LEVELS)
    colors = fr["rgb"].reshape(-1, 3)
    for l, level in enumerate(inputs.LEVELS):
        assert sorted(out[level].keys()) == ["colors", "normals", "points"]
        hit = torch.nonzero(~r32["empty"][l]).reshape(-1)                                   # every hit, in raster order
        assert torch.equal(out[level]["points"], r32["hit_points"][l][hit]) and torch.equal(out[level]["colors"], colors[hit])
        assert torch.equal(out[level]["normals"], r32["normals"][l][hit])
    few = model.compute_level_surface_points(cam, 50, mask=fr["mask"], surface_levels=(0.3,))
    assert list(few.keys()) == [0.3] and all(tuple(v.shape) == (50, 3) for v in few[0.3].values())
    rows = {tuple(p.tolist()) for p in few[0.3]["points"]}
    assert len(rows) == 50 and rows <= {tuple(p.tolist()) for p in r32["hit_points"][1][~r32["empty"][1]]}
    closest = gp["normals"][r32["closest"][:, 0].clamp(min=0)]
    assert {tuple(p.tolist()) for p in few[0.3]["normals"]} <= {tuple(p.tolist()) for p in closest}


def test_average_normals_raise_as_in_the_reference(dns, gold):
    from dn_splatter_amd import torch_levelset as tl

    _, gp, fr, cam = gold
    model = _Model(gp, fr)
    dns.install_level_sets(model)
    with pytest.raises(NotImplementedError):
        model.compute_level_surface_points(cam, 10, return_normal="average")
    with pytest.raises(NotImplementedError):
        tl.level_surface_points(gp["means"], gp["scales"], gp["quats"], gp["opacities"], gp["normals"], fr, cam, 10, return_normal="average")
    with pytest.raises(ValueError):
        tl.level_rays(gp["means"][:16], gp["scales"][:16], gp["quats"][:16], gp["opacities"][:16], fr["depth"], cam.camera_to_worlds,
                      cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height)


def test_level_args_layouts_match_the_c_compiler(dns, tmp_path):
    from dn_splatter_amd import _lib

    structs = {"dnsplat_level_rays_args": _lib.LevelRaysArgs, "dnsplat_level_points_args": _lib.LevelPointsArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){']
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append('printf("consts %d %d %d\\n", DNSPLAT_LEVEL_RANGE_POINTS, DNSPLAT_LEVEL_MAX_LEVELS, DNSPLAT_LEVEL_KNN);')
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = dict(l.split(maxsplit=1) for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"
    from dn_splatter_amd import levelset

    assert got["consts"].split() == [str(levelset.RANGE_POINTS), str(levelset.MAX_LEVELS), "16"]


def test_entry_points_check_their_arguments_without_a_launch(dns):
    from dn_splatter_amd import _lib

    L = dns.load_library()
    p = ctypes.c_void_p(64)                                              # never dereferenced: every call below returns before a launch
    assert L.dnsplat_level_rays(None, None) == -1 and L.dnsplat_level_points(None, None) == -1

    def rays(**kw):
        a = _lib.LevelRaysArgs()
        a.width, a.height, a.N, a.n_levels = 8, 8, 17, 3
        for k in ("depth", "xform", "range", "index", "records", "scales_log", "quats", "t_hit", "valid", "closest"):
            setattr(a, k, p)
        for k, v in kw.items():
            setattr(a, k, v)
        return L.dnsplat_level_rays(ctypes.byref(a), None)

    for bad in (dict(depth=None), dict(xform=None), dict(range=None), dict(records=None), dict(scales_log=None), dict(quats=None),
                dict(t_hit=None), dict(valid=None), dict(closest=None), dict(index=None), dict(width=0), dict(height=0), dict(n_levels=0),
                dict(n_levels=9), dict(N=16), dict(lane_map=2)):
        assert rays(**bad) == -1, bad
    assert rays(width=65536, height=32768) == -4

    def points(**kw):
        a = _lib.LevelPointsArgs()
        a.width, a.height, a.N, a.n_rows, a.capacity = 8, 8, 17, 4, 4
        for k in ("depth", "rgb", "indices", "xform", "t_hit", "closest", "gauss_normals", "index", "records", "points", "colors", "normals",
                  "state", "scratch"):
            setattr(a, k, p)
        for k, v in kw.items():
            setattr(a, k, v)
        return L.dnsplat_level_points(ctypes.byref(a), None)

    for bad in (dict(depth=None), dict(rgb=None), dict(indices=None), dict(xform=None), dict(t_hit=None), dict(points=None), dict(colors=None),
                dict(normals=None), dict(state=None), dict(scratch=None), dict(width=0), dict(capacity=0), dict(n_rows=-1), dict(normal_mode=2),
                dict(closest=None), dict(gauss_normals=None), dict(normal_mode=1, index=None), dict(normal_mode=1, N=16)):
        assert points(**bad) == -1, bad
    assert points(width=65536, height=32768) == -4
    assert points(n_rows=0) == 0
