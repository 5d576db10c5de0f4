"""TSDF fusion and the observed marching cubes, the parts of their C ABI that need no GPU: the exports, the layout of the two argument
structs as gcc sees include/dnsplat.h against their ctypes mirrors, the scratch query against the layout arithmetic, and the argument
checks, which return before any launch (the pointers here are host memory that nothing may touch)."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dnsplat.h")
SYMBOLS = ("dnsplat_tsdf_integrate", "dnsplat_tsdf_vertex_colors", "dnsplat_mc_observed_scratch_bytes", "dnsplat_mc_count_observed",
           "dnsplat_mc_emit_observed")


@pytest.fixture(scope="module")
def L(dns):
    dns.build_library()
    return dns.load_library()


def test_symbols_are_exported_and_declared_and_the_abi_stays(dns, L):
    from dn_splatter_amd import _lib

    raw = ctypes.CDLL(str(dns.build_library()))
    text = open(HEADER).read()
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS, name
        assert name + "(" in text, name
    for struct in ("dnsplat_tsdf_args", "dnsplat_mc_observed_args"):
        assert "} " + struct + ";" in text
    assert L.dnsplat_abi_version() == 15 and _lib.ABI_VERSION == 15              # additive: found by symbol, the version stays
    assert "PARITY UNPINNED AGAINST Open3D" in text
    for name in ("TSDFVolume", "fuse_tsdf_mesh", "tsdf", "torch_tsdf"):
        assert hasattr(dns, name) and name in dns.__all__


def test_struct_layouts_match_the_c_compiler(dns, tmp_path):
    from dn_splatter_amd import _lib

    structs = {"dnsplat_tsdf_args": _lib.TsdfArgs, "dnsplat_mc_observed_args": _lib.McObservedArgs, "dnsplat_mc_args": _lib.McArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){']
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"


def test_observed_scratch_is_the_layout_plus_one_word_per_64_points(L):
    for shape in ((2, 2, 2), (5, 6, 7), (17, 9, 33), (64, 64, 64), (512, 512, 512), (1, 9, 9)):
        n = shape[0] * shape[1] * shape[2]
        words = (n + 63) // 64
        plane = (words * 8 + 15) // 16 * 16
        assert L.dnsplat_mc_observed_scratch_bytes(*shape) == L.dnsplat_mc_scratch_bytes(*shape) + plane, shape
    assert L.dnsplat_mc_observed_scratch_bytes(0, 5, 5) == 0 and L.dnsplat_mc_observed_scratch_bytes(2048, 1024, 1024) == 0
    assert L.dnsplat_mc_scratch_bytes(512, 512, 512) == 512 ** 3 // 64 * 40 + 2 * 2048 * 16          # the unmasked layout is what it was


def _fake():
    buf = (ctypes.c_double * 64)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _tsdf_args(p):
    from dn_splatter_amd import _lib

    a = _lib.TsdfArgs()
    a.nx, a.ny, a.nz, a.C, a.width, a.height = 2, 3, 4, 1, 4, 4
    a.voxel, a.sdf_trunc, a.depth_trunc = 0.1, 0.03, 20.0
    a.fx = a.fy = 1.0
    for name in ("tsdf", "weight", "color", "w2c", "depth", "rgb", "ray_scale"):
        setattr(a, name, p)
    return a


def test_integrate_refuses_null_and_invalid_arguments_without_a_launch(L):
    assert L.dnsplat_tsdf_integrate(None, None) == -1
    buf, p = _fake()
    for missing in ("tsdf", "weight", "w2c", "depth", "ray_scale", "color", "rgb"):       # color without rgb, rgb without color
        a = _tsdf_args(p)
        setattr(a, missing, None)
        assert L.dnsplat_tsdf_integrate(ctypes.byref(a), None) == -1, missing
    for field in ("nx", "ny", "nz", "C", "width", "height"):
        for bad in (0, -1):
            a = _tsdf_args(p)
            setattr(a, field, bad)
            assert L.dnsplat_tsdf_integrate(ctypes.byref(a), None) == -1, field
    a = _tsdf_args(p)
    a.nx, a.ny, a.nz = 2048, 1024, 1024                                          # 2^31 voxels
    assert L.dnsplat_tsdf_integrate(ctypes.byref(a), None) == -1
    a.nx, a.ny, a.nz = 65536, 65536, 65536
    assert L.dnsplat_tsdf_integrate(ctypes.byref(a), None) == -1
    for field in ("voxel", "sdf_trunc", "depth_trunc"):
        for bad in (0.0, -1.0, float("nan")):
            a = _tsdf_args(p)
            setattr(a, field, bad)
            assert L.dnsplat_tsdf_integrate(ctypes.byref(a), None) == -1, field
    a = _tsdf_args(p)
    a.width, a.height = 65536, 32768                                             # 2^31 pixels
    assert L.dnsplat_tsdf_integrate(ctypes.byref(a), None) == -4
    assert not any(buf)


def test_vertex_colours_refuse_null_and_invalid_arguments_without_a_launch(L):
    buf, p = _fake()
    f = L.dnsplat_tsdf_vertex_colors
    assert f(None, 5, 6, 7, p, 4, p, None) == -1 and f(p, 5, 6, 7, None, 4, p, None) == -1 and f(p, 5, 6, 7, p, 4, None, None) == -1
    assert f(p, 5, 6, 7, p, -1, p, None) == -1
    for shape in ((1, 6, 7), (5, 1, 7), (5, 6, 1), (0, 6, 7), (2048, 1024, 1024)):
        assert f(p, *shape, p, 4, p, None) == -1, shape
    assert f(p, 5, 6, 7, p, 2 ** 31, p, None) == -4
    assert f(p, 5, 6, 7, None, 0, None, None) == 0                               # no vertex: nothing to do, nothing launched
    assert not any(buf)


def test_observed_marching_cubes_refuse_null_and_invalid_arguments_without_a_launch(L):
    from dn_splatter_amd import _lib

    buf, p = _fake()
    for fn in (L.dnsplat_mc_count_observed, L.dnsplat_mc_emit_observed):
        assert fn(None, None) == -1
        a = _lib.McObservedArgs()
        a.mc.nx, a.mc.ny, a.mc.nz = 5, 6, 7
        a.mc.scratch_bytes = L.dnsplat_mc_observed_scratch_bytes(5, 6, 7)
        a.mc.volume = a.mc.scratch = a.mc.counts = a.mc.status = p
        assert fn(ctypes.byref(a), None) == -1                                   # no weight
        a.weight = p
        for missing in ("volume", "scratch", "counts"):
            setattr(a.mc, missing, None)
            assert fn(ctypes.byref(a), None) == -1, missing
            setattr(a.mc, missing, p)
        a.mc.nx = 0
        assert fn(ctypes.byref(a), None) == -1
        a.mc.nx = 5
        a.mc.scratch_bytes = L.dnsplat_mc_scratch_bytes(5, 6, 7)                 # the unmasked size lacks the plane
        assert fn(ctypes.byref(a), None) == -2
        a.mc.scratch_bytes = L.dnsplat_mc_observed_scratch_bytes(5, 6, 7) - 1
        assert fn(ctypes.byref(a), None) == -2
    a.mc.scratch_bytes += 1
    a.mc.status = None
    assert L.dnsplat_mc_emit_observed(ctypes.byref(a), None) == -1
    a.mc.status = p
    a.mc.cap_v = -1
    assert L.dnsplat_mc_emit_observed(ctypes.byref(a), None) == -1
    a.mc.cap_v, a.mc.cap_t = 1, 0                                                # a capacity without its buffer
    assert L.dnsplat_mc_emit_observed(ctypes.byref(a), None) == -1
    assert not any(buf)


def test_python_surface_refuses_cpu_volumes(dns):
    import torch

    with pytest.raises(dns.DnsplatError, match="no CPU fallback"):
        dns.TSDFVolume((0, 0, 0), 0.1, (4, 4, 4), device="cpu")
    with pytest.raises(ValueError, match=str(2 ** 31 - 1)):
        dns.TSDFVolume.from_bounds((0, 0, 0), (13, 13, 13), 0.01)
    with pytest.raises(dns.DnsplatError, match="no CPU fallback"):
        dns.marching_cubes(torch.zeros(3, 3, 3), 0.0, weight=torch.ones(3, 3, 3))
