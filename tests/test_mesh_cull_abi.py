"""The mesh visibility culling, the parts of its C ABI that need no GPU: the exports, the layout of the three argument structs as gcc
sees include/dnsplat.h against their ctypes mirrors, the scratch queries, and the argument checks, which return before any launch."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dnsplat.h")
SYMBOLS = ("dnsplat_mesh_depth_scratch_bytes", "dnsplat_mesh_depth", "dnsplat_mesh_visibility", "dnsplat_mesh_cut_scratch_bytes",
           "dnsplat_mesh_cut_count", "dnsplat_mesh_cut_emit")


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
    for struct in ("dnsplat_mesh_depth_args", "dnsplat_mesh_visibility_args", "dnsplat_mesh_cut_args"):
        assert "} " + struct + ";" in text
    assert L.dnsplat_abi_version() == 15 and _lib.ABI_VERSION == 15              # additive: found by symbol, the version stays


def test_struct_layouts_match_the_c_compiler(dns, tmp_path):
    from dn_splatter_amd import _lib

    structs = {"dnsplat_mesh_depth_args": _lib.MeshDepthArgs, "dnsplat_mesh_visibility_args": _lib.MeshVisibilityArgs,
               "dnsplat_mesh_cut_args": _lib.MeshCutArgs}
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


def test_scratch_queries_are_host_functions(L):
    assert L.dnsplat_mesh_depth_scratch_bytes(1920, 1080) == (1920 + 1080) * 8
    assert L.dnsplat_mesh_depth_scratch_bytes(0, 5) == 0 and L.dnsplat_mesh_depth_scratch_bytes(65536, 32768) == 0
    small, big = L.dnsplat_mesh_cut_scratch_bytes(1, 1), L.dnsplat_mesh_cut_scratch_bytes(4_490_000, 8_960_000)
    assert 0 < small < big and big >= 4 * 4_490_000 + 8_960_000                   # a mark per vertex, a flag per triangle
    assert L.dnsplat_mesh_cut_scratch_bytes(0, 1) == 0 and L.dnsplat_mesh_cut_scratch_bytes(1, -1) == 0


def _fake():
    buf = (ctypes.c_double * 64)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_depth_refuses_null_and_invalid_arguments_without_a_launch(L):
    from dn_splatter_amd import _lib

    assert L.dnsplat_mesh_depth(None, None) == -1
    buf, p = _fake()
    a = _lib.MeshDepthArgs()
    a.V, a.T, a.C, a.width, a.height = 3, 1, 1, 4, 4
    a.fx = a.fy = 1.0
    a.znear, a.zfar = 0.01, 10.0
    pointers = ("vertices", "triangles", "w2c", "depth", "scratch")
    for missing in pointers:                                                      # each pointer in turn, every other one set
        for name in pointers:
            setattr(a, name, None if name == missing else p)
        assert L.dnsplat_mesh_depth(ctypes.byref(a), None) == -1, missing
    for name in pointers:
        setattr(a, name, p)
    for field, bad in (("V", 0), ("T", 0), ("C", 0), ("width", 0), ("height", -1), ("fx", 0.0), ("fy", float("nan")),
                       ("znear", 0.0), ("znear", 11.0), ("zfar", float("inf")), ("znear", float("nan"))):
        keep = getattr(a, field)
        setattr(a, field, bad)
        assert L.dnsplat_mesh_depth(ctypes.byref(a), None) == -1, field
        setattr(a, field, keep)
    a.C = 65536
    assert L.dnsplat_mesh_depth(ctypes.byref(a), None) == -4
    a.C, a.width, a.height = 1, 65536, 32768
    assert L.dnsplat_mesh_depth(ctypes.byref(a), None) == -4
    a.width, a.height = 4, 4
    a.scratch = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    assert L.dnsplat_mesh_depth(ctypes.byref(a), None) == -2                      # the rays are doubles


def test_visibility_refuses_null_and_invalid_arguments_without_a_launch(L):
    from dn_splatter_amd import _lib

    assert L.dnsplat_mesh_visibility(None, None) == -1
    buf, p = _fake()
    a = _lib.MeshVisibilityArgs()
    a.V, a.C, a.width, a.height = 3, 1, 4, 4
    pointers = ("vertices", "w2c", "obs", "invalid")
    for missing in pointers:
        for name in pointers:
            setattr(a, name, None if name == missing else p)
        assert L.dnsplat_mesh_visibility(ctypes.byref(a), None) == -1, missing
    for name in pointers:
        setattr(a, name, p)
    a.remove_occlusion = 1                                                        # the flag without its map
    assert L.dnsplat_mesh_visibility(ctypes.byref(a), None) == -1
    a.remove_occlusion, a.remove_missing_depth = 0, 1
    assert L.dnsplat_mesh_visibility(ctypes.byref(a), None) == -1
    a.remove_missing_depth = 0
    for field in ("V", "C", "width", "height"):
        keep = getattr(a, field)
        setattr(a, field, 0)
        assert L.dnsplat_mesh_visibility(ctypes.byref(a), None) == -1, field
        setattr(a, field, keep)
    a.width, a.height = 65536, 32768
    assert L.dnsplat_mesh_visibility(ctypes.byref(a), None) == -4


def test_cut_refuses_null_and_invalid_arguments_without_a_launch(L):
    from dn_splatter_amd import _lib

    buf, p = _fake()
    for fn in (L.dnsplat_mesh_cut_count, L.dnsplat_mesh_cut_emit):
        assert fn(None, None) == -1
        a = _lib.MeshCutArgs()
        a.V, a.T = 3, 1
        a.scratch_bytes = L.dnsplat_mesh_cut_scratch_bytes(3, 1)
        a.status = p
        pointers = ("vertices", "triangles", "obs", "invalid", "scratch", "counts")
        for missing in pointers:
            for name in pointers:
                setattr(a, name, None if name == missing else p)
            assert fn(ctypes.byref(a), None) == -1, missing
        for name in pointers:
            setattr(a, name, p)
        for field in ("V", "T"):
            setattr(a, field, 0)
            assert fn(ctypes.byref(a), None) == -1, field
            setattr(a, field, 3)
        a.scratch_bytes -= 1
        assert fn(ctypes.byref(a), None) == -2
        a.scratch_bytes += 1
        a.scratch = ctypes.c_void_p(ctypes.addressof(buf) + 2)
        assert fn(ctypes.byref(a), None) == -2
    a.scratch = p
    a.status = None
    assert L.dnsplat_mesh_cut_emit(ctypes.byref(a), None) == -1
    a.status = p
    a.cap_v = -1
    assert L.dnsplat_mesh_cut_emit(ctypes.byref(a), None) == -1
    a.cap_v, a.cap_t = 1, 0                                                       # a capacity without its buffer
    assert L.dnsplat_mesh_cut_emit(ctypes.byref(a), None) == -1
    a.cap_v, a.cap_t = 0, 1
    assert L.dnsplat_mesh_cut_emit(ctypes.byref(a), None) == -1


def test_python_surface_refuses_cpu_tensors(dns):
    import numpy as np
    import torch

    from dn_splatter_amd import DnsplatError, mesh_cull

    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)
    pose, K = np.eye(4)[None], np.eye(3)
    with pytest.raises(DnsplatError, match="no CPU fallback"):
        mesh_cull.render_mesh_depth(v, f, pose, K, 4, 4)
    with pytest.raises(DnsplatError, match="no CPU fallback"):
        mesh_cull.vertex_visibility(v, pose, K, 4, 4, remove_missing_depth=False, remove_occlusion=False)
    with pytest.raises(DnsplatError, match="no CPU fallback"):
        mesh_cull.cull_mesh((v, f), pose, K, 4, 4)
    for name in ("cull_mesh", "culled_mesh_metrics", "cut_mesh", "render_mesh_depth", "vertex_visibility", "mesh_cull", "torch_mesh_cull"):
        assert hasattr(dns, name) and name in dns.__all__
