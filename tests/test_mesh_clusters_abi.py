"""The mesh cluster filter, the parts of its C ABI that need no GPU: the exports, the layout of the two argument structs as gcc sees
include/dnsplat.h against their ctypes mirrors, the scratch queries against the layout arithmetic, and the argument checks, which return
before anything touches a device (the pointers here are host memory that nothing may touch)."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dnsplat.h")
SYMBOLS = ("dnsplat_mesh_clusters_scratch_bytes", "dnsplat_mesh_clusters", "dnsplat_mesh_filter_scratch_bytes", "dnsplat_mesh_filter_count",
           "dnsplat_mesh_filter_emit")
MAX_T = (2 ** 31 - 1) // 4


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
    for struct in ("dnsplat_mesh_clusters_args", "dnsplat_mesh_filter_args"):
        assert "} " + struct + ";" in text
    assert L.dnsplat_abi_version() == 15 and _lib.ABI_VERSION == 15              # additive: found by symbol, the version stays
    assert text.count("PARITY UNPINNED AGAINST Open3D") >= 2                     # the TSDF section's words, and this one's
    for name in ("mesh_clusters", "torch_mesh_clusters", "cluster_connected_triangles", "filter_small_clusters"):
        assert hasattr(dns, name) and name in dns.__all__
    from dn_splatter_amd import mesh_clusters

    assert "#define DNSPLAT_MESH_CLUSTERS_STATUS_INTERNAL %d\n" % mesh_clusters.STATUS_INTERNAL in text


def test_struct_layouts_match_the_c_compiler(dns, tmp_path):
    from dn_splatter_amd import _lib

    structs = {"dnsplat_mesh_clusters_args": _lib.MeshClustersArgs, "dnsplat_mesh_filter_args": _lib.MeshFilterArgs,
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


def test_scratch_queries_are_host_only_and_state_their_bytes(L):
    blocks = lambda n: (n + 255) // 256
    for V, T in ((1, 1), (9, 8), (4800, 9344), (200_000, 70_000), (18_600_000, 37_100_000), (5, MAX_T)):
        # a table of 4 T slots of 8 + 4 bytes (a load of 0.75 with 3 T distinct edges), one counter, three int32 per triangle, one per block
        assert L.dnsplat_mesh_clusters_scratch_bytes(V, T) == 4 * T * 12 + 8 + 3 * T * 4 + blocks(T) * 4, (V, T)
        # three histograms of 2048 bins and the selection's two words, the marks, both arrays of block counts, the keep flags
        assert L.dnsplat_mesh_filter_scratch_bytes(V, T) == (3 * 2048 + 2) * 8 + (V + blocks(T) + blocks(V)) * 4 + T, (V, T)
    for V, T in ((0, 5), (5, 0), (-1, 5), (5, -1)):
        assert L.dnsplat_mesh_clusters_scratch_bytes(V, T) == 0 and L.dnsplat_mesh_filter_scratch_bytes(V, T) == 0
    assert L.dnsplat_mesh_clusters_scratch_bytes(5, MAX_T + 1) == 0              # 4 T leaves the table's int32 index
    assert L.dnsplat_mesh_cut_scratch_bytes(4800, 9344) == (4800 + blocks(9344) + blocks(4800)) * 4 + 9344     # the cut's layout is what it was


def _fake():
    buf = (ctypes.c_double * 64)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _clusters_args(L, p, V=9, T=8):
    from dn_splatter_amd import _lib

    a = _lib.MeshClustersArgs()
    a.V, a.T = V, T
    a.scratch_bytes = L.dnsplat_mesh_clusters_scratch_bytes(V, T)
    for name in ("triangles", "scratch", "labels", "sizes", "counts", "status"):
        setattr(a, name, p)
    return a


def _filter_args(L, p, V=9, T=8):
    from dn_splatter_amd import _lib

    a = _lib.MeshFilterArgs()
    a.V, a.T, a.keep_largest, a.min_triangles = V, T, 50, 50
    a.scratch_bytes = L.dnsplat_mesh_filter_scratch_bytes(V, T)
    for name in ("triangles", "labels", "sizes", "cluster_counts", "scratch", "threshold", "counts", "vertex_index", "out_triangles", "status"):
        setattr(a, name, p)
    a.cap_v, a.cap_t = 4, 4
    return a


def test_clusters_refuse_null_and_invalid_arguments_without_touching_a_device(L):
    assert L.dnsplat_mesh_clusters(None, None) == -1
    buf, p = _fake()
    for missing in ("triangles", "scratch", "labels", "sizes", "counts", "status"):
        a = _clusters_args(L, p)
        setattr(a, missing, None)
        assert L.dnsplat_mesh_clusters(ctypes.byref(a), None) == -1, missing
    for field in ("V", "T"):
        for bad in (0, -1):
            a = _clusters_args(L, p)
            setattr(a, field, bad)
            assert L.dnsplat_mesh_clusters(ctypes.byref(a), None) == -1, field
    a = _clusters_args(L, p)
    a.T = MAX_T + 1
    a.scratch_bytes = 2 ** 62
    assert L.dnsplat_mesh_clusters(ctypes.byref(a), None) == -4
    a = _clusters_args(L, p)
    a.scratch_bytes -= 1
    assert L.dnsplat_mesh_clusters(ctypes.byref(a), None) == -2
    a = _clusters_args(L, p)
    a.scratch = ctypes.c_void_p(p.value + 4)                                     # 8-byte alignment
    assert L.dnsplat_mesh_clusters(ctypes.byref(a), None) == -2
    assert not any(buf)


def test_filter_refuses_null_and_invalid_arguments_without_touching_a_device(L):
    buf, p = _fake()
    for fn in (L.dnsplat_mesh_filter_count, L.dnsplat_mesh_filter_emit):
        assert fn(None, None) == -1
        for missing in ("triangles", "labels", "sizes", "cluster_counts", "scratch", "threshold", "counts"):
            a = _filter_args(L, p)
            setattr(a, missing, None)
            assert fn(ctypes.byref(a), None) == -1, missing
        for field in ("V", "T", "keep_largest", "min_triangles"):
            for bad in (0, -1):
                a = _filter_args(L, p)
                setattr(a, field, bad)
                assert fn(ctypes.byref(a), None) == -1, field
        a = _filter_args(L, p)
        a.scratch_bytes -= 1
        assert fn(ctypes.byref(a), None) == -2
        a = _filter_args(L, p)
        a.scratch = ctypes.c_void_p(p.value + 4)
        assert fn(ctypes.byref(a), None) == -2
    emit = L.dnsplat_mesh_filter_emit
    a = _filter_args(L, p)
    a.status = None
    assert emit(ctypes.byref(a), None) == -1
    for field in ("cap_v", "cap_t"):
        a = _filter_args(L, p)
        setattr(a, field, -1)
        assert emit(ctypes.byref(a), None) == -1, field
    for buffer in ("vertex_index", "out_triangles"):                             # a capacity without its buffer
        a = _filter_args(L, p)
        setattr(a, buffer, None)
        assert emit(ctypes.byref(a), None) == -1, buffer
    assert not any(buf)


def test_python_surface_refuses_cpu_tensors_and_bad_arguments(dns):
    import torch

    triangles = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    with pytest.raises(dns.DnsplatError, match="no CPU fallback"):
        dns.cluster_connected_triangles(triangles, 3)
    with pytest.raises(dns.DnsplatError, match="no CPU fallback"):
        dns.filter_small_clusters((torch.zeros(3, 3), triangles))
    with pytest.raises(ValueError, match="at least 1"):
        dns.filter_small_clusters((torch.zeros(3, 3), triangles), keep_largest=0)
