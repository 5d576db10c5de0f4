"""The point-cloud filters, the parts of their C ABI that need no GPU: the exports, the layout of the two argument structs as gcc sees
include/dnsplat.h against their ctypes mirrors, the scratch queries against the layout arithmetic, and the argument checks, which return
before anything touches a device (the pointers here are host memory that nothing may touch)."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dnsplat.h")
SYMBOLS = ("dnsplat_cloud_outlier_scratch_bytes", "dnsplat_cloud_neighbor_mean", "dnsplat_cloud_outlier_stats", "dnsplat_cloud_outlier_count",
           "dnsplat_cloud_outlier_emit", "dnsplat_voxel_scratch_bytes", "dnsplat_voxel_count", "dnsplat_voxel_emit")
MAX_VOXEL_N = (2 ** 31 - 1) // 2


@pytest.fixture(scope="module")
def L(dns):
    dns.build_library()
    return dns.load_library()


def test_symbols_are_exported_and_declared_and_the_abi_stays(dns, L):
    from dn_splatter_amd import _lib, cloud_filter, torch_cloud_filter

    raw = ctypes.CDLL(str(dns.build_library()))
    text = open(HEADER).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS, name
        assert name + "(" in text, name
        assert name in integration, name
    for struct in ("dnsplat_cloud_outlier_args", "dnsplat_voxel_args"):
        assert "} " + struct + ";" in text
    assert L.dnsplat_abi_version() == 15 and _lib.ABI_VERSION == 15              # additive: found by symbol, the version stays
    assert text.count("PARITY UNPINNED AGAINST Open3D") >= 3                     # the TSDF section's, the cluster filter's, and this one's
    for name in ("cloud_filter", "torch_cloud_filter", "remove_statistical_outlier", "voxel_down_sample"):
        assert hasattr(dns, name) and name in dns.__all__
    assert "#define DNSPLAT_CLOUD_OUTLIER_STATS_BYTES %d\n" % (8 * cloud_filter.STATS_WORDS) in text
    for name in ("INTERNAL", "NONFINITE", "EXTENT", "ATTRIBUTE"):
        assert "#define DNSPLAT_VOXEL_STATUS_%s %d\n" % (name, getattr(cloud_filter, "STATUS_" + name)) in text
    assert "#define DNSPLAT_KNN_MAX_K %d\n" % torch_cloud_filter.MAX_K in text
    assert cloud_filter.MAX_VOXEL_POINTS == MAX_VOXEL_N


def test_struct_layouts_match_the_c_compiler(dns, tmp_path):
    from dn_splatter_amd import _lib

    structs = {"dnsplat_cloud_outlier_args": _lib.CloudOutlierArgs, "dnsplat_voxel_args": _lib.VoxelArgs}
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
    for N in (1, 20, 256, 257, 66_000, 2_000_000, 2 ** 31 - 1):
        # two partials of 16 bytes and one count per block of 256 points
        assert L.dnsplat_cloud_outlier_scratch_bytes(N) == blocks(N) * 36, N
    for N in (1, 257, 66_000, 2_000_000, MAX_VOXEL_N):
        for n_attr in (0, 1, 2):
            # lo, a table of 2 N slots of 8 + 4 bytes, a row of 4 + 3 n_attr int64 sums and the slot per point, a count per block, 256 minima
            assert L.dnsplat_voxel_scratch_bytes(N, n_attr) == 32 + 2 * N * 12 + N * (8 * (4 + 3 * n_attr) + 4) + blocks(N) * 4 + 256 * 12, (N, n_attr)
    for N in (0, -1):
        assert L.dnsplat_cloud_outlier_scratch_bytes(N) == 0 and L.dnsplat_voxel_scratch_bytes(N, 0) == 0
    assert L.dnsplat_voxel_scratch_bytes(MAX_VOXEL_N + 1, 0) == 0                # 2 N leaves the table's int32 index
    assert L.dnsplat_voxel_scratch_bytes(5, 3) == 0 and L.dnsplat_voxel_scratch_bytes(5, -1) == 0


def _fake():
    buf = (ctypes.c_double * 64)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _outlier_args(L, p, N=300):
    from dn_splatter_amd import _lib

    a = _lib.CloudOutlierArgs()
    a.N, a.nb_neighbors, a.std_ratio = N, 20, 2.0
    a.scratch_bytes = L.dnsplat_cloud_outlier_scratch_bytes(N)
    for name in ("points", "index", "scratch", "avg", "stats", "ind"):
        setattr(a, name, p)
    a.capacity = 4
    return a


def _voxel_args(L, p, N=300):
    from dn_splatter_amd import _lib

    a = _lib.VoxelArgs()
    a.N, a.voxel_size = N, 0.05
    a.scratch_bytes = L.dnsplat_voxel_scratch_bytes(N, 2)
    for name in ("points", "normals", "colors", "scratch", "counts", "voxel_of", "out_points", "out_normals", "out_colors", "out_counts"):
        setattr(a, name, p)
    a.cap_v = 4
    return a


def test_outlier_calls_refuse_null_and_invalid_arguments_without_touching_a_device(L):
    buf, p = _fake()
    fns = {"mean": L.dnsplat_cloud_neighbor_mean, "stats": L.dnsplat_cloud_outlier_stats, "count": L.dnsplat_cloud_outlier_count,
           "emit": L.dnsplat_cloud_outlier_emit}
    required = {"mean": ("points", "index", "avg"), "stats": ("scratch", "avg", "stats"), "count": ("scratch", "avg", "stats"),
                "emit": ("scratch", "avg", "stats", "ind")}
    for which, fn in fns.items():
        assert fn(None, None) == -1
        for missing in required[which]:
            a = _outlier_args(L, p)
            setattr(a, missing, None)
            assert fn(ctypes.byref(a), None) == -1, (which, missing)
        for bad in (0, -1):
            a = _outlier_args(L, p)
            a.N = bad
            assert fn(ctypes.byref(a), None) == -1, which
        if which != "mean":                                                       # the search needs no scratch
            a = _outlier_args(L, p)
            a.scratch_bytes -= 1
            assert fn(ctypes.byref(a), None) == -2, which
            a = _outlier_args(L, p)
            a.scratch = ctypes.c_void_p(p.value + 4)                             # 8-byte alignment
            assert fn(ctypes.byref(a), None) == -2, which
    for bad, code in ((0, -1), (-3, -1), (33, -4)):                              # widening DNSPLAT_KNN_MAX_K is out of scope
        a = _outlier_args(L, p)
        a.nb_neighbors = bad
        assert L.dnsplat_cloud_neighbor_mean(ctypes.byref(a), None) == code, bad
    a = _outlier_args(L, p)
    a.std_ratio = float("nan")
    assert L.dnsplat_cloud_outlier_stats(ctypes.byref(a), None) == -1
    a = _outlier_args(L, p)
    a.capacity = -1
    assert L.dnsplat_cloud_outlier_emit(ctypes.byref(a), None) == -1
    a = _outlier_args(L, p)
    a.capacity, a.ind = 0, None                                                   # nothing to write: no launch
    assert L.dnsplat_cloud_outlier_emit(ctypes.byref(a), None) == 0
    assert not any(buf)


def test_voxel_calls_refuse_null_and_invalid_arguments_without_touching_a_device(L):
    buf, p = _fake()
    for fn in (L.dnsplat_voxel_count, L.dnsplat_voxel_emit):
        assert fn(None, None) == -1
        for missing in ("points", "scratch", "counts", "voxel_of"):
            a = _voxel_args(L, p)
            setattr(a, missing, None)
            assert fn(ctypes.byref(a), None) == -1, missing
        for bad in (0, -1):
            a = _voxel_args(L, p)
            a.N = bad
            assert fn(ctypes.byref(a), None) == -1
        for bad in (0.0, -0.05, float("inf"), float("nan")):
            a = _voxel_args(L, p)
            a.voxel_size = bad
            assert fn(ctypes.byref(a), None) == -1, bad
        a = _voxel_args(L, p)
        a.N = MAX_VOXEL_N + 1
        a.scratch_bytes = 2 ** 62
        assert fn(ctypes.byref(a), None) == -4
        a = _voxel_args(L, p)
        a.scratch_bytes -= 1
        assert fn(ctypes.byref(a), None) == -2
        a = _voxel_args(L, p)
        a.normals = None                                                          # one attribute array: a shorter row, the same scratch is enough
        a.scratch_bytes = L.dnsplat_voxel_scratch_bytes(a.N, 1) - 1
        assert fn(ctypes.byref(a), None) == -2
        a = _voxel_args(L, p)
        a.scratch = ctypes.c_void_p(p.value + 4)
        assert fn(ctypes.byref(a), None) == -2
    emit = L.dnsplat_voxel_emit
    a = _voxel_args(L, p)
    a.cap_v = -1
    assert emit(ctypes.byref(a), None) == -1
    for buffer in ("out_points", "out_normals", "out_colors"):                    # a capacity without the buffer of an array that was given
        a = _voxel_args(L, p)
        setattr(a, buffer, None)
        assert emit(ctypes.byref(a), None) == -1, buffer
    a = _voxel_args(L, p)
    a.cap_v = 0
    assert emit(ctypes.byref(a), None) == 0                                       # nothing to write: no launch
    assert not any(buf)


def test_python_surface_refuses_cpu_tensors_and_bad_arguments(dns):
    import torch

    points = torch.zeros(30, 3)
    with pytest.raises(dns.DnsplatError, match="no CPU fallback"):
        dns.remove_statistical_outlier(points)
    with pytest.raises(dns.DnsplatError, match="no CPU fallback"):
        dns.voxel_down_sample(points, 0.1)
    for bad in (0, 33, -1):
        with pytest.raises(ValueError, match="nb_neighbors"):
            dns.remove_statistical_outlier(points, nb_neighbors=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel_size"):
            dns.voxel_down_sample(points, bad)
    with pytest.raises(TypeError):
        dns.voxel_down_sample([[0.0, 0.0, 0.0]], 0.1)
    import inspect

    from dn_splatter_amd import export, geometry, levelset

    for fn in (export.OrientedPointCloud.finish, export.export_oriented_points, levelset.LevelSetCloud.finish, levelset.export_level_set_points):
        sig = inspect.signature(fn).parameters                                   # the new keywords default to what was
        assert sig["outlier_removal"].default is False and sig["std_ratio"].default == 2.0, fn
    assert inspect.signature(geometry.calculate_accuracy).parameters["down_sample_voxel"].default is None
    assert geometry.PDMetrics().down_sample_voxel is None and geometry.PDMetrics(down_sample_voxel=0.01).down_sample_voxel == 0.01
