"""The point-cloud normals, the parts of their C ABI that need no GPU: the exports, the header's text, the layout of the argument struct
as gcc sees include/dnsplat.h against its ctypes mirror, the scratch query against its stated formula, the argument checks, which return
before anything touches a device (the pointers here are host memory that nothing may touch), and the Python surface's refusals and
defaults."""
import ctypes
import inspect
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dnsplat.h")
SYMBOLS = ("dnsplat_cloud_normals_scratch_bytes", "dnsplat_cloud_normals")
INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def L(dns):
    dns.build_library()
    return dns.load_library()


def test_symbols_are_exported_and_declared_and_the_abi_stays(dns, L):
    from dn_splatter_amd import _lib, normals, torch_normals

    raw = ctypes.CDLL(str(dns.build_library()))
    text = open(HEADER).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS, name
        assert name + "(" in text, name
        assert name in integration, name
    assert "} dnsplat_cloud_normals_args;" in text
    assert L.dnsplat_abi_version() == 15 and _lib.ABI_VERSION == 15              # additive: found by symbol, the version stays
    section = text[text.index("point-cloud normals (added after ABI 15"):text.index("} dnsplat_cloud_normals_args;")]
    for phrase in ("PARITY UNPINNED AGAINST Open3D", "d2 < radius radius", "a strict test", "fma(dz, dz, fma(dy, dy, dx dx))",
                   "equal d2 go to the lowest index", "NOT Open3D's cumulants", "ONE FIXED TREE", "o = 32, 16, 8, 4, 2, 1",
                   "8 cyclic Jacobi sweeps", "(0, 0, 1), Open3D's fallback", "the lowest axis on equal magnitudes",
                   "a product of exactly 0\n *              does not flip", "Out of scope: a pure radius search"):
        assert phrase in section, phrase
    assert "Out of scope: estimate_normals" not in text                          # it left the filters' list
    for name in ("normals", "torch_normals", "estimate_normals", "points3D_normals", "depth_normals", "normal_consistency_mask"):
        assert hasattr(dns, name) and name in dns.__all__, name
    assert "#define DNSPLAT_NORMALS_MAX_K %d\n" % normals.MAX_K in text and normals.MAX_K == torch_normals.MAX_K == 256
    assert "#define DNSPLAT_NORMALS_STATUS_INTERNAL %d\n" % normals.STATUS_INTERNAL in text
    assert "-ffp-contract=off -c normals.hip" in open(os.path.join(ROOT, "dn-splatter_amd", "csrc", "build.sh")).read()
    for line in ("normal_nerfstudio.py:85-101", "depth_to_normal.py:150-213", "depth_normal_consistency.py:171-221", "dn_model.py:196-215"):
        assert line in integration, line
    for name in ("normals.hip", "normals_solve.h"):
        source = open(os.path.join(ROOT, "dn-splatter_amd", "csrc", name)).read()
        assert "asm" not in source and "atomicAdd" not in source                 # no inline assembly, no sum by atomics
    solve = open(os.path.join(ROOT, "dn-splatter_amd", "csrc", "normals_solve.h")).read()
    assert "constexpr int NM_SWEEPS = %d;" % torch_normals.SWEEPS in solve
    kernel = open(os.path.join(ROOT, "dn-splatter_amd", "csrc", "normals.hip")).read()
    assert "constexpr int NM_MIN_KP = DNS_WAVE;" in kernel and torch_normals.MIN_KP == torch_normals.WAVE == 64
    assert [torch_normals.buffer_capacity(k) for k in (3, 64, 65, 128, 129, 256)] == [128, 128, 256, 256, 512, 512]


def test_struct_layout_matches_the_c_compiler(dns, tmp_path):
    from dn_splatter_amd import _lib

    cname, cls = "dnsplat_cloud_normals_args", _lib.CloudNormalsArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){',
             f'printf("{cname} %zu\\n", sizeof({cname}));']
    for fname, _ in cls._fields_:
        lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got[cname]) == ctypes.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, fname


def test_scratch_query_is_host_only_and_states_its_bytes(L):
    for N, knn in ((1, 3), (2, 30), (257, 200), (3_000_000, 256), (INT_MAX, 3)):
        assert L.dnsplat_cloud_normals_scratch_bytes(N, knn) == 16, (N, knn)      # int32 [4], whatever the size
    for N, knn in ((0, 30), (-1, 30), (5, 2), (5, 0), (5, -1), (5, 257)):
        assert L.dnsplat_cloud_normals_scratch_bytes(N, knn) == 0, (N, knn)


def _fake():
    buf = (ctypes.c_double * 512)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _args(L, p, N=9, knn=30):
    from dn_splatter_amd import _lib

    a = _lib.CloudNormalsArgs()
    a.N, a.knn, a.radius, a.orient = N, knn, 0.1, 1
    a.toward[0], a.toward[1], a.toward[2] = 0.5, -1.0, 2.0
    a.scratch_bytes = L.dnsplat_cloud_normals_scratch_bytes(N, 30)
    for name in ("points", "index", "scratch", "normals", "covariance", "neighbors", "count", "status"):
        setattr(a, name, p)
    return a


def test_the_call_refuses_null_and_invalid_arguments_without_touching_a_device(L):
    buf, p = _fake()
    fn = L.dnsplat_cloud_normals
    assert fn(None, None) == -1
    for missing in ("points", "index", "scratch", "normals", "status"):
        a = _args(L, p)
        setattr(a, missing, None)
        assert fn(ctypes.byref(a), None) == -1, missing
    for field, values in (("N", (0, -1)), ("radius", (float("nan"),)), ("orient", (2, -1))):
        for bad in values:
            a = _args(L, p)
            setattr(a, field, bad)
            assert fn(ctypes.byref(a), None) == -1, (field, bad)
    a = _args(L, p)
    a.toward[1] = float("nan")
    assert fn(ctypes.byref(a), None) == -1
    for knn in (2, 257, 0, -3):                                                   # 3 <= knn <= DNSPLAT_NORMALS_MAX_K
        a = _args(L, p, knn=knn)
        assert fn(ctypes.byref(a), None) == -4, knn
    for knn in (3, 256):                                                          # the limits pass; the next check answers, still on the host
        a = _args(L, p, knn=knn)
        a.scratch_bytes -= 1
        assert fn(ctypes.byref(a), None) == -2, knn
    a = _args(L, p)
    a.scratch = ctypes.c_void_p(p.value + 4)                                      # 8-byte alignment
    assert fn(ctypes.byref(a), None) == -2
    assert not any(buf)


def test_python_surface_refuses_cpu_tensors_and_bad_arguments(dns):
    import numpy as np
    import torch

    points = torch.zeros(8, 3)
    with pytest.raises(dns.DnsplatError, match="no CPU fallback"):
        dns.estimate_normals(points)
    with pytest.raises(dns.DnsplatError, match="no CPU fallback"):
        dns.points3D_normals(points)
    with pytest.raises(dns.DnsplatError, match="no CPU fallback"):
        dns.depth_normals(torch.ones(4, 4), 1.0, 1.0, 2.0, 2.0, np.eye(4))
    with pytest.raises(TypeError):
        dns.estimate_normals(np.zeros((8, 3)))
    for knn in (2, 257):
        with pytest.raises(ValueError, match=r"knn must lie in \[3, 256\]"):
            dns.estimate_normals(points, knn=knn)
    with pytest.raises(ValueError, match="radius is nan"):
        dns.estimate_normals(points, radius=float("nan"))
    with pytest.raises(ValueError, match="orient_toward"):
        dns.estimate_normals(points, orient_toward=(0.0, float("nan"), 1.0))
    with pytest.raises(ValueError, match="orient_toward"):
        dns.estimate_normals(points, orient_toward=(0.0, 1.0))
    assert dns.normals._toward(torch.tensor([1.0, 2.0, 3.0])) == (1.0, 2.0, 3.0)  # a host tensor: nothing is read from a device
    sig = inspect.signature(dns.estimate_normals).parameters
    assert list(sig) == ["points", "knn", "radius", "orient_toward", "index", "return_covariance", "return_neighbors"]
    assert [sig[k].default for k in ("knn", "radius", "orient_toward", "index", "return_covariance", "return_neighbors")] == \
        [30, None, None, None, False, False]
    sig = inspect.signature(dns.points3D_normals).parameters
    assert [sig[k].default for k in ("transform_matrix", "knn", "radius")] == [None, 30, 0.1]
    assert inspect.signature(dns.depth_normals).parameters["knn"].default == 200
    assert inspect.signature(dns.normal_consistency_mask).parameters["degrees"].default == 10.0
    assert dns.normals.check_arguments(30, 0.0) == (30, None) and dns.normals.check_arguments(30, float("inf")) == (30, None)
