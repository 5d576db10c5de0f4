"""The mesh alignment, the parts of its C ABI that need no GPU: the exports, the layout of the argument struct as gcc sees
include/dnsplat.h against its ctypes mirror, the scratch query against its stated formula, and the argument checks, which return before
anything touches a device (the pointers here are host memory that nothing may touch)."""
import ctypes
import inspect
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dnsplat.h")
SYMBOLS = ("dnsplat_icp_scratch_bytes", "dnsplat_icp_begin", "dnsplat_icp_iterate", "dnsplat_icp_run", "dnsplat_transform_points",
           "dnsplat_knn_points")
IDENTITY = (ctypes.c_double * 16)(*[1.0 if k % 5 == 0 else 0.0 for k in range(16)])


@pytest.fixture(scope="module")
def L(dns):
    dns.build_library()
    return dns.load_library()


def test_symbols_are_exported_and_declared_and_the_abi_stays(dns, L):
    from dn_splatter_amd import _lib, icp, torch_icp

    raw = ctypes.CDLL(str(dns.build_library()))
    text = open(HEADER).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS, name
        assert name + "(" in text, name
        assert name in integration, name
    assert "} dnsplat_icp_args;" in text
    assert L.dnsplat_abi_version() == 15 and _lib.ABI_VERSION == 15              # additive: found by symbol, the version stays
    assert text.count("PARITY UNPINNED AGAINST Open3D") >= 4                     # the three sections before, and this one's
    for name in ("icp", "torch_icp", "registration_icp", "get_align_transformation", "transform_points", "transform_mesh", "ICPResult"):
        assert hasattr(dns, name) and name in dns.__all__, name
    assert "#define DNSPLAT_ICP_STATE_BYTES %d\n" % (8 * icp.STATE_WORDS) in text
    assert "#define DNSPLAT_ICP_STATUS_NO_CORRESPONDENCE %d\n" % torch_icp.STATUS_NO_CORRESPONDENCE in text
    assert "#define DNSPLAT_ICP_STATUS_DEGENERATE %d\n" % torch_icp.STATUS_DEGENERATE in text
    assert icp.STATUS_NO_CORRESPONDENCE == 1 and icp.STATUS_DEGENERATE == 2
    source = open(os.path.join(ROOT, "dn-splatter_amd", "csrc", "icp_solve.h")).read()
    assert "ICP_SWEEPS = %d;" % torch_icp.SWEEPS in source                        # the restatement sweeps as often as the kernel
    assert "-ffp-contract=off -c icp.hip" in open(os.path.join(ROOT, "dn-splatter_amd", "csrc", "build.sh")).read()
    assert "eval_mesh_vis_cull.py:269-287" in integration and ":427-431" in integration


def test_struct_layout_matches_the_c_compiler(dns, tmp_path):
    from dn_splatter_amd import _lib

    cname, cls = "dnsplat_icp_args", _lib.IcpArgs
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
    for M in (1, 255, 256, 257, 3000, 66_000, 2_000_000, 2 ** 31 - 1):
        assert L.dnsplat_icp_scratch_bytes(M) == 136 * ((M + 255) // 256), M      # n and 16 double sums per workgroup of 256 rows
    for M in (0, -1, 2 ** 31):
        assert L.dnsplat_icp_scratch_bytes(M) == 0, M


def _fake():
    buf = (ctypes.c_double * 64)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _args(L, p, M=300):
    from dn_splatter_amd import _lib

    a = _lib.IcpArgs()
    a.M, a.N, a.max_dist, a.relative_fitness, a.relative_rmse, a.max_iteration = M, 200, 0.1, 1e-6, 1e-6, 30
    a.scratch_bytes = L.dnsplat_icp_scratch_bytes(M)
    for name in ("source", "target", "index", "state", "trace", "idx", "dist2", "scratch"):
        setattr(a, name, p)
    return a


def test_calls_refuse_null_and_invalid_arguments_without_touching_a_device(L):
    buf, p = _fake()
    calls = {"begin": lambda a: L.dnsplat_icp_begin(a, IDENTITY, None), "iterate": lambda a: L.dnsplat_icp_iterate(a, None),
             "run": lambda a: L.dnsplat_icp_run(a, IDENTITY, None)}
    for which, fn in calls.items():
        assert fn(None) == -1, which
        for missing in ("source", "target", "index", "state", "scratch"):
            a = _args(L, p)
            setattr(a, missing, None)
            assert fn(ctypes.byref(a)) == -1, (which, missing)
        for field, values in (("M", (0, -1)), ("N", (0, -5)), ("max_dist", (0.0, -0.1, float("inf"), float("nan"))), ("max_iteration", (-1,)),
                              ("relative_fitness", (float("nan"),)), ("relative_rmse", (float("nan"),))):
            for bad in values:
                a = _args(L, p)
                setattr(a, field, bad)
                assert fn(ctypes.byref(a)) == -1, (which, field, bad)
        a = _args(L, p)
        a.M, a.scratch_bytes = 2 ** 31, 2 ** 62
        assert fn(ctypes.byref(a)) == -4, which
        a = _args(L, p)
        a.scratch_bytes -= 1
        assert fn(ctypes.byref(a)) == -2, which
        for field in ("scratch", "state"):                                        # 8-byte alignment
            a = _args(L, p)
            setattr(a, field, ctypes.c_void_p(p.value + 4))
            assert fn(ctypes.byref(a)) == -2, (which, field)
    for k in (0, 7, 15):                                                          # a non-finite init never reaches a launch
        for bad in (float("nan"), float("inf"), float("-inf")):
            init = (ctypes.c_double * 16)(*IDENTITY)
            init[k] = bad
            a = _args(L, p)
            assert L.dnsplat_icp_begin(ctypes.byref(a), init, None) == -1 and L.dnsplat_icp_run(ctypes.byref(a), init, None) == -1
    tp = L.dnsplat_transform_points
    assert tp(5, None, p, p, 0, None) == -1 and tp(5, p, None, p, 0, None) == -1 and tp(5, p, p, None, 0, None) == -1
    assert tp(-1, p, p, p, 0, None) == -1 and tp(2 ** 31, p, p, p, 0, None) == -4
    assert tp(0, None, p, None, 1, None) == 0                                     # nothing to move: no launch
    kp = L.dnsplat_knn_points
    assert kp(0, p, p, None) == -1 and kp(5, None, p, None) == -1 and kp(5, p, None, None) == -1
    assert not any(buf)


def test_python_surface_refuses_cpu_tensors_and_bad_arguments(dns):
    import numpy as np
    import torch

    src, tgt = torch.zeros(30, 3), torch.ones(40, 3)
    with pytest.raises(dns.DnsplatError, match="no CPU fallback"):
        dns.registration_icp(src, tgt, 0.1)
    with pytest.raises(dns.DnsplatError, match="no CPU fallback"):
        dns.transform_points(src, np.eye(4))
    with pytest.raises(dns.DnsplatError, match="no CPU fallback"):
        dns.get_align_transformation((src, None), (tgt, None))
    with pytest.raises(dns.DnsplatError, match="no CPU fallback"):
        dns.transform_mesh((src, None), np.eye(4))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_correspondence_distance"):
            dns.registration_icp(src, tgt, bad)
    with pytest.raises(ValueError, match="max_iteration"):
        dns.registration_icp(src, tgt, 0.1, max_iteration=-1)
    with pytest.raises(ValueError, match="nan"):
        dns.registration_icp(src, tgt, 0.1, relative_rmse=float("nan"))
    with pytest.raises(TypeError):
        dns.registration_icp([[0.0, 0.0, 0.0]], tgt, 0.1)
    sig = inspect.signature(dns.registration_icp).parameters
    assert [sig[k].default for k in ("init", "relative_fitness", "relative_rmse", "max_iteration", "index", "return_trace")] == \
        [None, 1e-6, 1e-6, 30, None, False]
    assert inspect.signature(dns.get_align_transformation).parameters["threshold"].default == 0.1
    sig = inspect.signature(dns.culled_mesh_metrics).parameters                  # the new keywords default to what was
    assert sig["align"].default is False and sig["align_threshold"].default == 0.1
