"""The subdivision of long triangles, the parts of its C ABI that need no GPU: the exports, the header's text, the layout of the
argument struct as gcc sees include/dnsplat.h against its ctypes mirror, the scratch query against its stated formula, the argument
checks, which return before anything touches a device (the pointers here are host memory that nothing may touch), and the Python
surface's refusals and defaults."""
import ctypes
import inspect
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dnsplat.h")
SYMBOLS = ("dnsplat_subdivide_scratch_bytes", "dnsplat_subdivide_count", "dnsplat_subdivide_emit")
INT_MAX = 2 ** 31 - 1
MAX_T = INT_MAX // 4


@pytest.fixture(scope="module")
def L(dns):
    dns.build_library()
    return dns.load_library()


def test_symbols_are_exported_and_declared_and_the_abi_stays(dns, L):
    from dn_splatter_amd import _lib, subdivide

    raw = ctypes.CDLL(str(dns.build_library()))
    text = open(HEADER).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS, name
        assert name + "(" in text, name
        assert name in integration, name
    assert "} dnsplat_subdivide_args;" in text
    assert L.dnsplat_abi_version() == 15 and _lib.ABI_VERSION == 15              # additive: found by symbol, the version stays
    assert "PARITY UNPINNED AGAINST trimesh" in text
    for phrase in ("L = sqrt((dx dx + dy dy) + dz dz)", "(cv[lo] + cv[hi]) / 2", "(a, m0, m2), (m0, b, m1),", "(m2, m1, c), (m0, m1, m2)",
                   "first appearance", "max_iter exceeded", "a nan is not long"):
        assert phrase in text, phrase
    for name in ("subdivide", "torch_subdivide", "subdivide_to_size", "subdivide_mesh"):
        assert hasattr(dns, name) and name in dns.__all__, name
    for bit, value in (("INTERNAL", subdivide.STATUS_INTERNAL), ("INDEX", subdivide.STATUS_INDEX), ("CAPACITY", subdivide.STATUS_CAPACITY)):
        assert "#define DNSPLAT_SUBDIVIDE_STATUS_%s %d\n" % (bit, value) in text
    assert subdivide.MAX_TRIANGLES == MAX_T and subdivide.INT_MAX == INT_MAX
    assert "-ffp-contract=off -c subdivide.hip" in open(os.path.join(ROOT, "dn-splatter_amd", "csrc", "build.sh")).read()
    assert "eval_mesh_vis_cull.py:190-193" in integration
    source = open(os.path.join(ROOT, "dn-splatter_amd", "csrc", "subdivide.hip")).read()
    assert "asm" not in source and "atomicAdd" not in source                     # no inline assembly, no sum by atomics


def test_struct_layout_matches_the_c_compiler(dns, tmp_path):
    from dn_splatter_amd import _lib

    cname, cls = "dnsplat_subdivide_args", _lib.SubdivideArgs
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
    def blocks(n):
        return (n + 255) // 256

    for V, T in ((1, 1), (8, 12), (255, 256), (257, 85), (300, 86), (66_000, 131_073), (3_000_000, 6_000_001), (INT_MAX, MAX_T)):
        want = 64 * T + 4 * V + 4 * (2 * blocks(T) + blocks(V) + blocks(3 * T))
        assert L.dnsplat_subdivide_scratch_bytes(V, T) == want, (V, T)
    for V, T in ((0, 5), (5, 0), (-1, 5), (5, -1), (5, MAX_T + 1)):
        assert L.dnsplat_subdivide_scratch_bytes(V, T) == 0, (V, T)


def _fake():
    buf = (ctypes.c_double * 512)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _args(L, p, V=9, T=5, emit=False):
    from dn_splatter_amd import _lib

    a = _lib.SubdivideArgs()
    a.V, a.T, a.max_edge = V, T, 0.5
    a.scratch_bytes = L.dnsplat_subdivide_scratch_bytes(V, T)
    for name in ("vertices", "triangles", "origin", "scratch", "counts", "status"):
        setattr(a, name, p)
    if emit:
        a.vertex_base, a.cap_v, a.cap_t, a.cap_long, a.cap_mid = 3, 4, 2, 3, 7
        for name in ("out_vertices", "out_triangles", "out_index", "next_vertices", "next_triangles", "next_origin"):
            setattr(a, name, p)
    return a


def test_calls_refuse_null_and_invalid_arguments_without_touching_a_device(L):
    buf, p = _fake()
    calls = {"count": (L.dnsplat_subdivide_count, False), "emit": (L.dnsplat_subdivide_emit, True)}
    for which, (fn, emit) in calls.items():
        assert fn(None, None) == -1, which
        for missing in ("vertices", "triangles", "origin", "scratch", "counts", "status"):
            a = _args(L, p, emit=emit)
            setattr(a, missing, None)
            assert fn(ctypes.byref(a), None) == -1, (which, missing)
        for field, values in (("V", (0, -1)), ("T", (0, -5)), ("max_edge", (0.0, -0.1, float("inf"), float("nan")))):
            for bad in values:
                a = _args(L, p, emit=emit)
                setattr(a, field, bad)
                assert fn(ctypes.byref(a), None) == -1, (which, field, bad)
        a = _args(L, p, emit=emit)
        a.T, a.scratch_bytes = MAX_T + 1, 2 ** 62                                 # the table would leave its int32 index
        assert fn(ctypes.byref(a), None) == -4, which
        a = _args(L, p, emit=emit)
        a.scratch_bytes -= 1
        assert fn(ctypes.byref(a), None) == -2, which
        a = _args(L, p, emit=emit)
        a.scratch = ctypes.c_void_p(p.value + 4)                                  # 8-byte alignment
        assert fn(ctypes.byref(a), None) == -2, which
    emit = L.dnsplat_subdivide_emit
    for field in ("vertex_base", "cap_v", "cap_t", "cap_long", "cap_mid"):
        a = _args(L, p, emit=True)
        setattr(a, field, -1)
        assert emit(ctypes.byref(a), None) == -1, field
    for missing in ("out_vertices", "out_triangles", "out_index", "next_vertices", "next_triangles", "next_origin"):
        a = _args(L, p, emit=True)
        setattr(a, missing, None)                                                 # a positive capacity without its buffer
        assert emit(ctypes.byref(a), None) == -1, missing
    # the limits: more than (2^31 - 1) / 4 children, V + n_mid or the emitted vertices past 2^31 - 1
    for field, ok, bad in (("cap_long", MAX_T // 4, MAX_T // 4 + 1), ("cap_mid", INT_MAX - 9, INT_MAX - 8), ("cap_v", INT_MAX - 3, INT_MAX - 2)):
        a = _args(L, p, emit=True)
        setattr(a, field, bad)
        assert emit(ctypes.byref(a), None) == -4, field
        a = _args(L, p, emit=True)
        setattr(a, field, ok)
        a.scratch_bytes -= 1                                                      # the limit passes; the next check answers, still on the host
        assert emit(ctypes.byref(a), None) == -2, field
    assert 4 * (MAX_T // 4) <= MAX_T < 4 * (MAX_T // 4 + 1)
    a = _args(L, p, emit=True)
    a.vertex_base = INT_MAX + 1
    assert emit(ctypes.byref(a), None) == -4
    assert not any(buf)


def test_python_surface_refuses_cpu_tensors_and_bad_arguments(dns):
    import numpy as np
    import torch

    v, f = torch.zeros(8, 3), torch.zeros(4, 3, dtype=torch.int32)
    with pytest.raises(dns.DnsplatError, match="no CPU fallback"):
        dns.subdivide_to_size(v, f, 0.1)
    with pytest.raises(dns.DnsplatError, match="no CPU fallback"):
        dns.subdivide_mesh((v, f), 0.1)
    if not torch.cuda.is_available():
        with pytest.raises(dns.DnsplatError, match="no CPU fallback"):
            dns.subdivide_to_size(np.zeros((8, 3)), np.zeros((4, 3), dtype=np.int32), 0.1)
    with pytest.raises(dns.DnsplatError, match="no CPU fallback"):
        dns.cull_mesh((v, f), np.eye(4)[None], np.eye(3), 4, 4, subdivide=True)
    sig = inspect.signature(dns.subdivide_to_size).parameters
    assert [sig[k].default for k in ("max_iter", "return_index")] == [10, False]
    assert inspect.signature(dns.subdivide_mesh).parameters["max_iter"].default == 10
    for fn in (dns.cull_mesh, dns.torch_mesh_cull.cull_mesh):                     # the new keywords default to what was
        sig = inspect.signature(fn).parameters
        assert [sig[k].default for k in ("subdivide", "max_edge", "max_iter")] == [False, 0.015, 10], fn
    sig = inspect.signature(dns.torch_subdivide.subdivide_to_size).parameters
    assert [sig[k].default for k in ("max_iter", "return_index", "midpoint_order")] == [10, False, "first"]
