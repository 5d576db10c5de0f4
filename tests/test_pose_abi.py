"""Camera pose gradient, the parts that need no GPU: the C ABI of dnsplat_project_bwd_pose (exports, struct layout, argument checks,
workspace query) and the fp64 reference helper the GPU tests compare against (tests/_pose_ref.py), held to autograd through the
committed oracle (oracle/dense_ref.py) with a single view matrix."""
import ctypes
import os
import subprocess

import pytest
import torch

from _scenes import gsplat_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dnsplat.h")


@pytest.fixture(scope="module")
def L(dns):
    dns.build_library()
    return dns.load_library()


def test_pose_symbols_are_exported_and_declared(dns, L):
    from dn_splatter_amd import _lib

    raw = ctypes.CDLL(str(dns.build_library()))
    text = open(HEADER).read()
    for name in ("dnsplat_pose_partial_rows", "dnsplat_project_bwd_pose"):
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS, name
        assert name + "(" in text, name
    assert "} dnsplat_pose_grads;" in text
    assert L.dnsplat_abi_version() == 15 and _lib.ABI_VERSION == 15          # additive: found by symbol, the version stays


def test_pose_struct_layout_matches_the_c_compiler(dns, tmp_path):
    from dn_splatter_amd import _lib

    cls, cname = _lib.PoseGrads, "dnsplat_pose_grads"
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
    assert [f for f, _ in cls._fields_] == ["partials", "v_viewmat", "c2w", "v_c2w"]
    for fname, _ in cls._fields_:
        assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, fname


def test_pose_entry_point_refuses_null_and_inconsistent_arguments(dns, L):
    from dn_splatter_amd import _lib

    assert L.dnsplat_project_bwd_pose(None, None, None, None, None, None) == -1
    s, c, o, g, p = _lib.Scene(), _lib.Camera(), _lib.ProjOut(), _lib.ProjGrads(), _lib.PoseGrads()
    refs = [ctypes.byref(x) for x in (s, c, o, g, p)]
    for i in range(5):                                      # each struct pointer in turn
        args = list(refs)
        args[i] = None
        assert L.dnsplat_project_bwd_pose(*args, None) == -1, i
    s.N = 128
    assert L.dnsplat_project_bwd_pose(*refs, None) == -1     # no output, no view matrix, no workspace
    buf = (ctypes.c_float * 64)()
    p.v_viewmat = ctypes.cast(buf, ctypes.c_void_p)
    c.viewmat = ctypes.cast(buf, ctypes.c_void_p)
    assert L.dnsplat_project_bwd_pose(*refs, None) == -1     # N > 0 without a workspace
    p.partials = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    assert L.dnsplat_project_bwd_pose(*refs, None) == -1     # workspace not 16-byte aligned (and no gradient tensors)
    p.partials = None
    s.N = 0
    p.c2w = ctypes.cast(buf, ctypes.c_void_p)
    assert L.dnsplat_project_bwd_pose(*refs, None) == -1     # c2w without v_c2w
    s.N = -1
    p.c2w = None
    assert L.dnsplat_project_bwd_pose(*refs, None) == -1


def test_pose_partial_rows_is_monotone_and_covers_every_workgroup(L):
    assert L.dnsplat_pose_partial_rows(0) == 0 and L.dnsplat_pose_partial_rows(-5) == 0
    ns = list(range(1, 40_000)) + [10 ** 5, 200_000, 10 ** 6, 10 ** 6 + 1, 5 * 10 ** 6, 10 ** 8, 2 ** 31 - 1]
    rows = [L.dnsplat_pose_partial_rows(n) for n in ns]
    assert all(r >= (n + 63) // 64 for n, r in zip(ns, rows))
    assert all(b >= a for a, b in zip(rows, rows[1:]))
    assert rows[ns.index(10 ** 6)] <= 15_625 + 2 * 62            # the level-1 sums are a per-cent of the rows


def _raster_level_cotangents(N, n_col, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1)
    return dict(means2d=r(N, 2), conics=r(N, 3), depths=r(N), opacities=r(N), colors=r(N, n_col))


@pytest.mark.parametrize("N,W,H,focal,aniso,sh_degree,aa", [
    (256, 64, 64, 40.0, False, 3, False), (256, 64, 64, 40.0, True, 3, True), (256, 64, 64, 40.0, True, None, True),
    (10_000, 256, 256, 160.0, True, 3, False), (10_000, 256, 256, 160.0, False, 2, True),
    (200_000, 640, 480, 400.0, True, 3, True)])
def test_per_gaussian_reference_sums_to_autograd_through_the_oracle(N, W, H, focal, aniso, sh_degree, aa):
    """S = sum_n g_n of the per-Gaussian helper == autograd through oracle/dense_ref.project + sh_colors with ONE matrix, to
    1e-12 x A entry by entry (A = sum_n |g_n|): both are fp64 evaluations of the same formulas, summed in a different order."""
    import _pose_ref
    from oracle import dense_ref  # noqa: F401  (the reference side of the comparison)

    inp, viewmat, K, _ = gsplat_inputs(N, W, H, focal=focal, seed=3 + N % 7, anisotropic=aniso)
    d = {k: v.double() for k, v in inp.items()}
    colors = d["colors"] if sh_degree is not None else torch.rand(N, 3, dtype=torch.float64)
    cot = _raster_level_cotangents(N, 3, seed=N)
    args = (d["means"], d["quats"], d["scales"], d["opacities"], colors)
    K64 = K[0].double()
    S, A = _pose_ref.pose_gradient_terms(*args, viewmat[0], K64, W, H, sh_degree, cot, antialiased=aa)
    V1 = viewmat[0].double().clone().requires_grad_(True)
    out = _pose_ref.stage_outputs(*args, V1, K64, W, H, sh_degree, antialiased=aa, per_gaussian=False)
    (ref,) = torch.autograd.grad(_pose_ref.contract(out, cot), V1)
    assert int((out["radii"] > 0).sum()) > N // 10
    assert torch.isfinite(S).all() and torch.isfinite(ref).all()
    ratio = ((S - ref).abs() / (1e-12 * A).clamp_min(1e-300))
    print(f"[pose] N={N}: |S - autograd| / A max {float(((S - ref).abs() / A.clamp_min(1e-300)).max()):.2e}; A / |S| max "
          f"{float((A / S.abs().clamp_min(1e-300))[A > 0].max()):.1f}")
    assert bool(((S - ref).abs() <= 1e-12 * A).all()), ratio
    assert bool((S[A == 0] == 0).all())
    if sh_degree is None:
        assert float(S[3].abs().max()) == 0.0 and float(A[3].abs().max()) == 0.0     # direct colours: no path through the inverse
    else:
        # the bottom row as the kernels form it: -(c . G) [c, 1] with c the camera centre and G = d loss / d c
        c = torch.inverse(viewmat[0].double())[:3, 3]
        row = ref[3]
        assert float(row[3].abs()) > 0
        assert torch.allclose(row[:3], row[3] * c, rtol=1e-9, atol=1e-12 * float(A[3].max()))
