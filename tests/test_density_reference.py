"""The Gaussian density field against vectors produced by THE REFERENCE's own code (tests/golden/make_reference_density_golden.py:
knn_sk, get_density and get_density_grad on the recipe of _density_inputs.py): the PyTorch restatement of torch_density — the fp64
yardstick of tests/test_gpu_density.py — the layout of the new argument struct and the argument checks of the entry points.

Tolerances.  The generator printed, for N = 4099 Gaussians and M = 2048 samples,
    e_ref: density 1.619e-06 (relative to max(value, 1e-4)), normals 4.509e-06 (component-wise)
— the error of the reference's own fp32 outputs against the fp64 restatement (_density_inputs.E_REF_DENSITY / E_REF_NORMAL; 0 samples
flagged at the >= 1 switch).  The HIP outputs get 4 x e_ref in test_gpu_density.py.  The fp32 restatement performs the reference's
operations and is therefore within 2 x e_ref of the reference's fp32 values (both lie within e_ref of the fp64 ones).  Indices are exact."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import _density_inputs as inputs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "dnsplat.h")


@pytest.fixture(scope="module")
def gold():
    return inputs.load_golden(os.path.join(HERE, "golden", inputs.GOLDEN))


def _rel(got, ref):
    return ((got.double() - ref.double()).abs() / ref.double().clamp_min(1e-4))


def test_the_fixture_is_the_recipe(gold):
    g, t = gold
    fresh = inputs.field_inputs()
    for k, v in fresh.items():
        assert torch.equal(v, t[k]), k
    assert g["closest"].shape == (inputs.M_FIX, 16) and g["density"].shape == (inputs.M_FIX,)
    assert inputs.smallest_rank_gap(t["means"], t["samples"]) >= inputs.GAP
    assert torch.unique(t["means"], dim=0).shape[0] == inputs.N_FIX


def test_brute_force_ranking_equals_knn_sk(gold):
    from dn_splatter_amd import torch_density as td

    g, t = gold
    closest = torch.from_numpy(g["closest"].astype(np.int64))
    assert torch.equal(td.closest(t["means"], t["samples"]), closest)
    # knn_sk drops the nearest Gaussian: column 0 of the reference is rank 1
    idx, d2 = td.knn(t["means"], t["samples"], 17, skip=0, return_d2=True)
    assert torch.equal(idx[:, 1:], closest) and bool((d2[:, 1:] >= d2[:, :-1]).all())
    with pytest.raises(ValueError):
        td.knn(t["means"][:16], t["samples"], 16, skip=1)


def test_e_ref_is_what_the_header_states(gold):
    """The reference's own fp32 error against the fp64 restatement: the numbers the GPU tolerance is built from."""
    from dn_splatter_amd import torch_density as td

    g, t = gold
    closest = torch.from_numpy(g["closest"].astype(np.int64))
    t64 = {k: v.double() for k, v in t.items()}
    flag = torch.from_numpy(np.unpackbits(g["switch_flag"])[:inputs.M_FIX].astype(bool))
    d64 = td.density(t64["means"], t64["scales"], t64["quats"], t64["opacities"], t64["samples"], closest)
    e_d = float(_rel(torch.from_numpy(g["density"]), d64)[~flag].max())
    e_n = max(float((torch.from_numpy(g[f"grad_{nc or 'all'}"]).double()
                     - td.density_grad(t64["means"], t64["scales"], t64["quats"], t64["samples"], nc, closest)).abs().max()) for nc in (None, 1, 5))
    print(f"e_ref density {e_d:.3e} normals {e_n:.3e}; file {g['e_ref']}")
    assert e_d <= inputs.E_REF_DENSITY * 1.001 and e_n <= inputs.E_REF_NORMAL * 1.001
    assert g["e_ref"][0] <= inputs.E_REF_DENSITY * 1.001 and g["e_ref"][1] <= inputs.E_REF_NORMAL * 1.001
    # the decisions of the switch: no unflagged sample within the envelope
    s64 = td.density_sum(t64["means"], t64["scales"], t64["quats"], t64["opacities"], t64["samples"], closest)
    assert torch.equal(flag, (s64 - 1.0).abs() <= inputs.SWITCH_ENVELOPE)
    assert 0 < int((s64 >= 1).sum()) < inputs.M_FIX


def test_fp32_restatement_equals_the_reference(gold):
    from dn_splatter_amd import torch_density as td

    g, t = gold
    closest = torch.from_numpy(g["closest"].astype(np.int64))
    d = td.density(t["means"], t["scales"], t["quats"], t["opacities"], t["samples"])
    err = float(_rel(d, torch.from_numpy(g["density"])).max())
    print(f"density: restatement vs reference {err:.3e}")
    assert err <= 2 * inputs.E_REF_DENSITY
    for nc in (None, 1, 5):
        n = td.density_grad(t["means"], t["scales"], t["quats"], t["samples"], nc, closest)
        err = float((n - torch.from_numpy(g[f"grad_{nc or 'all'}"])).abs().max())
        print(f"normals, num_closest {nc}: restatement vs reference {err:.3e}")
        assert err <= 2 * inputs.E_REF_NORMAL


def test_volume_equals_the_reference_lattice(gold):
    from dn_splatter_amd import torch_density as td

    g, t = gold
    R, radius = int(g["volume_spec"][0]), float(g["volume_spec"][1])
    for key, box in (("volume", None), ("volume_crop", inputs.crop_box())):
        vol = td.density_volume(t["means"], t["scales"], t["quats"], t["opacities"], R, radius, box)
        ref = torch.from_numpy(g[key])
        assert torch.equal(vol == -1e6, ref == -1e6), key
        inside = ref != -1e6
        assert float(_rel(vol[inside], ref[inside]).max()) <= 2 * inputs.E_REF_DENSITY, key
    X, Y, Z, grid = td.lattice(R, radius)
    assert torch.equal(X, torch.linspace(-1, 1, R) * radius) and grid.shape == (R ** 3, 3)
    assert torch.equal(grid.reshape(R, R, R, 3)[3, 5, 7], torch.stack([X[3], Y[5], Z[7]]))          # `ij` order, z fastest


def test_density_args_layout_matches_the_c_compiler(dns, tmp_path):
    """sizeof / offsetof of dnsplat_density_args as gcc sees the header == the ctypes mirror."""
    from dn_splatter_amd import _lib

    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){',
             'printf("size %zu\\n", sizeof(dnsplat_density_args));']
    for fname, _ in _lib.DensityArgs._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(dnsplat_density_args, {fname}));')
    lines.append('printf("maxk %d\\n", DNSPLAT_KNN_MAX_K);')
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(_lib.DensityArgs)
    for fname, _ in _lib.DensityArgs._fields_:
        assert int(got[fname]) == getattr(_lib.DensityArgs, fname).offset, fname
    from dn_splatter_amd import density

    assert int(got["maxk"]) == density.MAX_K


def test_argument_errors_are_return_codes_without_a_gpu(dns):
    from dn_splatter_amd import _lib

    dns.build_library()
    L = dns.load_library()
    assert L.dnsplat_knn_grid_dim(0) == 0 and L.dnsplat_knn_index_bytes(0) == 0 and L.dnsplat_knn_index_bytes(-5) == 0
    dims = [L.dnsplat_knn_grid_dim(n) for n in (1, 15, 16, 53, 54, 1000, 4099, 1_000_000, 2 ** 31 - 1)]
    assert dims == [1, 1, 2, 2, 3, 7, 12, 79, 128]                     # floor(cbrt(N / 2)), at most 128
    sizes = [L.dnsplat_knn_index_bytes(n) for n in (1, 1000, 4099, 1_000_000)]
    assert sizes == sorted(sizes) and sizes[0] >= 64 and all(s % 16 == 0 for s in sizes)
    assert sizes[3] >= 1_000_000 * 16 + 4 * 79 ** 3
    assert L.dnsplat_knn_build(0, None, None, None) == -1
    assert L.dnsplat_knn_build(8, None, None, None) == -1
    fake = ctypes.c_void_p(16)                                         # never dereferenced: every call below returns before a launch
    assert L.dnsplat_knn_query(100, None, 4, fake, 3, 0, fake, None, None) == -1
    assert L.dnsplat_knn_query(100, fake, 4, fake, 0, 0, fake, None, None) == -1          # k < 1
    assert L.dnsplat_knn_query(100, fake, 4, fake, 3, -1, fake, None, None) == -1
    assert L.dnsplat_knn_query(100, fake, 4, fake, 32, 1, fake, None, None) == -4         # k + skip > 32
    assert L.dnsplat_knn_query(16, fake, 4, fake, 16, 1, fake, None, None) == -1          # k + skip > N, as sklearn
    assert L.dnsplat_knn_query(100, fake, -1, fake, 3, 0, fake, None, None) == -1
    assert L.dnsplat_knn_query(100, fake, 0, None, 3, 0, None, None, None) == 0           # no query: nothing to do
    assert L.dnsplat_density_pack(0, fake, fake, fake, fake, fake, None) == -1
    assert L.dnsplat_density_pack(4, fake, None, fake, fake, fake, None) == -1
    assert L.dnsplat_density_eval(None, None) == -1
    a = _lib.DensityArgs()
    a.N, a.records, a.index, a.samples, a.M, a.k, a.skip = 100, 16, 16, 16, 4, 16, 1
    assert L.dnsplat_density_eval(ctypes.byref(a), None) == -1                            # neither density nor normals
    a.density = 16
    a.k = 40
    assert L.dnsplat_density_eval(ctypes.byref(a), None) == -4
    a.k, a.N = 16, 16
    assert L.dnsplat_density_eval(ctypes.byref(a), None) == -1                            # k + skip > N
    a.N, a.num_closest = 100, 17
    assert L.dnsplat_density_eval(ctypes.byref(a), None) == -1                            # more than k neighbours in the normal
    a.num_closest, a.samples = 0, None
    assert L.dnsplat_density_eval(ctypes.byref(a), None) == -1                            # no samples and no lattice
    a.samples, a.index = 16, None
    assert L.dnsplat_density_eval(ctypes.byref(a), None) == -1                            # neither neighbours nor an index
    a.M = 0
    a.index = 16
    assert L.dnsplat_density_eval(ctypes.byref(a), None) == 0                             # no sample: nothing to do


def test_cpu_tensors_are_refused(dns):
    from dn_splatter_amd import DnsplatError, density

    t = inputs.field_inputs(32, 8, far=0)
    with pytest.raises(DnsplatError, match="no CPU fallback"):
        density.knn(t["means"], t["samples"], 3)
    with pytest.raises(DnsplatError, match="no CPU fallback"):
        density.GaussianDensityField(t["means"], t["scales"], t["quats"], t["opacities"])
    with pytest.raises(ValueError):
        density._check_k(16, 16, 1)
    with pytest.raises(ValueError):
        density._check_k(100, 32, 1)
