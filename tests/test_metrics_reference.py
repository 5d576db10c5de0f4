"""The evaluation metrics against vectors produced by THE REFERENCE's own code (tests/golden/make_reference_metrics_golden.py:
DepthMetrics, NormalMetrics and mean_angular_error of dn_splatter/metrics.py on the recipe of _metrics_inputs.py): the PyTorch
restatements of torch_metrics — the fp64 yardstick of tests/test_gpu_metrics.py — the numerators and counts the kernel exposes, the
argument checks of the entry point and the bookkeeping of install_metrics.

The restatement performs the reference's float32 operations in the reference's order, so in float32 it must return the reference's
floats to the last bit on the same machine; the bound written here is fp32 rounding of the reference's own result (4 ulp), which also
holds where a library's reduction order differs.  Integers and the median are exact.  The psnr formula is NOT pinned by this fixture
(torchmetrics was not at hand when it was made)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _metrics_inputs as inputs

HERE = os.path.dirname(os.path.abspath(__file__))
ULP = 2.0 ** -23
ROUNDING = 4 * ULP          # of the reference's own float32 result


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "reference_metrics.npz"))


def _same(got, ref, what, exact=False):
    """nan where the reference is nan, inf where it is inf, else within fp32 rounding of its value (or equal)."""
    got = np.array([float(x) for x in got], dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, got, ref)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), (what, got, ref)
    if exact:
        assert np.array_equal(got[fin], ref[fin]), (what, got, ref)
    else:
        assert np.all(np.abs(got[fin] - ref[fin]) <= ROUNDING * np.abs(ref[fin])), (what, got, ref)


def _counts_agree(counts, metrics, what):
    """a_k of the reference == counts[k] / counts[0] in float32, exactly: the integers the kernel exposes are the reference's."""
    m = np.float32(int(counts[0]))
    for k in (1, 2, 3):
        want = np.float32(metrics[3 + k])
        if int(counts[0]) == 0:
            assert np.isnan(want), what
        else:
            assert np.float32(np.float32(int(counts[k])) / m) == want, (what, k, counts, metrics)


@pytest.mark.parametrize("H,W", inputs.FIXTURE_FRAMES)
def test_frames_equal_the_reference(g, H, W):
    from dn_splatter_amd import torch_metrics as tm

    assert H % 16 and W % 16 and float(g["tolerance"]) == inputs.TOLERANCE
    f = inputs.fixture_frame(g, H, W)
    pre = f"f{H}x{W}_"
    d = tm.depth_metrics(f["depth"].permute(2, 0, 1), f["gt_depth"].permute(2, 0, 1))
    _same(d, g[pre + "depth"], "depth")
    chw = lambda t: t.permute(2, 0, 1).unsqueeze(0)      # noqa: E731
    n = tm.normal_metrics(chw(f["normal"]), chw(f["gt_normal"]))
    _same(n[:3], g[pre + "normal"][:3], "normal")
    assert np.float32(float(n[3])) == g[pre + "normal"][3]                                   # the median: exact
    angle = tm.mean_angular_error(chw(f["normal"]), chw(f["gt_normal"]))
    assert np.allclose(angle.numpy(), g[pre + "angle"], rtol=ROUNDING, atol=0)
    # the numerators and counts: the metrics are their quotients
    sums, counts = tm.eval_sums(depth=f["depth"], gt_depth=f["gt_depth"], normal=f["normal"], gt_normal=f["gt_normal"])
    _counts_agree(counts, g[pre + "depth"], "frame")
    P = H * W
    assert 0 < int(counts[0]) < P and int(counts[4]) == int(counts[0]) and int(counts[5]) == 0
    m = float(counts[0])
    back = [sums[2] / m, sums[3] / m, torch.sqrt(sums[1] / m), sums[4] / float(counts[4])]
    assert np.allclose([float(x) for x in back], g[pre + "depth"][:4], rtol=1e-5, atol=0)
    back = [sums[5] / P, torch.sqrt(sums[6] / (3 * P)), sums[7] / (3 * P)]
    assert np.allclose([float(x) for x in back], g[pre + "normal"][:3], rtol=1e-5, atol=0)
    # float64 on the same float32 images: the same decisions, values within float32's distance
    s64, c64 = tm.eval_sums(depth=f["depth"].double(), gt_depth=f["gt_depth"].double(), normal=f["normal"].double(),
                            gt_normal=f["gt_normal"].double())
    assert torch.equal(c64, counts) and np.allclose(s64.numpy(), sums.numpy(), rtol=1e-5)
    d64 = tm.depth_metrics(f["depth"].double(), f["gt_depth"].double())
    assert np.allclose([float(x) for x in d64], g[pre + "depth"], rtol=1e-5, atol=0)


@pytest.mark.parametrize("name", sorted(inputs.DEPTH_EDGES))
def test_depth_edges_equal_the_reference(g, name):
    from dn_splatter_amd import torch_metrics as tm

    pred, gt = inputs.DEPTH_EDGES[name]
    ref = g["edge_depth_" + name]
    _same(tm.depth_metrics(pred, gt), ref, name)
    _, counts = tm.eval_sums(depth=pred, gt_depth=gt)
    _counts_agree(counts, ref, name)
    want = {"zero_prediction": [3, 1, 2, 2, 3], "negative_prediction": [4, 2, 4, 4, 3], "nan_prediction": [4, 1, 3, 3, 3],
            "nothing_above_tolerance": [0, 0, 0, 0, 0], "ground_truth_at_tolerance": [3, 1, 2, 2, 3],
            "t_exactly_1_25": [5, 0, 3, 4, 5], "only_negative_predictions": [2, 2, 2, 2, 0]}[name]
    assert counts[:5].tolist() == want, (name, counts)
    if name == "zero_prediction":
        assert np.isinf(ref[3]) and ref[3] > 0
    if name == "nothing_above_tolerance":
        assert np.isnan(ref).all()
    if name == "ground_truth_at_tolerance":
        assert float(gt[0]) > 0.1 and int(counts[0]) == 3                      # 0.1f (above 0.1 as a double) is NOT masked in; the float32 above it is
    if name in ("nan_prediction", "negative_prediction"):
        assert np.isfinite(ref[3])                                              # nanmean dropped the one nan term


@pytest.mark.parametrize("name", sorted(inputs.NORMAL_EDGES))
def test_normal_edges_equal_the_reference(g, name):
    from dn_splatter_amd import torch_metrics as tm

    pred, gt = inputs.NORMAL_EDGES[name]
    ref = g["edge_normal_" + name]
    got = tm.normal_metrics(pred, gt)
    _same(got[:3], ref[:3], name)
    _same(got[3:], ref[3:], name + " median", exact=True)
    diff = torch.abs(gt - pred).reshape(-1)
    n = diff.numel()
    if name == "a_nan_difference":
        assert np.isnan(ref[3])
    else:
        assert float(torch.sort(diff).values[(n - 1) // 2]) == float(ref[3])    # the LOWER median, inf sorting as a value
    assert (name == "mostly_inf") == bool(np.isinf(ref[3]))
    _, counts = tm.eval_sums(normal=pred[0].permute(1, 2, 0), gt_normal=gt[0].permute(1, 2, 0))
    assert int(counts[5]) == (1 if name == "a_nan_difference" else 0)


def test_psnr_formula_and_key_order():
    """Not pinned to torchmetrics: the published formula on a case with a closed form."""
    from dn_splatter_amd import torch_metrics as tm

    gt = torch.zeros(4, 5, 3)
    pred = torch.full((4, 5, 3), 0.1)
    assert abs(float(tm.mse(gt, pred)) - 0.01) < 1e-8 and abs(float(tm.psnr(gt, pred)) - 20.0) < 1e-4
    assert float(tm.psnr(gt, gt)) == float("inf")
    assert sorted(tm.METRIC_INDEX.values()) == list(range(13))
    assert set(tm.RGB_KEYS + tm.DEPTH_KEYS + tm.NORMAL_KEYS) == set(tm.METRIC_INDEX)


def test_header_indices_match_the_binding():
    """DNSPLAT_METRIC_* of include/dnsplat.h == torch_metrics.METRIC_INDEX; the ctypes mirror has the C layout."""
    import re
    import subprocess
    import tempfile

    from dn_splatter_amd import _lib, torch_metrics as tm

    header = os.path.join(os.path.dirname(HERE), "include", "dnsplat.h")
    defs = dict(re.findall(r"#define (DNSPLAT_METRIC_[A-Z0-9_]+) (\d+)", open(header).read()))
    names = {"rgb_mse": "RGB_MSE", "rgb_psnr": "RGB_PSNR", "normal_rsme": "NORMAL_RMSE"}
    for key, idx in tm.METRIC_INDEX.items():
        assert int(defs["DNSPLAT_METRIC_" + names.get(key, key.upper())]) == idx, key
    assert (int(defs["DNSPLAT_METRIC_COUNT"]), int(defs["DNSPLAT_METRIC_COUNTS"]), int(defs["DNSPLAT_METRIC_SUMS"])) == \
        (tm.METRIC_COUNT, tm.METRIC_COUNTS, tm.METRIC_SUMS)
    cls = _lib.EvalMetricsArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', 'int main(void){',
             'printf("size %zu\\n", sizeof(dnsplat_eval_metrics_args));']
    lines += [f'printf("{n} %zu\\n", offsetof(dnsplat_eval_metrics_args, {n}));' for n, _ in cls._fields_] + ['return 0;}']
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", src, "-o", exe], check=True)
        got = dict(l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(cls)
    for n, _ in cls._fields_:
        assert int(got[n]) == getattr(cls, n).offset, n


def test_entry_point_refuses_impossible_arguments_without_a_launch(dns):
    """Every invalid-argument return of dnsplat_eval_metrics: an error code, on a machine without a GPU."""
    from dn_splatter_amd import _lib, _ops

    dns.build_library()
    L = _lib.lib()
    # real buffers of the sizes a valid call needs, on the device where there is one (were a check ever lost, the call would run on
    # memory it may touch)
    dev = "cuda:0" if torch.cuda.is_available() else "cpu"
    W, H = 70, 45
    img = torch.full((H, W, 3), 0.5, device=dev)
    dep = torch.full((H, W), 0.5, device=dev)
    scratch = torch.zeros(L.dnsplat_eval_metrics_scratch_bytes(W, H) // 8, dtype=torch.float64, device=dev)
    metrics = torch.zeros(16, device=dev)
    counts = torch.zeros(8, dtype=torch.int64, device=dev)
    sums = torch.zeros(8, dtype=torch.float64, device=dev)
    ok = dict(width=W, height=H, rgb=img, gt_rgb=img, depth=dep, gt_depth=dep, depth_tolerance=0.1, normal=img, gt_normal=img,
              normal_layout=1, scratch=scratch, metrics=metrics, counts=counts, sums=sums)

    def call(**kw):
        a = _ops._eval_metrics_args(**{**ok, **kw})
        return L.dnsplat_eval_metrics(ctypes.byref(a), None)

    assert L.dnsplat_eval_metrics(None, None) == -1
    for name in ("scratch", "metrics", "counts"):
        assert call(**{name: None}) == -1, name
    for name in ("rgb", "gt_rgb", "depth", "gt_depth", "normal", "gt_normal"):
        assert call(**{name: None}) == -1, name                                              # half a pair
    assert call(rgb=None, gt_rgb=None, depth=None, gt_depth=None, normal=None, gt_normal=None) == -1
    assert call(width=0) == -1 and call(height=0) == -1 and call(width=-3) == -1
    assert call(normal_layout=2) == -1 and call(normal_layout=-1) == -1
    assert call(width=2 ** 16, height=2 ** 15) == -4                                         # 2^31 pixels: unsupported
    assert call(width=2 ** 31 - 1, height=2 ** 31 - 1) == -4
    assert L.dnsplat_eval_metrics_scratch_bytes(0, 5) == 0 and L.dnsplat_eval_metrics_scratch_bytes(5, -1) == 0
    assert L.dnsplat_eval_metrics_scratch_bytes(2 ** 16, 2 ** 15) == 0
    # the head (64 bytes of state, 2048 + 2048 + 512 bins of 8 bytes) and one 112-byte partial per 1024 pixels
    head = 64 + 8 * (2048 + 2048 + 512)
    assert L.dnsplat_eval_metrics_scratch_bytes(32, 32) == head + 112 and L.dnsplat_eval_metrics_scratch_bytes(1025, 1) == head + 2 * 112
    assert L.dnsplat_eval_metrics_scratch_bytes(2 ** 31 - 1, 1) == head + 112 * 2 ** 21


def _stand_in():
    """A model whose scoring modules look like the reference's (install_metrics goes by class NAMES)."""
    DepthMetrics = type("DepthMetrics", (torch.nn.Module,), {"tolerance": 0.25})
    NormalMetrics = type("NormalMetrics", (torch.nn.Module,), {})
    PeakSignalNoiseRatio = type("PeakSignalNoiseRatio", (torch.nn.Module,), {})
    Other = type("RGBMetrics", (torch.nn.Module,), {})
    m = torch.nn.Module()
    m.depth_metrics, m.normal_metrics, m.psnr = DepthMetrics(), NormalMetrics(), PeakSignalNoiseRatio()
    m.rgb_metrics, m.lpips, m.ssim = Other(), Other(), Other()
    return m


def test_install_metrics_swaps_the_three_modules_by_class_name():
    import dn_splatter_amd as dns
    from dn_splatter_amd import fused_loss, fused_metrics

    m = _stand_in()
    old = {k: getattr(m, k) for k in ("depth_metrics", "normal_metrics", "psnr", "rgb_metrics", "lpips", "ssim")}
    assert dns.install_metrics(m) == ["depth_metrics", "normal_metrics", "psnr", "ssim"]
    assert isinstance(m.depth_metrics, fused_metrics.DepthMetrics) and m.depth_metrics.tolerance == 0.25
    assert isinstance(m.normal_metrics, fused_metrics.NormalMetrics) and isinstance(m.psnr, fused_metrics.PSNR)
    assert isinstance(m.ssim, fused_loss.SSIM)
    assert m.rgb_metrics is old["rgb_metrics"] and m.lpips is old["lpips"]
    for k in ("depth_metrics", "normal_metrics", "psnr", "ssim"):
        assert getattr(m, "_dnsplat_original_" + k) is old[k], k
    now = {k: getattr(m, k) for k in old}
    assert dns.install_metrics(m) == [] and all(getattr(m, k) is now[k] for k in old)                   # idempotent
    assert m._dnsplat_original_depth_metrics is old["depth_metrics"]
    # a differently named module stays
    other = _stand_in()
    other.depth_metrics = type("MyDepthMetrics", (torch.nn.Module,), {})()
    keep = other.depth_metrics
    assert dns.install_metrics(other) == ["normal_metrics", "psnr", "ssim"] and other.depth_metrics is keep
    # there is no CPU path behind the drop-ins: a missing GPU is an error, not a fall-back to PyTorch
    x = torch.rand(1, 3, 4, 5)
    for fn in (lambda: m.depth_metrics(x, x), lambda: m.normal_metrics(x, x), lambda: m.psnr(x, x),
               lambda: dns.image_metrics({"rgb": x[0].permute(1, 2, 0)}, {"image": x[0].permute(1, 2, 0)}, ssim=False)):
        with pytest.raises(dns.DnsplatError):
            fn()
    with pytest.raises(NotImplementedError):
        m.normal_metrics(torch.rand(2, 3, 4, 5), torch.rand(2, 3, 4, 5))
    with pytest.raises(NotImplementedError):
        m.normal_metrics(torch.rand(1, 4, 4, 5), torch.rand(1, 4, 4, 5))
    with pytest.raises(ValueError, match=r"\(4, 5, 1\).*\(8, 10, 1\)"):
        dns.image_metrics({"rgb": torch.rand(4, 5, 3), "depth": torch.rand(4, 5, 1)},
                          {"image": torch.rand(4, 5, 3), "sensor_depth": torch.rand(8, 10, 1)})
