"""The evaluation-metric kernels (metrics.hip behind dnsplat_eval_metrics) against the PyTorch restatements of torch_metrics on the host
(pinned to the reference's own code by test_metrics_reference.py).

Two kinds of results, two rules:
  * DECISIONS — the integer counts (masked pixels, the three threshold counts, the non-nan log terms, the nan differences) and the
    median of |g - p|: EXACTLY the float32 restatement's.  Each is one correctly rounded fp32 operation on both sides (a comparison, an
    IEEE division, a subtraction), so there is no flagged-decision allowance and no entry is left out.
  * SUMS and finished metrics — against the float64 restatement under the rule of test_gpu_losses / test_gpu_ags:
    |v - v64| <= VALUE_TOL |v64| + FP32_ENVELOPE |v32 - v64|, with nan and inf where the restatement has them.

Shapes are the smallest at which each mechanism can go wrong: one pixel, one row, one column, fewer elements than a wave; the sweep's
workgroup span (1024 pixels) and one either side; the span of rounds two and three (4096 elements: 3 x 1365 = 4095 and 3 x 1366 = 4098
lie either side, and the shapes cover every remainder of 3 H W by 4, the float4 reads of those rounds); more workgroups than the last
launch folds in one trip (256)."""
import functools

import pytest
import torch

import _metrics_inputs as inputs
from _scenes import FP32_ENVELOPE
from test_gpu_losses import VALUE_TOL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SPAN = 1024              # metrics.hip MT_SPAN: pixels per workgroup of the sweep
HSPAN = 4096             # metrics.hip MT_HSPAN: elements per workgroup of rounds two and three
FOLD = 256               # metrics.hip MT_THREADS: partials dns_fold_partials takes per trip in the last launch
PAIRS = ("rgb", "depth", "normal")


# ---- the two sides ---------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=32)
def _frame(H, W, seed=0, identical=False):
    return inputs.frame(H, W, seed, identical)


def _off_16_bytes(t):
    """The same values in memory that starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)[1:].view(t.shape)
    buf.copy_(t)
    assert buf.data_ptr() % 16 == 4 and buf.is_contiguous()
    return buf


def _hip(f, pairs=PAIRS, layout="hwc", tolerance=inputs.TOLERANCE, unaligned=False):
    """(metrics [16], counts [8], sums [8]) of dnsplat_eval_metrics on the host; the images are uploaded."""
    from dn_splatter_amd import fused_metrics as fm

    H, W = f[pairs[0]].shape[0], f[pairs[0]].shape[1]
    kw = {}
    for k in pairs:
        pred, gt = f[k].to(DEV), f["gt_" + k].to(DEV)
        if k == "normal" and layout == "chw":
            pred, gt = pred.permute(2, 0, 1).contiguous(), gt.permute(2, 0, 1).contiguous()
        kw[k], kw["gt_" + k] = pred.contiguous(), gt.contiguous()
        if unaligned:
            kw[k], kw["gt_" + k] = _off_16_bytes(kw[k]), _off_16_bytes(kw["gt_" + k])
    m, c, s = fm.eval_metrics(W, H, depth_tolerance=tolerance, normal_layout=layout, with_sums=True, **kw)
    assert m.dtype == torch.float32 and c.dtype == torch.int64 and s.dtype == torch.float64
    return m.cpu(), c.cpu(), s.cpu()


@functools.lru_cache(maxsize=32)
def _restated_frame(H, W, seed=0, identical=False):
    return {dt: _restated(_frame(H, W, seed, identical), PAIRS, dt) for dt in (torch.float32, torch.float64)}


def _restated(f, pairs, dtype, tolerance=inputs.TOLERANCE):
    """(metrics dict, counts, sums) of torch_metrics on the host in ``dtype``."""
    from dn_splatter_amd import torch_metrics as tm

    t = {k: (f[k].to(dtype), f["gt_" + k].to(dtype)) for k in pairs}
    kw = {}
    for k in pairs:
        kw[k], kw["gt_" + k] = t[k]
    sums, counts = tm.eval_sums(tolerance=tolerance, **kw)
    out = {}
    if "rgb" in pairs:
        out["rgb_mse"], out["rgb_psnr"] = tm.mse(t["rgb"][1], t["rgb"][0]), tm.psnr(t["rgb"][1], t["rgb"][0])
    if "depth" in pairs:
        out.update(zip(tm.DEPTH_KEYS, tm.depth_metrics(t["depth"][0], t["depth"][1], tolerance)))
    if "normal" in pairs:
        chw = lambda x: x.permute(2, 0, 1).unsqueeze(0)      # noqa: E731
        out.update(zip(tm.NORMAL_KEYS, tm.normal_metrics(chw(t["normal"][0]), chw(t["normal"][1]))))
    return out, counts, sums


def _check_value(v, v64, v32, what):
    v, v64, v32 = float(v), float(v64), float(v32)
    if v64 != v64 or v64 in (float("inf"), float("-inf")):
        print(f"[metrics] {what}: {v!r} vs fp64 {v64!r}")
        assert (v != v) if v64 != v64 else v == v64, f"{what}: {v!r} vs fp64 {v64!r}"
        return
    env = FP32_ENVELOPE * abs(v32 - v64) if v32 == v32 else 0.0
    print(f"[metrics] {what}: {v:.9g} vs fp64 {v64:.9g}: error {abs(v - v64):.2e} (allowed {VALUE_TOL * abs(v64) + env:.2e})")
    assert abs(v - v64) <= VALUE_TOL * abs(v64) + env, f"{what}: {v!r} vs fp64 {v64!r} (fp32 {v32!r})"


def _same_bits(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float32).reshape(1), torch.as_tensor(b, dtype=torch.float32).reshape(1)
    return bool(torch.isnan(a)) and bool(torch.isnan(b)) or bool(a.view(torch.int32) == b.view(torch.int32))


SUM_PAIR = ("rgb", "depth", "depth", "depth", "depth", "normal", "normal", "normal")          # DNSPLAT_METRIC_SUM_*


def _check(f, pairs, what, layout="hwc", ref=None, tolerance=inputs.TOLERANCE):
    """Counts and the median exactly; the sums, then the metrics, against fp64.  Absent pairs: nan metrics, zero counts and sums."""
    from dn_splatter_amd import torch_metrics as tm

    m, c, s = _hip(f, pairs, layout, tolerance)
    r32, r64 = ref if ref is not None else (_restated(f, pairs, torch.float32, tolerance), _restated(f, pairs, torch.float64, tolerance))
    print(f"[metrics] {what}: counts {c.tolist()}")
    assert c.tolist() == r32[1].tolist(), f"{what}: counts {c.tolist()} vs the fp32 restatement's {r32[1].tolist()}"
    assert [r64[1][k] for k in (0, 4, 5)] == [r32[1][k] for k in (0, 4, 5)]          # the mask is the same in float64
    for k in range(tm.METRIC_SUMS):
        if SUM_PAIR[k] in pairs:
            _check_value(s[k], r64[2][k], r32[2][k], f"{what} sum {k}")
        else:
            assert float(s[k]) == 0.0
    for key, idx in tm.METRIC_INDEX.items():
        if key not in r64[0]:
            assert bool(torch.isnan(m[idx])), f"{what}: {key} of an absent pair is {float(m[idx])}"
        elif key == "normal_med_err":
            assert _same_bits(m[idx], r32[0][key]), f"{what}: median {float(m[idx])!r} vs {float(r32[0][key])!r}"
        else:
            _check_value(m[idx], r64[0][key], r32[0][key], f"{what} {key}")
    assert m[13:].tolist() == [0.0, 0.0, 0.0] and c[6:].tolist() == [0, 0]
    return m, c, s


# ---- shapes ----------------------------------------------------------------------------------------------------------------------

SHAPES = [(1, 1), (1, 150), (150, 1), (3, 5),            # one pixel, one row, one column, fewer elements than a wave
          (31, 33), (32, 32), (25, 41),                  # 1023, 1024, 1025 pixels: the sweep's span and one either side
          (15, 91), (2, 683),                            # 4095 and 4098 elements: either side of the span of rounds two and three
          (513, 512)]                                    # 257 workgroups: a second trip of the fold
assert [h * w for h, w in SHAPES[4:7]] == [SPAN - 1, SPAN, SPAN + 1] and [3 * h * w for h, w in SHAPES[7:9]] == [HSPAN - 1, HSPAN + 2]
assert (SHAPES[-1][0] * SHAPES[-1][1] + SPAN - 1) // SPAN > FOLD and {3 * h * w % 4 for h, w in SHAPES} == {0, 1, 2, 3}


@pytest.mark.parametrize("H,W", SHAPES)
def test_shapes_match_the_restatement(dns, H, W):
    f = _frame(H, W)
    r = _restated_frame(H, W)
    m, c, _ = _check(f, PAIRS, f"{H}x{W}", ref=(r[torch.float32], r[torch.float64]))
    if H * W >= 1024:
        assert 0 < int(c[1]) < int(c[2]) < int(c[3]) < int(c[0]) < H * W          # the mask and every threshold select and reject


@pytest.mark.parametrize("pairs", [("rgb",), ("depth",), ("normal",)])
def test_each_pair_alone(dns, pairs):
    """The same numbers as with all three pairs given, bit for bit; the other entries nan / 0."""
    from dn_splatter_amd import torch_metrics as tm

    H, W = 45, 70
    f = _frame(H, W)
    m, c, s = _check(f, pairs, f"{pairs[0]} alone")
    m3, c3, s3 = _hip(f)
    keys = {"rgb": tm.RGB_KEYS, "depth": tm.DEPTH_KEYS, "normal": tm.NORMAL_KEYS}[pairs[0]]
    for k in keys:
        assert _same_bits(m[tm.METRIC_INDEX[k]], m3[tm.METRIC_INDEX[k]]), k
    for k in range(tm.METRIC_SUMS):
        assert SUM_PAIR[k] != pairs[0] or float(s[k]) == float(s3[k])


def test_both_normal_layouts_give_the_same_bits(dns):
    H, W = 33, 130
    f = _frame(H, W, 1)
    a, b = _hip(f, layout="hwc"), _hip(f, layout="chw")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    _check(f, PAIRS, "chw", layout="chw")


@pytest.mark.parametrize("H,W", [(15, 91), (45, 70)])
def test_images_off_a_16_byte_boundary_give_the_same_bits(dns, H, W):
    """Rounds two and three read float4 where both normal images start on 16 bytes and single floats where not: the same bits."""
    f = _frame(H, W)
    a, b = _hip(f), _hip(f, unaligned=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert not bool(torch.isnan(a[0][:13]).any())


def test_two_calls_give_the_same_bits(dns):
    H, W = SHAPES[-1]
    f = _frame(H, W)
    a, b = _hip(f), _hip(f)
    assert not bool(torch.isnan(a[0][:13]).any())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_identical_images(dns):
    """Prediction == ground truth: every difference is 0 (ONE bin in every round), mse 0, psnr inf, a1 = a2 = a3 = 1."""
    from dn_splatter_amd import torch_metrics as tm

    H, W = 50, 70
    m, c, s = _check(_frame(H, W, 0, True), PAIRS, "identical")
    ix = tm.METRIC_INDEX
    assert float(m[ix["rgb_mse"]]) == 0.0 and float(m[ix["rgb_psnr"]]) == float("inf") and float(m[ix["normal_med_err"]]) == 0.0
    assert float(m[ix["depth_a1"]]) == 1.0 and float(m[ix["depth_rmse_log"]]) == 0.0 and int(c[1]) == int(c[0]) > 0


@pytest.mark.parametrize("H,W", inputs.FIXTURE_FRAMES)
def test_fixture_frames_equal_the_reference(dns, H, W):
    """The reference's stored outputs: the median exactly, the rest within VALUE_TOL (the reference's own fp32 sums are inside it)."""
    import os

    import numpy as np
    from dn_splatter_amd import torch_metrics as tm

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_metrics.npz"))
    f = inputs.fixture_frame(g, H, W)
    m, _, _ = _check(f, ("depth", "normal"), f"fixture {H}x{W}")
    pre = f"f{H}x{W}_"
    for k, want in zip(tm.DEPTH_KEYS, g[pre + "depth"]):
        assert abs(float(m[tm.METRIC_INDEX[k]]) - float(want)) <= VALUE_TOL * abs(float(want)), (k, float(m[tm.METRIC_INDEX[k]]), want)
    for k, want in zip(tm.NORMAL_KEYS[:3], g[pre + "normal"][:3]):
        assert abs(float(m[tm.METRIC_INDEX[k]]) - float(want)) <= VALUE_TOL * abs(float(want)), (k, float(m[tm.METRIC_INDEX[k]]), want)
    assert _same_bits(m[tm.METRIC_INDEX["normal_med_err"]], float(g[pre + "normal"][3]))


# ---- the explicit edge vectors -----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", sorted(inputs.DEPTH_EDGES))
def test_depth_edges(dns, name):
    """A zero, a negative, a nan prediction; nothing above the tolerance; a ground truth AT the tolerance; t exactly at a threshold."""
    pred, gt = inputs.DEPTH_EDGES[name]
    f = dict(depth=pred.reshape(1, -1, 1), gt_depth=gt.reshape(1, -1, 1))
    _check(f, ("depth",), name)


@pytest.mark.parametrize("name", sorted(inputs.NORMAL_EDGES))
def test_normal_edges(dns, name):
    pred, gt = inputs.NORMAL_EDGES[name]
    f = dict(normal=pred[0].permute(1, 2, 0).contiguous(), gt_normal=gt[0].permute(1, 2, 0).contiguous())
    _check(f, ("normal",), name)


# ---- the selection ---------------------------------------------------------------------------------------------------------------

SEL_P = 1500            # 4500 values: more than one workgroup in every round (the sweep's span is 1024 pixels, the rounds' 4096 values)


def _median_case(values):
    """The kernel's median and nan count for a normal pair whose 3 P differences |0 - pred| are exactly ``values`` (float32 [3 P])."""
    n = values.numel()
    assert n % 3 == 0
    f = dict(normal=values.reshape(1, n // 3, 3).clone(), gt_normal=torch.zeros(1, n // 3, 3))
    m, c, _ = _hip(f, ("normal",))
    want = torch.median(torch.abs(f["gt_normal"] - f["normal"]))                # float32, on the host
    got = m[12]
    assert _same_bits(got, want), f"median {float(got)!r} (bits {int(got.view(torch.int32)):#x}) vs torch.median {float(want)!r}"
    assert int(c[5]) == int(torch.isnan(values).sum())
    return got


def _bits(ints):
    return torch.tensor(ints, dtype=torch.int32).view(torch.float32)


def test_selection_all_differences_equal(dns):
    assert float(_median_case(torch.full((3 * SEL_P,), 0.3))) == float(torch.tensor(0.3))


@pytest.mark.parametrize("n", [3 * SEL_P, 3 * SEL_P + 3])       # an even and an odd count
@pytest.mark.parametrize("where", ["last_of_lower", "first_of_upper"])
def test_selection_two_values_at_the_rank(dns, n, where):
    """The rank (n - 1) // 2 falls on the last element of the lower group, or on the first of the upper."""
    k = (n - 1) // 2
    n_low = k + 1 if where == "last_of_lower" else k
    lo, hi = 0.25, 0.2500001
    v = torch.cat([torch.full((n_low,), lo), torch.full((n - n_low,), hi)])
    v = v[torch.randperm(n, generator=torch.Generator().manual_seed(n))]
    assert float(_median_case(v)) == float(torch.tensor(lo if where == "last_of_lower" else hi))


def test_selection_values_differ_in_the_lowest_nine_bits_only(dns):
    g = torch.Generator().manual_seed(9)
    low = torch.randint(0, 512, (3 * SEL_P,), generator=g, dtype=torch.int32)
    _median_case(_bits((0x3E800000 + low).tolist()))


@pytest.mark.parametrize("n", [3 * SEL_P, 3 * SEL_P + 3])
def test_selection_across_the_exponent_range(dns, n):
    """0, a denormal, the smallest normal, ..., inf: non-negative floats order as their bit patterns."""
    pool = _bits([0x00000000, 0x00000001, 0x00000400, 0x00800000, 0x0DA24260, 0x3A83126F, 0x3F800000, 0x60AD78EC, 0x7F7FFFFF, 0x7F800000])
    g = torch.Generator().manual_seed(n)
    _median_case(pool[torch.randint(0, pool.numel(), (n,), generator=g)])
    # the denormal itself is the median
    v = torch.cat([torch.zeros(n // 2 - 5), pool[1].expand(11), torch.ones(n - n // 2 - 6)])
    assert int(_median_case(v[torch.randperm(n, generator=g)]).view(torch.int32)) == 1


@pytest.mark.parametrize("which", ["first", "last"])
def test_selection_rank_in_the_first_or_last_populated_bin(dns, which):
    n = 3 * SEL_P
    g = torch.Generator().manual_seed(3)
    if which == "first":       # most values in the lowest populated bin of every round
        v = torch.cat([_bits([0x00000000] * (n - 40)), torch.rand(40, generator=g) + 0.5])
    else:                      # most values in the highest: inf
        v = torch.cat([torch.rand(40, generator=g), _bits([0x7F800000] * (n - 40))])
    got = _median_case(v[torch.randperm(n, generator=g)])
    assert float(got) == (0.0 if which == "first" else float("inf"))


@pytest.mark.parametrize("at", [0, 3 * SEL_P // 2, 3 * SEL_P - 1])
def test_selection_single_nan(dns, at):
    v = torch.rand(3 * SEL_P, generator=torch.Generator().manual_seed(at))
    v[at] = float("nan")
    assert bool(torch.isnan(_median_case(v)))


# ---- the public interface --------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=1)
def _rendered():
    import dn_splatter_amd as dns
    from dn_splatter_amd import synthetic

    W, H = 96, 64
    gp = synthetic.make_gauss_params(2000, sh_rest_std=0.1, seed=3)
    params = {k: v.detach().to(DEV) for k, v in gp.items()}
    with torch.no_grad():
        out = dns.DNSplatterRenderer(params, fused=True).get_outputs(synthetic.orbit_camera(1, width=W, height=H, focal=60.0).to(DEV))
    f = _frame(H, W)
    batch = {"image": f["gt_rgb"].to(DEV), "sensor_depth": f["gt_depth"].double().to(DEV), "normal": f["gt_normal"].to(DEV),
             "mask": (torch.rand(H, W, 1, generator=torch.Generator().manual_seed(1)) > 0.2).float().to(DEV)}
    return {k: out[k].detach() for k in ("rgb", "depth", "normal")}, batch


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("with_normal", [False, True])
@pytest.mark.parametrize("with_depth", [False, True])
def test_image_metrics_keys_and_values(dns, with_depth, with_normal, with_mask):
    """Exactly the reference's keys for the batch at hand; the values are the restatement's on the same tensors; the dict of floats is
    the dict of tensors; nothing on the path synchronises with the host."""
    from dn_splatter_amd import torch_metrics as tm

    out, full = _rendered()
    batch = {k: v for k, v in full.items() if k == "image" or (k == "sensor_depth" and with_depth) or (k == "normal" and with_normal)
             or (k == "mask" and with_mask)}
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = dns.image_metrics(out, batch)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    want_keys = {"rgb_mse", "rgb_psnr", "rgb_ssim"} | (set(tm.DEPTH_KEYS) if with_depth else set()) | (set(tm.NORMAL_KEYS) if with_normal else set())
    assert set(got) == want_keys
    assert all(v.dim() == 0 and v.is_cuda for v in got.values())
    as_floats = dns.image_metrics_dict(out, batch)
    assert set(as_floats) == want_keys and all(isinstance(v, float) for v in as_floats.values())
    assert all(_same_bits(as_floats[k], got[k].cpu()) for k in want_keys)
    cpu = lambda d: {k: v.cpu() for k, v in d.items()}      # noqa: E731
    r32 = tm.image_metrics(cpu(out), cpu(batch))
    r64 = tm.image_metrics({k: v.double() for k, v in cpu(out).items()}, {k: v.double() for k, v in cpu(batch).items()})
    for k in want_keys - {"rgb_ssim"}:
        if k == "normal_med_err":
            assert _same_bits(got[k].cpu(), r32[k]), k
        else:
            _check_value(got[k].cpu(), r64[k], r32[k], k)
    assert 0.0 < float(got["rgb_ssim"]) < 1.0
    assert set(dns.image_metrics(out, batch, ssim=False)) == want_keys - {"rgb_ssim"}


def test_image_metrics_refuses_other_sizes(dns):
    out, batch = _rendered()
    small = {"image": batch["image"], "sensor_depth": batch["sensor_depth"][:32, :48]}
    with pytest.raises(ValueError, match=r"\(64, 96, 1\).*\(32, 48, 1\)"):
        dns.image_metrics(out, small)
    with pytest.raises(ValueError, match=r"\(64, 96, 3\).*\(32, 48, 3\)"):
        dns.image_metrics(out, {"image": batch["image"], "normal": batch["normal"][:32, :48]})


def test_drop_in_modules(dns):
    """DepthMetrics / NormalMetrics / PSNR as the model calls them (dn_model.py:854, :882-884, :907-910); NormalMetrics reads the
    permuted view of an [H,W,3] image in place and gives the bits it gives on a contiguous copy."""
    from dn_splatter_amd import fused_metrics as fm, torch_metrics as tm

    H, W = 45, 70
    f = {k: v.to(DEV) for k, v in _frame(H, W).items()}
    r32, r64 = _restated(_frame(H, W), PAIRS, torch.float32)[0], _restated(_frame(H, W), PAIRS, torch.float64)[0]
    chw = lambda t: t.permute(2, 0, 1).unsqueeze(0)      # noqa: E731
    d = fm.DepthMetrics()(f["depth"].permute(2, 0, 1), f["gt_depth"].permute(2, 0, 1))
    assert len(d) == 7
    for k, v in zip(tm.DEPTH_KEYS, d):
        _check_value(v.cpu(), r64[k], r32[k], "DepthMetrics " + k)
    view = fm.NormalMetrics()(chw(f["normal"]), chw(f["gt_normal"]))
    copy = fm.NormalMetrics()(chw(f["normal"]).contiguous(), chw(f["gt_normal"]).contiguous())
    assert len(view) == 4 and all(_same_bits(a.cpu(), b.cpu()) for a, b in zip(view, copy))
    for k, v in zip(tm.NORMAL_KEYS[:3], view):
        _check_value(v.cpu(), r64[k], r32[k], "NormalMetrics " + k)
    assert _same_bits(view[3].cpu(), r32["normal_med_err"])
    p = fm.PSNR()(chw(f["gt_rgb"]), chw(f["rgb"]))
    _check_value(p.cpu(), r64["rgb_psnr"], r32["rgb_psnr"], "PSNR")
    # another tolerance; tensors of any (equal) shape
    d2 = fm.DepthMetrics(tolerance=3.0)(f["depth"].reshape(-1), f["gt_depth"].reshape(-1))
    w2 = tm.depth_metrics(_frame(H, W)["depth"].double(), _frame(H, W)["gt_depth"].double(), 3.0)
    for k, v, w in zip(tm.DEPTH_KEYS, d2, w2):
        _check_value(v.cpu(), w, w.float(), "DepthMetrics(3.0) " + k)
    with pytest.raises(NotImplementedError):
        fm.NormalMetrics()(torch.zeros(2, 3, 4, 5, device=DEV), torch.zeros(2, 3, 4, 5, device=DEV))


def test_image_metrics_casts_other_dtypes(dns):
    """A float64 image / normal map in the batch (a dataparser's dtype) is cast to float32 like the sensor depth: the same bits as for
    the float32 batch, and still no synchronisation."""
    out, batch = _rendered()
    want = dns.image_metrics(out, batch, ssim=False)
    other = dict(batch, image=batch["image"].double(), normal=batch["normal"].double(), sensor_depth=batch["sensor_depth"].float(),
                 mask=batch["mask"] > 0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = dns.image_metrics(out, other, ssim=False)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert set(got) == set(want) and all(v.dtype == torch.float32 for v in got.values())
    assert all(_same_bits(got[k].cpu(), want[k].cpu()) for k in want), {k: (float(got[k]), float(want[k])) for k in want}


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 1, 7, 5), (2, 17), (1, 3, 7, 5)])       # 1, 35, 34 and 105 elements: all of n % 3
def test_psnr_takes_any_shape(dns, shape):
    """The PSNR drop-in on tensors that are no three-channel images (torchmetrics' module takes any shape): the mean is over the true
    element count."""
    from dn_splatter_amd import fused_metrics as fm, torch_metrics as tm

    g = torch.Generator().manual_seed(sum(shape))
    gt, pred = torch.rand(*shape, generator=g), torch.rand(*shape, generator=g)
    got = fm.PSNR()(gt.to(DEV), pred.to(DEV))
    assert got.dim() == 0 and got.is_cuda and got.dtype == torch.float32
    _check_value(got.cpu(), tm.psnr(gt.double(), pred.double()), tm.psnr(gt, pred), f"PSNR {shape}")
