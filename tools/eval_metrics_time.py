"""Time of the evaluation metrics of one frame (dn_model.py:809-926 less SSIM and LPIPS) on the GPU, three things in one process:

  torch    torch_metrics.image_metrics on device tensors: the reference's operations, boolean-mask gathers and one .item() per result;
  hip      image_metrics_dict(ssim=False): one dnsplat_eval_metrics call and ONE device-to-host copy;
  kernels  the dnsplat_eval_metrics call alone on prepared buffers (no host read), for the GB/s figure;
  ags      dnsplat_ags_normal_loss (mode 0, both gradients and the selection written) on the same frame: the yardstick for a streaming
           kernel of this library.

Inputs: (a) uniform random images; (b) the prediction = the ground truth + noise of 1e-3, where nearly all |g - p| share a few
histogram bins; (c) the prediction = the ground truth: every |g - p| in ONE bin of every round.  HIP events around each iteration, 20 warm-up + 100 timed iterations, median and p10 / p90.

    python tools/eval_metrics_time.py [--out profiles/eval_metrics.txt] [--note TEXT]

DNSPLAT_LIB=<path> times another build of the library (for instance metrics.hip compiled with -DMT_PEEL=0); --note goes into the
header of the output so that the file says which build it was.
"""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = ((1600, 1200), (1920, 1080))
WARMUP, TIMED = 20, 100
METRIC_BYTES = 56          # per pixel, read once: 2 x (3 + 1 + 3) floats
MEDIAN_BYTES = 48          # per pixel: rounds two and three read the two normal images again
AGS_BYTES = 60             # ags.hip: 36 B read, 24 B written per pixel


def inputs(W, H, kind, dev):
    g = torch.Generator().manual_seed(W + H)
    r = lambda *s: torch.rand(*s, generator=g)      # noqa: E731
    gt_rgb, gt_normal, gt_depth = r(H, W, 3), r(H, W, 3), r(H, W, 1) * 6 + 0.05
    if kind == "random":
        rgb, normal, depth = r(H, W, 3), r(H, W, 3), r(H, W, 1) * 6 + 0.05
    elif kind == "identical":
        rgb, normal, depth = gt_rgb.clone(), gt_normal.clone(), gt_depth.clone()
    else:
        rgb, normal = (gt_rgb + 1e-3 * torch.randn(H, W, 3, generator=g)).clamp(0, 1), (gt_normal + 1e-3 * torch.randn(H, W, 3, generator=g)).clamp(0, 1)
        depth = gt_depth + 1e-3 * torch.randn(H, W, 1, generator=g)
    out = {"rgb": rgb.to(dev), "depth": depth.to(dev), "normal": normal.to(dev)}
    batch = {"image": gt_rgb.to(dev), "sensor_depth": gt_depth.to(dev), "normal": gt_normal.to(dev)}
    return out, batch


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(TIMED):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], ms[len(ms) // 10], ms[(9 * len(ms)) // 10]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "eval_metrics.txt"))
    ap.add_argument("--note", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_metrics_time.py measures on the GPU; there is none here")
    import dn_splatter_amd as dns
    from dn_splatter_amd import _lib, fused_metrics as fm, torch_metrics as tm
    from dn_splatter_amd._ops import _eval_metrics_args
    from dn_splatter_amd.fused_loss import AGS_LAYOUT

    dev = torch.device("cuda:0")
    L = _lib.lib()
    lines = ["evaluation metrics of one frame (depth, normal, mse / psnr; no SSIM, no LPIPS); HIP events around each iteration, "
             f"{WARMUP} warm-up + {TIMED} timed, median [p10 .. p90] in ms",
             f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; library {_lib.LIB_PATH.name}" + (f"; {args.note}" if args.note else "")]
    for W, H in SIZES:
        for kind in ("random", "near-identical", "identical"):
            out, batch = inputs(W, H, kind, dev)
            P = W * H
            ref = tm.image_metrics(out, batch)
            got = dns.image_metrics_dict(out, batch, ssim=False)
            worst = max(abs(got[k] - ref[k]) / max(abs(ref[k]), 1e-30) for k in ref if ref[k] == ref[k] and abs(ref[k]) != float("inf"))
            assert set(got) == set(ref) and worst < 1e-3, (worst, got, ref)
            assert got["normal_med_err"] == ref["normal_med_err"]
            t_torch = timed(lambda: tm.image_metrics(out, batch))
            t_hip = timed(lambda: dns.image_metrics_dict(out, batch, ssim=False))
            p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            # both kernels-alone figures through the C ABI: buffers and the argument struct prepared once, nothing allocated per call
            m_scratch = torch.empty(L.dnsplat_eval_metrics_scratch_bytes(W, H) // 8, dtype=torch.float64, device=dev)
            m_metrics = torch.empty(tm.METRIC_COUNT, dtype=torch.float32, device=dev)
            m_counts = torch.empty(tm.METRIC_COUNTS, dtype=torch.int64, device=dev)
            m_args = _eval_metrics_args(W, H, out["rgb"], batch["image"], out["depth"], batch["sensor_depth"], 0.1, out["normal"],
                                        batch["normal"], AGS_LAYOUT["hwc"], m_scratch, m_metrics, m_counts, None)
            t_kern = timed(lambda: _lib.check(L.dnsplat_eval_metrics(ctypes.byref(m_args), stream), "eval_metrics"))
            again = fm.eval_metrics(W, H, rgb=out["rgb"], gt_rgb=batch["image"], depth=out["depth"], gt_depth=batch["sensor_depth"],
                                    normal=out["normal"], gt_normal=batch["normal"])[0]
            assert torch.equal(m_metrics.view(torch.int32), again.view(torch.int32))
            scratch = torch.empty(L.dnsplat_ags_normal_scratch_bytes(W, H) // 8, dtype=torch.float64, device=dev)
            v_s, v_p = torch.empty(H, W, 3, device=dev), torch.empty(H, W, 3, device=dev)
            sel = torch.empty(3, H, W, dtype=torch.bool, device=dev)
            sums, count = torch.empty(2, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.int64, device=dev)
            t_ags = timed(lambda: _lib.check(L.dnsplat_ags_normal_loss(W, H, p(out["normal"]), p(batch["normal"]), p(out["rgb"]), 1, 0, 0.1,
                                                                       p(v_s), p(v_p), p(sel), p(scratch), p(sums), p(count), stream), "ags"))
            gbs = lambda b, t: b * P / (t[0] * 1e-3) / 1e9      # noqa: E731
            f = lambda t: f"{t[0]:8.4f} [{t[1]:.4f} .. {t[2]:.4f}]"      # noqa: E731
            lines += ["", f"{W} x {H}, {kind} (largest relative difference of a finite metric from the torch path {worst:.1e}; median equal)",
                      f"  torch    {f(t_torch)}    restatement on the device, {len(ref)} .item() reads",
                      f"  hip      {f(t_hip)}    image_metrics_dict(ssim=False), one read; {t_torch[0] / t_hip[0]:.1f} x faster",
                      f"  kernels  {f(t_kern)}    dnsplat_eval_metrics alone, prepared buffers: {gbs(METRIC_BYTES, t_kern):.0f} GB/s of the {METRIC_BYTES} B/pixel read once "
                      f"({gbs(METRIC_BYTES + MEDIAN_BYTES, t_kern):.0f} GB/s counting the median's two re-reads)",
                      f"  ags      {f(t_ags)}    dnsplat_ags_normal_loss: {gbs(AGS_BYTES, t_ags):.0f} GB/s of its {AGS_BYTES} B/pixel"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
