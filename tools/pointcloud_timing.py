"""The per-frame tail of the mesh exporter at 1920 x 1080, 20 000 samples per frame (2 M points over 100 frames), on one rendered
frame of the C2 scene (1 M Gaussians): (a) torch_export.frame_points on the device — the PyTorch restatement that
tests/golden/reference_export.npz pins to the reference, with its conv-free edge map, its nonzero + CPU randperm + index upload, its
back-projection of all pixels and its gathers — against (b) export.OrientedPointCloud.add_frame on the three dnsplat_* entry points;
each with the depth-edge filter off and on (10 dilation rounds).

Per configuration: median ms per frame (host clock around a device synchronise, regions of several frames); then, from one traced frame
in a run of its own, the number of kernel launches (torch's profiler) and of host synchronisations (torch's synchronisation check in
"warn" mode).

    python tools/pointcloud_timing.py        # every configuration in a child process under `timeout -k 10`; stops at the first failure

The output is meant to be kept as profiles/pointcloud_export.txt.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, W, H, FOCAL = 1_000_000, 1920, 1080, 1200.0          # bench.py's C2
SAMPLES = 20_000
CONFIGS = [("hip", False), ("torch", False), ("hip", True), ("torch", True)]
CASE_SECONDS = 150
REGION_SECONDS = 0.25
CALIBRATION_FRAMES = 5


def rendered_frame():
    import torch

    import dn_splatter_amd as dns
    from dn_splatter_amd import synthetic

    gp = synthetic.make_gauss_params(N, sh_rest_std=0.1, seed=0, device="cuda:0")
    cam = synthetic.orbit_camera(0, n_views=8, width=W, height=H, focal=FOCAL).to("cuda:0")
    renderer = dns.DNSplatterRenderer({k: v.detach() for k, v in gp.items()})
    renderer.training = False
    with torch.no_grad():
        out = renderer.get_outputs(cam)
    out = {k: out[k].detach().clone() for k in ("depth", "rgb", "surface_normal")}
    torch.cuda.synchronize()
    del renderer, gp
    torch.cuda.empty_cache()
    return out, cam


def one(variant, filter_edges, regions, warmup, count=False):
    import torch

    assert torch.cuda.is_available(), "needs the GPU: nothing is timed on a CPU"
    from dn_splatter_amd import export, torch_export

    out, cam = rendered_frame()
    depth = out["depth"]
    print(f"\n{variant}, filter_edges={filter_edges}: {W} x {H}, {SAMPLES} samples per frame; depth is nonzero at "
          f"{float((depth != 0).float().mean()):.3f} of the pixels", flush=True)
    if variant == "hip":
        cloud = export.OrientedPointCloud(SAMPLES, "cuda:0")
        seeds = iter(range(10 ** 9))

        def frame():
            cloud.state.zero_()                              # the same rows again: the buffers of one frame are enough
            cloud.add_frame(out, cam, samples_per_frame=SAMPLES, filter_edges=filter_edges, seed=next(seeds))
    else:
        def frame():
            return torch_export.frame_points(out, cam, SAMPLES, filter_edges=filter_edges)

    for _ in range(warmup):
        frame()
    torch.cuda.synchronize()
    if variant == "hip":
        rows, overflow, bad = cloud.state.tolist()
        assert (overflow, bad) == (0, 0), (rows, overflow, bad)
    else:
        res = frame()
        rows = 0 if res is None else len(res[0])
    print(f"  rows per frame: {rows}", flush=True)
    if count:
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                frame()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        syncs = sum("synchroniz" in str(w.message).lower() for w in seen)
        torch.cuda.synchronize()
        print(f"  host synchronisations per frame: {syncs} ({'synchronised' if syncs else 'did not synchronise'})", flush=True)
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            frame()
            torch.cuda.synchronize()
        kernels = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower()]
        print(f"  kernel launches per frame: {len(kernels) if kernels else 'not measured (the profiler recorded no device activity)'}", flush=True)
        return
    t = time.perf_counter()
    for _ in range(CALIBRATION_FRAMES):
        frame()
    torch.cuda.synchronize()
    per = (time.perf_counter() - t) / CALIBRATION_FRAMES
    iters = max(CALIBRATION_FRAMES, min(2000, round(REGION_SECONDS / per)))
    ms = []
    for _ in range(regions):
        t = time.perf_counter()
        for _ in range(iters):
            frame()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3 / iters)
    print(f"  median {statistics.median(ms):8.4f} ms / frame   min {min(ms):8.4f}   max {max(ms):8.4f}   ({regions} regions of {iters} frames)",
          flush=True)


def time_all(regions, warmup):
    print("oriented points of one frame: edge filter (optional), sampling, back-projection, colours, world normals; "
          "time per frame by the host clock around a device synchronise", flush=True)
    # the timings first, then one traced frame of each configuration (launches, synchronisations) in children of their own
    for extra in ([], ["--count"]):
        for variant, filter_edges in CONFIGS:
            # check=True: a failure raises here and nothing more is started on the device after it
            subprocess.run(["timeout", "-k", "10", str(CASE_SECONDS), sys.executable, os.path.abspath(__file__), "--one", variant,
                            str(int(filter_edges)), "--regions", str(regions), "--warmup", str(warmup)] + extra, check=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--one", nargs=2, metavar=("VARIANT", "FILTER_EDGES"))
    ap.add_argument("--count", action="store_true", help="with --one: count launches and synchronisations of one frame instead of timing")
    a = ap.parse_args()
    if a.one:
        import torch

        if a.one == ["hip", "0"] and not a.count:
            print(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
        one(a.one[0], bool(int(a.one[1])), a.regions, a.warmup, a.count)
    else:
        time_all(a.regions, a.warmup)
