"""Point-cloud normals at the sizes the reference runs them at.

  frame   one 1920 x 1080 depth frame rendered from the C2 scene (1 M Gaussians, the benchmark's orbit, tools/tsdf_time.py's frames),
          back-projected as scripts/depth_to_normal.py does: the back-projection and the removal of the pixels without depth (PyTorch),
          the index build, ``dnsplat_cloud_normals`` at knn = 200 (KDTreeSearchParamKNN(200)) and at knn = 30, radius = 0.1
          (KDTreeSearchParamHybrid), with and without the optional outputs, the whole ``depth_normals``; then the same frame with 1 %
          more points scattered through its box, for the price of the isolated points
  sfm     1 M SfM-like points — a thin shell of radius 2 (sigma 0.01) with 1 % of the points scattered through a cube of side 12 — at the
          dataparsers' hybrid search (0.1, 30): the index build, the call, the whole ``points3D_normals``
  cpu     what a ROCm box has instead of Open3D: scipy's ``cKDTree`` build plus ``query(k, workers=16)`` and numpy's ``cov`` sums and
          ``eigh`` on CPU_ROWS points of a seeded permutation of the same clouds — a stated SUBSAMPLE (a sparser cloud, the same number
          of neighbours per row)

Each device line also gives the widest ring a query reached and the most selections one query ran.  Device times: HIP events around the
call, the median of --reps repetitions (10) after one warm-up, the count stated on every line.  Nothing here asserts a speed.

    python tools/normals_time.py        # each part in a child process under `timeout -k 10`; stops at the first failure

The output is meant to be kept as profiles/normals.txt.
"""
import argparse
import ctypes
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

N_GAUSS, W, H, FOCAL = 1_000_000, 1920, 1080, 1200.0
N_SFM, SFM_SCATTER = 990_000, 10_000
CPU_ROWS = 200_000
CASES = [["gpu", "frame"], ["gpu", "sfm"], ["cpu", "frame"], ["cpu", "sfm"]]
CASE_SECONDS = 500


def timed(fn, reps):
    """(median ms, min ms, max ms, the last result, the repetitions)"""
    import torch

    out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1], out, reps


def line(what, t, extra=""):
    print(f"  {what:<92s} {t[0]:10.3f} ms   (median of {t[4]}; min {t[1]:.3f}, max {t[2]:.3f}){extra}", flush=True)


def the_frame(dev):
    """(depth float32 [H,W] on the device, the OpenCV camera-to-world 4x4 float64 on the host) of the orbit's first camera"""
    import numpy as np
    import torch

    import dn_splatter_amd as dns
    from dn_splatter_amd import synthetic

    gp = synthetic.make_gauss_params(N_GAUSS, sh_rest_std=0.1, seed=0, device=dev)
    camera = synthetic.orbit_camera(0, n_views=8, width=W, height=H, focal=FOCAL).to(dev)
    with torch.no_grad():
        out = list(dns.DNSplatterRenderer(gp, fused=True).get_outputs_batch([camera], max_batch=1))[0]
    depth = out["depth"].detach()[..., 0].float().contiguous()
    c2w = np.eye(4)
    c2w[:3] = camera.camera_to_worlds[0].double().cpu().numpy()
    return depth, c2w @ np.diag([1.0, -1.0, -1.0, 1.0])


def frame_cloud(dev):
    import torch

    from dn_splatter_amd import torch_normals

    depth, c2w = the_frame(dev)
    world = torch_normals.backproject(depth, FOCAL, FOCAL, W / 2.0, H / 2.0, c2w).float()
    return depth, c2w, world[torch_normals.valid_depth(depth).reshape(-1)].contiguous()


def sfm_cloud():
    import _cloud_filter_inputs as inputs

    return inputs.cloud(0, N_SFM, SFM_SCATTER) * 2.0


def scattered(points, share=0.01, seed=3):
    import torch

    lo, hi = points.min(dim=0).values, points.max(dim=0).values
    g = torch.Generator().manual_seed(seed)
    extra = torch.rand(int(points.shape[0] * share), 3, generator=g).to(points.device) * (hi - lo) + lo
    return torch.cat([points, extra]).contiguous()


def kernel_lines(points, knn, radius, reps, label):
    """The index build and the one launch, alone and with every optional output."""
    import torch

    from dn_splatter_amd import _lib
    from dn_splatter_amd._ops import _cloud_normals_args, _stream
    from dn_splatter_amd.density import KnnIndex

    dev, N, L = points.device, points.shape[0], _lib.lib()
    t = timed(lambda: KnnIndex(points), reps)
    line(f"{label}: dnsplat_knn_build, N = {N} (grid {L.dnsplat_knn_grid_dim(N)}^3)", t)
    index = t[3]
    search = torch.zeros(4, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    normals = torch.empty(N, 3, dtype=torch.float64, device=dev)
    a = _cloud_normals_args(points, index.buffer, knn, radius, (0.0, 0.0, 0.0), search, normals, status)
    t = timed(lambda: _lib.run("dnsplat_cloud_normals", L.dnsplat_cloud_normals, ctypes.byref(a), _stream()), reps)
    ring, selections = search[:2].tolist()
    line(f"{label}: dnsplat_cloud_normals, knn = {knn}, radius = {radius}, normals alone (1 launch)", t,
         f"   {1e3 * t[0] / N:.3f} us per point; widest ring {ring}, most selections {selections}, status {int(status)}")
    cov = torch.empty(N, 6, dtype=torch.float64, device=dev)
    nbr = torch.empty(N, knn, dtype=torch.int32, device=dev)
    count = torch.empty(N, dtype=torch.int32, device=dev)
    a = _cloud_normals_args(points, index.buffer, knn, radius, (0.0, 0.0, 0.0), search, normals, status, cov, nbr, count)
    t = timed(lambda: _lib.run("dnsplat_cloud_normals", L.dnsplat_cloud_normals, ctypes.byref(a), _stream()), reps)
    line(f"{label}: the same with covariance, neighbors ({4 * N * knn / 2 ** 20:.0f} MiB) and count", t,
         f"   mean count {float(count.double().mean()):.1f}, rows with fewer than 3: {int((count < 3).sum())}")


def gpu_frame(reps):
    import torch

    from dn_splatter_amd import normals, torch_normals

    dev = "cuda:0"
    depth, c2w, cloud = frame_cloud(dev)
    print(f"\ngpu frame: {W} x {H} depth of the C2 scene ({N_GAUSS} Gaussians), {cloud.shape[0]} pixels with depth "
          f"({100 * cloud.shape[0] / (W * H):.1f} %); device {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {reps} repetitions", flush=True)
    line("back-projection of every pixel and removal of those without depth (PyTorch)", timed(
        lambda: torch_normals.backproject(depth, FOCAL, FOCAL, W / 2.0, H / 2.0, c2w).float()[torch_normals.valid_depth(depth).reshape(-1)], reps))
    kernel_lines(cloud, 200, None, reps, "frame")
    kernel_lines(cloud, 30, 0.1, reps, "frame")
    line("depth_normals: back-projection, index build, the launch at knn = 200, the scatter, the host reads", timed(
        lambda: normals.depth_normals(depth, FOCAL, FOCAL, W / 2.0, H / 2.0, c2w), reps))
    kernel_lines(scattered(cloud), 200, None, reps, "frame + 1 % scattered")


def gpu_sfm(reps):
    import torch

    from dn_splatter_amd import normals

    dev = "cuda:0"
    cloud = sfm_cloud().to(dev)
    print(f"\ngpu sfm: {cloud.shape[0]} points, a shell of radius 2 (sigma 0.01) with {SFM_SCATTER} scattered; device "
          f"{torch.cuda.get_device_name(0)}; {reps} repetitions", flush=True)
    kernel_lines(cloud, 30, 0.1, reps, "sfm")
    line("points3D_normals: index build, the launch, normalisation, float32", timed(lambda: normals.points3D_normals(cloud), reps))


def cpu_case(which):
    import numpy as np
    import torch
    from scipy.spatial import cKDTree

    if which == "frame":
        cloud, knn, radius = frame_cloud("cuda:0")[2].cpu(), 200, None
    else:
        cloud, knn, radius = sfm_cloud(), 30, 0.1
    rows = min(cloud.shape[0], CPU_ROWS if knn <= 30 else CPU_ROWS // 2)       # [rows, knn, 3] float64 temporaries
    perm = torch.randperm(cloud.shape[0], generator=torch.Generator().manual_seed(1))[:rows]
    p = cloud[perm].double().numpy()
    t0 = time.perf_counter()
    tree = cKDTree(p)
    build = time.perf_counter() - t0
    t0 = time.perf_counter()
    d, idx = tree.query(p, k=knn, workers=16, **({} if radius is None else {"distance_upper_bound": radius}))
    query = time.perf_counter() - t0
    t0 = time.perf_counter()
    kept = np.isfinite(d)
    q = np.where(kept[..., None], p[np.where(kept, idx, 0)], 0.0)
    n = np.maximum(kept.sum(axis=1), 1)[:, None]
    dlt = np.where(kept[..., None], q - q.sum(axis=1, keepdims=True) / n[..., None], 0.0)
    cov = np.einsum("nka,nkb->nab", dlt, dlt) / n[..., None]
    moments = time.perf_counter() - t0
    t0 = time.perf_counter()
    np.linalg.eigh(cov)
    eigh = time.perf_counter() - t0
    print(f"\ncpu {which}: a SUBSAMPLE, {rows} of {cloud.shape[0]} points (a seeded permutation), knn = {knn}, radius = {radius}: scipy cKDTree build "
          f"{build:.2f} s, query(k = {knn}, workers = 16) {query:.2f} s, the covariances in numpy {moments:.2f} s, numpy eigh {eigh:.2f} s: "
          f"{1e6 * (build + query + moments + eigh) / rows:.2f} us per point ({os.cpu_count()} CPUs visible, 16 used by the query)", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--one", nargs="+")
    ap.add_argument("--cases", default="gpu,cpu")
    a = ap.parse_args()
    if a.one:
        {("gpu", "frame"): lambda: gpu_frame(a.reps), ("gpu", "sfm"): lambda: gpu_sfm(a.reps), ("cpu", "frame"): lambda: cpu_case("frame"),
         ("cpu", "sfm"): lambda: cpu_case("sfm")}[tuple(a.one)]()
    else:
        print(f"point-cloud normals: device times by HIP events, the median of {a.reps} repetitions after one warm-up", flush=True)
        for case in CASES:
            if case[0] not in a.cases.split(","):
                continue
            # check=True: a failure raises here and nothing more is started on the device after it
            subprocess.run(["timeout", "-k", "10", str(CASE_SECONDS), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--one"] + case,
                           check=True)
