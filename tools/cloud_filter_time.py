"""The two point-cloud filters at the size the exporters produce: the synthetic thin shell of tests/_cloud_filter_inputs.py at 2 M points with
1 % outliers (a unit sphere's shell of thickness 0.01 plus 20 000 points scattered through a cube of side 6).

  gpu   the index build, ``dnsplat_cloud_neighbor_mean`` (20 neighbours), ``dnsplat_cloud_outlier_stats``, count + emit and the whole
        ``remove_statistical_outlier`` with its index build and host read; ``neighbor_mean`` again over the shell alone and over the
        shell with the outliers as QUERIES of the shell's index, for the share of the time that goes to the isolated points (the
        README's thin-shell note: a point far from the surface widens its search ring by ring); ``voxel_down_sample`` at voxel sizes 0.01
        and 0.1 with and without attributes, and its two calls
  cpu   what a ROCm box has instead: scipy's ``cKDTree`` build plus ``query(k=20, workers=16)`` and the moments in numpy, and a numpy
        ``unique`` + ``add.at`` down-sample, on the first CPU_ROWS points of a seeded permutation — a stated SUBSAMPLE where the cloud has more

Device times: HIP events around the call, median of the repetitions after one warm-up.  Nothing here asserts a speed.

    python tools/cloud_filter_time.py      # each part in a child process under `timeout -k 10`; stops at the first failure

The output is meant to be kept as profiles/cloud_filter.txt.
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

N_SHELL, N_OUT = 1_980_000, 20_000
CPU_ROWS = 500_000
NB, RATIO = 20, 2.0
CASES = [["gpu", "outlier"], ["gpu", "voxel"], ["cpu", "outlier"], ["cpu", "voxel"]]
CASE_SECONDS = 300


def the_cloud():
    import _cloud_filter_inputs as inputs

    return inputs.cloud(0, N_SHELL, N_OUT)


def timed(fn, reps):
    """(median ms, min ms, max ms, the last result)"""
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
    return ms[len(ms) // 2], ms[0], ms[-1], out


def line(what, t):
    print(f"  {what:<86s} {t[0]:9.3f} ms   (min {t[1]:.3f}, max {t[2]:.3f})", flush=True)


def gpu_outlier(reps):
    import torch

    from dn_splatter_amd import _lib, cloud_filter
    from dn_splatter_amd._ops import _cloud_outlier_args, _stream
    from dn_splatter_amd.density import KnnIndex

    dev = "cuda:0"
    points = the_cloud().to(dev)
    N = points.shape[0]
    L = _lib.lib()
    print(f"\ngpu outlier removal: N = {N} points ({N_SHELL} on the shell, {N_OUT} outliers), nb_neighbors = {NB}, std_ratio = {RATIO}; device "
          f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}; {reps} repetitions", flush=True)
    t = timed(lambda: KnnIndex(points), reps)
    line(f"dnsplat_knn_build (grid {L.dnsplat_knn_grid_dim(N)}^3)", t)
    index = t[3]
    scratch = torch.empty((L.dnsplat_cloud_outlier_scratch_bytes(N) + 7) // 8, dtype=torch.int64, device=dev)
    avg = torch.empty(N, dtype=torch.float64, device=dev)
    record = torch.empty(8, dtype=torch.float64, device=dev)
    a = _cloud_outlier_args(points, index.buffer, NB, RATIO, scratch, avg, record)
    run = lambda name: _lib.run(name, getattr(L, name), ctypes.byref(a), _stream())
    t_all = timed(lambda: run("dnsplat_cloud_neighbor_mean"), max(3, reps // 4))
    line("dnsplat_cloud_neighbor_mean, the whole cloud (1 launch)", t_all)
    line("dnsplat_cloud_outlier_stats (4 launches)", timed(lambda: run("dnsplat_cloud_outlier_stats"), reps))
    line("dnsplat_cloud_outlier_count (2 launches)", timed(lambda: run("dnsplat_cloud_outlier_count"), reps))
    stats = cloud_filter.OutlierStats(avg, record)
    n_kept = int(stats.n_kept)
    ind = torch.empty(n_kept, dtype=torch.int64, device=dev)
    a = _cloud_outlier_args(points, index.buffer, NB, RATIO, scratch, avg, record, ind)
    line("dnsplat_cloud_outlier_emit (1 launch)", timed(lambda: run("dnsplat_cloud_outlier_emit"), reps))
    print(f"  mean = {float(stats.mean):.6g}, std = {float(stats.std):.6g}, threshold = {float(stats.threshold):.6g}, n_valid = {int(stats.n_valid)}, "
          f"n_kept = {n_kept}: {N - n_kept} removed, of them {int(N_SHELL - (ind < N_SHELL).sum())} shell points and "
          f"{int(N_OUT - (ind >= N_SHELL).sum())} of the {N_OUT} outliers", flush=True)
    line("remove_statistical_outlier: index build + 3 calls + host read + emit", timed(lambda: cloud_filter.remove_statistical_outlier(
        points, NB, RATIO), max(3, reps // 4)))
    # the share of the isolated points: the shell alone, and the same search with the outliers left out of the QUERIES only
    shell = points[:N_SHELL].contiguous()
    shell_index = KnnIndex(shell)
    avg_s = torch.empty(N_SHELL, dtype=torch.float64, device=dev)
    a_s = _cloud_outlier_args(shell, shell_index.buffer, NB, RATIO, scratch, avg_s, record)
    t_shell = timed(lambda: _lib.run("dnsplat_cloud_neighbor_mean", L.dnsplat_cloud_neighbor_mean, ctypes.byref(a_s), _stream()), max(3, reps // 4))
    line(f"dnsplat_cloud_neighbor_mean, the shell alone ({N_SHELL} points, its own index, grid {L.dnsplat_knn_grid_dim(N_SHELL)}^3)", t_shell)
    t_q = timed(lambda: index.query(shell, NB), max(3, reps // 4))
    line("dnsplat_knn_query, k = 20: the shell's points as queries of the WHOLE cloud's index", t_q)
    t_o = timed(lambda: index.query(points[N_SHELL:].contiguous(), NB), max(3, reps // 4))
    line(f"dnsplat_knn_query, k = 20: the {N_OUT} outliers alone as queries of the whole cloud's index", t_o)
    print(f"  the isolated points: {100 * N_OUT / N:.1f} % of the rows; the whole cloud takes {t_all[0] / t_shell[0]:.2f} x the shell alone; the outliers "
          f"alone take {100 * t_o[0] / t_all[0]:.1f} % of the whole cloud's time when launched by themselves", flush=True)


def gpu_voxel(reps):
    import torch

    import _cloud_filter_inputs as inputs

    from dn_splatter_amd import _lib, cloud_filter
    from dn_splatter_amd._ops import _stream, _voxel_args

    dev = "cuda:0"
    points = the_cloud().to(dev)
    normals, colors = (x.to(dev) for x in inputs.attributes(points.cpu()))
    N = points.shape[0]
    L = _lib.lib()
    print(f"\ngpu voxel down-sampling: N = {N} points; device {torch.cuda.get_device_name(0)}; {reps} repetitions", flush=True)
    for voxel_size in (0.01, 0.1, 10.0):
        for n_attr, (nn, cc) in ((0, (None, None)), (2, (normals, colors))):
            nbytes = L.dnsplat_voxel_scratch_bytes(N, n_attr)
            scratch = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
            counts = torch.empty(2, dtype=torch.int64, device=dev)
            voxel_of = torch.empty(N, dtype=torch.int32, device=dev)
            a = _voxel_args(points, nn, cc, voxel_size, scratch, counts, voxel_of)
            t = timed(lambda: _lib.run("dnsplat_voxel_count", L.dnsplat_voxel_count, ctypes.byref(a), _stream()), reps)
            V, status = counts.tolist()
            outs = [torch.empty(V, 3, dtype=torch.float64, device=dev) for _ in range(1 + n_attr)]
            out_counts = torch.empty(V, dtype=torch.int32, device=dev)
            a = _voxel_args(points, nn, cc, voxel_size, scratch, counts, voxel_of, outs[0], outs[1] if n_attr else None, outs[2] if n_attr else None,
                            out_counts)
            te = timed(lambda: _lib.run("dnsplat_voxel_emit", L.dnsplat_voxel_emit, ctypes.byref(a), _stream()), reps)
            tw = timed(lambda: cloud_filter.voxel_down_sample(points, voxel_size, nn, cc), reps)
            what = "points, normals and colours" if n_attr else "points alone"
            print(f"  voxel_size = {voxel_size}, {what}: V = {V} voxels, the largest {int(out_counts.max())} points, status = {status}, scratch "
                  f"{nbytes / 2 ** 20:.0f} MiB", flush=True)
            line("    dnsplat_voxel_count (8 launches)", t)
            line("    dnsplat_voxel_emit (1 launch)", te)
            line("    voxel_down_sample: both calls, the allocations and the host read", tw)


def subsample():
    import torch

    points = the_cloud()
    rows = min(points.shape[0], CPU_ROWS)
    perm = torch.randperm(points.shape[0], generator=torch.Generator().manual_seed(1))[:rows]
    what = "the whole cloud" if rows == points.shape[0] else f"a SUBSAMPLE, {rows} of {points.shape[0]} points (a seeded permutation)"
    return points[perm].double().numpy(), what


def cpu_outlier():
    import numpy as np
    from scipy.spatial import cKDTree

    p, what = subsample()
    t0 = time.perf_counter()
    tree = cKDTree(p)
    build = time.perf_counter() - t0
    t0 = time.perf_counter()
    d, _ = tree.query(p, k=NB, workers=16)
    query = time.perf_counter() - t0
    t0 = time.perf_counter()
    avg = d.sum(axis=1) / NB
    mean = avg[avg > 0].sum() / len(avg)
    std = np.sqrt(((avg[avg > 0] - mean) ** 2).sum() / (len(avg) - 1))
    keep = np.nonzero((avg > 0) & (avg < mean + RATIO * std))[0]
    rest = time.perf_counter() - t0
    print(f"\ncpu outlier removal on {what}: scipy cKDTree build {build:.2f} s, query(k = {NB}, workers = 16) {query:.2f} s, the moments and the "
          f"mask in numpy {1e3 * rest:.1f} ms; {len(keep)} kept ({os.cpu_count()} CPUs visible)", flush=True)


def cpu_voxel():
    import numpy as np

    p, what = subsample()
    for voxel_size in (0.01, 0.1):
        t0 = time.perf_counter()
        lo = p.min(axis=0) - voxel_size / 2
        idx = np.floor((p - lo) / voxel_size).astype(np.int64)
        key = idx[:, 0] | (idx[:, 1] << 21) | (idx[:, 2] << 42)
        uniq, inverse = np.unique(key, return_inverse=True)
        s = np.zeros((len(uniq), 3))
        np.add.at(s, inverse.reshape(-1), p)
        mean = s / np.bincount(inverse.reshape(-1))[:, None]
        seconds = time.perf_counter() - t0
        print(f"\ncpu voxel down-sampling on {what}, voxel_size = {voxel_size}: numpy unique + add.at {seconds:.2f} s, {len(mean)} voxels (one CPU)",
              flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--one", nargs="+")
    ap.add_argument("--cases", default="gpu,cpu")
    a = ap.parse_args()
    if a.one:
        {("gpu", "outlier"): lambda: gpu_outlier(a.reps), ("gpu", "voxel"): lambda: gpu_voxel(a.reps), ("cpu", "outlier"): cpu_outlier,
         ("cpu", "voxel"): cpu_voxel}[tuple(a.one)]()
    else:
        print("point-cloud filters: device times by HIP events, median of the repetitions after one warm-up", flush=True)
        for case in CASES:
            if case[0] not in a.cases.split(","):
                continue
            # check=True: a failure raises here and nothing more is started on the device after it
            subprocess.run(["timeout", "-k", "10", str(CASE_SECONDS), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--one"] + case,
                           check=True)
