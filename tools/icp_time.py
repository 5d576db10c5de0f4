"""The mesh alignment at the size the evaluation chain produces: the vertices of the C2 scene's marching-cubes mesh (tools/geometry_bench.py
``mesh()``; a seeded SUBSAMPLE of ROWS of them when there are more) as the target, and the same points moved rigidly by the inverse of
a known pose (1 degree, 0.02) as the source, threshold 0.1 — what ``get_align_transformation`` is given.

  gpu   the index build; ``dnsplat_cloud_distances`` on the same two clouds (the same search, another fold) beside one ICP pass
        (``dnsplat_icp_begin`` + ``dnsplat_icp_iterate``: icp_corr_kernel + icp_solve_kernel) and ``dnsplat_icp_begin`` alone; a pass over
        256 rows (one workgroup of the search: the fold, the solve and the launches are what is left); ``dnsplat_icp_run`` and the whole
        ``registration_icp`` with its allocations, index build and host read, with the pass count; the idle launches: 31 passes on a
        state whose ``done`` is set
  cpu   what a ROCm box has instead: scipy's ``cKDTree`` build + ``query(workers=16)`` + a numpy Kabsch per pass, on CPU_ROWS rows — a
        stated SUBSAMPLE where the clouds have more

Device times: HIP events around the call, median of the repetitions after one warm-up.  Nothing here asserts a speed.

    python tools/icp_time.py      # each part in a child process under `timeout -k 10`; stops at the first failure

The output is meant to be kept as profiles/icp.txt.
"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROWS = 1_000_000
CPU_ROWS = 200_000
THRESHOLD = 0.1
ANGLE, TAU = 1.0, 0.02
CASES = [["gpu"], ["cpu"]]
CASE_SECONDS = 400


def timed(fn, reps):
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
    return statistics.median(ms), min(ms), max(ms), out


def line(what, t):
    print(f"  {what:<92s} {t[0]:9.3f} ms   (min {t[1]:.3f}, max {t[2]:.3f})", flush=True)


def clouds(rows):
    """(source, target float32 [n,3] on the device, T0 float64 numpy, what)"""
    import numpy as np
    import torch

    import _icp_inputs as inputs
    import geometry_bench

    vertices, _ = geometry_bench.mesh()
    V = vertices.shape[0]
    what = f"all {V} vertices"
    if V > rows:
        perm = torch.randperm(V, generator=torch.Generator().manual_seed(1))[:rows].to(vertices.device)
        vertices = vertices[perm].contiguous()
        what = f"a SUBSAMPLE, {rows} of {V} vertices (a seeded permutation)"
    T0 = inputs.pose(ANGLE, TAU)
    R, t = torch.from_numpy(T0[:3, :3]).to(vertices.device), torch.from_numpy(T0[:3, 3]).to(vertices.device)
    source = ((vertices.double() - t) @ R).float().contiguous()
    return source, vertices, T0, what


def gpu(reps):
    import numpy as np
    import torch

    from dn_splatter_amd import _lib, geometry, icp
    from dn_splatter_amd._ops import _icp_args, _stream
    from dn_splatter_amd.density import KnnIndex

    source, target, T0, what = clouds(ROWS)
    M, dev = source.shape[0], source.device
    L = _lib.lib()
    print(f"\ngpu mesh alignment: the C2 marching-cubes mesh, {what}, against its copy moved by {ANGLE} degree and tau = {TAU}; threshold "
          f"{THRESHOLD}; device {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {reps} repetitions", flush=True)
    t = timed(lambda: KnnIndex(target), reps)
    line(f"dnsplat_knn_build over the target (grid {L.dnsplat_knn_grid_dim(M)}^3)", t)
    index = t[3]
    t_cd = timed(lambda: geometry.cloud_distances(source, index, with_idx=True), reps)
    line("cloud_distances(source, index): dnsplat_cloud_distances with its allocations (1 memset + 13 launches)", t_cd)

    def args(rows, max_iteration=30):
        state = torch.empty(icp.STATE_WORDS, dtype=torch.float64, device=dev)
        scratch = torch.empty(L.dnsplat_icp_scratch_bytes(rows) // 8, dtype=torch.float64, device=dev)
        return _icp_args(source[:rows], target, index.buffer, THRESHOLD, 1e-6, 1e-6, max_iteration, state, scratch), (state, scratch)

    a, keep = args(M)
    begin = lambda x: _lib.run("dnsplat_icp_begin", L.dnsplat_icp_begin, ctypes.byref(x), None, _stream())
    iterate = lambda x: _lib.run("dnsplat_icp_iterate", L.dnsplat_icp_iterate, ctypes.byref(x), _stream())
    t_begin = timed(lambda: begin(a), reps)
    line("dnsplat_icp_begin (1 launch)", t_begin)
    t_pass = timed(lambda: (begin(a), iterate(a)), reps)
    line("dnsplat_icp_begin + dnsplat_icp_iterate: one pass from the identity (icp_corr_kernel + icp_solve_kernel)", t_pass)
    one = t_pass[0] - t_begin[0]
    print(f"  one pass less the begin: {one:.3f} ms = {one / t_cd[0]:.2f} x cloud_distances on the same clouds (the same search; 16 double sums "
          f"per row and a {L.dnsplat_icp_scratch_bytes(M) // 136}-partial fold instead of 8 sums and a six-round radix selection)", flush=True)
    small, keep_small = args(256)
    t_small = timed(lambda: (begin(small), iterate(small)), reps)
    line("the same over 256 rows: one workgroup of the search, the solve, three launches", t_small)
    t_run = timed(lambda: _lib.run("dnsplat_icp_run", L.dnsplat_icp_run, ctypes.byref(a), None, _stream()), max(3, reps // 2))
    state = keep[0].cpu()
    passes, iterations = int(state.view(torch.int64)[icp.STATE_PASSES]), int(state.view(torch.int64)[icp.STATE_ITERATIONS])
    line(f"dnsplat_icp_run (63 launches; {passes} passes ran, {iterations} updates, {31 - passes} idle pairs)", t_run)
    t_idle = timed(lambda: [iterate(a) for _ in range(31)], reps)
    line("31 x dnsplat_icp_iterate on the finished state: 62 launches that return at their first load", t_idle)
    t_all = timed(lambda: icp.registration_icp(source, target, THRESHOLD), max(3, reps // 2))
    r = t_all[3]
    line("registration_icp(source, target): the index build, the allocations, the run and the host read", t_all)
    err = np.abs(r.transformation.cpu().numpy() - T0).max()
    print(f"  fitness = {r.fitness:.6f}, inlier_rmse = {r.inlier_rmse:.3e}, iterations = {r.iterations}, status = {r.status}, max |T - T0| = {err:.3e}; "
          f"scratch {L.dnsplat_icp_scratch_bytes(M) / 2 ** 10:.0f} KiB", flush=True)
    t_tp = timed(lambda: icp.transform_points(source, r.transformation), reps)
    line("transform_points(source, T) (1 launch)", t_tp)


def cpu():
    import numpy as np
    from scipy.spatial import cKDTree

    source, target, T0, what = clouds(CPU_ROWS)
    s, g = source.double().cpu().numpy(), target.double().cpu().numpy()
    t0 = time.perf_counter()
    tree = cKDTree(g)
    build = time.perf_counter() - t0
    T, passes, prev, per_pass = np.eye(4), 0, None, []
    for k in range(31):
        t0 = time.perf_counter()
        q = s @ T[:3, :3].T + T[:3, 3]
        d, j = tree.query(q, workers=16, distance_upper_bound=THRESHOLD)
        ok = np.isfinite(d)
        n = int(ok.sum())
        fitness, rmse = n / len(s), float(np.sqrt((d[ok] ** 2).sum() / max(n, 1)))
        passes += 1
        stop = n == 0 or k == 30 or (prev is not None and abs(fitness - prev[0]) < 1e-6 and abs(rmse - prev[1]) < 1e-6)
        if not stop:
            qq, gg = q[ok], g[j[ok]]
            mq, mg = qq.mean(axis=0), gg.mean(axis=0)
            u, _, vt = np.linalg.svd((gg - mg).T @ (qq - mq) / n)
            sgn = -1.0 if np.linalg.det(u) * np.linalg.det(vt) < 0 else 1.0
            R = u @ np.diag([1.0, 1.0, sgn]) @ vt
            U = np.eye(4)
            U[:3, :3], U[:3, 3] = R, mg - R @ mq
            T = U @ T
        per_pass.append(time.perf_counter() - t0)
        prev = (fitness, rmse)
        if stop:
            break
    print(f"\ncpu mesh alignment on {what}: scipy cKDTree build {build:.2f} s; {passes} passes of query(workers = 16) + numpy Kabsch, "
          f"{statistics.median(per_pass):.2f} s per pass (median), {sum(per_pass):.2f} s in all; max |T - T0| = {np.abs(T - T0).max():.3e} "
          f"({os.cpu_count()} CPUs visible)", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--one", nargs="+")
    ap.add_argument("--cases", default="gpu,cpu")
    a = ap.parse_args()
    if a.one:
        {("gpu",): lambda: gpu(a.reps), ("cpu",): cpu}[tuple(a.one)]()
    else:
        print("mesh alignment (point-to-point ICP): device times by HIP events, median of the repetitions after one warm-up", flush=True)
        for case in CASES:
            if case[0] not in a.cases.split(","):
                continue
            # check=True: a failure raises here and nothing more is started on the device after it
            subprocess.run(["timeout", "-k", "10", str(CASE_SECONDS), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--one"] + case,
                           check=True)
