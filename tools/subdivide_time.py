"""The subdivision of long triangles at the sizes the evaluation chain meets.

  box     the box room of the tests (12 triangles, 5 x 4 x 3) at the reference's max_edge = 0.015: 10 rounds, 12 * 4^9 = 3.1 M triangles
  mc256   the C2 scene's 256^3 marching-cubes mesh (tools/geometry_bench.py ``mesh()``) at HALF its voxel edge: every triangle is long
          once or twice
  cull    ``cull_mesh(subdivide=True)`` beside ``subdivide=False`` on the 256^3 TSDF mesh of tools/tsdf_time.py (eight 1920 x 1080
          frames), max_edge = 0.015, the reference's
  numpy   what a ROCm box has instead, on the same box: the numpy statement of the rule (tests/_subdivide_inputs.py) plus the
          device-to-host and host-to-device copies it needs

Per round: ``dnsplat_subdivide_count`` and ``dnsplat_subdivide_emit`` by HIP events (median of the repetitions after one warm-up; both
calls may be repeated on the same state), the scratch bytes, and the one host read; then the whole ``subdivide_to_size`` with its
allocations and reads.  Nothing here asserts a speed.

    python tools/subdivide_time.py      # each part in a child process under `timeout -k 10`; stops at the first failure

The output is meant to be kept as profiles/subdivide.txt.
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

BOX_EDGE = 0.015
CASES = [["box"], ["mc256"], ["cull"], ["numpy"]]
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


def rounds(vertices, triangles, max_edge, reps, max_iter=10):
    """``subdivide.subdivide_to_size`` round by round, each call timed; prints a line per round."""
    import torch

    from dn_splatter_amd import _lib
    from dn_splatter_amd._ops import _stream, _subdivide_args

    L = _lib.lib()
    dev = vertices.device
    cv, cf = vertices.to(torch.float64).contiguous(), triangles.to(torch.int32).contiguous()
    ci = torch.arange(cf.shape[0], dtype=torch.int32, device=dev)
    word = torch.zeros(5, dtype=torch.int64, device=dev)
    base, total_count, total_emit, total_v, total_t, peak = 0, 0.0, 0.0, 0, 0, 0
    print(f"  {'round':>5s} {'triangles':>11s} {'long':>11s} {'vertices':>11s} {'done V':>10s} {'done T':>10s} {'midpoints':>10s} "
          f"{'scratch MiB':>11s} {'count ms':>9s} {'emit ms':>9s}", flush=True)
    for r in range(max_iter + 1):
        V, T = cv.shape[0], cf.shape[0]
        nbytes = L.dnsplat_subdivide_scratch_bytes(V, T)
        peak = max(peak, nbytes)
        scratch = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
        a = _subdivide_args(cv, cf, ci, max_edge, scratch, word[:4], word[4:])
        t_count = timed(lambda: _lib.run("dnsplat_subdivide_count", L.dnsplat_subdivide_count, ctypes.byref(a), _stream()), reps)
        n_v, n_t, n_long, n_mid, flags = word.tolist()                           # the round's one host read
        assert flags == 0, flags
        done = [torch.empty(n_v, 3, dtype=torch.float64, device=dev), torch.empty(n_t, 3, dtype=torch.int32, device=dev),
                torch.empty(n_t, dtype=torch.int32, device=dev)]
        nxt = [None, None, None]
        if n_long:
            nxt = [torch.empty(V + n_mid, 3, dtype=torch.float64, device=dev), torch.empty(4 * n_long, 3, dtype=torch.int32, device=dev),
                   torch.empty(4 * n_long, dtype=torch.int32, device=dev)]
        b = _subdivide_args(cv, cf, ci, max_edge, scratch, word[:4], word[4:], base, *done, *nxt)
        t_emit = timed(lambda: _lib.run("dnsplat_subdivide_emit", L.dnsplat_subdivide_emit, ctypes.byref(b), _stream()), reps)
        print(f"  {r:5d} {T:11d} {n_long:11d} {V:11d} {n_v:10d} {n_t:10d} {n_mid:10d} {nbytes / 2 ** 20:11.1f} {t_count[0]:9.3f} {t_emit[0]:9.3f}",
              flush=True)
        total_count, total_emit, total_v, total_t, base = total_count + t_count[0], total_emit + t_emit[0], total_v + n_v, total_t + n_t, base + n_v
        if n_long == 0:
            break
        cv, cf, ci = nxt
    assert int(word[4]) == 0
    print(f"  {r + 1} rounds, {r + 1} host reads (5 words each): V' = {total_v}, T' = {total_t}; the kernels {total_count + total_emit:.3f} ms "
          f"(count {total_count:.3f} + emit {total_emit:.3f}); scratch at its largest {peak / 2 ** 20:.1f} MiB (64 B per triangle + 4 B per vertex)",
          flush=True)


def whole(vertices, triangles, max_edge, reps):
    from dn_splatter_amd import subdivide

    t = timed(lambda: subdivide.subdivide_to_size(vertices, triangles, max_edge, return_index=True), reps)
    print(f"  subdivide_to_size(...) with its allocations, host reads and the final cat: median {t[0]:.3f} ms (min {t[1]:.3f}, max {t[2]:.3f}); "
          f"{t[3][1].shape[0]} triangles out", flush=True)


def box(reps):
    import torch

    import _subdivide_inputs as inputs

    v, f = inputs.box_room()
    v, f = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    print(f"\nbox: the box room, max_edge = {BOX_EDGE}; device {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {reps} repetitions", flush=True)
    rounds(v, f, BOX_EDGE, reps)
    whole(v, f, BOX_EDGE, reps)


def mc256(reps):
    import torch

    import density_time
    import geometry_bench
    from dn_splatter_amd import torch_subdivide

    v, f = geometry_bench.mesh()
    voxel = 2.0 * density_time.RADIUS / (geometry_bench.RESOLUTION - 1)
    longest = float(torch.cat([torch_subdivide.edge_lengths(v, f[s:s + 2_000_000]).max()[None] for s in range(0, f.shape[0], 2_000_000)]).max())
    reps = max(3, reps // 3)
    print(f"\nmc256: the C2 scene's {geometry_bench.RESOLUTION}^3 marching-cubes mesh, {v.shape[0]} vertices, {f.shape[0]} triangles, voxel edge "
          f"{voxel:.5f}, longest edge {longest:.5f}; max_edge = {voxel / 2:.5f} (half the voxel edge); {reps} repetitions", flush=True)
    rounds(v, f, voxel / 2, reps)
    whole(v, f, voxel / 2, reps)


def cull(reps):
    import torch

    import tsdf_time
    from dn_splatter_amd import mesh_cull

    dev = "cuda:0"
    depth, rgb, poses, K = tsdf_time.frames(dev)
    vol = tsdf_time.volume(256, dev)
    vol.integrate(depth, rgb, poses, K)
    mesh = vol.extract_mesh()[:2]
    c2w = torch.eye(4, dtype=torch.float64).repeat(poses.shape[0], 1, 1)
    c2w[:, :3] = poses.double().cpu()
    args = (c2w.numpy(), K, tsdf_time.H, tsdf_time.W)
    reps = max(3, reps // 3)
    print(f"\ncull: cull_mesh on the 256^3 TSDF mesh of eight {tsdf_time.W} x {tsdf_time.H} frames ({mesh[0].shape[0]} vertices, {mesh[1].shape[0]} "
          f"triangles, voxel {2.0 * tsdf_time.HALF / 255:.4f}), 8 poses, no sensor depth, obs_threshold 0; {reps} repetitions", flush=True)
    t0 = timed(lambda: mesh_cull.cull_mesh(mesh, *args, obs_threshold=0), reps)
    print(f"  subdivide=False: median {t0[0]:.3f} ms (min {t0[1]:.3f}, max {t0[2]:.3f}); kept {t0[3][1].shape[0]} triangles", flush=True)
    t1 = timed(lambda: mesh_cull.cull_mesh(mesh, *args, obs_threshold=0, subdivide=True, max_edge=BOX_EDGE), reps)
    print(f"  subdivide=True, max_edge = {BOX_EDGE}: median {t1[0]:.3f} ms (min {t1[1]:.3f}, max {t1[2]:.3f}); kept {t1[3][1].shape[0]} triangles",
          flush=True)
    rounds(mesh[0], mesh[1], BOX_EDGE, reps)


def numpy_case():
    import torch

    import _subdivide_inputs as inputs

    v, f = inputs.box_room()
    t0 = time.perf_counter()
    out_v, out_f, out_i, r = inputs.numpy_subdivide_to_size(v, f, BOX_EDGE)
    seconds = time.perf_counter() - t0
    print(f"\nnumpy: the numpy statement of the rule on the box room, max_edge = {BOX_EDGE}, the WHOLE input (no subsample): {len(r)} rounds, "
          f"{out_f.shape[0]} triangles, {out_v.shape[0]} vertices in {seconds:.2f} s ({os.cpu_count()} CPUs visible)", flush=True)
    if torch.cuda.is_available():
        # the copies a host subdivision sits between, at a mesh of the OUTPUT's size each way (a scan's input is already millions of rows)
        dv, df = torch.from_numpy(out_v).cuda(), torch.from_numpy(out_f.astype("int32")).cuda()
        down = timed(lambda: (dv.cpu(), df.cpu()), 5)
        up = timed(lambda: (torch.from_numpy(out_v).cuda(), torch.from_numpy(out_f.astype("int32")).cuda()), 5)
        print(f"  copies of a mesh of that size, pageable host memory: device-to-host {down[0]:.1f} ms, host-to-device {up[0]:.1f} ms", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--one", nargs="+")
    ap.add_argument("--cases", default="box,mc256,cull,numpy")
    a = ap.parse_args()
    if a.one:
        {"box": lambda: box(a.reps), "mc256": lambda: mc256(a.reps), "cull": lambda: cull(a.reps), "numpy": numpy_case}[a.one[0]]()
    else:
        print("mesh subdivision (subdivide_to_size): device times by HIP events, median of the repetitions after one warm-up", flush=True)
        for case in CASES:
            if case[0] not in a.cases.split(","):
                continue
            # check=True: a failure raises here and nothing more is started on the device after it
            subprocess.run(["timeout", "-k", "10", str(CASE_SECONDS), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--one"] + case,
                           check=True)
