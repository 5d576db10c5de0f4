"""Marching cubes at the size of the reference's ``gs-mesh marching`` exporter: the density lattice of 1 M Gaussians of the C2 scene's
law (tools/density_time.py's scene) at 256^3 and 512^3, level 0.5.

  gpu R      ``mc_count`` (dnsplat_mc_count: the one pass over the volume, the case counts, the scan), ``mc_emit`` (dnsplat_mc_emit into
             buffers of exactly V and T rows) and the whole ``marching_cubes_mesh`` (density_volume + count + the host read of the two
             counts + emit + world mapping + vertex colours through ``closest``); V, T and the bytes per second of the count pass against
             the volume's own size (4 R^3 bytes)
  cpu R      the ONLY CPU alternative that exists where no marching-cubes library is installed — NOT mcubes: the device-to-host copy of the
             lattice (host clock) plus the numpy restatement (torch_marching, the tests' yardstick, not written for speed) on the central
             CPU_SUB^3 sub-lattice, small enough to finish; a full lattice is (R / CPU_SUB)^3 times that many cells

Device times: HIP events around the call, median of the repetitions after one warm-up.  Nothing here asserts a speed.

    python tools/marching_time.py       # every case in a child process under `timeout -k 10`; stops at the first failure

The output is meant to be kept as profiles/marching_cubes.txt.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LEVEL = 0.5
CPU_SUB = 128
CASES = [["gpu", "256"], ["gpu", "512"], ["cpu", "256"], ["cpu", "512"]]
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
    print(f"  {what:<64s} median {t[0]:10.3f} ms   min {t[1]:10.3f}   max {t[2]:10.3f}", flush=True)


def lattice(R):
    import density_time

    from dn_splatter_amd import density

    gp, _ = density_time.scene("cuda:0")
    field = density.GaussianDensityField(gp["means"], gp["scales"], gp["quats"], gp["opacities"])
    return field, density.density_volume(field, R, density_time.RADIUS)


def gpu_case(R, reps):
    import torch

    import density_time

    from dn_splatter_amd import marching

    field, volume = lattice(R)
    print(f"\ngpu: {R}^3 = {R ** 3} lattice points ({4 * R ** 3 / 2 ** 20:.0f} MiB), level {LEVEL}, {field.N} Gaussians; "
          f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {reps} repetitions", flush=True)
    scratch = torch.empty((marching.scratch_bytes(volume.shape) + 7) // 8, dtype=torch.int64, device=volume.device)
    t = timed(lambda: marching.mc_count(volume, LEVEL, scratch), reps)
    line("mc_count: masks + case counts + scan (4 launches)", t)
    count = t[3]
    V, T = count.counts.tolist()
    print(f"  V = {V} vertices, T = {T} triangles; the count pass moves the volume at {4 * R ** 3 / t[0] / 1e9:.3f} TB/s; "
          f"scratch {scratch.numel() * 8 / 2 ** 20:.1f} MiB", flush=True)
    vertices = torch.empty(V, 3, dtype=torch.float32, device=volume.device)
    triangles = torch.empty(T, 3, dtype=torch.int32, device=volume.device)
    line("mc_emit: vertices + triangles (2 launches)", timed(lambda: marching.mc_emit(count, vertices, triangles), reps))
    line("marching_cubes: count + host read of V, T + allocate + emit", timed(lambda: marching.marching_cubes(volume, LEVEL), reps))
    colors = torch.rand(field.N, 3, device=volume.device)
    line("marching_cubes_mesh: density_volume .. vertex colours",
         timed(lambda: marching.marching_cubes_mesh(field, R, density_time.RADIUS, LEVEL, colors=colors), reps))


def cpu_case(R):
    import torch

    from dn_splatter_amd import torch_marching

    _, volume = lattice(R)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = volume.cpu().numpy()
    t1 = time.perf_counter()
    lo = (R - CPU_SUB) // 2
    sub = host[lo:lo + CPU_SUB, lo:lo + CPU_SUB, lo:lo + CPU_SUB].copy()
    t2 = time.perf_counter()
    v, t = torch_marching.marching_cubes(sub, LEVEL)
    t3 = time.perf_counter()
    print(f"\ncpu (the numpy restatement, NOT mcubes: no marching-cubes library is installed): {R}^3 lattice; host clock", flush=True)
    print(f"  device-to-host copy of the lattice ({4 * R ** 3 / 2 ** 20:.0f} MiB, pageable)          {1e3 * (t1 - t0):10.1f} ms", flush=True)
    print(f"  restatement on the central {CPU_SUB}^3 sub-lattice: V = {len(v)}, T = {len(t)}    {1e3 * (t3 - t2):10.1f} ms   "
          f"(the full lattice has {(R / CPU_SUB) ** 3:.0f} times the cells)", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--one", nargs="+")
    a = ap.parse_args()
    if a.one:
        if a.one[0] == "gpu":
            gpu_case(int(a.one[1]), a.reps)
        else:
            cpu_case(int(a.one[1]))
    else:
        print("Marching cubes: device times by HIP events, median of the repetitions after one warm-up", flush=True)
        for case in CASES:
            # check=True: a failure raises here and nothing more is started on the device after it
            subprocess.run(["timeout", "-k", "10", str(CASE_SECONDS), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--one"] + case,
                           check=True)
