"""Paired A/B timing of ONE C-ABI entry point across several builds of libdnsplat.so, inside one process and on identical
arguments: the benchmark frame is rendered once with the default library; when the chosen entry point is reached its
argument struct (alive at that moment) is replayed against every variant library, round-robin, bracketed by HIP events.
Box-to-box and run-to-run drift (2-3 % on this pool) cancels; the minimum and median per variant are printed.

    python tools/ab_kernels.py --entry dnsplat_raster_bwd --libs gpurun_ab/lib_base.so,gpurun_ab/lib_sym.so [--workload c2]

``--workload mc256`` / ``mc512``: instead of the frame, ``marching_cubes`` at level 0.5 on the density lattice of the C2 scene
(tools/marching_time.py's), for ``--entry dnsplat_mc_count`` or ``dnsplat_mc_emit``; ``mc256cut`` / ``mc512cut``: ``cut_mesh`` on that
mesh under seeded votes, for ``--entry dnsplat_mesh_cut_count`` or ``dnsplat_mesh_cut_emit``.
"""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import dn_splatter_amd as dns  # noqa: E402
from dn_splatter_amd import _lib, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--entry", default="dnsplat_raster_bwd")
ap.add_argument("--libs", required=True)
ap.add_argument("--workload", default="c2")
ap.add_argument("--rounds", type=int, default=12)
ap.add_argument("--iters", type=int, default=4)
args = ap.parse_args()
WL = {"c2": (1_000_000, 1920, 1080), "c3": (3_000_000, 1600, 1200), "c5": (5_000_000, 1600, 1200)}
N, W, H = WL.get(args.workload, WL["c2"])
dev = "cuda:0"
paths = [os.path.abspath(p) for p in args.libs.split(",")]
libs = [(os.path.basename(p), ctypes.CDLL(p)) for p in paths]
results = {}
armed = False
orig_run = _lib.run


def run(name, fn, *a):
    if name != args.entry or results or not armed:
        return orig_run(name, fn, *a)
    # zero-initialised accumulators (v_splats) keep growing across replays: harmless for timing
    times = {n: [] for n, _ in libs}
    for n, L in libs:                      # warm each library's code object
        f = getattr(L, name)
        f.restype = ctypes.c_int
        assert f(*a) == 0
    torch.cuda.synchronize()
    for r in range(args.rounds):
        order = libs if r % 2 == 0 else libs[::-1]
        for n, L in order:
            f = getattr(L, name)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                f(*a)
            e1.record()
            torch.cuda.synchronize()
            times[n].append(e0.elapsed_time(e1) / args.iters)
    results.update(times)
    return orig_run(name, fn, *a)


_lib.run = run
if args.workload.startswith("mc"):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import marching_time  # noqa: E402

    from dn_splatter_amd import marching  # noqa: E402

    cut = args.workload.endswith("cut")    # mc256cut / mc512cut: cut_mesh on that mesh under seeded votes
    _, volume = marching_time.lattice(int(args.workload[2:5]))
    if cut:
        from dn_splatter_amd import mesh_cull  # noqa: E402

        vertices, triangles = marching.marching_cubes(volume, marching_time.LEVEL)
        gen = torch.Generator(device=dev).manual_seed(2)
        obs = torch.randint(0, 8, (vertices.shape[0],), device=dev, generator=gen, dtype=torch.int32)
        invalid = torch.randint(0, 8, (vertices.shape[0],), device=dev, generator=gen, dtype=torch.int32)
    for it in range(2):
        armed = it == 1                    # first mesh: warm-up with the default library only
        if cut:
            mesh_cull.cut_mesh(vertices, triangles, obs, invalid)
        else:
            marching.marching_cubes(volume, marching_time.LEVEL)
    torch.cuda.synchronize()
    for n, _ in libs:
        t = results[n]
        print(f"{args.entry} {args.workload} {n:28s} median {statistics.median(t):.4f} ms  min {min(t):.4f} ms  "
              f"({100 * (statistics.median(t) / statistics.median(results[libs[0][0]]) - 1):+.2f} % vs first)")
    sys.exit(0)
gp = synthetic.make_gauss_params(N, sh_rest_std=0.1, seed=0, device=dev)
cam = synthetic.orbit_camera(0, n_views=8, width=W, height=H, focal=1200.0).to(dev)
r = dns.DNSplatterRenderer(gp, fused=True)
gen = torch.Generator(device=dev).manual_seed(1)
keys = ("rgb", "depth", "normal", "accumulation")
for it in range(2):
    armed = it == 1                        # first frame: warm-up with the default library only
    for k in gp:
        gp[k].grad = None
    out = r.get_outputs(cam)
    cot = [torch.rand(out[k].shape, device=dev, generator=gen) * 2 - 1 for k in keys]
    torch.autograd.backward([out[k] for k in keys], cot)
torch.cuda.synchronize()
base = None
for n, _ in libs:
    t = results[n]
    med, mn = statistics.median(t), min(t)
    base = base or med
    print(f"{args.entry} {args.workload} {n:28s} median {med:.4f} ms  min {mn:.4f} ms  ({100 * (med / base - 1):+.2f} % vs first)")
