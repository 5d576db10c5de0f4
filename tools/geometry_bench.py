"""The geometry scores at the size the papers report them: two draws of 1 M and of 4 M surface samples from the marching-cubes mesh of
the C2 scene's law (tools/density_time.py's scene, ``marching_cubes_mesh`` at 256^3, level 0.5), scored against each other.

  gpu S          ``sample_mesh_surface`` (areas + cumsum + dnsplat_mesh_sample), the index build over one draw (dnsplat_knn_build), each
                 direction of ``cloud_distances`` (one dnsplat_cloud_distances call: search, partials, the six selection rounds, the
                 finish), the selection's share of it (an UPPER BOUND: the same call against a ONE-point target, whose search reads one
                 point), and ``cloud_metrics`` (two builds, two directions).  Then the same direction with 1 % of the source replaced by
                 points scattered uniformly through the bounding box.
                 The uniform grid was sized for clouds that fill their box (about two points per cell).  A surface cloud fills few cells:
                 the occupancy printed below is the number of points per OCCUPIED cell, which is what a query walks.  A query far from
                 the surface widens its cube ring by ring, O(r^2) rows of cells per ring, and holds its whole wave for that long: the
                 scattered case prices it.  Both effects are stated here, not hidden; another index for surfaces is future work.
  room S         the thin-shell case the C2 mesh is not (its level set is a foam that fills the box): S points on three walls of a 4 x 3 x
                 2.5 room against a second draw with 0.01 noise, and the same with 1 % scattered through the box — few cells hold all
                 the points, and a scattered query is far from every one of them.
  scipy S        the reference's way on this box's CPU: ``cKDTree(target)`` and ``tree.query(source)`` as distance_p2p calls them (one
                 worker), host clock.  At 1 M on the full clouds; at 4 M on a 200 000-point subsample of each cloud, and the line says so.

Device times: HIP events around the call, median of the repetitions after one warm-up (a call longer than 5 s is not repeated: the host
clock around the first one).  Nothing here asserts a speed.

    python tools/geometry_bench.py       # every case in a child process under `timeout -k 10`; stops at the first failure

The output is meant to be kept as profiles/geometry_metrics.txt.
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

RESOLUTION, LEVEL = 256, 0.5
SCATTER = 0.01
SUBSAMPLE = 200_000
LONG_CALL_MS = 5_000.0
CASES = [["gpu", "1000000"], ["gpu", "4000000"], ["room", "1000000"], ["scipy", "1000000"], ["scipy", "4000000"]]
CASE_SECONDS = 420


def timed(fn, reps):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    first = (time.perf_counter() - t0) * 1e3
    if first > LONG_CALL_MS:
        return first, first, first, out
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
    print(f"  {what:<72s} median {t[0]:10.3f} ms   min {t[1]:10.3f}   max {t[2]:10.3f}", flush=True)


def mesh():
    import density_time

    from dn_splatter_amd import density, marching

    gp, _ = density_time.scene("cuda:0")
    field = density.GaussianDensityField(gp["means"], gp["scales"], gp["quats"], gp["opacities"])
    world, triangles, _ = marching.marching_cubes_mesh(field, RESOLUTION, density_time.RADIUS, LEVEL)
    return world.float().contiguous(), triangles


def clouds(S):
    from dn_splatter_amd import geometry

    vertices, triangles = mesh()
    a = geometry.sample_mesh_surface(vertices, triangles, count=S, seed=0)
    b = geometry.sample_mesh_surface(vertices, triangles, count=S, seed=1)
    return vertices, triangles, a, b


def scattered(points, seed=2):
    """A copy with SCATTER of the rows replaced by uniform points of the bounding box."""
    import torch

    g = torch.Generator(device=points.device).manual_seed(seed)
    out = points.clone()
    n = int(points.shape[0] * SCATTER)
    rows = torch.randperm(points.shape[0], generator=g, device=points.device)[:n]
    lo, hi = points.min(dim=0).values, points.max(dim=0).values
    out[rows] = lo + (hi - lo) * torch.rand(n, 3, generator=g, device=points.device)
    return out, n


def occupancy(points):
    """(cells per axis, occupied cells, mean and max points per occupied cell) of the index's grid over ``points``."""
    import torch

    from dn_splatter_amd import _lib

    G = _lib.lib().dnsplat_knn_grid_dim(points.shape[0])
    lo, hi = points.min(dim=0).values, points.max(dim=0).values
    c = ((points - lo) * (G / (hi - lo))).floor().clamp(0, G - 1).long()
    counts = torch.unique((c[:, 2] * G + c[:, 1]) * G + c[:, 0], return_counts=True)[1]
    return G, counts.numel(), float(counts.double().mean()), int(counts.max())


def room(S, seed, noise):
    """S points on the floor and two walls of a 4 x 3 x 2.5 box, uniform by area, with the walls' normals."""
    import torch

    g = torch.Generator(device="cuda:0").manual_seed(seed)
    box = torch.tensor([4.0, 3.0, 2.5], device="cuda:0")
    areas = torch.tensor([4.0 * 3.0, 3.0 * 2.5, 4.0 * 2.5], device="cuda:0")
    wall = torch.multinomial(areas / areas.sum(), S, replacement=True, generator=g)
    flat = 2 - wall                                                     # the axis that is 0 on the wall: z, x, y
    points = torch.rand(S, 3, generator=g, device="cuda:0") * box
    points.scatter_(1, flat[:, None], 0.0)
    normals = torch.zeros(S, 3, device="cuda:0").scatter_(1, flat[:, None], 1.0)
    if noise:
        points = points + noise * torch.randn(S, 3, generator=g, device="cuda:0")
    return points.contiguous(), normals


def gpu_case(S, reps, shell=False):
    import torch

    from dn_splatter_amd import density, geometry

    if shell:
        (sp, sn), (tp, tn) = room(S, 1, 0.01), room(S, 0, 0.0)
        print(f"\nroom: 2 x {S} points on three walls of a 4 x 3 x 2.5 box (the source with 0.01 noise); {reps} repetitions", flush=True)
    else:
        vertices, triangles, (sp, sn, _), (tp, tn, _) = clouds(S)
        print(f"\ngpu: 2 x {S} surface samples of a mesh of {vertices.shape[0]} vertices / {triangles.shape[0]} triangles; device "
              f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}; {reps} repetitions", flush=True)
    G, occupied, mean, most = occupancy(tp)
    print(f"  index grid {G}^3 = {G ** 3} cells for {S} points; {occupied} cells hold points ({100.0 * occupied / G ** 3:.2f} %): {mean:.1f} points "
          f"per occupied cell on average, {most} at most (a volume-filling cloud: about 2)", flush=True)
    if not shell:
        line("sample_mesh_surface: areas + cumsum + dnsplat_mesh_sample", timed(lambda: geometry.sample_mesh_surface(vertices, triangles, count=S, seed=0), reps))
    t = timed(lambda: density.KnnIndex(tp), reps)
    line("index build over the target (dnsplat_knn_build)", t)
    index = t[3]
    t = timed(lambda: geometry.cloud_distances(sp, index, sn, tn, with_idx=False), reps)
    line("cloud_distances, one direction with normals (on a built index)", t)
    r = t[3]
    print(f"    mean d {r.mean_d:.6f}   p90 {r.percentile:.6f}   share <= 0.05 {r.share_le:.4f}   mean |dot| {r.mean_absdot:.4f}", flush=True)
    line("cloud_distances, the same without normals", timed(lambda: geometry.cloud_distances(sp, index, with_idx=False), reps))
    one = density.KnnIndex(tp[:1].contiguous())
    line("  of it the selection, upper bound: the call against a 1-point target", timed(lambda: geometry.cloud_distances(sp, one, with_idx=False), reps))
    line("cloud_metrics: 2 index builds + 2 directions with normals", timed(lambda: geometry.cloud_metrics(sp, sn, tp, tn), reps))
    far, n = scattered(sp)
    # a pilot on 1 / 64 of the rows first: a kernel that would run for minutes is not started on a shared device
    pilot = timed(lambda: geometry.cloud_distances(far[:S // 64].contiguous(), index, with_idx=False), 3)
    line(f"pilot: the first {S // 64} rows of the scattered copy", pilot)
    if pilot[0] * 64 > 20_000.0:
        print(f"  the full scattered case is NOT run: the pilot extrapolates to {pilot[0] * 64 / 1e3:.1f} s", flush=True)
        return
    t = timed(lambda: geometry.cloud_distances(far, index, with_idx=False), max(3, reps // 4))
    line(f"cloud_distances with {n} sources ({100 * SCATTER:.0f} %) scattered through the box", t)
    print(f"    mean d {t[3].mean_d:.6f}   max d {t[3].max_d:.4f}", flush=True)


def scipy_case(S):
    import numpy as np
    from scipy.spatial import cKDTree

    _, _, (sp, _, _), (tp, _, _) = clouds(S)
    src, tgt = sp.cpu().numpy().astype(np.float64), tp.cpu().numpy().astype(np.float64)
    note = "the full clouds"
    if S > 1_000_000:
        rng = np.random.default_rng(0)
        src, tgt = src[rng.choice(S, SUBSAMPLE, replace=False)], tgt[rng.choice(S, SUBSAMPLE, replace=False)]
        note = f"a SUBSAMPLE of {SUBSAMPLE} points of each cloud, not the {S}"
    t0 = time.perf_counter()
    tree = cKDTree(tgt)
    t1 = time.perf_counter()
    dist, _ = tree.query(src)
    t2 = time.perf_counter()
    print(f"\nscipy (the reference's distance_p2p, one worker, host clock) at {S}: {note}", flush=True)
    print(f"  cKDTree build over {len(tgt)} points {1e3 * (t1 - t0):10.1f} ms   query of {len(src)} points {1e3 * (t2 - t1):10.1f} ms   "
          f"(mean d {dist.mean():.6f}); the reference does this twice per compute_metrics call, plus the device-to-host copies", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--one", nargs="+")
    a = ap.parse_args()
    if a.one:
        if a.one[0] in ("gpu", "room"):
            gpu_case(int(a.one[1]), a.reps, shell=a.one[0] == "room")
        else:
            scipy_case(int(a.one[1]))
    else:
        print("Geometry scores: device times by HIP events, median of the repetitions after one warm-up", flush=True)
        for case in CASES:
            # check=True: a failure raises here and nothing more is started on the device after it
            subprocess.run(["timeout", "-k", "10", str(CASE_SECONDS), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--one"] + case,
                           check=True)
