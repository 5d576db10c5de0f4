"""The Gaussian density field at the size of the marching-cubes exporter: 1 M Gaussians of the C2 scene's law, batches of 2 M samples
(export_mesh.py:711 ``batch_size``), and the 256^3 and 512^3 lattices.

  field      density.GaussianDensityField: index build + record pack, ``closest`` (the [M,16] tensor), ``density`` with the search inside
             the kernel, ``density`` on given neighbours, ``density_grad(num_closest_gaussians=1)``.  The reference's torch operations on
             the same GPU (the [M,16,3,3] gathers and the batched product of get_density) are NOT timed: at this batch size they ended
             in an illegal memory access inside torch's own operators, after every dnsplat call had completed, and the cause was not
             found — so nothing here starts them
  sklearn    the reference's neighbour search for the same means: sklearn's NearestNeighbors as knn_sk calls it (n_jobs unset) and with
             n_jobs=16, on SKLEARN_SAMPLES of the samples (the full batch is that many times longer), fit and query timed apart
  volume R   ``density_volume`` on the R^3 lattice over the box of the means

Device times: HIP events around the call, median of the repetitions after one warm-up (a call above 15 s is timed once, by the host clock).  Nothing here asserts a speed.

    python tools/density_time.py        # every case in a child process under `timeout -k 10`; stops at the first failure

The output is meant to be kept as profiles/density_field.txt.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, M = 1_000_000, 2_000_000
SKLEARN_SAMPLES = 100_000
RADIUS = 5.0
CASES = [["field"], ["volume", "256"], ["volume", "512"], ["sklearn"]]
CASE_SECONDS = 240
LONG_CALL_MS = 15_000.0


def scene(device):
    import torch

    from dn_splatter_amd import synthetic

    gp = synthetic.make_gauss_params(N, sh_degree=0, seed=0, scale_init="closed_form", device=device)
    g = torch.Generator().manual_seed(1)
    samples = ((torch.rand(M, 3, generator=g) - 0.5) * 10).to(device)
    return {k: gp[k].detach() for k in ("means", "scales", "quats", "opacities")}, samples


def timed(fn, reps):
    import torch

    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    first = (time.perf_counter() - t0) * 1e3
    if first > LONG_CALL_MS:                                   # a long call is not repeated: the host clock around the first one
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
    print(f"  {what:<64s} median {t[0]:10.3f} ms   min {t[1]:10.3f}   max {t[2]:10.3f}", flush=True)


def field_case(reps):
    import torch

    from dn_splatter_amd import density

    gp, samples = scene("cuda:0")
    print(f"\nfield: {N} Gaussians, {M} samples in the box of the means; device {torch.cuda.get_device_name(0)}, torch {torch.__version__}", flush=True)
    line("index build (dnsplat_knn_build)", timed(lambda: density.build_index(gp["means"]), reps))
    t = timed(lambda: density.GaussianDensityField(gp["means"], gp["scales"], gp["quats"], gp["opacities"]), reps)
    line("GaussianDensityField: index build + record pack", t)
    field = t[3]
    t = timed(lambda: field.closest(samples), reps)
    line("closest: [M,16] int64, ranks 1 .. 16 in float64", t)
    closest = t[3]
    line("density, the search inside the kernel (no [M,16] tensor)", timed(lambda: field.density(samples), reps))
    line("density on given neighbours (int64)", timed(lambda: field.density(samples, closest_gaussians=closest), reps))
    line("density_grad(num_closest_gaussians=1), search inside", timed(lambda: field.density_grad(samples, 1), reps))
    got = field.density(samples)
    print(f"  {int((got >= 0.5).sum())} of {M} densities at or above 0.5, {int((got <= 1e-4).sum())} at the floor", flush=True)


def volume_case(R, reps):
    import torch

    from dn_splatter_amd import density

    gp, _ = scene("cuda:0")
    field = density.GaussianDensityField(gp["means"], gp["scales"], gp["quats"], gp["opacities"])
    print(f"\nvolume: {R}^3 = {R ** 3} lattice points, radius {RADIUS}, {N} Gaussians", flush=True)
    t = timed(lambda: density.density_volume(field, R, RADIUS), reps)
    line(f"density_volume({R})", t)
    print(f"  {R ** 3 / t[0] / 1e3:.1f} M lattice points per second; {int((t[3] >= 0.5).sum())} at or above 0.5", flush=True)


def sklearn_case():
    try:
        from sklearn.neighbors import NearestNeighbors
    except ImportError:
        print("\nsklearn: not importable here; no CPU yardstick", flush=True)
        return
    gp, samples = scene("cpu")
    x, y = gp["means"].numpy(), samples[:SKLEARN_SAMPLES].numpy()
    print(f"\nsklearn: NearestNeighbors(n_neighbors=17) on {N} means, {SKLEARN_SAMPLES} of the {M} samples "
          f"(a batch is {M // SKLEARN_SAMPLES} times this); host clock", flush=True)
    for jobs in (None, 16):
        t0 = time.perf_counter()
        nn = NearestNeighbors(n_neighbors=17, algorithm="auto", metric="euclidean", n_jobs=jobs).fit(x)
        t1 = time.perf_counter()
        nn.kneighbors(y)
        t2 = time.perf_counter()
        print(f"  n_jobs={jobs}: fit {1e3 * (t1 - t0):10.1f} ms   query {1e3 * (t2 - t1):10.1f} ms   "
              f"=> {1e3 * (t2 - t1) * M / SKLEARN_SAMPLES:12.1f} ms per batch of {M}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--one", nargs="+")
    a = ap.parse_args()
    if a.one:
        if a.one[0] == "field":
            field_case(a.reps)
        elif a.one[0] == "volume":
            volume_case(int(a.one[1]), a.reps)
        else:
            sklearn_case()
    else:
        print("Gaussian density field: device times by HIP events, median of the repetitions after one warm-up", flush=True)
        for case in CASES:
            # check=True: a failure raises here and nothing more is started on the device after it
            subprocess.run(["timeout", "-k", "10", str(CASE_SECONDS), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--one"] + case,
                           check=True)
