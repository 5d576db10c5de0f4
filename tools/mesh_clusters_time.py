"""The mesh cluster filter at the sizes the project already measures: the C2 scene's marching-cubes meshes at 256^3 and 512^3
(tools/marching_time.py's lattice, level 0.5) and the mesh of a TSDF volume fused from eight 1920 x 1080 frames at 512^3
(tools/tsdf_time.py's frames and volume).

  gpu MESH    ``dnsplat_mesh_clusters`` (eight launches), ``dnsplat_mesh_filter_count`` (one memset and nine launches) and
              ``dnsplat_mesh_filter_emit`` (two launches) at the reference's (50, 50), each by HIP events around the call; the whole
              ``filter_small_clusters`` with its host read and the gather of the vertices; n_clusters, the threshold, the share of
              triangles and vertices removed, the status words and the scratch bytes
  cpu MESH    the only alternative a ROCm box has: the device-to-host copy of the triangles (host clock) plus scipy's
              ``connected_components`` over the triangle pairs of an edge sort (the independent statement of
              tests/test_mesh_clusters_reference.py), on the first CPU_ROWS triangles where the mesh has more — a stated SUBSAMPLE

Device times: HIP events around the call, median of the repetitions after one warm-up.  Nothing here asserts a speed.

    python tools/mesh_clusters_time.py      # every case in a child process under `timeout -k 10`; stops at the first failure

The output is meant to be kept as profiles/mesh_clusters.txt.
"""
import argparse
import ctypes
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KEEP_LARGEST, MIN_TRIANGLES = 50, 50
CPU_ROWS = 9_000_000
CASES = [["gpu", "mc256"], ["gpu", "mc512"], ["gpu", "tsdf512"], ["cpu", "mc256"], ["cpu", "mc512"], ["cpu", "tsdf512"]]
CASE_SECONDS = 400


def mesh(name):
    """(vertices, triangles int32 [T,3]) on the device."""
    import marching_time
    import tsdf_time

    from dn_splatter_amd import marching

    if name.startswith("mc"):
        _, volume = marching_time.lattice(int(name[2:]))
        return marching.marching_cubes(volume, marching_time.LEVEL)
    dev = "cuda:0"
    depth, rgb, poses, K = tsdf_time.frames(dev)
    vol = tsdf_time.volume(int(name[4:]), dev)
    vol.integrate(depth, rgb, poses, K)
    return vol.extract_mesh()[:2]


def gpu_case(name, reps):
    import torch

    from marching_time import line, timed

    from dn_splatter_amd import _lib, mesh_clusters
    from dn_splatter_amd._ops import _mesh_filter_args, _stream

    vertices, triangles = mesh(name)
    dev, V, T = triangles.device, vertices.shape[0], triangles.shape[0]
    L = _lib.lib()
    cluster_bytes, filter_bytes = L.dnsplat_mesh_clusters_scratch_bytes(V, T), L.dnsplat_mesh_filter_scratch_bytes(V, T)
    print(f"\ngpu {name}: V = {V} vertices, T = {T} triangles; device {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {reps} repetitions",
          flush=True)
    t = timed(lambda: mesh_clusters.cluster_buffers(triangles, V), reps)
    line("dnsplat_mesh_clusters (8 launches; the scratch allocated per call)", t)
    b = t[3]
    n_clusters, n_valid = b.counts.tolist()
    sizes = b.sizes[:n_clusters]
    print(f"  n_clusters = {n_clusters}, valid triangles = {n_valid}, largest cluster = {int(sizes.max())}, clusters under {MIN_TRIANGLES} triangles = "
          f"{int((sizes < MIN_TRIANGLES).sum())}, status = {b.status.tolist()}", flush=True)
    scratch = torch.empty((filter_bytes + 7) // 8, dtype=torch.int64, device=dev)
    threshold = torch.empty(1, dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    a = _mesh_filter_args(V, triangles, b.labels, b.sizes, b.counts, KEEP_LARGEST, MIN_TRIANGLES, scratch, threshold, counts)
    line("dnsplat_mesh_filter_count (1 memset + 9 launches)", timed(lambda: _lib.run("dnsplat_mesh_filter_count", L.dnsplat_mesh_filter_count,
                                                                                     ctypes.byref(a), _stream()), reps))
    n_v, n_t = counts.tolist()
    vertex_index = torch.empty(n_v, dtype=torch.int32, device=dev)
    out = torch.empty(n_t, 3, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    a = _mesh_filter_args(V, triangles, b.labels, b.sizes, b.counts, KEEP_LARGEST, MIN_TRIANGLES, scratch, threshold, counts, vertex_index, out, status)
    line("dnsplat_mesh_filter_emit (2 launches)", timed(lambda: _lib.run("dnsplat_mesh_filter_emit", L.dnsplat_mesh_filter_emit, ctypes.byref(a),
                                                                         _stream()), reps))
    print(f"  ({KEEP_LARGEST}, {MIN_TRIANGLES}): threshold = {int(threshold.item())}, T' = {n_t} ({100 * (T - n_t) / T:.2f} % of the triangles removed), "
          f"V' = {n_v} ({100 * (V - n_v) / V:.2f} % of the vertices), status = {status.tolist()}", flush=True)
    line("filter_small_clusters: clusters + count + host read + emit + gather", timed(lambda: mesh_clusters.filter_small_clusters(
        (vertices, triangles), KEEP_LARGEST, MIN_TRIANGLES), reps))
    print(f"  scratch: clusters {cluster_bytes / 2 ** 20:.1f} MiB ({cluster_bytes / T:.1f} B per triangle), filter {filter_bytes / 2 ** 20:.1f} MiB",
          flush=True)


def scipy_components(t, n_vertices):
    """The number of components of the valid triangles and the label per triangle: triangle pairs from an edge sort."""
    import numpy as np
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    t = t.astype(np.int64)
    T = t.shape[0]
    valid = ((t >= 0) & (t < n_vertices)).all(axis=1)
    tri = np.repeat(np.arange(T), 3)
    ends = np.stack([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]], axis=1).reshape(-1, 2)
    use = np.repeat(valid, 3) & (ends[:, 0] != ends[:, 1])
    tri, ends = tri[use], np.sort(ends[use], axis=1)
    key = ends[:, 0] * np.int64(n_vertices) + ends[:, 1]
    order = np.argsort(key, kind="stable")
    key, tri = key[order], tri[order]
    same = key[1:] == key[:-1]
    graph = coo_matrix((np.ones(int(same.sum()), dtype=np.int8), (tri[:-1][same], tri[1:][same])), shape=(T, T))
    n, labels = connected_components(graph, directed=False)
    return n - int((~valid).sum()), labels


def cpu_case(name):
    import torch

    vertices, triangles = mesh(name)
    V, T = vertices.shape[0], triangles.shape[0]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = triangles.cpu().numpy()
    copy = time.perf_counter() - t0
    rows = min(T, CPU_ROWS)
    t0 = time.perf_counter()
    n, _ = scipy_components(host[:rows], V)
    seconds = time.perf_counter() - t0
    what = "the whole mesh" if rows == T else f"a SUBSAMPLE, the first {rows} of {T} triangles"
    print(f"\ncpu {name}: device-to-host copy of {T} triangles ({12 * T / 2 ** 20:.0f} MiB) {1e3 * copy:.1f} ms; scipy connected_components over the "
          f"edge-sort pairs on {what}: {seconds:.2f} s, {n} components ({os.cpu_count()} CPUs visible, one used)", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--one", nargs="+")
    ap.add_argument("--cases", default="gpu,cpu")
    a = ap.parse_args()
    if a.one:
        gpu_case(a.one[1], a.reps) if a.one[0] == "gpu" else cpu_case(a.one[1])
    else:
        print("mesh cluster filter: device times by HIP events, median of the repetitions after one warm-up", flush=True)
        for case in CASES:
            if case[0] not in a.cases.split(","):
                continue
            # check=True: a failure raises here and nothing more is started on the device after it
            subprocess.run(["timeout", "-k", "10", str(CASE_SECONDS), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--one"] + case,
                           check=True)
