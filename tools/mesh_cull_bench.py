"""The mesh visibility culling at the size the project's meshes have: the marching-cubes mesh of the C2 scene's law (tools/density_time.py's
scene, ``marching_cubes_mesh`` at 256^3, level 0.5: 4.49 M vertices, 8.96 M triangles), 1920 x 1080 frames, an 8-pose orbit inside
the scene's box.

  gpu     ``render_mesh_depth`` (dnsplat_mesh_depth, all 8 poses in one call, reported per camera), ``vertex_visibility``
          (dnsplat_mesh_visibility, likewise), ``cut_mesh`` (count, the host read of (V', T'), emit) and the whole ``cull_mesh``.  The four
          are replayed in turn inside one loop (paired: every round runs each of them once on the same inputs, so a drift of the box
          reaches all four alike); the median of the rounds after one warm-up round is reported, with min and max.
          Beside them, from the counters of dnsplat_mesh_depth (``stats``), per camera: the triangle setups that kept a non-empty pixel
          box, the accepted fragments (pixel tests that passed edge functions and depth range) and the atomics issued behind the
          plain-load filter; and from those the fragment rate and the atomic rate.  These two rates are what decides whether a
          tile-binned z-buffer in LDS is worth building.
  numpy   the reference's way for the votes on this box's CPU: the loop of get_grid_culling_pattern restated in numpy (per pose: the
          projection of every vertex in float64, the two depth look-ups), host clock, on a 200 000-vertex subsample of the mesh with the
          device's depth maps, and the line says so.  The reference's depth render (pyrender through OpenGL / EGL) cannot run here at all.

Nothing here asserts a speed.

    python tools/mesh_cull_bench.py       # every case in a child process under `timeout -k 10`; stops at the first failure

The output is meant to be kept as profiles/mesh_cull.txt.
"""
import argparse
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HEIGHT, WIDTH, FOCAL = 1080, 1920, 1200.0
POSES, ORBIT_RADIUS, ORBIT_HEIGHT = 8, 3.0, 0.4
OBS_THRESHOLD = 0          # the reference's 3 is meant for hundreds of frames; on 8 poses it keeps nothing of a foam, and a cut that keeps nothing emits nothing
SUBSAMPLE = 200_000
LONG_CALL_MS = 5_000.0
CASES = [["gpu"], ["numpy"]]
CASE_SECONDS = 420


def intrinsics():
    import numpy as np

    return np.array([[FOCAL, 0.0, WIDTH / 2], [0.0, FOCAL, HEIGHT / 2], [0.0, 0.0, 1.0]])


def orbit():
    """POSES camera-to-world matrices (OpenGL: the camera looks down -z, y up) on a circle around the origin, looking at it."""
    import numpy as np

    poses = []
    for i in range(POSES):
        a = 2 * math.pi * i / POSES
        eye = np.array([ORBIT_RADIUS * math.cos(a), ORBIT_HEIGHT, ORBIT_RADIUS * math.sin(a)])
        back = eye / np.linalg.norm(eye)
        right = np.cross([0.0, 1.0, 0.0], back)
        right /= np.linalg.norm(right)
        c2w = np.eye(4)
        c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, np.cross(back, right), back, eye
        poses.append(c2w)
    return np.stack(poses)


def mesh():
    import geometry_bench

    return geometry_bench.mesh()


def event_ms(fn):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def line(what, ms, per=1):
    ms = [m / per for m in ms]
    print(f"  {what:<76s} median {statistics.median(ms):10.3f} ms   min {min(ms):10.3f}   max {max(ms):10.3f}", flush=True)


def gpu_case(reps):
    import torch

    from dn_splatter_amd import mesh_cull

    vertices, triangles = mesh()
    poses, K = orbit(), intrinsics()
    V, T = vertices.shape[0], triangles.shape[0]
    print(f"\ngpu: a mesh of {V} vertices / {T} triangles, {POSES} poses on an orbit of radius {ORBIT_RADIUS}, frames {WIDTH} x {HEIGHT}, "
          f"focal {FOCAL:.0f}; device {torch.cuda.get_device_name(0)}, torch {torch.__version__}", flush=True)
    # a pilot on ONE camera first: a kernel that would run for minutes is not repeated on a shared device
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stats = torch.zeros(3, dtype=torch.int64, device=vertices.device)
    mesh_cull.render_mesh_depth(vertices, triangles, poses[:1], K, HEIGHT, WIDTH, stats=stats)
    torch.cuda.synchronize()
    pilot = (time.perf_counter() - t0) * 1e3
    print(f"  pilot: one camera, first call, host clock {pilot:.1f} ms; counters {stats.tolist()}", flush=True)
    if pilot > LONG_CALL_MS:
        print("  the repetitions are NOT run: one camera takes longer than 5 s", flush=True)
        return
    depth = mesh_cull.render_mesh_depth(vertices, triangles, poses, K, HEIGHT, WIDTH)
    gt = depth.clone()
    gt[:, :HEIGHT // 8] = 0.0                                                     # a sensor that saw nothing in the upper eighth
    obs, invalid = mesh_cull.vertex_visibility(vertices, poses, K, HEIGHT, WIDTH, depth, gt)
    calls = {
        "depth": lambda: mesh_cull.render_mesh_depth(vertices, triangles, poses, K, HEIGHT, WIDTH, out=depth),
        "votes": lambda: mesh_cull.vertex_visibility(vertices, poses, K, HEIGHT, WIDTH, depth, gt),
        "cut": lambda: mesh_cull.cut_mesh(vertices, triangles, obs, invalid, obs_threshold=OBS_THRESHOLD),
        "cull": lambda: mesh_cull.cull_mesh((vertices, triangles), poses, K, HEIGHT, WIDTH, depth_gt=gt, camera_batch=POSES,
                                            obs_threshold=OBS_THRESHOLD),
    }
    ms = {k: [] for k in calls}
    out = {}
    for r in range(reps + 1):
        for k, fn in calls.items():
            t, out[k] = event_ms(fn)
            if r:
                ms[k].append(t)
    print(f"  {reps} paired rounds after one warm-up round", flush=True)
    line(f"render_mesh_depth, per camera (one dnsplat_mesh_depth call of {POSES})", ms["depth"], POSES)
    line(f"vertex_visibility, per camera (one dnsplat_mesh_visibility call of {POSES})", ms["votes"], POSES)
    line(f"cut_mesh at obs > {OBS_THRESHOLD}: count + host read of V', T' + allocate + emit", ms["cut"])
    line(f"cull_mesh at obs > {OBS_THRESHOLD}: the {POSES} poses in one batch, votes, cut", ms["cull"])
    print(f"    covered pixels {100.0 * float((depth > 0).double().mean()):.1f} %; obs > 3 for {int((obs > 3).sum())} vertices, obs > {OBS_THRESHOLD} for "
          f"{int((obs > OBS_THRESHOLD).sum())}; the cut keeps {out['cull'][0].shape[0]} vertices / {out['cull'][1].shape[0]} triangles", flush=True)
    stats.zero_()
    mesh_cull.render_mesh_depth(vertices, triangles, poses, K, HEIGHT, WIDTH, out=depth, stats=stats)
    setups, fragments, atomics = (s / POSES for s in stats.tolist())
    ms_counted = [event_ms(lambda: mesh_cull.render_mesh_depth(vertices, triangles, poses, K, HEIGHT, WIDTH, out=depth, stats=stats))[0]
                  for _ in range(max(3, reps // 4))]
    per_camera_s = statistics.median(ms["depth"]) / POSES * 1e-3
    print(f"    per camera: {setups:.0f} setups with a pixel box ({100.0 * setups / T:.1f} % of the triangles), {fragments:.0f} accepted fragments "
          f"({fragments / (WIDTH * HEIGHT):.1f} per pixel), {atomics:.0f} atomics issued ({100.0 * atomics / max(fragments, 1):.1f} % of the fragments)",
          flush=True)
    print(f"    fragment rate {fragments / per_camera_s / 1e9:.2f} G fragments/s, atomic rate {atomics / per_camera_s / 1e9:.3f} G atomics/s, "
          f"setup rate {T / per_camera_s / 1e9:.2f} G (camera, triangle) pairs/s (all three over the whole call: setup, walk and atomics overlap)",
          flush=True)
    line("  the same call with the counters on, per camera", ms_counted, POSES)


def numpy_votes(points, w2c, K, depth, gt):
    """get_grid_culling_pattern restated in numpy: float64 projection, the two look-ups, summed over the poses."""
    import numpy as np

    H, W = depth.shape[1:]
    obs, invalid = np.zeros(len(points)), np.zeros(len(points))
    for c in range(len(w2c)):
        M = w2c[c].reshape(3, 4)
        uvz = (K @ (M[:, :3] @ points.T + M[:, 3:])).T
        pz = uvz[:, 2] + 1e-8
        px, py = uvz[:, 0] / pz, uvz[:, 1] / pz
        inside = (0 <= px) & (px <= W - 1) & (0 <= py) & (py <= H - 1) & (pz > 0)
        u, v = np.clip(px, 0, W - 1).astype(np.int32), np.clip(py, 0, H - 1).astype(np.int32)
        obs += inside & (pz < depth[c][v, u] + 0.02)
        invalid += inside & (gt[c][v, u] <= 0.0)
    return obs, invalid


def numpy_case():
    import numpy as np
    import torch

    from dn_splatter_amd import mesh_cull, torch_mesh_cull

    vertices, triangles = mesh()
    poses, K = orbit(), intrinsics()
    depth = mesh_cull.render_mesh_depth(vertices, triangles, poses, K, HEIGHT, WIDTH)
    rows = np.random.default_rng(0).choice(vertices.shape[0], SUBSAMPLE, replace=False)
    sub = vertices[torch.from_numpy(rows).to(vertices.device)].contiguous()
    want = mesh_cull.vertex_visibility(sub, poses, K, HEIGHT, WIDTH, depth, depth)
    points, maps = sub.cpu().numpy().astype(np.float64), depth.cpu().numpy()
    w2c = torch_mesh_cull.opencv_w2c(poses).numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        t0 = time.perf_counter()
        obs, invalid = numpy_votes(points, w2c, K, maps, maps)
        t1 = time.perf_counter()
    differ = int((obs != want[0].cpu().numpy()).sum())
    print(f"\nnumpy (the vote loop of get_grid_culling_pattern, host clock): a SUBSAMPLE of {SUBSAMPLE} vertices, not the {vertices.shape[0]}; "
          f"{POSES} poses", flush=True)
    print(f"  {1e3 * (t1 - t0):10.1f} ms = {1e3 * (t1 - t0) / POSES:.1f} ms per camera ({differ} of {SUBSAMPLE} vote counts differ from the device's); the "
          f"reference does this on every vertex, after copying the maps to the host", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--one", nargs="+")
    a = ap.parse_args()
    if a.one:
        gpu_case(a.reps) if a.one[0] == "gpu" else numpy_case()
    else:
        print("Mesh visibility culling: device times by HIP events, median of paired rounds after one warm-up round", flush=True)
        for case in CASES:
            # check=True: a failure raises here and nothing more is started on the device after it
            subprocess.run(["timeout", "-k", "10", str(CASE_SECONDS), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--one"] + case,
                           check=True)
