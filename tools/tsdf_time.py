"""TSDF fusion at the size of the reference's ``gs-mesh o3dtsdf`` exporter: the C2 scene (1 M Gaussians in [-5, 5]^3, eight 1920 x 1080 frames
from the benchmark's orbit) fused into a dense colour volume over the scene's box at 256^3 and 512^3, sdf_trunc = 3 voxels.

  integrate R   ``TSDFVolume.integrate`` (dnsplat_tsdf_integrate, one launch) with 1 and with 8 frames per call: ms per call and per frame,
                beside the bytes the call must move — 20 B read + 20 B written per voxel that a frame of the call updates (8 + 8 without
                colour), plus the frames' pixels once — and the same work done by the PyTorch restatement (torch_tsdf.integrate) on the
                same GPU, the only alternative that runs where Open3D is not installed
  extract R     on the volume fused from the eight frames: ``mc_count`` / ``mc_emit`` over the observed voxels beside the unmasked
                ``mc_count`` / ``mc_emit`` on the same lattice, the whole ``extract_mesh`` (count + host read + emit + colours + world
                mapping), V, T, and the device bytes of the volume and the scratch

Device times: HIP events around the call, median of the repetitions after one warm-up.  Nothing here asserts a speed.

    python tools/tsdf_time.py           # every case in a child process under `timeout -k 10`; stops at the first failure

The output is meant to be kept as profiles/tsdf.txt.
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

N, W, H, FRAMES, HALF = 1_000_000, 1920, 1080, 8, 5.0
CASES = [["integrate", "256"], ["integrate", "512"], ["extract", "256"], ["extract", "512"]]
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
    print(f"  {what:<72s} median {t[0]:10.3f} ms   min {t[1]:10.3f}   max {t[2]:10.3f}", flush=True)


def frames(dev):
    """The eight frames of the benchmark's orbit: (depth [8,H,W], rgb [8,H,W,3], poses [8,3,4], K)."""
    import torch

    import dn_splatter_amd as dns
    from dn_splatter_amd import synthetic

    gp = synthetic.make_gauss_params(N, sh_rest_std=0.1, seed=0, device=dev)
    cameras = [synthetic.orbit_camera(i, n_views=FRAMES, width=W, height=H, focal=1200.0).to(dev) for i in range(FRAMES)]
    renderer = dns.DNSplatterRenderer(gp, fused=True)
    with torch.no_grad():
        outs = list(renderer.get_outputs_batch(cameras, max_batch=FRAMES))
    depth = torch.stack([o["depth"].detach()[..., 0] for o in outs]).float().contiguous()
    rgb = torch.stack([o["rgb"].detach() for o in outs]).float().contiguous()
    poses = torch.stack([c.camera_to_worlds[0] for c in cameras])
    K = [[1200.0, 0.0, W / 2.0], [0.0, 1200.0, H / 2.0], [0.0, 0.0, 1.0]]
    return depth, rgb, poses, K


def volume(R, dev):
    from dn_splatter_amd import tsdf

    voxel = 2.0 * HALF / (R - 1)
    return tsdf.TSDFVolume((-HALF,) * 3, voxel, (R,) * 3, sdf_trunc=3.0 * voxel, depth_trunc=20.0, pixel_offset=0.0, color=True, device=dev)


def integrate_case(R, reps):
    import torch

    from dn_splatter_amd import torch_tsdf
    from dn_splatter_amd.torch_mesh_cull import opencv_w2c

    dev = "cuda:0"
    depth, rgb, poses, K = frames(dev)
    print(f"\nintegrate: {R}^3 = {R ** 3} voxels with colour ({20 * R ** 3 / 2 ** 20:.0f} MiB), {W} x {H} frames, sdf_trunc 3 voxels; device "
          f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}; {reps} repetitions", flush=True)
    for batch in (1, FRAMES):
        vol = volume(R, dev)
        vol.integrate(depth[:batch], rgb[:batch], poses[:batch], K)
        updates = float(vol.weight.sum())                   # the number of (voxel, frame) updates of the call
        touched = int((vol.weight > 0).sum())
        t = timed(lambda: vol.integrate(depth[:batch], rgb[:batch], poses[:batch], K), reps)
        line(f"integrate, {batch} frame(s) per call (one launch)", t)
        must = 40 * touched + batch * W * H * 16 + W * H * 4
        print(f"    {t[0] / batch:.3f} ms per frame; {touched} voxels touched ({100 * touched / R ** 3:.1f} %), {updates:.0f} updates; bytes the call must move "
              f"{must / 2 ** 20:.0f} MiB = {must / t[0] / 1e9:.3f} TB/s at the median", flush=True)
    # the same work by the restatement on the same GPU (fp64 tensors of R^3 elements: one repetition after a warm-up of one frame)
    w2c = opencv_w2c(poses)
    scale = torch_tsdf.ray_scale(K, H, W).to(dev)
    for batch in (1, FRAMES):
        vol = volume(R, dev)
        args = (vol.tsdf, vol.weight, vol.color, vol.origin, vol.voxel_size, w2c[:batch], K, depth[:batch], rgb[:batch], scale, vol.sdf_trunc,
                vol.depth_trunc, vol.pixel_offset)
        t = timed(lambda: torch_tsdf.integrate(*args), 2)
        line(f"torch_tsdf.integrate on the GPU, {batch} frame(s) per call", t)
        print(f"    peak device memory of the restatement {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB", flush=True)


def extract_case(R, reps):
    import torch

    from dn_splatter_amd import marching

    dev = "cuda:0"
    depth, rgb, poses, K = frames(dev)
    vol = volume(R, dev)
    vol.integrate(depth, rgb, poses, K)
    seen = int((vol.weight > 0).sum())
    print(f"\nextract: {R}^3 volume fused from {FRAMES} frames, {seen} voxels observed ({100 * seen / R ** 3:.1f} %); {reps} repetitions", flush=True)
    shape = vol.tsdf.shape
    plain = torch.empty((marching.scratch_bytes(shape) + 7) // 8, dtype=torch.int64, device=dev)
    masked = torch.empty((marching.scratch_bytes(shape, True) + 7) // 8, dtype=torch.int64, device=dev)
    for name, kw, scratch in (("unmasked (the lattice as it is)", {}, plain), ("observed (weight > 0)", {"weight": vol.weight}, masked)):
        t = timed(lambda: marching.mc_count(vol.tsdf, 0.0, scratch, **kw), reps)
        line(f"mc_count, {name}", t)
        count = t[3]
        V, T = count.counts.tolist()
        vertices = torch.empty(V, 3, dtype=torch.float32, device=dev)
        triangles = torch.empty(T, 3, dtype=torch.int32, device=dev)
        line(f"mc_emit, {name}: V = {V}, T = {T}", timed(lambda: marching.mc_emit(count, vertices, triangles), reps))
        del vertices, triangles
    t = timed(lambda: vol.extract_mesh(), reps)
    line("extract_mesh: count + host read + emit + vertex colours + world mapping", t)
    v = t[3][0]
    line("  of which dnsplat_tsdf_vertex_colors", timed(lambda: vol.vertex_colors(v.float()), reps))
    table = sum(x.numel() * 4 for x in vol._ray_scale.values())
    print(f"  device bytes: tsdf + weight {8 * R ** 3 / 2 ** 20:.0f} MiB, colour {12 * R ** 3 / 2 ** 20:.0f} MiB, ray table {table / 2 ** 20:.1f} MiB, "
          f"extraction scratch {masked.numel() * 8 / 2 ** 20:.1f} MiB (unmasked: {plain.numel() * 8 / 2 ** 20:.1f} MiB)", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--one", nargs="+")
    a = ap.parse_args()
    if a.one:
        (integrate_case if a.one[0] == "integrate" else extract_case)(int(a.one[1]), a.reps)
    else:
        print("TSDF fusion: device times by HIP events, median of the repetitions after one warm-up", flush=True)
        for case in CASES:
            # check=True: a failure raises here and nothing more is started on the device after it
            subprocess.run(["timeout", "-k", "10", str(CASE_SECONDS), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--one"] + case,
                           check=True)
