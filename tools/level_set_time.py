"""The level-set ray search at the size of the exporter: one rendered 1920 x 1080 frame of the C2 scene (1 M Gaussians), the fused
renderer's own depth.

  fused      levelset.level_rays (dnsplat_level_rays) with the search inside the kernel and on given neighbours, each with both lane
             mappings (a wave on an 8 x 8 block of pixels / on 64 consecutive pixels); dnsplat_level_points for 10 000 rows in both
             normal modes; the whole levelset.level_surface_points call (20 000 samples per level, three levels)
  unfused    the composition a user has without this module: export.get_colored_points_from_depth, a boolean gather of the pixels with
             depth, GaussianDensityField.closest, the ray step and the 21 samples per ray in torch, GaussianDensityField.density on the
             expanded samples with given neighbours in passes of 2 M samples, torch for the scan of the three levels

The reference's own torch statements are NOT run at this size (profiles/density_field.txt: they ended in an illegal memory access inside
torch's operators); its sklearn search is quoted from that file.  Device times: HIP events around the call, median of the repetitions
after one warm-up; both cases run in the same child process on the same rendered frame.  Nothing here asserts a speed.

    python tools/level_set_time.py        # the cases in one child process under `timeout -k 10`; stops at the first failure

The output is meant to be kept as profiles/level_set.txt.
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, W, H, FOCAL = 1_000_000, 1920, 1080, 1200.0          # bench.py's C2
LEVELS = (0.1, 0.3, 0.5)
ROWS = 10_000
SAMPLES = 20_000
PASS = 2_000_000
CASES = ["both"]
CASE_SECONDS = 480
_FRAME = []


def rendered_frame():
    if not _FRAME:
        _FRAME.append(_render_frame())
    return _FRAME[0]


def _render_frame():
    import torch

    import dn_splatter_amd as dns
    from dn_splatter_amd import synthetic

    gp = synthetic.make_gauss_params(N, sh_rest_std=0.1, seed=0, device="cuda:0")
    cam = synthetic.orbit_camera(0, n_views=8, width=W, height=H, focal=FOCAL).to("cuda:0")
    gp = {k: v.detach() for k, v in gp.items()}
    renderer = dns.DNSplatterRenderer(gp)
    renderer.training = False
    with torch.no_grad():
        out = renderer.get_outputs(cam)
    out = {k: out[k].detach().clone() for k in ("depth", "rgb")}
    torch.cuda.synchronize()
    del renderer
    torch.cuda.empty_cache()
    field = dns.GaussianDensityField(gp["means"], gp["scales"], gp["quats"], gp["opacities"])
    normals = gp["normals"] if "normals" in gp else torch.nn.functional.normalize(torch.randn(N, 3, device="cuda:0"), dim=-1)
    return out, cam, field, gp, normals


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


def head(out):
    import torch

    depth = out["depth"]
    print(f"{W} x {H} = {W * H} pixels, {N} Gaussians, levels {LEVELS}; depth > 0 at {float((depth > 0).float().mean()):.3f} of the pixels; "
          f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}", flush=True)


def fused_case(reps):
    import torch

    from dn_splatter_amd import export, levelset

    out, cam, field, gp, normals = rendered_frame()
    print("\nfused:", end=" ")
    head(out)
    pts, _ = export.get_colored_points_from_depth(out["depth"], out["rgb"], export._export_c2w(cam.camera_to_worlds), cam.fx, cam.fy, cam.cx,
                                                  cam.cy, (W, H))
    nb = field.closest(pts).to(torch.int32)
    results = {}
    for name, given in (("search in the thread", None), ("given neighbours (int32 [P,16])", nb)):
        for lane_map, map_name in ((levelset.MAP_BLOCK, "8 x 8 block per wave"), (levelset.MAP_ROW, "64 pixels of a row per wave")):
            t = timed(lambda: levelset.level_rays(field, out["depth"], cam, surface_levels=LEVELS, neighbors=given, lane_map=lane_map), reps)
            line(f"dnsplat_level_rays, {name}, {map_name}", t)
            results[(name, lane_map)] = t[3]
    first = None
    for r in results.values():
        if first is None:
            first = r
        assert all(torch.equal(r[k].view(torch.int32) if r[k].dtype == torch.float32 else r[k],
                               first[k].view(torch.int32) if first[k].dtype == torch.float32 else first[k]) for k in ("t_hit", "valid", "closest"))
    print(f"  the four variants agree to the bit; hits per level: {[int(v) for v in first['valid'].sum(dim=1)]} of "
          f"{int((first['closest'] >= 0).sum())} participating rays", flush=True)
    scratch = export._scratch(W, H, ROWS, "cuda:0")
    indices, counts = export.sample_valid_pixels(first["valid"][1].reshape(H, W), None, ROWS, 0, scratch)
    bufs = [torch.empty(ROWS, 3, device="cuda:0") for _ in range(3)]
    state = torch.zeros(3, dtype=torch.int64, device="cuda:0")
    for mode in ("closest_gaussian", "analytical"):
        def points():
            state.zero_()
            levelset.level_points(field, out["depth"], out["rgb"], cam, first["t_hit"][1], first["closest"], indices, counts, points=bufs[0],
                                  colors=bufs[1], normals=bufs[2], state=state, gauss_normals=normals, return_normal=mode, scratch=scratch)
        line(f"dnsplat_level_points, {ROWS} rows of level {LEVELS[1]}, {mode}", timed(points, reps))
    for mode in ("closest_gaussian", "analytical"):
        t = timed(lambda: levelset.level_surface_points(field, out, cam, SAMPLES, normals=normals, surface_levels=LEVELS, return_normal=mode), reps)
        line(f"level_surface_points, {SAMPLES} samples per level, {mode} (reads the cursors back)", t)


def unfused_case(reps):
    import torch

    from dn_splatter_amd import export, torch_levelset

    out, cam, field, gp, normals = rendered_frame()
    print("\nunfused:", end=" ")
    head(out)
    c2w = export._export_c2w(cam.camera_to_worlds)
    origin = cam.camera_to_worlds.reshape(3, 4)[:, 3]
    r = torch_levelset.range_table("cuda:0")
    levels = [torch_levelset.level_value(L, torch.float32).to("cuda:0") for L in LEVELS]
    steps = torch.arange(21, device="cuda:0")
    stage = {}

    def run():
        e = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        e[0].record()
        pts, _ = export.get_colored_points_from_depth(out["depth"], out["rgb"], c2w, cam.fx, cam.fy, cam.cx, cam.cy, (W, H))
        pts = pts[out["depth"].reshape(-1) > 0]
        e[1].record()
        nb = field.closest(pts)
        e[2].record()
        dirs = torch.nn.functional.normalize(pts - origin, dim=-1)
        std = torch_levelset.ray_std(gp["means"], gp["scales"], gp["quats"], origin, nb[:, 0])
        T = r[None, :] * std[:, None]
        D = torch.empty(pts.shape[0], 21, device="cuda:0")
        per = PASS // 21
        for i in range(0, pts.shape[0], per):
            s = (pts[i:i + per, None, :] + T[i:i + per, :, None] * dirs[i:i + per, None, :]).reshape(-1, 3)
            n = nb[i:i + per, None, :].expand(-1, 21, -1).reshape(-1, 16)
            D[i:i + per] = field.density(s, closest_gaussians=n).reshape(-1, 21)
        e[3].record()
        hits = []
        for L in levels:
            first = torch.where(D > L, steps[None, :], torch.full_like(steps, 21)[None, :]).min(dim=-1).values
            empty = ~(D[:, 0] < L) | (first == 21) | (first == 0)
            a = torch.where(empty, torch.ones_like(first), first)[:, None]
            Da, Db, Ta, Tb = D.gather(1, a)[:, 0], D.gather(1, a - 1)[:, 0], T.gather(1, a)[:, 0], T.gather(1, a - 1)[:, 0]
            t = (L - Db) / (Da - Db) * (Ta - Tb) + Tb
            hits.append(torch.where(empty, torch.full_like(t, float("nan")), t))
        e[4].record()
        stage["events"] = e
        return hits

    t = timed(run, reps)
    line("back-projection + closest + 21 P densities in passes of 2 M + torch scan", t)
    e = stage["events"]
    names = ("back-projection and the gather of the pixels with depth", "GaussianDensityField.closest ([n,16] int64)",
             "ray step, samples and density on given neighbours, in passes", "torch scan of the three levels")
    for k, name in enumerate(names):
        print(f"    last repetition: {name:<64s} {e[k].elapsed_time(e[k + 1]):10.3f} ms", flush=True)
    print(f"  hits per level: {[int((~torch.isnan(h)).sum()) for h in t[3]]} (get_density floors at 1e-4: a timing baseline, not a restatement)",
          flush=True)
    print("  the reference's own neighbour search for such a batch, quoted from profiles/density_field.txt (sklearn on the host, 2 M queries of\n"
          "  1 M means): 11761.6 ms with n_jobs unset as knn_sk calls it, 5220.9 ms with n_jobs=16", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--one")
    a = ap.parse_args()
    if a.one:
        for case in {"fused": [fused_case], "unfused": [unfused_case], "both": [fused_case, unfused_case]}[a.one]:
            case(a.reps)
    else:
        print("level-set surface points: device times by HIP events, median of the repetitions after one warm-up", flush=True)
        for case in CASES:
            # check=True: a failure raises here and nothing more is started on the device after it
            subprocess.run(["timeout", "-k", "10", str(CASE_SECONDS), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--one", case],
                           check=True)
