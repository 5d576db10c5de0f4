"""Forward + backward of the PearsonDepth branch (whole-frame term + depth_lambda x the local term over the default 128-boxes) at the
two benchmark frame sizes: (a) the reference-shaped PyTorch loop (torch_losses.pearson_depth + local_pearson_depth, which brings
the origins to the host once per step where the reference slices every box with device scalars) against (b) the HIP path (fused_loss.pearson_depth_combined on
dnsplat_pearson_depth).  Both draw their origins with the two randint calls of the reference, on the device, every step.

    python tools/pearson_timing.py                      # times: regions of (a) and (b) alternate; medians and spread of the regions
    python tools/pearson_timing.py --launches OUT_DIR   # kernel launches per step from rocprofv3 --kernel-trace --stats (child runs)

Both outputs together are meant to be kept as profiles/pearson_depth_loss.txt.
"""
import argparse
import csv
import glob
import os
import signal
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(1920, 1080), (1600, 1200)]
LAMBDA = 0.2
CALIBRATION_STEPS = 5       # steps timed after the warm-up to size the timed regions
REGION_SECONDS = 0.25
TRACE_SECONDS = 150         # limit of one traced child run


def make_step(variant, W, H):
    import torch

    from dn_splatter_amd import fused_loss, torch_losses

    g = torch.Generator().manual_seed(W)
    p = torch.rand(H, W, 1, generator=g) * 4 + 1
    gt = (0.6 * p + 1.5 * torch.rand(H, W, 1, generator=g) + 0.3).to("cuda:0")
    pred = p.to("cuda:0").requires_grad_(True)

    def step():
        pred.grad = None
        rows, cols = fused_loss.draw_pearson_boxes(pred)
        if variant == "a":
            loss = torch_losses.pearson_depth(pred, gt) + LAMBDA * torch_losses.local_pearson_depth(pred, gt, rows, cols)
        else:
            loss = fused_loss.pearson_depth_combined(pred, gt, rows, cols, 128, 1.0, LAMBDA)
        loss.backward()
        return loss

    return step, pred


def time_all(regions, warmup):
    import torch

    assert torch.cuda.is_available(), "needs the GPU: nothing is timed on a CPU"
    print(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    for W, H in SIZES:
        n_corr = int(0.5 * (H // 128) * (W // 128))
        steps = {v: make_step(v, W, H) for v in "ab"}
        torch.manual_seed(0)
        la = steps["a"][0](); ga = steps["a"][1].grad.clone()
        torch.manual_seed(0)
        lb = steps["b"][0](); gb = steps["b"][1].grad.clone()
        torch.cuda.synchronize()
        print(f"\n{W} x {H}, {n_corr} boxes of 128: same seed, (a) {float(la):.7f}  (b) {float(lb):.7f}; "
              f"largest gradient difference {float((ga - gb).abs().max()):.2e} of {float(ga.abs().max()):.2e}")
        iters = {}
        for v in "ab":
            for _ in range(warmup):
                steps[v][0]()
            torch.cuda.synchronize()
            t = time.perf_counter()                                 # calibration: a region lasts about REGION_SECONDS
            for _ in range(CALIBRATION_STEPS):
                steps[v][0]()
            torch.cuda.synchronize()
            per_step = (time.perf_counter() - t) / CALIBRATION_STEPS
            iters[v] = max(CALIBRATION_STEPS, min(5000, round(REGION_SECONDS / per_step)))
        ms = {"a": [], "b": []}
        for _ in range(regions):                                    # alternating, so that drift of the machine reaches both
            for v in "ab":
                t = time.perf_counter()
                for _ in range(iters[v]):
                    steps[v][0]()
                torch.cuda.synchronize()
                ms[v].append((time.perf_counter() - t) * 1e3 / iters[v])
        for v, name in (("a", "(a) PyTorch loop"), ("b", "(b) HIP path    ")):
            m = ms[v]
            print(f"  {name}: median {statistics.median(m):9.4f} ms / step   min {min(m):9.4f}   max {max(m):9.4f}   "
                  f"({regions} regions of {iters[v]} steps, host clock around a device synchronise)")
        print(f"  median (a) / median (b) = {statistics.median(ms['a']) / statistics.median(ms['b']):.1f}")


def traced(variant, W, H, n):
    step, _ = make_step(variant, W, H)
    import torch

    for _ in range(n):
        step()
    torch.cuda.synchronize()


def run_group(cmd):
    """Run ``cmd`` in a process group of its own; at the time limit the whole group goes (the profiler AND the program it started)."""
    child = subprocess.Popen(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, start_new_session=True)
    try:
        rc = child.wait(timeout=TRACE_SECONDS)
    except subprocess.TimeoutExpired:
        os.killpg(child.pid, signal.SIGKILL)
        child.wait()
        raise
    if rc != 0:
        raise subprocess.CalledProcessError(rc, cmd)


def launches(out_dir):
    """Kernel dispatches per step: the difference between a traced run of 3 steps and one of 1 step, halved (set-up cancels)."""
    os.makedirs(out_dir, exist_ok=True)
    for W, H in SIZES:
        for v in "ab":
            counts, names = {}, {}
            for n in (1, 3):
                d = os.path.join(out_dir, f"trace_{v}_{W}x{H}_{n}")
                run_group(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--",
                           sys.executable, os.path.abspath(__file__), "--traced", v, str(W), str(H), str(n)])
                rows = [r for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True) for r in csv.DictReader(open(f))]
                counts[n] = len(rows)
                names[n] = {}
                for r in rows:
                    k = r.get("Kernel_Name", "")
                    names[n][k] = names[n].get(k, 0) + 1
            per_step = (counts[3] - counts[1]) / 2
            ours = {k: (c - names[1].get(k, 0)) / 2 for k, c in names[3].items() if "pearson" in k}
            print(f"{W} x {H} ({v}): {per_step:.0f} kernel launches per forward + backward step"
                  + (f", of which pearson.hip: {sum(ours.values()):.0f} ({', '.join(sorted(k.split('(')[0].split('::')[-1] for k in ours))})" if ours else ""))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", metavar="OUT_DIR")
    ap.add_argument("--traced", nargs=4, metavar=("VARIANT", "W", "H", "STEPS"))
    a = ap.parse_args()
    if a.traced:
        traced(a.traced[0], int(a.traced[1]), int(a.traced[2]), int(a.traced[3]))
    elif a.launches:
        launches(a.launches)
    else:
        time_all(a.regions, a.warmup)
