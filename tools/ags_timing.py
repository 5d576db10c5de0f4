"""Forward + backward of the AGS-Mesh normal loss (AGSMeshRegularization.get_normal_loss) at the two benchmark frame sizes, in both
modes (the edge map before normal_mask_steps, the confidence filter from then on): (a) torch_losses.ags_normal_loss on the device —
the PyTorch restatement tests/golden/reference_ags.npz pins to the reference, with its conv-shaped stencils and its two
boolean-mask gathers — against (b) fused_loss.ags_normal_loss on dnsplat_ags_normal_loss.  The surface normal is detached and the
predicted normal requires its gradient, as the model calls the method.

Per variant: time per call (host clock around a device synchronise, regions of (a) and (b) alternating), the time the HOST is held
inside one call that starts on an idle device (with a synchronising gather that is the device time up to the gather; without one it
is the launch overhead), and the number of host synchronisations per call (torch's synchronisation check in "warn" mode).

    python tools/ags_timing.py          # every (size, mode) in a child process of its own, each under a time limit; stops at the
                                        # first one that fails

The output is meant to be kept as profiles/ags_mesh_loss.txt.
"""
import argparse
import os
import signal
import statistics
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = [(1920, 1080), (1600, 1200)]
MODES = [("edge map", 8000), ("confidence", 20000)]
CALIBRATION_STEPS = 5       # steps timed after the warm-up to size the timed regions
REGION_SECONDS = 0.25
CASE_SECONDS = 120          # limit of one child (one size, one mode, both variants)
HOST_SAMPLES = 15


def make_step(variant, W, H, step_no):
    import torch

    import _ags_inputs as inputs
    from dn_splatter_amd import fused_loss, torch_losses

    _, surf, gt, pred = inputs.normal_inputs(H, W)
    surf, gt = surf.to("cuda:0"), gt.to("cuda:0")
    pred = pred.to("cuda:0").requires_grad_(True)
    fn = torch_losses.ags_normal_loss if variant == "a" else fused_loss.ags_normal_loss

    def step():
        pred.grad = None
        loss = fn(surf, gt, pred, step_no)
        loss.backward()
        return loss

    return step, pred


def one(W, H, mode, regions, warmup):
    import torch

    assert torch.cuda.is_available(), "needs the GPU: nothing is timed on a CPU"
    name, step_no = MODES[mode]
    steps = {v: make_step(v, W, H, step_no) for v in "ab"}
    la = steps["a"][0](); ga = steps["a"][1].grad.clone()
    lb = steps["b"][0](); gb = steps["b"][1].grad.clone()
    torch.cuda.synchronize()
    print(f"\n{W} x {H}, {name} (step {step_no}): (a) {float(la):.7f}  (b) {float(lb):.7f}; "
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
    host, syncs = {}, {}
    for v in "ab":
        h = []
        for _ in range(HOST_SAMPLES):                           # one call on an idle device: how long the host is held in it
            torch.cuda.synchronize()
            t = time.perf_counter()
            steps[v][0]()
            h.append((time.perf_counter() - t) * 1e3)
        torch.cuda.synchronize()
        host[v] = statistics.median(h)
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                steps[v][0]()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        syncs[v] = sum("synchroniz" in str(w.message).lower() for w in seen)
        torch.cuda.synchronize()
    for v, label in (("a", "(a) PyTorch restatement"), ("b", "(b) HIP path           ")):
        m = ms[v]
        print(f"  {label}: median {statistics.median(m):8.4f} ms / call   min {min(m):8.4f}   max {max(m):8.4f}   "
              f"({regions} regions of {iters[v]} calls); host held {host[v]:7.4f} ms in a call on an idle device; "
              f"{syncs[v]} host synchronisations per call")
    print(f"  median (a) / median (b) = {statistics.median(ms['a']) / statistics.median(ms['b']):.1f}")


def run_case(cmd):
    """Run ``cmd`` in a process group of its own under CASE_SECONDS; at the limit the whole group goes."""
    child = subprocess.Popen(cmd, start_new_session=True)
    try:
        rc = child.wait(timeout=CASE_SECONDS)
    except subprocess.TimeoutExpired:
        os.killpg(child.pid, signal.SIGKILL)
        child.wait()
        raise
    if rc != 0:
        raise subprocess.CalledProcessError(rc, cmd)


def time_all(regions, warmup):
    print("forward + backward of get_normal_loss; time per call by the host clock around a device synchronise", flush=True)
    for W, H in SIZES:
        for mode in range(len(MODES)):
            # a failure raises here: nothing more is started on the device after it
            run_case([sys.executable, os.path.abspath(__file__), "--one", str(W), str(H), str(mode), "--regions", str(regions),
                      "--warmup", str(warmup)])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--one", nargs=3, metavar=("W", "H", "MODE"))
    a = ap.parse_args()
    if a.one:
        import torch

        if a.one[2] == "0" and a.one[:2] == [str(SIZES[0][0]), str(SIZES[0][1])]:
            print(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
        one(int(a.one[0]), int(a.one[1]), int(a.one[2]), a.regions, a.warmup)
    else:
        time_all(a.regions, a.warmup)
