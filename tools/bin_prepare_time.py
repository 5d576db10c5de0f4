"""Time of dnsplat_bin_prepare (depth order, scans, emit records) alone at Gaussian counts bench.py has no workload for:
    DNSPLAT_LIB=... [DNSPLAT_BIN_DEPTH_SORT=partition] python tools/bin_prepare_time.py 2000000 3000000 3900000
Random-init scene of bench.py (synthetic.make_gauss_params, orbit camera 0 of 8, 1600x1200, focal 1200), fused forward under
no_grad; the stage is bracketed with HIP events (_lib.StageTimer).  Prints one line per count: median and min / max over the frames."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dn_splatter_amd as dns  # noqa: E402
from dn_splatter_amd import _lib, synthetic  # noqa: E402

FRAMES, WARMUP = 24, 4
dev = torch.device("cuda", 0)
tag = os.environ.get("TAG", os.path.basename(os.environ.get("DNSPLAT_LIB", "libdnsplat.so")))
for n in [int(a) for a in sys.argv[1:]]:
    gp = synthetic.make_gauss_params(n, sh_rest_std=0.1, seed=0, device=dev)
    cam = synthetic.orbit_camera(0, n_views=8, width=1600, height=1200, focal=1200.0).to(dev)
    m = dns.DNSplatterRenderer(gp, fused=True)
    with torch.no_grad():
        for _ in range(WARMUP):
            m.get_outputs(cam)
        torch.cuda.synchronize()
        _lib.TIMER = _lib.StageTimer(only={"dnsplat_bin_prepare"})
        for _ in range(FRAMES):
            m.get_outputs(cam)
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in _lib.TIMER.events["dnsplat_bin_prepare"]]
        _lib.TIMER = None
    visible = int((m.last_info["radii"] > 0).sum())
    print(f"{tag} | N {n} visible {visible} | bin_prepare median {statistics.median(ms) * 1e3:.1f} us  min {min(ms) * 1e3:.1f}  max {max(ms) * 1e3:.1f}  ({len(ms)} frames)")
    del m, gp
    torch.cuda.empty_cache()
