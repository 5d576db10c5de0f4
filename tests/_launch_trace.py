"""Records the sequence of C-ABI calls the op layer (dn-splatter_amd/_ops.py) issues, for tests/test_gpu_op_layer_trace.py.

Every C call of the op layer goes through ``_lib.run(name, fn, *args)``.  ``record()`` replaces it for the duration of one scenario
and appends one entry per call — the entry point, whether the current stream is the one the scenario started on, and every
argument: scalars by value (floats as ``float.hex()``), pointers as "null" / "ptr" (never their value), a ``byref(struct)`` as the
dict of its fields under the same rule, ``RasterArgs.dn`` followed into ``DnPost`` — then calls the real ``run``.

The fixture tests/golden/op_layer_trace.json is what ``python -m tests._launch_trace --write`` recorded on an MI355X with the
op layer as it stood BEFORE its argument builders were factored out: the test pins the launch sequence of that file, call for call
and field for field.  Re-record it only for a change that is meant to alter a launch, never to make a refactor pass.

Every scenario starts from fresh host state (scratch buffers, capacity guesses, bin policy, arena, exchange, switches), so the
grow-only scratch sizes and the capacity guesses among the arguments are functions of the scenario alone.
"""
from __future__ import annotations

import ctypes
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "op_layer_trace.json")
DEV = "cuda:0"
N, W, H, FOCAL = 2000, 96, 64, 60.0       # 6 x 4 tiles

# Fields left out of the comparison because two recordings of the same code differ in them: (struct or entry point, field) -> reason.
# Null-ness of pointers, entry-point names, the order of calls and the stream are never listed here.
EXCLUDED: dict = {}

_CARG = type(ctypes.byref(ctypes.c_int()))


def _value(v):
    if v is None:
        return "null"
    if isinstance(v, bool):
        return int(v)
    if isinstance(v, int):
        return v
    if isinstance(v, float):
        return v.hex()
    if isinstance(v, ctypes.c_void_p):
        return "ptr" if v.value else "null"
    if isinstance(v, _CARG):
        return _struct(v._obj)
    if isinstance(v, ctypes._Pointer):
        return _struct(v.contents) if v else "null"
    if isinstance(v, ctypes.Structure):
        return _struct(v)
    raise TypeError(f"launch trace: argument of type {type(v)}")


def _struct(s):
    out = {}
    for name, ctype in s._fields_:
        if (type(s).__name__, name) in EXCLUDED:
            continue
        v = getattr(s, name)
        if ctype is ctypes.c_void_p:
            out[name] = "ptr" if v else "null"
        else:
            out[name] = _value(v)
    return {type(s).__name__: out}


class Recorder:
    def __init__(self, real_run):
        self.real_run = real_run
        self.entries = []
        self.stream0 = torch.cuda.current_stream().cuda_stream

    def frame(self, k):
        self.entries.append({"frame": k})

    def run(self, name, fn, *args):
        stream = "start" if torch.cuda.current_stream().cuda_stream == self.stream0 else "other"
        self.entries.append({"call": name, "stream": stream,
                             "args": [_value(a) for i, a in enumerate(args) if (name, i) not in EXCLUDED]})
        return self.real_run(name, fn, *args)


def record(scenario):
    """Runs ``scenario(mp)`` (``mp``: a pytest MonkeyPatch the scenario may use for its own settings) from fresh host state and
    returns the list of entries; everything is restored afterwards."""
    from dn_splatter_amd import _lib, _ops

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_ops, "BUFFERS", _ops._Buffers())
        mp.setitem(_ops.BIN_POLICY, "mode", "sync")
        mp.setitem(_ops.DETERMINISTIC, "on", False)
        for name, v in (("GRAD_ARENA", None), ("SH_EXCHANGE", None), ("PAIR_COUNTERS", None), ("KEEP_MASKS", True), ("TIGHT_TILES", True),
                        ("SATURATION_FLAG", True), ("FORWARD_ZERO_FILL", True), ("SKIP_CULLED_RECORDS", True), ("SPLIT_COLOURS", False)):
            mp.setattr(_ops, name, v)
        mp.setattr(_lib, "TIMER", None)
        mp.delenv("DNSPLAT_SH_ZERO_STATE", raising=False)
        rec = Recorder(_lib.run)
        mp.setattr(_lib, "run", rec.run)
        try:
            scenario(rec, mp)
            torch.cuda.synchronize()
            _ops.verify_pending_counts(torch.device(DEV), block=True)
        finally:
            torch.cuda.synchronize()
    return rec.entries


# --------------------------------------------------------------------------------------------------
# scenarios


def _params(seed=0):
    from dn_splatter_amd import synthetic

    gp = synthetic.make_gauss_params(N, sh_rest_std=0.2, seed=seed)
    return {k: v.detach().to(DEV).requires_grad_(k != "normals") for k, v in gp.items()}


def _camera(view=0):
    from dn_splatter_amd import synthetic

    return synthetic.orbit_camera(view, width=W, height=H, focal=FOCAL).to(DEV)


def _clear(tensors):
    for t in tensors:
        t.grad = None


def _dropin(rec, mp, policy="sync", views=(0,), direct=False, frames=3):
    import dn_splatter_amd as dns

    mp.setitem(dns._ops.BIN_POLICY, "mode", policy)
    gp = _params()
    with torch.no_grad():
        quats = gp["quats"] / gp["quats"].norm(dim=-1, keepdim=True)
        colors = torch.sigmoid(gp["features_dc"]) if direct else torch.cat([gp["features_dc"][:, None], gp["features_rest"]], 1)
        inp = [gp["means"], quats, torch.exp(gp["scales"]), torch.sigmoid(gp["opacities"]).squeeze(-1), colors]
    inp = [t.detach().clone().requires_grad_(True) for t in inp]
    cams = [_camera(v) for v in views]
    viewmats = torch.cat([dns.get_viewmat(c.camera_to_worlds) for c in cams])
    Ks = torch.cat([c.get_intrinsics_matrices().to(DEV) for c in cams])
    for k in range(frames):
        rec.frame(k)
        _clear(inp)
        r, a, _info = dns.rasterization(*inp, viewmats, Ks, W, H, packed=False, sh_degree=None if direct else 3,
                                        render_mode="RGB+ED", absgrad=True)
        (r.sum() + a.sum()).backward()


def _fused_loss(out):
    return out["rgb"].sum() + out["depth"].sum() + out["normal"].sum() + out["accumulation"].sum()


def _fused(rec, mp, policy="sync", frames=3, sigmoid_colors=False, pose=False, scales_per_frame=None, arena=False, exchange=None):
    import dn_splatter_amd as dns
    from dn_splatter_amd import _ops, dp
    from dn_splatter_amd.model import RendererConfig

    mp.setitem(_ops.BIN_POLICY, "mode", policy)
    gp = _params()
    cam = _camera()
    if pose:
        cam.camera_to_worlds = cam.camera_to_worlds.detach().clone().requires_grad_(True)
    if arena:
        mp.setenv("DNSPLAT_SH_ZERO_STATE", "1")
        bucket = dp.GradArena(gp)
        assert bucket.sh_state is not None
        mp.setattr(_ops, "GRAD_ARENA", bucket)
    ex = None
    if exchange is not None:
        exchange = dict(exchange)
        deferred = exchange.pop("deferred", False)
        ex = dp.ShFactorExchange(**exchange)
        ex.deferred = deferred
        mp.setattr(_ops, "SH_EXCHANGE", ex)
    m = dns.DNSplatterRenderer(gp, RendererConfig(sh_degree=0) if sigmoid_colors else None, fused=True)
    leaves = [v for k, v in gp.items() if k != "normals"] + ([cam.camera_to_worlds] if pose else [])
    for k in range(frames):
        rec.frame(k)
        _clear(leaves)
        if scales_per_frame is not None:
            with torch.no_grad():
                gp["scales"].fill_(scales_per_frame[k])
        _fused_loss(m.get_outputs(cam)).backward()
        if ex is not None:
            ex.meta = None          # the factors are not rebuilt here: one rank, and the rebuild is not part of the op layer


def _fused_overflow(rec, mp):
    # frame 0: about one tile per Gaussian, so the capacity guess it leaves is at most 1.25 x 2000 + 4096 = 6596; frames 1, 2: the same
    # Gaussians large enough for at least four tiles each — frame 1 outgrows the guess and is emitted and composited a second time
    import math

    _fused(rec, mp, policy="capacity", scales_per_frame=[math.log(0.01), math.log(1.5), math.log(1.5)])


def _split_colours(rec, mp):
    from dn_splatter_amd import _ops

    mp.setattr(_ops, "SPLIT_COLOURS", True)
    _fused(rec, mp)


def _batch(rec, mp):
    from dn_splatter_amd import fused

    gp = _params()
    cams = [_camera(0), _camera(2)]
    bg = torch.tensor([0.1490, 0.1647, 0.2157], device=DEV)
    leaves = [v for k, v in gp.items() if k != "normals"]
    for k in range(3):
        rec.frame(k)
        _clear(leaves)
        out, _info = fused.render_dn_outputs_batch(gp["means"], gp["quats"], gp["scales"], gp["opacities"], gp["features_dc"],
                                                   gp["features_rest"], cams, W, H, sh_degree=3, background_rgb=bg)
        _fused_loss(out).backward()


def _deterministic(inner):
    def scenario(rec, mp):
        from dn_splatter_amd import _ops

        mp.setitem(_ops.DETERMINISTIC, "on", True)
        inner(rec, mp)
    return scenario


def _legacy(rec, mp):
    import dn_splatter_amd as dns

    gp = _params()
    cam = _camera()
    rec.frame("projection")
    with torch.no_grad():
        _r, _a, info = dns.rasterization(gp["means"], gp["quats"] / gp["quats"].norm(dim=-1, keepdim=True), torch.exp(gp["scales"]),
                                         torch.sigmoid(gp["opacities"]).squeeze(-1), torch.sigmoid(gp["features_dc"]),
                                         dns.get_viewmat(cam.camera_to_worlds), cam.get_intrinsics_matrices().to(DEV), W, H,
                                         packed=False, sh_degree=None)
    g = torch.Generator().manual_seed(3)
    leaves = [info["means2d"][0].clone().requires_grad_(True), info["conics"][0].clone().requires_grad_(True),
              torch.rand(N, 3, generator=g).to(DEV).requires_grad_(True), torch.rand(N, 1, generator=g).to(DEV).requires_grad_(True)]
    xys, conics, colors, opacity = leaves
    for k in range(3):
        rec.frame(k)
        _clear(leaves)
        out, alpha = dns.rasterize_gaussians(xys, info["depths"][0], info["radii"][0], conics, info["tiles_per_gauss"][0], colors, opacity,
                                             H, W, 16, return_alpha=True)
        (out.sum() + alpha.sum()).backward()


def _with(fn, **kw):
    return lambda rec, mp: fn(rec, mp, **kw)


SCENARIOS = {
    "dropin_sync": _dropin,
    "dropin_two_cameras_capacity": _with(_dropin, policy="capacity", views=(0, 2)),
    "dropin_direct_colours": _with(_dropin, direct=True),
    "fused_sync": _fused,
    "fused_capacity": _with(_fused, policy="capacity"),
    "fused_deferred": _with(_fused, policy="deferred"),
    "fused_static": _with(_fused, policy="static"),
    "fused_capacity_overflow": _fused_overflow,
    "fused_pose": _with(_fused, pose=True),
    "fused_sigmoid_colours": _with(_fused, sigmoid_colors=True),
    "fused_split_colours": _split_colours,
    "fused_batch_two_cameras": _batch,
    "fused_arena_zero_state": _with(_fused, arena=True, frames=2),
    "fused_exchange_rebuild": _with(_fused, exchange=dict(own_rows=False)),
    "fused_exchange_rebuild_deferred": _with(_fused, exchange=dict(own_rows=False, deferred=True)),
    "fused_exchange_own_rows": _with(_fused, exchange=dict(own_rows=True)),
    "fused_exchange_packed": _with(_fused, exchange=dict(packed=True, capacity=1024)),
    "dropin_sync_deterministic": _deterministic(_dropin),
    "fused_sync_deterministic": _deterministic(_fused),
    "legacy_rasterize_gaussians": _legacy,
}


def _calls(entries, frame, name):
    k, n = None, 0
    for e in entries:
        if "frame" in e:
            k = e["frame"]
        elif k == frame and e["call"] == name:
            n += 1
    return n


def main(argv):
    out = FIXTURE
    if "--out" in argv:
        out = argv[argv.index("--out") + 1]
    if "--write" not in argv:
        raise SystemExit("usage: python -m tests._launch_trace --write [--out FILE]")
    traces = {name: record(fn) for name, fn in SCENARIOS.items()}
    # the branches the scenarios are there to reach: checked when the fixture is written
    over = traces["fused_capacity_overflow"]
    assert _calls(over, 1, "dnsplat_bin_emit_sort") == 2 and _calls(over, 1, "dnsplat_raster_fwd") == 2, "frame 1 did not overflow its guess"
    assert _calls(over, 0, "dnsplat_bin_emit_sort") == 1 and _calls(over, 2, "dnsplat_bin_emit_sort") == 1
    assert _calls(traces["fused_pose"], 0, "dnsplat_project_bwd_pose") == 1
    assert _calls(traces["fused_split_colours"], 0, "dnsplat_project_fwd_colours") == 1
    assert _calls(traces["fused_sync_deterministic"], 0, "dnsplat_det_reduce") == 1
    assert _calls(traces["fused_exchange_rebuild"], 0, "dnsplat_sh_factors") == 1
    assert _calls(traces["fused_exchange_packed"], 0, "dnsplat_visible_index") == 1
    with open(out, "w") as f:          # one entry per line, so that a change shows up as the lines it touches
        f.write("{\n" + ",\n".join(json.dumps(name) + ": [\n" + ",\n".join(json.dumps(e, sort_keys=True, separators=(",", ":")) for e in entries)
                                   + "\n]" for name, entries in sorted(traces.items())) + "\n}\n")
    print(f"wrote {out}: " + ", ".join(f"{k} {sum('call' in e for e in v)}" for k, v in traces.items()))


if __name__ == "__main__":
    main(sys.argv[1:])
