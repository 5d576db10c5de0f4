"""The kernels of the SH gradient exchange (csrc/project.hip), each called directly and held per row: ``visible_mask_kernel`` +
``visible_scan_kernel`` (dnsplat_visible_index), ``sh_factors_kernel`` (dnsplat_sh_factors), the slab writes of ``project_bwd_kernel``
(dnsplat_proj_grads.sh_factors / sh_packed) and the twelve instantiations of ``sh_from_factors_kernel`` (dnsplat_sh_grads_from_factors,
_add_factors, _from_packed: SPLIT / CAT / DIRECT layout x dense / packed slabs x rebuild / add).  No multi-rank hardware run
exercises them, and the whole-pipeline tests of test_gpu_parity.py run them at one size each under a frame-level
tolerance; here every index, mask and select is compared as bits with its restatement in tests/_dp_ref.py, and every rebuilt row
with ``rebuild_ref64`` under  ||row error||_2 <= KAPPA 2^-24 ||A_row||_2  (KAPPA comes from the CPU measurement in
test_sh_exchange_reference.py, not from what the kernels give).  The only other tolerance is the camera centre's rounding bound.

Every case asserts, from the constants below, that its size lies on the side of the edge it is named for;
``test_constants_are_the_kernels`` reads the constants out of the sources."""
import os
import re

import pytest
import torch

import _dp_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
U24 = 2.0 ** -24

WAVE = 64                       # splat_common.h DNS_WAVE: Gaussians per mask word
STAGE_THREADS = 64              # project.hip SH_STAGE_THREADS = DNS_WAVE: Gaussians per workgroup of the rebuild kernels
REC_CH0 = 6                     # splat_common.h: the first colour channel of a record
REC = 16                        # include/dnsplat.h DNSPLAT_RECORD_FLOATS
SCAN_THREADS = 1024             # project.hip VIS_SCAN_THREADS: visible_scan_kernel's one workgroup
FLAT_THREADS = 256              # visible_mask_kernel, sh_factors_kernel: threads per workgroup, on a grid of (N + 256) / 256
GUARD = 64                      # words (or rows) behind every buffer a kernel writes, which must keep their contents
SENTINEL = 0x7FC0BEEF           # a NaN with a payload, as int32

INDEX_N = (1, 63, 64, 65, 65_536, 65_537, 1_000_003)
FACTOR_N = (1, 255, 256, 257)
DEGREES = (0, 1, 2, 3)


def _ceil(a, b):
    return (a + b - 1) // b


def _api():
    from dn_splatter_amd import _lib, _ops

    return _lib, _ops._ptr, _ops._stream


def _bits(t):
    return t.contiguous().view(torch.int32)


def _viewmat(seed):
    """A world-to-camera matrix [4,4] float32: a random rotation (not exactly orthonormal once rounded) and translation."""
    g = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    vm = torch.eye(4, dtype=torch.float64)
    vm[:3, :3], vm[:3, 3] = q, torch.randn(3, generator=g, dtype=torch.float64) * 5
    return vm.float().contiguous()


def _assert_centre(got, vm, what):
    """-R^T t of the float32 matrix in float64; three products and two sums, one unit of slack for contraction."""
    R, t = vm[:3, :3].double(), vm[:3, 3].double()
    terms = R * t[:, None]                                                       # [i, j] = R_ij t_i
    want, bound = -terms.sum(0), 4 * U24 * terms.abs().sum(0)
    err = (got.double().cpu() - want).abs()
    assert bool((err <= bound).all()), (what, err.tolist(), bound.tolist())


# ---- 0. constants --------------------------------------------------------------------------------------------------------------------


def _index_patterns(N):
    """(name, radii [N] int32, capacities) of section 1.  Capacities: that of a slab with room, exactly the visible count, one less,
    none."""
    g = torch.Generator().manual_seed(8100 + N % 997)
    size = torch.randint(1, 50, (N,), generator=g, dtype=torch.int32)
    seen = torch.rand(N, generator=g) < 0.72
    zero = torch.zeros(N, dtype=torch.int32)
    block = torch.arange(N) // WAVE
    only_first, only_last = zero.clone(), zero.clone()
    only_first[0], only_last[-1] = 3, 7
    patterns = [("random", torch.where(seen, size, zero)), ("none", zero), ("all", size), ("first", only_first), ("last", only_last),
                ("culled_blocks", torch.where(seen & (block % 3 != 1) & (block % 7 != 4), size, zero)),
                ("negative", torch.where(seen, size, -size))]
    out = []
    for name, radii in patterns:
        count = int((radii > 0).sum())
        out.append((name, radii.contiguous(), sorted({N, count, max(count - 1, 0), 0})))
    return out


def test_constants_are_the_kernels(dns):
    """The constants the cases below reason from are the ones the sources compile, and the slab layout of _dp_ref.packed_layout is
    dns_packed_rows_offset / dns_packed_slab_words, dnsplat_packed_slab_floats and dp.ShFactorExchange.slab_floats."""
    from dn_splatter_amd import _lib, dp

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
    project = open(os.path.join(csrc, "project.hip")).read()
    common = open(os.path.join(csrc, "splat_common.h")).read()
    header = open(os.path.join(root, "include", "dnsplat.h")).read()

    def rhs(text, name):
        found = re.search(r"(?:constexpr int|#define)\s+" + name + r"\b\s*=?\s*([^;\n/]+)", text)
        assert found, name
        return found.group(1).strip()

    assert int(rhs(common, "DNS_WAVE")) == WAVE and int(rhs(common, "REC_CH0")) == REC_CH0
    assert rhs(common, "DNS_REC") == "DNSPLAT_RECORD_FLOATS" and int(rhs(header, "DNSPLAT_RECORD_FLOATS")) == REC
    assert rhs(project, "SH_STAGE_THREADS") == "DNS_WAVE" and int(rhs(common, "DNS_WAVE")) == STAGE_THREADS == WAVE
    assert int(rhs(project, "VIS_SCAN_THREADS")) == SCAN_THREADS
    assert "__launch_bounds__(VIS_SCAN_THREADS) void visible_scan_kernel(" in project
    assert "hipLaunchKernelGGL(visible_scan_kernel, dim3(1), dim3(VIS_SCAN_THREADS)," in project
    assert "const int per = (nblk + VIS_SCAN_THREADS - 1) / VIS_SCAN_THREADS;" in project
    for kernel in ("visible_mask_kernel", "sh_factors_kernel"):
        assert f"__launch_bounds__({FLAT_THREADS}) void {kernel}(" in project, kernel
        assert f"hipLaunchKernelGGL({kernel}, dim3((N + {FLAT_THREADS}) / {FLAT_THREADS}), dim3({FLAT_THREADS})," in project, kernel
    assert "__launch_bounds__(SH_STAGE_THREADS) void sh_from_factors_kernel(" in project
    assert re.search(r"dns_packed_rows_offset\(int nb\) \{ return \(\(size_t\)8 \+ 3 \* \(size_t\)nb \+ 3\) & ~\(size_t\)3; \}", project)
    assert "return (dns_packed_rows_offset(nb) + 3 * (size_t)capacity + 3) & ~(size_t)3;" in project

    pairs = set()
    for N in INDEX_N:
        for _, _, caps in _index_patterns(N):
            pairs |= {(N, c) for c in caps}
    for n, w in ref.EXCHANGE_CASES + (ref.EXCHANGE_BIG,):
        inp = ref.exchange_inputs(n, w)
        pairs |= {(n, cap) for _, _, cap, _ in ref.exchange_forms(inp) if cap is not None}
    pairs |= {(5003, c) for c in (0, 1, 4998, 5003)}                            # the frame of section 3 (its capacities depend on the render)
    assert len(pairs) > 40
    for N, cap in sorted(pairs):
        nb, rows0, total = ref.packed_layout(N, cap)
        assert nb == _ceil(N, WAVE) and rows0 == (8 + 3 * nb + 3) // 4 * 4 and total == (rows0 + 3 * cap + 3) // 4 * 4
        assert _lib.lib().dnsplat_packed_slab_floats(N, cap) == total, (N, cap)
        assert dp.ShFactorExchange(packed=True, capacity=cap).slab_floats(N) == total, (N, cap)


# ---- 1. dnsplat_visible_index ----------------------------------------------------------------------------------------------------------


def _assert_index_edge(N):
    nblk = _ceil(N, WAVE)
    per = _ceil(nblk, SCAN_THREADS)
    busy = _ceil(nblk, per)                                                      # threads of the scan with a non-empty range
    last = busy - 1
    last_len = min(nblk, last * per + per) - last * per
    if N == 1:
        assert nblk == 1 and N < WAVE
    elif N == 63:
        assert nblk == 1 and N == WAVE - 1
    elif N == 64:
        assert nblk == 1 and N == WAVE
    elif N == 65:
        assert nblk == 2 and N == WAVE + 1 and per == 1
    elif N == 65_536:
        assert nblk == SCAN_THREADS and per == 1 and busy == SCAN_THREADS and N % WAVE == 0
    elif N == 65_537:
        assert nblk == SCAN_THREADS + 1 and per == 2 and busy == SCAN_THREADS // 2 + 1 and last == 512 and last_len == 1 < per
    elif N == 1_000_003:
        assert (nblk, per) == (15_626, 16) and busy < SCAN_THREADS and last * per + per > nblk and 0 < last_len < per
    else:
        raise KeyError(N)
    return nblk, per


@pytest.mark.parametrize("N", INDEX_N)
def test_visible_index_bytes_equal_the_restatement(dns, N):
    """Header words 0 and 4 .. 7, every mask word and every offset against pack_slab_ref, as bits; the rows region and the guard behind
    the slab untouched; the camera centre the bits dnsplat_sh_factors writes and within its rounding bound of -R^T t; the overflow
    visible to ShFactorExchange.overflowed()."""
    from dn_splatter_amd import dp

    _lib, ptr, stream = _api()
    nblk, per = _assert_index_edge(N)
    vm = _viewmat(100 + N % 89)
    vm_dev = vm.to(DEV)
    # the centre as dnsplat_sh_factors writes it (N = 0: the tail alone)
    tail = torch.full((4 + GUARD,), float("nan"), device=DEV)
    _lib.check(_lib.lib().dnsplat_sh_factors(0, None, ptr(vm_dev), None, None, ptr(tail), stream()), "dnsplat_sh_factors")
    _assert_centre(tail[:3], vm, "tail of dnsplat_sh_factors")
    assert float(tail[3]) == 0.0 and bool(torch.isnan(tail[4:]).all())
    scratch = torch.empty(nblk, dtype=torch.int32, device=DEV)
    no_colours = torch.zeros(N, 3)
    for name, radii, caps in _index_patterns(N):
        vis = radii > 0
        count = int(vis.sum())
        if name == "culled_blocks" and nblk >= 8:
            per_block = torch.bincount(torch.nonzero(vis).reshape(-1) // WAVE, minlength=nblk)
            assert int((per_block == 0).sum()) >= nblk // 4 and int((per_block > 0).sum()) >= nblk // 4
        if name == "negative":
            assert int((radii < 0).sum()) == N - count
        if name == "random" and N >= 65_536:
            assert 0.70 * N < count < 0.74 * N
        radii_dev = radii.to(DEV)
        # masks and offsets do not depend on the capacity: one restatement per pattern, header word 4 set per call
        want = _bits(ref.pack_slab_ref(no_colours, vis, tail[:3].cpu(), 0)).clone()
        assert want.numel() == ref.packed_layout(N, 0)[2] >= 8 + 3 * nblk
        for cap in caps:
            _, rows0, total = ref.packed_layout(N, cap)
            want[4] = cap
            slab = torch.full((total + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
            _lib.check(_lib.lib().dnsplat_visible_index(N, cap, ptr(radii_dev), ptr(vm_dev), ptr(slab), ptr(scratch), stream()),
                       "dnsplat_visible_index")
            got = slab[:8 + 3 * nblk].cpu()
            what = (N, name, cap)
            assert int(got[0]) == count and got[4:8].tolist() == [cap, N, 0, 0], what
            assert torch.equal(got[1:4], _bits(tail[:3]).cpu()), what           # the centre: the bits dnsplat_sh_factors writes
            assert torch.equal(got[8:8 + 2 * nblk], want[8:8 + 2 * nblk]), (what, "masks")
            wrong = torch.nonzero(got[8 + 2 * nblk:] != want[8 + 2 * nblk:8 + 3 * nblk]).reshape(-1)
            assert wrong.numel() == 0, f"{what}: {wrong.numel()} offsets differ, the first at block {int(wrong[0])} of {nblk}"
            assert torch.equal(got, want[:8 + 3 * nblk]), what
            assert bool((slab[rows0:] == SENTINEL).all()), what                # rows region and guard
            ex = dp.ShFactorExchange(packed=True, capacity=cap)
            ex.gathered = slab[:total].view(torch.float32)[None]
            assert ex.overflowed() == (count > cap) == bool(got[0] > got[4]), what
        if count > 0:
            assert count - 1 in caps and count in caps and 0 in caps


# ---- 2. dnsplat_sh_factors -----------------------------------------------------------------------------------------------------------

_NAN_PAYLOAD = 0x7FC12345
_SUBNORMAL = 1                  # the bits of the smallest positive subnormal
# (record colour bits, gradient bits, radius) planted in a row: what each decision of the select sits on
_SPECIALS = (("plus_zero", 0x00000000, 0x3FC00000, 5), ("minus_zero", 0x80000000 - (1 << 32), 0x3FC00000, 5),
             ("subnormal", _SUBNORMAL, 0x3FC00000, 5), ("nan_record", 0x7FC00000, 0x3FC00000, 5),
             ("nan_gradient", 0x3F000000, _NAN_PAYLOAD, 5), ("inf_gradient", 0x3F000000, 0x7F800000, 5),
             ("minus_inf_gradient", 0x3F000000, 0xFF800000 - (1 << 32), 5), ("radius_zero", 0x3F000000, 0x3FC00000, 0),
             ("radius_negative", 0x3F000000, 0x3FC00000, -4))


_PASSES = ("subnormal", "nan_gradient", "inf_gradient", "minus_inf_gradient")   # the specials whose gradient reaches the slab


def _factor_inputs(N, planted):
    """Random records and gradient records with EVERY channel non-zero (nothing but channels 0 .. 2 of a record may reach the slab),
    radii of either sign and zero, and the specials ``planted`` = [(row, channel, special)]."""
    g = torch.Generator().manual_seed(8300 + N)
    splats = torch.randn(N, REC, generator=g)
    v_splats = torch.randn(N, REC, generator=g)
    splats[splats == 0], v_splats[v_splats == 0] = 0.25, 0.25
    radii = torch.randint(-3, 12, (N,), generator=g, dtype=torch.int32)
    sb, vb = _bits(splats).view(N, REC), _bits(v_splats).view(N, REC)            # views: writes go through to the floats
    for row, ch, (_, rec_bits, grad_bits, radius) in planted:
        sb[row, REC_CH0 + ch], vb[row, REC_CH0 + ch], radii[row] = rec_bits, grad_bits, radius
    return splats, v_splats, radii


@pytest.mark.parametrize("N", FACTOR_N)
def test_sh_factors_is_an_exact_select(dns, N):
    """where(radii > 0 and rec[REC_CH0 + i] > 0, v_rec[REC_CH0 + i], 0) as bits, the tail = centre, 0, nothing behind it."""
    _lib, ptr, stream = _api()
    grid = (N + FLAT_THREADS) // FLAT_THREADS
    assert grid == {1: 1, 255: 1, 256: 2, 257: 2}[N]
    vm = _viewmat(300 + N)
    vm_dev = vm.to(DEV)
    if N == 1:
        plans = [[(0, 1, s)] for s in _SPECIALS]                                 # one Gaussian: one special per call
    else:
        plans = [[(N - 1 - 28 * j, j % 3, s) for j, s in enumerate(_SPECIALS)]]   # rows N - 1, N - 29, ...: the last row, both workgroups at 257
        assert min(p[0] for p in plans[0]) >= 0
    for planted in plans:
        splats, v_splats, radii = _factor_inputs(N, planted)
        keep = (radii > 0)[:, None] & (splats[:, REC_CH0:REC_CH0 + 3] > 0)
        want = _bits(torch.where(keep, v_splats[:, REC_CH0:REC_CH0 + 3], torch.zeros(N, 3))).reshape(N, 3)
        for row, ch, (name, rec_bits, grad_bits, radius) in planted:            # each special does what it is named for
            assert int(_bits(splats).view(N, REC)[row, REC_CH0 + ch]) == rec_bits and int(radii[row]) == radius
            assert int(want[row, ch]) == (grad_bits if name in _PASSES else 0), name
        assert N == 1 or (0.1 < float(keep.float().mean()) < 0.9)
        out = torch.full((3 * N + 4 + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
        on_dev = [t.to(DEV) for t in (radii, splats, v_splats)]                  # held until the result is read
        _lib.check(_lib.lib().dnsplat_sh_factors(N, ptr(on_dev[0]), ptr(vm_dev), ptr(on_dev[1]), ptr(on_dev[2]), ptr(out), stream()),
                   "dnsplat_sh_factors")
        got = out.cpu()
        wrong = torch.nonzero(got[:3 * N].reshape(N, 3) != want)
        names = [s[0] for r, c, s in planted if [r, c] in wrong.tolist()]
        assert wrong.numel() == 0, (N, "wrong (row, channel):", wrong[:8].tolist(), "specials among them:", names)
        _assert_centre(got[3 * N:3 * N + 3].view(torch.float32), vm, (N, "tail"))
        assert int(got[3 * N + 3]) == 0 and bool((got[3 * N + 4:] == SENTINEL).all())


# ---- 3. one camera's slab, every way of producing it -----------------------------------------------------------------------------------


@pytest.mark.usefixtures("hip_deterministic")
def test_every_way_of_producing_a_slab_gives_the_same_bits(dns):
    """One small frame, its backward once per ShFactorExchange form: dnsplat_sh_factors ahead of the projection backward, the
    projection backward's own sh_factors write (deferred, and with own_rows), packed slabs with room and five rows short, and the
    four mini slabs of the eager SlicedShExchange."""
    from dn_splatter_amd import dp, synthetic

    N, W, H = 5003, 160, 128
    gp0 = synthetic.make_gauss_params(N, sh_rest_std=0.2, seed=21)
    cam = synthetic.orbit_camera(2, width=W, height=H, focal=110.0).to(DEV)

    def backward(exchange):
        gp = {k: v.detach().to(DEV).clone().requires_grad_(k != "normals") for k, v in gp0.items()}
        dns.set_sh_exchange(exchange)
        try:
            m = dns.DNSplatterRenderer(gp, fused=True)
            out = m.get_outputs(cam)
            ((out["rgb"] * torch.linspace(0.5, 1.5, 3, device=DEV)).sum() + out["depth"].sum() + out["normal"].sum()).backward()
        finally:
            dns.set_sh_exchange(None)
        torch.cuda.synchronize()
        assert exchange.meta is not None
        exchange.meta = None
        return m.radii.reshape(-1).cpu()

    early = dp.ShFactorExchange(own_rows=False)
    radii = backward(early)
    vis = radii > 0
    count = int(vis.sum())
    assert 64 < count < N - 64                                                   # culled and visible Gaussians both
    slab = early.mine.cpu()
    assert slab.shape == (3 * N + 4,) and float(slab[-1]) == 0.0
    cols, centre = slab[:3 * N].reshape(N, 3), slab[3 * N:3 * N + 3]
    assert bool((cols[~vis] == 0).all()) and int((cols[vis] != 0).any(-1).sum()) > count // 2

    deferred = dp.ShFactorExchange(own_rows=False)
    deferred.deferred = True
    own = dp.ShFactorExchange(own_rows=True)
    for name, ex in (("deferred", deferred), ("own_rows", own)):
        assert torch.equal(backward(ex), radii)
        assert torch.equal(_bits(ex.mine.cpu()), _bits(slab)), name              # the tail included

    nblk = _ceil(N, WAVE)
    for cap, fill in ((count + 9, 0), (count - 5, SENTINEL)):
        ex = dp.ShFactorExchange(own_rows=False, packed=True, capacity=cap)
        total = ex.slab_floats(N)
        assert total == ref.packed_layout(N, cap)[2] and ex.packed_capacity(N) == cap
        big = torch.full((total + GUARD,), fill, dtype=torch.int32, device=DEV)
        ex.mine = big[:total].view(torch.float32)
        assert torch.equal(backward(ex), radii)
        assert ex.mine.data_ptr() == big.data_ptr()                              # begin() kept the tensor it was handed
        got = big.cpu()
        rows0 = ref.packed_layout(N, cap)[1]
        want = _bits(ref.pack_slab_ref(cols, vis, centre, cap))
        written = torch.zeros(total, dtype=torch.bool)
        written[:8 + 3 * nblk] = True
        written[rows0:rows0 + 3 * min(count, cap)] = True
        want = torch.where(written, want, torch.full_like(want, fill))           # what nobody writes keeps what it held
        assert torch.equal(got[:total], want), cap                               # the whole slab, byte for byte
        assert bool((got[total:] == fill).all()), cap                            # the guard behind it
        back, pos = ref.unpack_slab_ref(got[:total].view(torch.float32), N, cap)
        assert torch.equal(_bits(pos), _bits(centre))
        order = torch.cumsum(vis.long(), 0) - vis.long()
        kept = vis & (order < cap)                                               # the first `cap` visible Gaussians in row order
        assert int(kept.sum()) == min(count, cap)
        assert torch.equal(_bits(back[kept]), _bits(cols[kept])) and bool((_bits(back[~kept]) == 0).all()), cap
        ex.gathered = ex.mine[None]
        assert ex.overflowed() == (cap < count)
        if cap >= count:
            assert torch.equal(_bits(back), _bits(cols))                         # unpack(packed) == the dense [N,3]

    sliced = dp.SlicedShExchange(4)
    assert torch.equal(backward(sliced), radii)
    assert len(sliced.bounds) == 4 and sliced.bounds[0][0] == 0 and sliced.bounds[-1][1] == N
    minis = [sliced.slab(k).cpu() for k in range(4)]
    assert torch.equal(_bits(torch.cat([s[:-4] for s in minis])), _bits(slab[:3 * N]))
    for s in minis:
        assert torch.equal(_bits(s[-4:]), _bits(slab[-4:]))                      # every mini slab carries the centre
    sliced.works = None


# ---- 4. the rebuild and add kernels, per row against fp64 ------------------------------------------------------------------------------

#   name        K   kind     offset (floats)     the path sh_layout() picks
LAYOUTS = (("split", 16, "split", 0),          # SPLIT: features_dc [N,3] + features_rest [N,15,3]
           ("cat", 16, "cat", 0),              # CAT: [N,16,3]
           ("cat_off4", 16, "cat", 1),         # DIRECT: the CAT tensor 4 bytes off a 16-byte boundary
           ("k4_cat", 4, "cat", 0),            # DIRECT: sh_K != 16
           ("k4_split", 4, "split", 0),
           ("k9_cat", 9, "cat", 0),
           ("k9_split", 9, "split", 0),
           ("k1_null", 1, "split", 0),         # DIRECT: v_shN == NULL
           ("k25_split", 25, "split", 0),      # DIRECT: 27 floats of the rest row beyond the 45 the kernel computes
           ("k25_cat", 25, "cat", 0))
SPLIT, CAT, DIRECT = "SPLIT", "CAT", "DIRECT"


def _scale(w):
    return float(torch.tensor(1.0 / w, dtype=torch.float32))


class _Rows:
    """[n + GUARD, K, 3] coefficient-gradient rows on the device in one of the LAYOUTS, initialised from ``full``."""

    def __init__(self, kind, K, offset, full):
        self.kind, self.K, self.rows = kind, K, full.shape[0]
        if kind == "cat":
            self.store = torch.empty(full.numel() + 4, dtype=torch.float32, device=DEV)
            self.flat = self.store[offset:offset + full.numel()]
            self.flat.copy_(full.reshape(-1))
            self.p0, self.pN, self.s0, self.sN = self.flat, (self.flat[3:] if K > 1 else None), 3 * K, 3 * K
        else:
            self.v0 = full[:, 0].clone(memory_format=torch.contiguous_format)
            self.vN = full[:, 1:].clone(memory_format=torch.contiguous_format) if K > 1 else None
            self.p0, self.pN, self.s0, self.sN = self.v0, self.vN, 3, 3 * (K - 1)

    def path(self):
        """sh_layout() of project.hip, restated."""
        b0, bN = self.p0.data_ptr(), (self.pN.data_ptr() if self.pN is not None else 0)
        if self.K != 16 or not bN:
            return DIRECT
        if bN == b0 + 12 and self.s0 == 48 and self.sN == 48 and b0 % 16 == 0:
            return CAT
        if self.s0 == 3 and self.sN == 45 and bN % 16 == 0:
            return SPLIT
        return DIRECT

    def read(self):
        if self.kind == "cat":
            return self.flat.view(self.rows, self.K, 3).clone()
        return self.v0[:, None].clone() if self.vN is None else torch.cat([self.v0[:, None], self.vN], 1)


def _launch(rows, n, w, skip, slabs, cap, means, degree, scale):
    _lib, ptr, stream = _api()
    L = _lib.lib()
    tail = (ptr(means), degree, rows.K, scale, ptr(rows.p0), rows.s0, ptr(rows.pN), rows.sN, stream())
    if cap is not None:
        _lib.check(L.dnsplat_sh_grads_from_packed(n, cap, w, skip, ptr(slabs), *tail), "dnsplat_sh_grads_from_packed")
    elif skip >= 0:
        _lib.check(L.dnsplat_sh_grads_add_factors(n, w, skip, ptr(slabs), *tail), "dnsplat_sh_grads_add_factors")
    else:
        _lib.check(L.dnsplat_sh_grads_from_factors(n, w, ptr(slabs), *tail), "dnsplat_sh_grads_from_factors")


def _initial(n, K, own):
    """Rebuild (own None): NaN everywhere.  Add: the own rows, recognisable positive floats in the bands beyond 16 and in the guard."""
    if own is None:
        return torch.full((n + GUARD, K, 3), float("nan"), device=DEV)
    full = 3000.0 + (torch.arange((n + GUARD) * K * 3, device=DEV) % 1013).float().reshape(n + GUARD, K, 3)
    k = min(K, 16)
    full[:n, :k] = own[:, :k]
    return full


def _check_rows(got, init, want, mag, touched, n, K, degree, add, what, bad):
    """One call's result [n + GUARD, K, 3] against the float64 rows: the bound on every row over the active bands, everything else as
    bits.  Appends what it finds to ``bad``; returns the worst ratio."""
    nb = (degree + 1) ** 2
    k = min(K, 16)
    ratio, dead_wrong = ref.row_ratio(got[:n, :k], want[:, :k], mag[:, :k], degree)
    if not ratio <= ref.KAPPA:
        bad.append((what, f"worst row at {ratio:.2f} x 2^-24 ||A||, allowed {ref.KAPPA}"))
    if dead_wrong:
        bad.append((what, f"{dead_wrong} rows with A = 0 differ from the reference"))
    if not torch.equal(_bits(got[n:]), _bits(init[n:])):
        bad.append((what, "rows behind N were written"))
    if add:
        if not torch.equal(_bits(got[:n, nb:]), _bits(init[:n, nb:])):
            bad.append((what, "add form: bands above the degree changed"))
        if not torch.equal(_bits(got[:n][~touched]), _bits(init[:n][~touched])):
            bad.append((what, "add form: a row no other view touches changed"))
    else:
        if not bool((got[:n, nb:] == 0).all()):
            bad.append((what, "rebuild form: bands above the degree are not zero"))
        if not bool((got[:n][~touched] == 0).all()):
            bad.append((what, "rebuild form: a row with A = 0 is not zero"))
    return ratio


def _run_case(n, w, degree, layouts, packed_only=False):
    inp = ref.exchange_inputs(n, w)
    scale = _scale(w)
    means_dev = inp["means"].to(DEV)
    dense = ref.dense_slabs(inp["cols"], inp["pos"]).to(DEV)
    forms = ref.exchange_forms(inp, packed_only=packed_only)
    counts = inp["vis"].sum(1)
    bad, worst, results = [], 0.0, {}
    for name, skip, cap, cols in forms:
        if cap is None:
            slabs = dense
        else:
            slabs = ref.packed_slabs(inp["cols"], inp["vis"], inp["pos"], cap).to(DEV)
            assert slabs.shape[1] == ref.packed_layout(n, cap)[2]
            overflow = int((counts > cap).sum())
            assert (overflow >= 1 and not bool((counts <= cap).all())) if "overflow" in name else overflow == 0, (name, cap)
        own = ref.own_rows(inp["cols"], inp["pos"], inp["means"], degree, scale, skip) if skip >= 0 else None
        want, mag = ref.rebuild_ref64(cols, inp["pos"], inp["means"], degree, scale, skip, own)
        others = [v for v in range(w) if v != skip]
        touched = (cols[others] != 0).any(-1).any(0).to(DEV)
        want, mag = want.to(DEV), mag.to(DEV)
        own_dev = None if own is None else own.to(DEV)
        for lname, K, kind, offset in layouts:
            if K < (degree + 1) ** 2:
                continue
            what = (n, degree, lname, name)
            init = _initial(n, K, own_dev)
            out = []
            for _ in range(2):                                                   # twice: the same bits
                rows = _Rows(kind, K, offset, init)
                expect = {"split": SPLIT, "cat": CAT}[lname] if lname in ("split", "cat") else DIRECT
                assert rows.path() == expect, (what, rows.path())
                _launch(rows, n, w, skip, slabs, cap, means_dev, degree, scale)
                out.append(rows.read())
            if not torch.equal(_bits(out[0]), _bits(out[1])):
                bad.append((what, "two calls differ"))
            worst = max(worst, _check_rows(out[0], init, want, mag, touched, n, K, degree, skip >= 0, what, bad))
            results[(lname, name)] = out[0]
            if name.startswith("packed") and "overflow" not in name:            # packed with room == dense, bit for bit
                twin = results.get((lname, name.replace("packed", "dense", 1)))
                if twin is not None and not torch.equal(_bits(out[0]), _bits(twin)):
                    bad.append((what, "differs from the dense form over the same colours"))
    print(f"N = {n}, w = {w}, degree {degree}: worst row ratio {worst:.3f} (KAPPA {ref.KAPPA}, CPU restatement {ref.CPU_RATIO})")
    assert not bad, f"{len(bad)} findings, the first: {bad[:6]}"
    return worst


@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("n,w", ref.EXCHANGE_CASES)
def test_rebuild_and_add_rows_against_fp64(dns, n, w, degree):
    """Every layout x {dense, packed with room, packed one row short} x {rebuild, add with every skip_view}: each row within KAPPA
    2^-24 ||A_row||_2 of rebuild_ref64, rows with A = 0 exactly zero (rebuild) or untouched (add), bands above the degree zero or
    untouched, the block behind N untouched, two calls equal, packed with room equal to dense."""
    assert w == 3 and _ceil(n, STAGE_THREADS) == {1: 1, 63: 1, 64: 1, 65: 2, 10_007: 157}[n]
    assert n != 10_007 or n % STAGE_THREADS == 23                               # a short last workgroup
    _run_case(n, w, degree, LAYOUTS)


def test_packed_rebuild_behind_1025_mask_words(dns):
    """N = 65 537: the reader's offsets at hdr + 8 + 2 nblk sit behind 1025 mask words, the rows behind 3075 words and a pad."""
    n, w = ref.EXCHANGE_BIG
    nblk = _ceil(n, WAVE)
    assert nblk == SCAN_THREADS + 1 and ref.packed_layout(n, 0)[1] == 8 + 3 * nblk + 1
    _run_case(n, w, 3, [l for l in LAYOUTS if l[0] in ("split", "cat", "cat_off4")], packed_only=True)


@pytest.mark.parametrize("lname", ["split", "cat"])
@pytest.mark.parametrize("packed", [False, True])
def test_staged_add_writes_only_the_rows_another_view_touches(dns, lname, packed):
    """The add form of the staged layouts moves a workgroup's rows through LDS: a 64-block no other view touches keeps every bit
    (whatever the bits), a block touched in one lane keeps the bits of its other 63 rows, the short last block leaves the rows
    behind N alone."""
    n, w, skip, degree = 5 * STAGE_THREADS + 37, 3, 0, 3
    g = torch.Generator().manual_seed(8400)
    inp = ref.exchange_inputs(n, w, seed=5)
    block = torch.arange(n) // STAGE_THREADS
    lane = torch.arange(n) % STAGE_THREADS
    cols = torch.zeros(w, n, 3)
    cols[0] = torch.randn(n, 3, generator=g)                                     # the skipped view: whatever it holds is not read
    cols[1][(block == 1) & (lane == 17)] = torch.tensor([0.3, -0.7, 0.01])
    cols[2][block == 3] = torch.randn(STAGE_THREADS, 3, generator=g)
    cols[2][(block == 5) & ((lane == 3) | (lane == 36))] = torch.tensor([-0.2, 0.0, 0.9])
    vis = (cols != 0).any(-1)
    vis[1][block == 2] = True                                                    # visible with zero colours: still untouched
    touched = (cols[1:] != 0).any(-1).any(0)
    assert int(touched.sum()) == 1 + STAGE_THREADS + 2 and n - 1 == 5 * STAGE_THREADS + 36
    cap = int(vis.sum(1).max())
    slabs = (ref.packed_slabs(cols, vis, inp["pos"], cap) if packed else ref.dense_slabs(cols, inp["pos"])).to(DEV)
    scale = _scale(w)
    init = torch.randint(-2 ** 31, 2 ** 31 - 1, (n + GUARD, 16, 3), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)
    own = torch.randn(n, 16, 3, generator=g)
    init[:n][touched] = own[touched]
    want, mag = ref.rebuild_ref64(cols, inp["pos"], inp["means"], degree, scale, skip, init[:n].double().nan_to_num(0.0, 0.0, 0.0))
    init = init.to(DEV)
    _, K, kind, offset = [l for l in LAYOUTS if l[0] == lname][0]
    rows = _Rows(kind, K, offset, init)
    assert rows.path() == {"split": SPLIT, "cat": CAT}[lname]
    _launch(rows, n, w, skip, slabs, cap if packed else None, inp["means"].to(DEV), degree, scale)
    got = rows.read()
    keep = torch.ones(n + GUARD, dtype=torch.bool)
    keep[:n] = ~touched
    assert torch.equal(_bits(got[keep.to(DEV)]), _bits(init[keep.to(DEV)]))       # untouched blocks, the other 63 lanes, the rows behind N
    hit = touched.to(DEV)
    ratio, _ = ref.row_ratio(got[:n][hit], want[touched].to(DEV), mag[touched].to(DEV), degree)
    print(f"staged add, {lname}, packed {packed}: worst touched row {ratio:.3f} (KAPPA {ref.KAPPA})")
    assert ratio <= ref.KAPPA
    assert bool((got[:n][hit] != init[:n][hit]).reshape(int(hit.sum()), -1).any(1).all())     # and every touched row did receive its share


@pytest.mark.parametrize("lname", ["split", "cat", "k9_cat"])
def test_add_form_with_one_view_launches_nothing(dns, lname):
    n, degree = 130, 2
    inp = ref.exchange_inputs(n, 1)
    _, K, kind, offset = [l for l in LAYOUTS if l[0] == lname][0]
    init = _initial(n, K, ref.own_rows(inp["cols"], inp["pos"], inp["means"], degree, 1.0, 0).to(DEV))
    cap = int(inp["vis"].sum())
    for slabs, c in ((ref.dense_slabs(inp["cols"], inp["pos"]), None), (ref.packed_slabs(inp["cols"], inp["vis"], inp["pos"], cap), cap)):
        rows = _Rows(kind, K, offset, init)
        _launch(rows, n, 1, 0, slabs.to(DEV), c, inp["means"].to(DEV), degree, 1.0)
        assert torch.equal(_bits(rows.read()), _bits(init))
