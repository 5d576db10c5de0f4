"""The bound behind the compositing kernels' fast loops (csrc/splat_common.h, dns_conic_benign): for a conic (a, b, c) with
b^2 <= (1 - 2^-12) a c and a, c in [2^-40, 2^40], the kernels' own operation sequence for the exponent,

    na, nb, nc = fl(k a), fl(k b), fl(k c),  k = -log2(e) / 2
    u = fma(nb, dy, fl(na dx)),  w = fma(nc, dy, fl(nb dx)),  e = fma(dx, u, fl(dy w)),

cannot round to a positive number, so the test `e <= 0` is dead weight in a frame whose visible conics all pass the rule.
Restated here in numpy float32 (an FMA = exact float64 product plus addend, rounded once to fp32; the float64 sum keeps the sign of
the exact one, which is all that is asked of it) and, for a subset, in exact rationals rounded to nearest-even per operation.
No GPU, no library: this file checks arithmetic."""
import os
import re
from fractions import Fraction

import numpy as np

F32 = np.float32
K = F32(-0.5) * F32(1.4426950408889634)        # (-0.5f * DNS_LOG2E), exact in fp32 (a power of two times the constant)
RULE = F32(1.0) - F32(2.0 ** -12)              # exact in fp32
LO, HI = F32(2.0 ** -40), F32(2.0 ** 40)
EPS = 2.0 ** -24


def benign(a, b, c):
    """dns_conic_benign, fp32 operation by operation."""
    a, b, c = F32(a), F32(b), F32(c)
    with np.errstate(over="ignore", invalid="ignore"):
        return (a >= LO) & (a <= HI) & (c >= LO) & (c <= HI) & (b * b <= RULE * (a * c))


def fma(x, y, z):
    return (x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)).astype(F32)


def exponent(a, b, c, dx, dy):
    """dns_conic_e + dns_exponent on fp32 arrays -> e (fp32)."""
    na, nb, nc = K * a, K * b, K * c
    u = fma(nb, dy, na * dx)
    w = fma(nc, dy, nb * dx)
    return fma(dx, u, dy * w)


def into_rule(a, b, c):
    """Pull b towards 0, one fp32 step at a time, until the fp32 predicate holds: nothing is filtered out."""
    b = b.copy()
    for _ in range(64):
        bad = ~benign(a, b, c)
        if not bad.any():
            return b
        b[bad] = np.nextafter(b[bad], F32(0))
    raise AssertionError("could not move the conics into the rule")


def conics(rng, n, edge):
    """n fp32 conics that satisfy the rule.  Magnitudes 1e-6 ... 1e6 for a and c independently; rho^2 = b^2 / (a c) uniform in
    [0, rule] (edge = False) or within 1 % of the rule's edge (edge = True); both signs of b."""
    a = (10.0 ** rng.uniform(-6, 6, n)).astype(F32)
    c = np.where(rng.random(n) < 0.5, a.astype(np.float64) * 10.0 ** rng.uniform(-3, 3, n), 10.0 ** rng.uniform(-6, 6, n))
    c = np.clip(c, 1e-6, 1e6).astype(F32)
    rule = 1.0 - 2.0 ** -12
    rho2 = rule * (1.0 - 0.01 * rng.random(n) ** 4) if edge else rule * rng.random(n)
    b = (np.sqrt(rho2 * a.astype(np.float64) * c.astype(np.float64)) * rng.choice([-1.0, 1.0], n)).astype(F32)
    return a, into_rule(a, b, c), c


def offsets(rng, a, b, c):
    """Per conic, a list of (dx, dy) fp32 offsets with |d| from 2^-14 (and, beyond what is asked, 2^-25: the smallest non-zero
    difference of a mean and a pixel centre) to 2^12: random directions, pixel-grid differences, the near-null direction of the form
    (the minimiser of the form along each axis, where the cross term cancels most of the squares) exact and a few ulps off,
    single-axis offsets, and d = 0."""
    n = a.shape[0]
    a64, b64, c64 = a.astype(np.float64), b.astype(np.float64), c.astype(np.float64)
    out = []
    r = 2.0 ** rng.uniform(-14, 12, n)
    th = rng.uniform(0, 2 * np.pi, n)
    out.append((r * np.cos(th), r * np.sin(th)))
    # a mean in the image minus pixel centres k + 1/2, as the kernels form it
    mx, my = rng.uniform(0, 4096, n).astype(F32), rng.uniform(0, 4096, n).astype(F32)
    px, py = np.floor(rng.uniform(0, 4096, n)).astype(F32) + F32(0.5), np.floor(rng.uniform(0, 4096, n)).astype(F32) + F32(0.5)
    out.append((mx - px, my - py))
    near = rng.integers(-8, 9, n).astype(F32)
    out.append((mx - (np.floor(mx) + F32(0.5) + near), my - (np.floor(my) + F32(0.5) - near)))
    # near-null directions: dx = -(b / a) dy minimises the form over dx, dy = -(b / c) dx over dy
    for scale_lo, scale_hi in ((-14, 12), (-25, -14)):
        s = 2.0 ** rng.uniform(scale_lo, scale_hi, n) * rng.choice([-1.0, 1.0], n)
        out.append((-(b64 / a64) * s, s))
        out.append((s, -(b64 / c64) * s))
        dxn = (-(b64 / a64) * s).astype(F32)
        out.append((np.nextafter(dxn, F32(np.inf)) if scale_lo == -14 else np.nextafter(dxn, F32(-np.inf)), s))
    # the eigenvector of the smaller eigenvalue
    ang = 0.5 * np.arctan2(2 * b64, a64 - c64) + np.pi / 2
    s = 2.0 ** rng.uniform(-14, 12, n)
    out.append((s * np.cos(ang), s * np.sin(ang)))
    z = np.zeros(n)
    out.append((z, r)); out.append((r, z)); out.append((z, z))
    res = []
    for dx, dy in out:
        dx, dy = np.asarray(dx, dtype=np.float64), np.asarray(dy, dtype=np.float64)
        m = np.maximum(np.abs(dx), np.abs(dy))
        k = np.where(m > 4096.0, 4096.0 / np.maximum(m, 1e-300), 1.0)     # keep |d| within 2^12 (scaled, never dropped)
        res.append(((dx * k).astype(F32), (dy * k).astype(F32)))
    return res


def test_rule_in_the_header_is_the_rule_tested_here():
    src = open(os.path.join(os.path.dirname(__file__), "..", "dn-splatter_amd", "csrc", "splat_common.h")).read()
    body = re.search(r"bool dns_conic_benign\(float a, float b, float c\)\s*\{(.*?)\n\}", src, re.S).group(1)
    assert "fp contract(off)" in body
    assert "0x1p-40f" in body and "0x1p40f" in body and "(1.f - 0x1p-12f) * (a * c)" in body and "b * b <=" in body
    assert src.count("dns_conic_benign(float") == 1, "one statement of the rule"


def test_predicate_edges():
    assert benign(1, 0, 1) and benign(1e-6, 0, 1e6) and benign(2.0 ** -40, 0, 2.0 ** 40)
    assert not benign(1, 1, 1) and not benign(1, -1, 1)              # degenerate
    assert not benign(1, 2, 1) and not benign(-1, 0, 1) and not benign(1, 0, 0) and not benign(0, 0, 0)
    assert not benign(2.0 ** -41, 0, 1) and not benign(1, 0, 2.0 ** 41)
    inf, nan = float("inf"), float("nan")
    for bad in (inf, -inf, nan):
        assert not benign(bad, 0, 1) and not benign(1, bad, 1) and not benign(1, 0, bad)
    assert not benign(2.0 ** 40, 2.0 ** 70, 2.0 ** 40)               # b^2 overflows: inf <= finite is false
    # the edge itself: rho^2 = 1 - 2^-12 exactly passes, one fp32 step beyond fails
    a = c = F32(1.0)
    b = F32(np.sqrt(np.float64(RULE)))
    b = into_rule(np.array([a]), np.array([b]), np.array([c]))[0]
    assert benign(a, b, c) and not benign(a, np.nextafter(np.nextafter(b, F32(2)), F32(2)), c)


def test_exponent_never_positive_under_the_rule():
    """> 10^6 conics under the rule x 13 offsets each: e is never positive and never NaN; no case is excluded."""
    rng = np.random.default_rng(20240607)
    sets = [conics(rng, 600_000, edge=False), conics(rng, 500_000, edge=True)]
    # axis-aligned conics
    n = 100_000
    a = (10.0 ** rng.uniform(-6, 6, n)).astype(F32)
    c = (10.0 ** rng.uniform(-6, 6, n)).astype(F32)
    sets.append((a, np.zeros(n, F32), c))
    total = 0
    worst = 0.0
    for a, b, c in sets:
        assert bool(benign(a, b, c).all())
        for dx, dy in offsets(rng, a, b, c):
            e = exponent(a, b, c, dx, dy)
            total += e.size
            assert not bool(np.isnan(e).any())
            assert not bool((e > 0).any()), "the exponent of a benign conic rounded to a positive number"
            zero = (dx == 0) & (dy == 0)
            assert bool((e[zero] == 0).all())                       # a pixel at the mean: e = 0, which passes `<= 0`
            # how much of the margin the rounding uses: |e - E| / |E| against the derivation's 2.93e-3
            na, nb, nc = (K * a).astype(np.float64), (K * b).astype(np.float64), (K * c).astype(np.float64)
            x, y = dx.astype(np.float64), dy.astype(np.float64)
            E = na * x * x + 2 * nb * x * y + nc * y * y            # float64: good to ~1e-12 of S, enough for this figure
            nz = E < 0
            worst = max(worst, float(np.max(np.abs(e.astype(np.float64)[nz] - E[nz]) / -E[nz], initial=0.0)))
    assert total >= 13 * 1_200_000
    print(f"{total} pairs, largest |e - E| / |E| = {worst:.3e} (bound 2.93e-3)")
    assert worst <= 2.93e-3 + 1e-8


def _round_f32(q: Fraction) -> Fraction:
    """q rounded to the nearest fp32 (ties to even), exactly."""
    if q == 0:
        return Fraction(0)
    c = F32(float(q))
    cands = {c, np.nextafter(c, F32(np.inf)), np.nextafter(c, F32(-np.inf))}
    best = None
    for v in cands:
        fv = Fraction(float(v))
        d = abs(fv - q)
        even = (int(np.array(v, F32).view(np.uint32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even):
            best = (d, fv)
    return best[1]


def _exponent_exact(a, b, c, dx, dy):
    """The sequence with every operation exact and rounded once (a true FMA) -> (e as Fraction, E exact, S exact)."""
    k = Fraction(float(K))
    a, b, c, dx, dy = (Fraction(float(v)) for v in (a, b, c, dx, dy))
    na, nb, nc = _round_f32(k * a), _round_f32(k * b), _round_f32(k * c)
    u = _round_f32(nb * dy + _round_f32(na * dx))
    w = _round_f32(nc * dy + _round_f32(nb * dx))
    e = _round_f32(dx * u + _round_f32(dy * w))
    E = na * dx * dx + 2 * nb * dx * dy + nc * dy * dy
    S = abs(na) * dx * dx + 2 * abs(nb * dx * dy) + abs(nc) * dy * dy
    return e, E, S


def test_cross_check_with_exact_rationals():
    """A subset (edge conics, every offset kind) recomputed with fractions: the numpy emulation gives the same e, the exact form E
    is negative, |e - E| stays within ((1 + eps)^3 - 1) S and S within (1 + rho) / (1 - rho) |E| — the two steps of the derivation."""
    rng = np.random.default_rng(7)
    a, b, c = conics(rng, 40, edge=True)
    n = 0
    for dx, dy in offsets(rng, a, b, c):
        e_np = exponent(a, b, c, dx, dy)
        for i in range(a.shape[0]):
            e, E, S = _exponent_exact(a[i], b[i], c[i], dx[i], dy[i])
            assert e == Fraction(float(e_np[i])), (a[i], b[i], c[i], dx[i], dy[i])
            assert e <= 0 and E <= 0
            assert abs(e - E) <= (Fraction(1 + EPS) ** 3 - 1) * S
            assert S * Fraction(2.0 ** -14.001) <= -E                # (1 + rho) / (1 - rho) <= 2^14.001
            n += 1
    assert n >= 500


def test_why_the_rule_exists():
    """Outside the rule the test is needed.  Two recorded conics, positive definite in exact arithmetic but with
    1 - b^2 / (a c) ~ 1e-7, whose exponent along the near-null direction rounds to e > 0 (found by random search over such conics;
    with 1 - rho^2 >= 2^-22 the same search over 4e5 conics found none: the rule's margin is real, and it is needed)."""
    cases = [(0.11497959494590759, -1.0039863586425781, 8.766674995422363, 800.991943359375, 91.73206329345703),
             (12.391048431396484, -17.35302734375, 24.302024841308594, 0.04666747525334358, 0.03332323208451271)]
    for case in cases:
        a, b, c, dx, dy = (np.array([v], F32) for v in case)
        assert all(float(v[0]) == w for v, w in zip((a, b, c, dx, dy), case)), "the recorded numbers are fp32 values"
        assert not bool(benign(a, b, c)[0])
        assert Fraction(case[0]) * Fraction(case[2]) > Fraction(case[1]) ** 2          # positive definite, exactly
        e = exponent(a, b, c, dx, dy)[0]
        ex, E, _ = _exponent_exact(a[0], b[0], c[0], dx[0], dy[0])
        # a true FMA rounds it positive as well (E, the exact form of the ROUNDED na, nb, nc, may itself have lost definiteness:
        # either way the pair must be skipped, and only the test on e sees it)
        assert e > 0 and ex == Fraction(float(e))
        print(f"conic {case[:3]} at d = {case[3:]}: e = {float(e):.3e}, exact E = {float(E):.3e}")
