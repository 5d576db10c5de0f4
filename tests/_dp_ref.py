"""Torch restatements of the exchange step's HIP kernels for the CPU (gloo) tests — test infrastructure, as the oracle is:
the packed (visible rows only) colour-gradient slab of include/dnsplat.h (dnsplat_visible_index + dnsplat_proj_grads.sh_packed) and the
rebuild / add kernels (dnsplat_sh_grads_from_factors, _add_factors, _from_packed).  tests/test_gpu_sh_exchange.py compares the kernels
with these restatements on the GPU — the slabs as bytes, the rebuilt rows per Gaussian against ``rebuild_ref64`` — and
tests/test_sh_exchange_reference.py holds the restatements themselves (against autograd, and the inputs' conditioning) without one."""
import torch


def packed_layout(n: int, capacity: int):
    nb = (n + 63) // 64
    rows0 = (8 + 3 * nb + 3) & ~3
    return nb, rows0, (rows0 + 3 * capacity + 3) & ~3


def pack_slab_ref(cols: torch.Tensor, visible: torch.Tensor, campos: torch.Tensor, capacity: int) -> torch.Tensor:
    """[N,3] colour gradients + bool [N] -> one packed slab (float32 words; integers through a view), as the kernels write it."""
    n = cols.shape[0]
    nb, rows0, total = packed_layout(n, capacity)
    slab = torch.zeros(total, dtype=torch.float32)
    ints = slab.view(torch.int32)
    vis = visible.bool()
    ints[0], ints[4], ints[5] = int(vis.sum()), capacity, n
    slab[1:4] = campos.float()
    bits = torch.zeros(nb * 64, dtype=torch.int64)
    bits[:n] = vis.long()
    words = (bits.view(nb, 64) << torch.arange(64)).sum(1)          # bit b of word w = Gaussian 64 w + b (wraps into the sign bit)
    ints[8:8 + 2 * nb] = words.view(torch.int32)
    counts = bits.view(nb, 64).sum(1)
    ints[8 + 2 * nb:8 + 3 * nb] = (torch.cumsum(counts, 0) - counts).int()
    rows = cols[vis][:capacity].float()
    slab[rows0:rows0 + 3 * rows.shape[0]] = rows.reshape(-1)
    return slab


def unpack_slab_ref(slab: torch.Tensor, n: int, capacity: int):
    """-> ([N,3] colour gradients with zeros for the Gaussians the slab does not hold, camera position [3])."""
    nb, rows0, _ = packed_layout(n, capacity)
    ints = slab.view(torch.int32)
    words = ints[8:8 + 2 * nb].contiguous().view(torch.int64)
    bits = ((words[:, None] >> torch.arange(64)) & 1).reshape(-1)[:n].bool()
    offs = ints[8 + 2 * nb:8 + 3 * nb].long()
    k = torch.cumsum(bits.long(), 0) - bits.long()                   # = offs[block] + popcount below: a global exclusive count
    assert torch.equal(k[::64][:nb], offs), "block offsets are not the exclusive prefix sum of the mask popcounts"
    cols = torch.zeros(n, 3)
    ok = bits & (k < int(ints[4]))
    cols[ok] = slab[rows0:].reshape(-1)[: 3 * int(ints[4])].reshape(-1, 3)[k[ok]]
    return cols, slab[1:4].clone()


def make_rebuild_ref(dense_ref):
    """The stand-in the gloo tests install as ``dp.ShFactorExchange._rebuild``: autograd through the oracle's dense SH evaluation,
    summed over the views; ``skip_view >= 0`` ADDS the other views to rows that hold that view's pre-scaled share."""

    def rebuild_ref(gathered, means_, n, w, deg, K, v_coeffs, v_sh0, v_shN, skip_view=-1, packed_capacity=None, scale=None):
        tot = torch.zeros(n, K, 3)
        for v in range(w):
            if v == skip_view:
                continue
            if packed_capacity is not None:
                cols_v, pos_v = unpack_slab_ref(gathered[v].clone(), n, packed_capacity)
            else:
                cols_v, pos_v = gathered[v, :3 * n].reshape(n, 3).clone(), gathered[v, 3 * n:3 * n + 3].clone()
            co = torch.zeros(n, K, 3, requires_grad=True)
            (dense_ref.sh_colors(deg, torch.nn.functional.normalize(means_ - pos_v, dim=-1), co) * cols_v).sum().backward()
            tot += co.grad
        tot *= (1.0 / w) if scale is None else scale
        if skip_view >= 0:
            v_sh0.add_(tot[:, 0])
            v_shN.add_(tot[:, 1:])
        else:
            v_sh0.copy_(tot[:, 0])
            v_shN.copy_(tot[:, 1:])

    return rebuild_ref


# ---- the rebuild per row (tests/test_sh_exchange_reference.py, tests/test_gpu_sh_exchange.py) --------------------------------------------

U24 = 2.0 ** -24
# How far a plain fp32 restatement of the rebuild (``rebuild_ref(..., dtype=torch.float32)``) lies from ``rebuild_ref64``, as the worst
# ratio of ||row error||_2 to 2^-24 ||A_row||_2 over every case of ``EXCHANGE_CASES`` x degrees 0 .. 3 x every form — measured on the CPU
# and asserted by test_sh_exchange_reference.py (the inputs are benign) — and the bound the kernels are held to: four times that, rounded
# up.  The kernel differs from the restatement by `1.f / sqrtf` and by nothing else that is more than a few roundings (project.hip is
# compiled without FMA contraction).
CPU_RATIO = 5.2
KAPPA = 21

#   (N, views): the sizes of the rebuild cases — one Gaussian, one short of / exactly / one past a 64-row workgroup, many workgroups with
#   a short last one, and (packed only) 1025 mask words in front of the offsets
EXCHANGE_CASES = ((1, 3), (63, 3), (64, 3), (65, 3), (10_007, 3))
EXCHANGE_BIG = (65_537, 2)

_SH = (0.2820947917738781, 0.48860251190292, 1.092548430592079, 0.5462742152960395, 0.9461746957575601, 0.3153915652525201,
       2.285228997322329, 0.4570457994644658, 1.445305721320277, 0.5900435899266435, 1.865881662950577, 1.119528997770346)


def sh_basis_ref(degree: int, d: torch.Tensor, absolute: bool = False) -> torch.Tensor:
    """[..., 3] unit directions -> [..., 16] real SH basis in d's dtype, the operations of project.hip's sh_basis in their order; bands
    above ``degree`` are zero.  ``absolute``: every monomial of every polynomial in absolute value (the magnitude roundings act on)."""
    x, y, z = d.unbind(-1)
    m = -1.0
    if absolute:
        x, y, z, m = x.abs(), y.abs(), z.abs(), 1.0
    c0, c1, c2b, c2a, c2c, c2d, c3a, c3b, c3c, c3d, c3e, c3f = _SH
    bas = [torch.full_like(x, c0)]
    if degree >= 1:
        bas += [(m * c1) * y, c1 * z, (m * c1) * x]
    if degree >= 2:
        z2 = z * z
        t0b = (m * c2b) * z
        fc1 = x * x + m * (y * y)
        fs1 = 2.0 * x * y
        bas += [c2a * fs1, t0b * y, c2c * z2 + m * c2d, t0b * x, c2a * fc1]
    if degree >= 3:
        t0c = (m * c3a) * z2 + c3b
        t1b = c3c * z
        fc2 = x * fc1 + m * (y * fs1)
        fs2 = x * fs1 + y * fc1
        bas += [(m * c3d) * fs2, t1b * fs1, t0c * y, z * (c3e * z2 + m * c3f), t0c * x, t1b * fc1, (m * c3d) * fc2]
    bas += [torch.zeros_like(x)] * (16 - len(bas))
    return torch.stack(bas, -1)


def rebuild_ref(cols: torch.Tensor, pos: torch.Tensor, means: torch.Tensor, degree: int, scale: float, skip_view: int = -1,
                own: torch.Tensor = None, dtype=torch.float64):
    """``cols`` [w,N,3], ``pos`` [w,3], ``means`` [N,3] (float32, taken as exact) -> (rows [N,16,3], A [N,16,3]) in closed form:
    rows = scale sum_v Y(d_v) (x) cols_v with d_v = normalize(means - pos_v), the views in order, ``skip_view`` left out, ``own``
    ([N,16,3], the add form) added last; computed in ``dtype``.  A (always float64) = |scale| sum_v Ybar(d_v) (x) |cols_v|, plus
    |own + rows| in the add form: the magnitude the kernel's roundings act on."""
    w, n = cols.shape[:2]
    acc = torch.zeros(n, 16, 3, dtype=dtype)
    mag = torch.zeros(n, 16, 3, dtype=torch.float64)
    for v in range(w):
        if v == skip_view:
            continue
        delta = means.to(dtype) - pos[v].to(dtype)
        inorm = 1.0 / torch.sqrt(delta[:, 0] * delta[:, 0] + delta[:, 1] * delta[:, 1] + delta[:, 2] * delta[:, 2])
        d = delta * inorm[:, None]
        acc += sh_basis_ref(degree, d)[:, :, None] * cols[v].to(dtype)[:, None, :]
        d64 = torch.nn.functional.normalize(means.double() - pos[v].double(), dim=-1)
        mag += sh_basis_ref(degree, d64, absolute=True)[:, :, None] * cols[v].double().abs()[:, None, :]
    rows = torch.tensor(scale, dtype=dtype) * acc
    mag *= abs(scale)
    if own is not None:
        rows = own.to(dtype) + rows
        mag = mag + rows.double().abs()
    return rows, mag


def rebuild_ref64(cols, pos, means, degree, scale, skip_view=-1, own=None):
    return rebuild_ref(cols, pos, means, degree, scale, skip_view, own, torch.float64)


def row_ratio(got: torch.Tensor, ref: torch.Tensor, mag: torch.Tensor, degree: int):
    """[N,K,3] rows against the float64 ones -> (worst ||got - ref||_2 / (2^-24 ||A||_2) over the rows with A != 0 — over the active bands
    k < (degree + 1)^2, the others are compared as bits by the callers — and the number of rows with A == 0 that are not exactly ref)."""
    nb = (degree + 1) ** 2
    k = min(nb, got.shape[1])
    err = (got[:, :k].double() - ref[:, :k]).reshape(got.shape[0], -1).norm(dim=1)
    a = mag[:, :k].reshape(got.shape[0], -1).norm(dim=1)
    live = a > 0
    ratio = float((err[live] / (U24 * a[live])).max()) if bool(live.any()) else 0.0
    return ratio, int((err[~live] != 0).sum())


def exchange_inputs(n: int, w: int, seed: int = 0):
    """Synthetic inputs of the rebuild: means in a box of half side 4, ``w`` camera centres on the sphere of radius 9 (so every
    |mean - pos| >= 9 - 4 sqrt 3 > 2), a visibility mask of about 78 %, colour gradients whose magnitudes span three decades (a dim
    Gaussian beside a bright one), zero where invisible, at a further 5 % of the visible (v, g), and in EVERY view for the Gaussians
    with g % 11 == 5: about 30 % of (v, g) exactly zero.  -> dict(means [n,3], pos [w,3], vis bool [w,n], cols [w,n,3]), float32."""
    g = torch.Generator().manual_seed(7700 + 31 * seed + n % 9973 + 1000 * w)
    means = ((torch.rand(n, 3, generator=g) - 0.5) * 8).float()
    pos = (torch.nn.functional.normalize(torch.randn(w, 3, generator=g), dim=-1) * 9).float()
    dead = (torch.arange(n) % 11) == 5
    vis = (torch.rand(w, n, generator=g) > 0.22) & ~dead
    cols = torch.randn(w, n, 3, generator=g) * torch.pow(10.0, -3 * torch.rand(w, n, 1, generator=g))
    cols = cols * (vis & (torch.rand(w, n, generator=g) > 0.05))[..., None]
    assert float((means[None] - pos[:, None]).double().norm(dim=-1).min()) >= 1.0
    return dict(means=means.contiguous(), pos=pos.contiguous(), vis=vis, cols=cols.float().contiguous())


def dense_slabs(cols: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """[w,N,3], [w,3] -> [w, 3 N + 4]: the slabs dnsplat_sh_factors writes."""
    w = cols.shape[0]
    return torch.cat([cols.reshape(w, -1), pos, torch.zeros(w, 1)], -1).float().contiguous()


def packed_slabs(cols: torch.Tensor, vis: torch.Tensor, pos: torch.Tensor, capacity: int) -> torch.Tensor:
    return torch.stack([pack_slab_ref(cols[v], vis[v], pos[v], capacity) for v in range(cols.shape[0])]).contiguous()


def overflow_capacity(vis: torch.Tensor) -> int:
    """One row less than the fullest view holds: that view overflows."""
    return max(int(vis.sum(1).max()) - 1, 0)


def own_rows(cols, pos, means, degree, scale, view, K=16):
    """The rows view ``view``'s own projection backward leaves for the add form: its share, in float32, in the active bands; a
    recognisable pattern of positive floats in the others (which the add form must leave as they are)."""
    share, _ = rebuild_ref64(cols[view:view + 1], pos[view:view + 1], means, degree, scale)
    n = means.shape[0]
    pattern = 1000.0 + (torch.arange(n * 16 * 3) % 977).float().reshape(n, 16, 3)
    active = (torch.arange(16) < (degree + 1) ** 2)[None, :, None]
    return torch.where(active, share.float(), pattern)


def exchange_forms(inp, packed_only: bool = False):
    """The forms one set of inputs is run in: (name, skip_view, capacity or None for dense slabs, the colours the reference reads).
    Dense rebuild and dense add with every skip_view; the same over packed slabs with room for every view's rows (same colours: they are
    zero where invisible) and with one row too few for the fullest view (the colours ``unpack_slab_ref`` gives back: the same rows
    dropped)."""
    w, n = inp["cols"].shape[:2]
    roomy = int(inp["vis"].sum(1).max())
    tight = overflow_capacity(inp["vis"])
    over = packed_slabs(inp["cols"], inp["vis"], inp["pos"], tight)
    kept = torch.stack([unpack_slab_ref(over[v], n, tight)[0] for v in range(w)])
    forms = []
    for name, cap, cols in (("dense", None, inp["cols"]), ("packed", roomy, inp["cols"]), ("packed_overflow", tight, kept)):
        if packed_only and cap is None:
            continue
        forms.append((name, -1, cap, cols))
        forms += [(f"{name}_add_skip{s}", s, cap, cols) for s in range(w)]
    return forms
