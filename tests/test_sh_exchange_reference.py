"""The restatements tests/test_gpu_sh_exchange.py holds the SH gradient exchange kernels to (tests/_dp_ref.py), checked here without a
GPU: ``rebuild_ref64`` against autograd through the oracle's dense SH evaluation, the packed slab's round trip, the conditions the
synthetic inputs are meant to meet, and the distance of a plain fp32 restatement of the rebuild from ``rebuild_ref64`` — the figure the
kernels' bound KAPPA is four times of."""
import math

import pytest
import torch

import _dp_ref as ref

DEGREES = (0, 1, 2, 3)


def _scale(w):
    return float(torch.tensor(1.0 / w, dtype=torch.float32))          # what the kernel receives: 1 / w as a float


@pytest.mark.parametrize("degree", DEGREES)
def test_rebuild_ref64_equals_autograd(degree):
    """The closed form against ``make_rebuild_ref`` (autograd through oracle.dense_ref.sh_colors) run in float64: every row to 1e-12
    of its own norm, the rebuild form and the add form with every skip_view; bands above the degree are zero / the own rows'."""
    from oracle import dense_ref

    n, w = 65, 3
    inp = ref.exchange_inputs(n, w)
    scale = _scale(w)
    autograd = ref.make_rebuild_ref(dense_ref)
    slabs = ref.dense_slabs(inp["cols"], inp["pos"]).double()
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        for skip in (-1, 0, 1, 2):
            own = ref.own_rows(inp["cols"], inp["pos"], inp["means"], degree, scale, skip).double() if skip >= 0 else None
            v0 = torch.full((n, 3), float("nan")) if own is None else own[:, 0].clone()
            vN = torch.full((n, 15, 3), float("nan")) if own is None else own[:, 1:].clone()
            autograd(slabs, inp["means"].double(), n, w, degree, 16, None, v0, vN, skip_view=skip, scale=scale)
            got = torch.cat([v0[:, None], vN], 1)
            want, mag = ref.rebuild_ref64(inp["cols"], inp["pos"], inp["means"], degree, scale, skip, own)
            assert want.dtype == torch.float64 and mag.dtype == torch.float64
            err = (got - want).reshape(n, -1).norm(dim=1)
            size = want.reshape(n, -1).norm(dim=1)
            assert bool((err <= 1e-12 * size).all()), (degree, skip, float((err / size.clamp_min(1e-300)).max()))
            assert bool((mag >= want.abs() * (1 - 1e-12)).all())                 # A bounds the rows it is the magnitude of
            nb = (degree + 1) ** 2
            if own is None:
                assert bool((want[:, nb:] == 0).all()) and bool((mag[:, nb:] == 0).all())
            else:
                assert torch.equal(want[:, nb:], own[:, nb:])
    finally:
        torch.set_default_dtype(prev)


def test_absolute_basis_bounds_the_basis():
    d = torch.nn.functional.normalize(torch.randn(4096, 3, generator=torch.Generator().manual_seed(3), dtype=torch.float64), dim=-1)
    for degree in DEGREES:
        y, ybar = ref.sh_basis_ref(degree, d), ref.sh_basis_ref(degree, d, absolute=True)
        assert bool((ybar >= y.abs()).all()) and bool((ybar[:, (degree + 1) ** 2:] == 0).all())
        assert bool((ybar[:, :(degree + 1) ** 2] > 0).all())
    z = torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float64)                      # on the axis: band 6 is 0.9462 - 0.3154, its magnitude the sum
    assert math.isclose(float(ref.sh_basis_ref(2, z)[0, 6]), 0.9461746957575601 - 0.3153915652525201)
    assert math.isclose(float(ref.sh_basis_ref(2, z, absolute=True)[0, 6]), 0.9461746957575601 + 0.3153915652525201)


@pytest.mark.parametrize("n,w", ref.EXCHANGE_CASES + (ref.EXCHANGE_BIG,))
def test_inputs_meet_their_conditions(n, w):
    inp = ref.exchange_inputs(n, w)
    dist = (inp["means"][None].double() - inp["pos"][:, None].double()).norm(dim=-1)
    assert float(dist.min()) >= 1.0
    zero = (inp["cols"] == 0).all(-1)
    assert bool(zero[~inp["vis"]].all())                                        # invisible: zero, so packed and dense slabs hold the same colours
    if n >= 63:
        assert bool(zero.all(0).any()) and bool((zero & inp["vis"]).any())      # zero in every view; visible and zero
    if n >= 10_000:
        assert 0.25 < float(zero.float().mean()) < 0.40
        live = inp["cols"].abs().amax(-1)[~zero]
        assert float(live.max() / live.min()) > 1e3                            # dim rows beside bright ones
    counts = inp["vis"].sum(1)
    tight = ref.overflow_capacity(inp["vis"])
    if int(counts.max()) > 0:
        assert int((counts > tight).sum()) >= 1 and tight == int(counts.max()) - 1


@pytest.mark.parametrize("n,w", ref.EXCHANGE_CASES + (ref.EXCHANGE_BIG,))
def test_packed_slab_round_trip(n, w):
    """pack_slab_ref -> unpack_slab_ref gives the colours back (zeros where invisible); with one row too few, the rows of the first
    ``capacity`` visible Gaussians and zeros behind them; the layout is the kernels' formula."""
    inp = ref.exchange_inputs(n, w)
    nb = (n + 63) // 64
    for v in range(w):
        vis, cols = inp["vis"][v], inp["cols"][v]
        count = int(vis.sum())
        for cap in {n, count, max(count - 1, 0), 0}:
            nblk, rows0, total = ref.packed_layout(n, cap)
            assert nblk == nb and rows0 % 4 == 0 and total % 4 == 0 and rows0 >= 8 + 3 * nb and total >= rows0 + 3 * cap
            slab = ref.pack_slab_ref(cols, vis, inp["pos"][v], cap)
            assert slab.numel() == total
            ints = slab.view(torch.int32)
            assert (int(ints[0]), int(ints[4]), int(ints[5]), int(ints[6]), int(ints[7])) == (count, cap, n, 0, 0)
            back, pos = ref.unpack_slab_ref(slab, n, cap)
            assert torch.equal(pos, inp["pos"][v])
            order = torch.cumsum(vis.long(), 0) - vis.long()
            kept = vis & (order < cap)
            assert int(kept.sum()) == min(count, cap)
            assert torch.equal(back[kept].view(torch.int32), cols[kept].view(torch.int32)) and bool((back[~kept] == 0).all())


def test_fp32_restatement_lies_within_cpu_ratio_of_ref64():
    """The rebuild written in plain fp32 torch against ``rebuild_ref64``, every row of every case, degree and form: the worst
    ||row error||_2 / (2^-24 ||A_row||_2) is _dp_ref.CPU_RATIO (rounded up) and KAPPA is four times that, rounded up."""
    worst, where = 0.0, None
    for n, w in ref.EXCHANGE_CASES + (ref.EXCHANGE_BIG,):
        inp = ref.exchange_inputs(n, w)
        scale = _scale(w)
        for degree in DEGREES:
            for name, skip, cap, cols in ref.exchange_forms(inp, packed_only=(n, w) == ref.EXCHANGE_BIG):
                if name.startswith("packed") and not name.startswith("packed_overflow"):
                    continue                                                     # the colours of the dense form
                own = ref.own_rows(inp["cols"], inp["pos"], inp["means"], degree, scale, skip) if skip >= 0 else None
                want, mag = ref.rebuild_ref64(cols, inp["pos"], inp["means"], degree, scale, skip, own)
                got, _ = ref.rebuild_ref(cols, inp["pos"], inp["means"], degree, scale, skip, own, dtype=torch.float32)
                assert got.dtype == torch.float32
                ratio, dead_wrong = ref.row_ratio(got, want, mag, degree)
                assert dead_wrong == 0, (n, degree, name)
                if ratio > worst:
                    worst, where = ratio, (n, degree, name)
    print(f"fp32 restatement: worst row ratio {worst:.3f} at {where}; CPU_RATIO {ref.CPU_RATIO}, KAPPA {ref.KAPPA}")
    assert worst <= ref.CPU_RATIO
    assert ref.CPU_RATIO <= 1.25 * worst                                        # the recorded figure is the measured one, not a loose cap
    assert ref.KAPPA == math.ceil(4 * ref.CPU_RATIO)
