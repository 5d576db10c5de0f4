"""CPU checks of the scenes and of the comparator behind tests/test_gpu_projection_edges.py (tests/_proj_ref.py): every scene builder
produces what it advertises — judged with the fp64 oracle alone —, the exclusion masks stay under their caps (conditions on the INPUTS,
so a GPU run cannot pass by excluding its failures), and the comparator rejects nine subtly wrong kernels while it accepts the fp32
oracle at k = 1."""
import pytest
import torch

import _proj_ref as P

CAT = P.catalogue()


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(name):
        if name not in cache:
            s = CAT[name][0]()
            cache[name] = P.reference(s, P.make_cotangents(s.N, s.cfg, **P.ALL_ROUTES))
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(CAT))
def test_scene_is_what_it_advertises(name, refs, orc):
    r = refs(name)
    s = r.scene
    vis = r.out["radii"] > 0
    if name.startswith("n") and name[1:].isdigit():
        assert s.N == int(name[1:])
    if name.startswith("pattern_"):
        assert s.N == 128 + 37
        assert not bool(r.edge.any())
        assert P.wave_words(vis) == P.wave_words(P.pattern_mask(name[len("pattern_"):]))
    if s.visible is not None:
        judged = ~r.edge
        assert torch.equal(vis[judged], s.visible[judged]), "the fp64 decision is not the advertised one"
    shares = r.shares()
    if name in P.CONSTRUCTED:
        # only the Gaussians deliberately put on the boundary may be flagged: judged on the RAW mask of oracle.project_edge
        allowed = s.may_be_edge
        if name.startswith("depth_boundary"):
            # project_edge's depth envelope is 4e-6 |z| = 2^-17.9 |z|: it also flags j = 18 .. 20.  Reference.edge drops those flags
            # (cut to j >= 21), so they are judged like every other member
            j = s.tags["j"]
            allowed = j >= 18
            assert bool((vis == s.visible)[j <= 20].all()) and not bool(r.edge[j <= 20].any())
        assert bool((r.edge_raw <= allowed).all()), torch.nonzero(r.edge_raw & ~allowed).flatten().tolist()
        assert bool((r.edge <= s.may_be_edge).all())
        assert not bool(r.clamp_edge.any())
        # rank-one covariances have two zero scales: the normal's axis is tied for every member, by construction
        assert bool(r.normal_tie.all()) if name.startswith("singular") else not bool(r.normal_tie.any())
    else:
        for k, cap in P.CAPS.items():
            assert shares[k] <= cap, (k, shares[k])
    if s.cfg.tight_tiles:
        # compare() leaves the tight boxes that hinge on the last place of logf / sqrtf unjudged: that share is a condition on the inputs too
        assert int(r.tight_near.sum()) <= P.TIGHT_NEAR_CAP * s.N, torch.nonzero(r.tight_near).flatten().tolist()
    # the fp32 oracle is within k = 1 of the reference by construction of (a)
    fails, ratios, _ = P.compare(P.as_got(r.out32), r, dict(fwd=1.0, geo=1.0, sh=1.0))
    assert not fails, fails
    assert max(ratios.values()) <= 1.0


@pytest.mark.parametrize("name", [n for n in CAT if CAT[n][1] != ("colors",)])
def test_layout_the_binding_chooses(name):
    s = CAT[name][0]()
    for layout in CAT[name][1]:
        t = P.layout_tensors(s.coeffs, layout)
        want = P.INTENDED_LAYOUT[layout] if s.coeffs.shape[1] == 16 else "direct"
        assert P.binding_layout(s.cfg, **t) == want, (layout, want)
        cat = torch.cat([t["sh0"][:, None], t["shN"]], 1) if "sh0" in t else t["coeffs"]
        assert torch.equal(cat.detach(), s.coeffs)


def _radial_quat_gradient(r):
    """What a backward WITHOUT the projection onto the tangent of q / |q| adds to v_quats: (vqn . qn) qn / |q|, vqn the gradient with
    respect to the normalised quaternion of the kernel's rotation formula R(qn) (which does not normalise again).  That formula is
    quadratic in qn apart from the ones on the diagonal, R(lambda qn) = I + lambda^2 (R - I), so vqn . qn = d loss / d lambda at 1
    = 2 d loss / d mu at mu = 1 with R(mu) = I + mu (R - I): one fp64 autograd pass through the dense projection with that rotation."""
    import _pose_ref
    from oracle import dense_ref

    s, cfg, cot = r.scene, r.scene.cfg, r.cot
    N = s.N
    q = s.quats.double()
    mu = torch.ones(N, dtype=torch.float64, requires_grad=True)
    eye = torch.eye(3, dtype=torch.float64)
    R_of = dense_ref.quat_to_rotmat
    Rm = eye + mu[:, None, None] * (R_of(q) - eye)
    sc = torch.exp(s.scales.double()) if cfg.scales_are_log else s.scales.double()
    op = torch.sigmoid(s.opacities.double()) if cfg.opacities_are_logit else s.opacities.double()
    pr = _pose_ref.project_per_gaussian(s.means.double(), q, sc, s.viewmat.double()[None].repeat(N, 1, 1), s.K.double(), P.W, P.H,
                                        eps2d=cfg.eps2d, near=cfg.near_plane, far=cfg.far_plane, radius_clip=cfg.radius_clip, rotmats=Rm)
    vr = cot["v_splats"].double()
    vis = (r.out["radii"] > 0)
    loss = (pr["conics"] * (vr[:, 2:5] + cot["v_conics"].double()))[vis].sum()
    v_comp = cot["v_compensations"].double() + vr[:, 5] * op          # antialiased: the record's opacity is opacity x compensation
    loss = loss + (pr["compensations"] * v_comp)[vis].sum()
    ch = 6 + 3 + int(cfg.with_depth)
    kmin = torch.argmin(s.scales, dim=-1)
    col = Rm[torch.arange(N), :, kmin]
    n = col / col.norm(dim=-1, keepdim=True)
    sgn = torch.sign((r.out["normals_world"] * R_of(q)[torch.arange(N), :, kmin]).sum(-1))
    ncam = (n * sgn[:, None]) @ s.nf[:9].double().reshape(3, 3).T
    loss = loss + (ncam * vr[:, ch:ch + 3])[vis].sum()
    (dmu,) = torch.autograd.grad(loss, mu)
    qn = q / q.norm(dim=-1, keepdim=True)
    return (2.0 * dmu / q.norm(dim=-1))[:, None] * qn


def _mutations(r):
    s, cfg = r.scene, r.scene.cfg
    vis = r.out["radii"] > 0
    v = torch.nonzero(vis).flatten()

    def conic_b_sign(g):
        g["conics"][:, 1] *= -1; g["splats"][:, 3] *= -1

    def radius_off_by_one(g):
        g["radii"][v[0]] += 1

    def box_one_tile_short(g):
        wide = torch.nonzero((g["tile_boxes"][:, 1] & 0xffff) > 1).flatten()[0]
        g["tile_boxes"][wide, 1] -= 1
        w, h = int(g["tile_boxes"][wide, 1]) & 0xffff, int(g["tile_boxes"][wide, 1]) >> 16
        g["tiles_bin"][wide] = w * h

    def colour_without_half(g):
        g["splats"][:, 6:9] = torch.where(vis[:, None], torch.clamp_min(g["splats"][:, 6:9] - 0.5, 0.0), g["splats"][:, 6:9])

    def sh_band_shifted(g):
        g["v_shN"] = g["v_shN"].clone(); g["v_shN"][:, 3:8] = torch.roll(g["v_shN"][:, 3:8], 1, dims=1)
        g["v_coeffs"] = None

    def quat_without_tangent_projection(g):
        g["v_quats"] = g["v_quats"] + _radial_quat_gradient(r).float()

    def scales_without_exp(g):
        g["v_scales"] = g["v_scales"] / torch.exp(s.scales)

    def opacity_without_compensation(g):
        g["splats"][:, 5] = torch.where(vis, torch.sigmoid(s.opacities), g["splats"][:, 5])

    def lanes_63_and_64_swapped(g):
        # the staged store of the coefficient-gradient rows: the last row of one workgroup and the first of the next change places
        assert bool(vis[63]) and bool(vis[64])
        g["v_shN"] = g["v_shN"].clone(); g["v_shN"][[63, 64]] = g["v_shN"][[64, 63]]
        g["v_coeffs"] = None

    assert cfg.antialiased and cfg.scales_are_log and cfg.opacities_are_logit
    return [conic_b_sign, radius_off_by_one, box_one_tile_short, colour_without_half, sh_band_shifted, quat_without_tangent_projection,
            scales_without_exp, opacity_without_compensation, lanes_63_and_64_swapped]


def test_comparator_rejects_subtly_wrong_kernels(orc):
    culled = P._some_culled(200, 70)
    culled[63] = culled[64] = False
    s = P.random_scene(200, P.base_cfg(**P.FULL, antialiased=True, with_depth=True, with_normals=True, want_normals_world=True), seed=70,
                       culled=culled)
    r = P.reference(s, P.make_cotangents(s.N, s.cfg, **P.ALL_ROUTES))
    k1 = dict(fwd=1.0, geo=1.0, sh=1.0)
    fails, _, _ = P.compare(P.as_got(r.out32), r, k1)
    assert not fails, fails
    for mutate in _mutations(r):
        got = P.as_got(r.out32)
        mutate(got)
        # at k = 64, four times the largest k the GPU test uses
        fails, _, _ = P.compare(got, r, dict(fwd=64.0, geo=64.0, sh=64.0))
        assert fails, f"the comparator accepted: {mutate.__name__}"
