"""Thin lens on the CPU: the product's generate_path / lens_point / camera_ray_lens (tests/emu/lens_emu.cpp compiles
gpuspectral_amd/csrc/pt_stages.h for the host) against the oracle's render and RNG, the apertures' uniform densities, a float64
restatement of the lens ray, and the analytic circle of confusion."""
import numpy as np
import pytest

from lens_util import CIRCLE, HEXAGON_ROT, LENSES, PENTAGON, LensEmu, inside_polygon, polygon_vertices, same
from test_pixel_filter_cpu import BOX, GAUSSIAN, NONE, TENT, FilterEmu, ks, pairs

N_DENSITY = 1 << 17
ALPHA = 1e-3                                              # significance of every distribution test below
KS_BOUND = np.sqrt(-0.5 * np.log(ALPHA / 2)) / np.sqrt(N_DENSITY)  # asymptotic Kolmogorov quantile: P(D_n > bound) = ALPHA
Z_ALPHA = 3.0902                                          # standard normal quantile of 1 - ALPHA


def chi2_quantile(k):
    """Wilson-Hilferty approximation of the (1 - ALPHA) quantile of chi-square with k degrees of freedom."""
    return k * (1 - 2 / (9 * k) + Z_ALPHA * np.sqrt(2 / (9 * k))) ** 3


@pytest.fixture(scope="module")
def lemu():
    return LensEmu()


@pytest.fixture(scope="module")
def femu():
    return FilterEmu()


# ---- radius 0 is the reference ----------------------------------------------------------------------------------------------
def test_radius_zero_equals_the_oracle(lemu, oracle_mod, cornell):
    W, H, SPP = 40, 32, 4
    ref, ost = oracle_mod.Oracle(cornell).render(W, H, spp=SPP)
    for lens in (None, dict(radius=0.0, focus_distance=3.0, blades=6, rotation=0.7), dict(radius=0.0, focus_distance=0.0, blades=16, rotation=-2.0)):
        img, st = lemu.scene(cornell).render(W, H, SPP, lens=lens)
        assert same(img, ref)
        assert st["extension_rays"] == ost["extension_rays"] and st["shadow_rays"] == ost["shadow_rays"]
    img, _ = lemu.scene(cornell).render(W, H, SPP, lens=CIRCLE)
    assert not same(img, ref)


# ---- draw order and seed hand-off: integers -------------------------------------------------------------------------------
def stream4(orc, width, gids, tss):
    """(u[n,4] as float32, states[n,5]: before any draw and after each of four) from the oracle's own RNG functions."""
    u = np.zeros((len(gids), 4), np.float32)
    st = np.zeros((len(gids), 5), np.uint32)
    for i, (g, t) in enumerate(zip(gids, tss)):
        s = orc.pcg_hash(orc.tea(int(width * (g // width) + g % width), int(t)))
        st[i, 0] = s
        for k in range(4):
            out, s = orc.rand_pcg(s, 1)
            st[i, k + 1] = s
            u[i, k] = np.float32(out[0]) * np.float32(2.0 ** -32)
    return u, st


def lens_point_f64(lens, u3, u4):
    """The header's two samplers in float64 from the float32 variates."""
    R, n, rot = lens["radius"], lens["blades"], lens["rotation"]
    u3 = u3.astype(np.float64)
    u4 = u4.astype(np.float64)
    if n == 0:
        ux, uy = 2 * u3 - 1, 2 * u4 - 1
        big = np.abs(ux) > np.abs(uy)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(big, ux, uy)
            th = np.where(big, (np.pi / 4) * (uy / ux), np.pi / 2 - (np.pi / 4) * (ux / uy))
        zero = (ux == 0) & (uy == 0)
        return np.where(zero[:, None], 0.0, R * np.stack([r * np.cos(th), r * np.sin(th)], 1))
    t = np.float32(u3).astype(np.float32) * np.float32(n)  # (k is decided by the float32 product, as in the header)
    k = np.minimum(t.astype(np.uint32), n - 1)
    a = np.sqrt(t.astype(np.float64) - k)
    v = polygon_vertices(R, n, rot)
    v0, v1 = v[k], v[(k + 1) % n]
    return a[:, None] * ((1 - u4)[:, None] * v0 + u4[:, None] * v1)


@pytest.mark.parametrize("name", list(LENSES))
@pytest.mark.parametrize("filt,param", [(NONE, 0.0), (BOX, 0.0), (TENT, 1.5), (GAUSSIAN, 0.0)])
def test_draw_order_and_seed(lemu, femu, oracle_mod, cornell, name, filt, param):
    lens = LENSES[name]
    W, H = 96, 64
    gids, tss = pairs(W, H, 600, 31 + filt)
    o, d, lp, seed = lemu.generate(cornell, W, H, lens, gids, tss, filt, param)
    u, st = stream4(oracle_mod, W, gids, tss)
    first = 0 if filt == NONE else 2  # u3, u4 come directly after the filter's two draws, or directly after the seed
    assert np.array_equal(seed, st[:, first + 2])  # prd.seed = the state after them
    ref = lens_point_f64(lens, u[:, first], u[:, first + 1])
    assert np.abs(lp - ref).max() <= 8 * np.spacing(np.float32(lens["radius"]))  # float32 formulas against float64: rounding only
    # the filter's own draws are the ones a filtered pinhole frame makes
    if filt != NONE:
        _, _, off, fseed = femu.generate(cornell, W, H, filt, param, gids, tss)
        assert np.array_equal(fseed, st[:, 2])
    # the lens point is what the product's sampler gives from that state, bit for bit
    pts, after = lemu.points(lens["radius"], lens["blades"], lens["rotation"], st[:, first])
    assert same(pts, lp) and np.array_equal(after, seed)
    # radius 0 draws nothing: the seed is the filtered / unfiltered pinhole's
    _, _, lp0, seed0 = lemu.generate(cornell, W, H, dict(lens, radius=0.0), gids, tss, filt, param)
    assert np.array_equal(seed0, st[:, first]) and not lp0.any()


# ---- aperture density -------------------------------------------------------------------------------------------------------
def states(n, seed):
    return np.random.RandomState(seed).randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)


def circle_statistics(pts, R):
    """KS distances of r^2 / R^2 and of the angle against the uniform law (a uniform disc has both uniform)."""
    p = pts.astype(np.float64)
    r2 = (p ** 2).sum(1) / R ** 2
    ang = (np.arctan2(p[:, 1], p[:, 0]) / (2 * np.pi)) % 1.0
    return ks(r2, lambda x: np.clip(x, 0, 1)), ks(ang, lambda x: np.clip(x, 0, 1))


def polygon_statistics(pts, R, n, rot, cells=24):
    """(chi-square of the per-sector counts, its dof; chi-square of the counts of the grid cells that lie wholly inside, their number).
    A cell's count is Binomial(N, p): (O - E)^2 / (E (1 - p)) summed over cells is chi-square with one degree per cell up to the
    cells' slight negative correlation, which only lowers it."""
    p = pts.astype(np.float64)
    N = len(p)
    sector = np.floor((((np.arctan2(p[:, 1], p[:, 0]) - rot) / (2 * np.pi)) % 1.0) * n).astype(int) % n
    cnt = np.bincount(sector, minlength=n)
    chi_sector = float(((cnt - N / n) ** 2 / (N / n)).sum())
    verts = polygon_vertices(R, n, rot)
    area = 0.5 * n * R * R * np.sin(2 * np.pi / n)
    h = 2 * R / cells
    ix = np.floor((p[:, 0] + R) / h).astype(int)
    iy = np.floor((p[:, 1] + R) / h).astype(int)
    ok = (ix >= 0) & (ix < cells) & (iy >= 0) & (iy < cells)
    grid = np.bincount(ix[ok] * cells + iy[ok], minlength=cells * cells).reshape(cells, cells)
    chi = 0.0
    k = 0
    for i in range(cells):
        for j in range(cells):
            corners = np.array([[-R + (i + a) * h, -R + (j + b) * h] for a in (0, 1) for b in (0, 1)])
            if inside_polygon(corners, verts, 0.0).all():
                pc = h * h / area
                chi += (grid[i, j] - N * pc) ** 2 / (N * pc * (1 - pc))
                k += 1
    return chi_sector, n - 1, chi, k


def test_circle_density(lemu):
    R = 0.37
    pts, _ = lemu.points(R, 0, 0.0, states(N_DENSITY, 1))
    assert (np.hypot(pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)) <= R * (1 + 4e-7)).all()  # inside, to float32 rounding
    d_r, d_a = circle_statistics(pts, R)
    print("circle: KS r^2 %.5f, KS angle %.5f, bound %.5f" % (d_r, d_a, KS_BOUND))
    assert d_r <= KS_BOUND and d_a <= KS_BOUND
    # the same statistic rejects the radius without the square root (r = R u: too many points near the centre)
    rng = np.random.RandomState(2)
    rr, th = R * rng.uniform(size=N_DENSITY), 2 * np.pi * rng.uniform(size=N_DENSITY)
    wrong = np.stack([rr * np.cos(th), rr * np.sin(th)], 1)
    assert circle_statistics(wrong, R)[0] > 10 * KS_BOUND


@pytest.mark.parametrize("n,rot", [(5, 0.0), (6, 0.4)])
def test_polygon_density(lemu, n, rot):
    R = 0.37
    st = states(N_DENSITY, 3 + n)
    pts, _ = lemu.points(R, n, rot, st)
    assert inside_polygon(pts.astype(np.float64), polygon_vertices(R, n, rot), 4e-7 * R).all()
    cs, ks_, cg, kg = polygon_statistics(pts, R, n, rot)
    print("%d blades: sectors chi2 %.2f (dof %d, bound %.2f), grid chi2 %.1f (%d cells, bound %.1f)" % (n, cs, ks_, chi2_quantile(ks_), cg, kg, chi2_quantile(kg)))
    assert kg > 100
    assert cs <= chi2_quantile(ks_) and cg <= chi2_quantile(kg)
    # the same statistic rejects a = t - k without the square root (points pile up at the centre)
    u = np.random.RandomState(9).uniform(size=(N_DENSITY, 2))
    t = u[:, 0] * n
    k = np.minimum(t.astype(int), n - 1)
    v = polygon_vertices(R, n, rot)
    wrong = (t - k)[:, None] * ((1 - u[:, 1])[:, None] * v[k] + u[:, 1][:, None] * v[(k + 1) % n])
    assert inside_polygon(wrong, v, 1e-12).all()
    assert polygon_statistics(wrong, R, n, rot)[2] > 10 * chi2_quantile(kg)


# ---- convergence on the plane of focus ------------------------------------------------------------------------------------
# Bound of the test below, in float32 ulps of the focus distance: the next power of two above the maximum measured against the
# float64 restatement (profiles/lens_cpu_check.txt), as DESIGN 14 did for the filtered ray.
CONVERGENCE_BOUND_ULP = 0.5


def lens_ray_f64(sc, W, H, c, frag, lpts):
    """The header's camera ray in float64 from the float32 inputs (fragCoord, lens point, zplane, s): (origin, direction, the
    pinhole ray's point on the plane of focus), world space."""
    tw = np.asarray(sc.to_world, np.float64).reshape(4, 4)  # glm memory order: tw[c][r]
    lin = lambda v: np.stack([v[:, 0:1] * tw[0, :3] + v[:, 1:2] * tw[1, :3] + v[:, 2:3] * tw[2, :3]], 0)[0] * np.array([1.0, -1.0, 1.0])
    x = frag[:, 0].astype(np.float64) - W / 2.0
    y = frag[:, 1].astype(np.float64) - H / 2.0
    s, D = float(c["s"]), float(c["focus"])
    pf = np.stack([-x * s, y * s, np.full(len(x), D)], 1)
    l = np.concatenate([lpts.astype(np.float64), np.zeros((len(x), 1))], 1)
    dl = pf - l
    dl /= np.linalg.norm(dl, axis=1, keepdims=True)
    eye = tw[3, :3]
    return eye + lin(l), lin(dl), eye + lin(pf)


@pytest.mark.parametrize("name", list(LENSES))
def test_lens_rays_meet_on_the_plane_of_focus(lemu, cornell, name):
    lens = dict(LENSES[name], radius=0.3)
    W, H = 96, 64
    rng = np.random.RandomState(17)
    n = 20000
    frag = rng.uniform(0, [W, H], (n, 2)).astype(np.float32)
    pts, _ = lemu.points(lens["radius"], lens["blades"], lens["rotation"], states(n, 21))
    o, d = lemu.ray_through(cornell, W, H, lens, frag, pts)
    c = lemu.consts(cornell, W, H, lens)
    o64, d64, P = lens_ray_f64(cornell, W, H, c, frag, pts)
    # (1) against the restatement, in float32 ulps of the VECTOR's size (1 for the direction): pf - l cancels, so a component's
    # error is relative to its operands, not to itself
    err_d = (np.abs(d.astype(np.float64) - d64) / np.spacing(np.float32(1.0))).max()
    err_o = (np.abs(o.astype(np.float64) - o64) / np.spacing(np.abs(o64).max(1).astype(np.float32))[:, None]).max()
    # (2) the float32 ray passes the pinhole ray's point on the plane of focus: distance of P from the line, in ulps of D
    of, df = o.astype(np.float64), d.astype(np.float64)
    t = ((P - of) * df).sum(1) / (df * df).sum(1)
    miss = np.linalg.norm(P - of - t[:, None] * df, axis=1) / np.spacing(np.float32(lens["focus_distance"]))
    # ... and so does the restatement, to float64 rounding (the formulas, not only the arithmetic, converge)
    t64 = ((P - o64) * d64).sum(1)
    miss64 = np.linalg.norm(P - o64 - t64[:, None] * d64, axis=1)
    print("%s: direction %.2f ulp, origin %.2f ulp, miss on the plane of focus %.3f ulp of D (float64 restatement: %.2e)"
          % (name, err_d, err_o, miss.max(), miss64.max()))
    assert miss64.max() < 1e-12
    # direction: the operations of the pinhole ray (bound 4 ulp in test_pixel_filter_cpu.test_ray_through_offset_float64) plus one
    # product and one difference per component, each at most half an ulp of a vector no longer than the difference it enters,
    # before the normalisation: 4 + 1.  Origin: a 3x3 map of a vector far shorter than the eye's distance + one sum: 1
    assert err_d <= 5.0 and err_o <= 1.0
    assert miss.max() <= CONVERGENCE_BOUND_ULP
    # two lens points of one fragCoord give different rays through the same point
    assert np.abs(d[::2] - lemu.ray_through(cornell, W, H, lens, frag[::2], pts[1::2])[1]).max() > 1e-3


# ---- optics: the circle of confusion ----------------------------------------------------------------------------------------
EYE_Z, FOV = 5.0, 40.0


def emitter_at(depth, half):
    """One small emitting square (two triangles) on the optical axis at camera-space depth `depth`, facing the camera; nothing
    else: a black background."""
    from gpuspectral_amd import scenes

    b = scenes.SceneBuilder()
    black = b.diffuse((0.0, 0.0, 0.0))
    b.camera_lookat((0, 0, EYE_Z), (0, 0, 0), fov_deg=FOV)
    z = EYE_Z - depth
    q = np.array([[-half, -half, z], [half, -half, z], [half, half, z], [-half, -half, z], [half, half, z], [-half, half, z]], np.float32)
    mesh = b.add_mesh(q, np.tile(np.array([0, 0, 1], np.float32), (6, 1)))
    b.add_object(mesh, np.eye(4, dtype=np.float32).reshape(16), black, twofaced=True, emission=np.array([5.0, 5.0, 5.0], np.float32))
    return b.build()


def window(W, H, half):
    xs = np.arange(W // 2 - half, W // 2 + half)
    return (xs[None, :] + W * np.arange(H // 2 - half, H // 2 + half)[:, None]).reshape(-1).astype(np.uint32)


def hit_mask(orc, o, d):
    rays = np.zeros((len(o), 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, 0.0, d, 1e10
    return orc.trace(rays)["prim"] >= 0


def test_circle_of_confusion(lemu, femu, oracle_mod):
    """Emitter at depth z = 5, focus at D = 2.5, R = 0.25, BOX pixel filter (fragCoords uniform over the window).  The samples
    that hit are draws from (aperture disc scaled to the image) convolved with (the emitter's image): the mean of |fragCoord - c|^2
    over them estimates rc^2 / 2 + 2 a^2 / 3 (rc = the circle of confusion's radius, a = the square's half-size, both in pixels);
    its standard error is that of a mean of independent draws.  Bound: 4 standard errors."""
    W = H = 64
    z, D, R, half = 5.0, 2.5, 0.25, 0.05
    sc = emitter_at(z, half)
    orc = oracle_mod.Oracle(sc)
    lens = dict(radius=R, focus_distance=D, blades=0, rotation=0.0)
    zplane = float(lemu.consts(sc, W, H, lens)["zplane"])
    rc = 0.5 * (2 * R * abs(z - D) / z * zplane / D)  # half the analytic diameter of the issue
    a = half * zplane / z
    gids = window(W, H, 8)
    assert rc + a * np.sqrt(2) < 7.5  # the window holds the whole blur
    g2 = []
    for ts in range(1500):
        tss = np.full(len(gids), ts, np.uint32)
        o, d, _, _ = lemu.generate(sc, W, H, lens, gids, tss, BOX, 0.0)
        off = femu.generate(sc, W, H, BOX, 0.0, gids, tss)[2]
        hit = hit_mask(orc, o, d)
        frag = np.stack([gids % W, gids // W], 1).astype(np.float32) + off
        g2.append((((frag[hit].astype(np.float64) - [W / 2.0, H / 2.0]) ** 2).sum(1)))
    g2 = np.concatenate(g2)
    est, se = g2.mean(), g2.std(ddof=1) / np.sqrt(len(g2))
    expect = rc * rc / 2 + 2 * a * a / 3
    print("circle of confusion: %d hits, second moment %.4f +- %.4f px^2, analytic %.4f (rc %.3f px, a %.3f px): %.2f sigma"
          % (len(g2), est, se, expect, rc, a, (est - expect) / se))
    assert len(g2) > 3000
    assert abs(est - expect) <= 4 * se
    # ... and a pinhole has the emitter's own second moment only (the estimator sees the difference)
    assert expect > 10 * (2 * a * a / 3)


def test_in_focus_image_equals_pinhole(lemu, oracle_mod):
    """Emitter on the plane of focus, its edges half-way between pixel centres' rays: every lens sample hits exactly when the
    pinhole ray of its pixel does, so the two images are equal."""
    W = H = 64
    z = 5.0
    lens = dict(radius=0.25, focus_distance=z, blades=0, rotation=0.0)
    zplane = float(lemu.consts(emitter_at(z, 0.1), W, H, lens)["zplane"])
    sc = emitter_at(z, 3.5 * z / zplane)  # 3.5 pixels: the edges fall between the integer fragCoords around c = (32, 32)
    orc = oracle_mod.Oracle(sc)
    gids = window(W, H, 8)
    o, d, _, _ = lemu.generate(sc, W, H, None, gids, np.zeros(len(gids), np.uint32))
    pin = hit_mask(orc, o, d)
    assert pin.sum() == 49  # 7 x 7 fragCoords inside (-3.5, 3.5)^2
    moved = 0.0
    for ts in range(64):
        o, d, lp, _ = lemu.generate(sc, W, H, lens, gids, np.full(len(gids), ts, np.uint32))
        assert np.array_equal(hit_mask(orc, o, d), pin), ts
        moved = max(moved, float(np.abs(lp).max()))
    assert moved > 0.2  # (the lens points did span the aperture)
    # out of focus the same emitter's image does change
    o, d, _, _ = lemu.generate(sc, W, H, dict(lens, focus_distance=2.5), gids, np.zeros(len(gids), np.uint32))
    assert not np.array_equal(hit_mask(orc, o, d), pin)


def test_hexagon_blur_support(lemu, femu, oracle_mod):
    """6 blades: every fragCoord that sees the (tiny) emitter lies in the aperture hexagon scaled to the image -- mirrored
    through the centre for an emitter behind the plane of focus -- grown by the emitter's own image; and some lie outside the
    hexagon's inscribed circle, i.e. the support is the polygon, not a smaller disc."""
    W = H = 64
    z, D, R, half = 5.0, 2.5, 0.25, 0.01
    lens = dict(radius=R, focus_distance=D, blades=6, rotation=0.4)
    sc = emitter_at(z, half)
    orc = oracle_mod.Oracle(sc)
    zplane = float(lemu.consts(sc, W, H, lens)["zplane"])
    scale = -(1 - z / D) * zplane / z  # camera-space lens offset -> image-plane v = (-(fx - W/2), fy - H/2), see the docstring above
    a = half * zplane / z
    verts = scale * polygon_vertices(R, 6, 0.4)
    # (a negative scale is a point reflection: the counter-clockwise order stays)
    gids = window(W, H, 8)
    vs = []
    for ts in range(4000):  # (BOX filter: the fragCoords cover the window, not only its lattice)
        tss = np.full(len(gids), ts, np.uint32)
        o, d, lp, _ = lemu.generate(sc, W, H, lens, gids, tss, BOX, 0.0)
        hit = hit_mask(orc, o, d)
        frag = (np.stack([gids % W, gids // W], 1).astype(np.float32) + femu.generate(sc, W, H, BOX, 0.0, gids, tss)[2])[hit]
        fx, fy = frag[:, 0].astype(np.float64), frag[:, 1].astype(np.float64)
        v = np.stack([-(fx - W / 2.0), fy - H / 2.0], 1)
        vs.append(v)
        # exact geometry: the ray from lens point l crosses depth z at l (1 - z / D) + v z / zplane, inside the square
        x = lp[hit].astype(np.float64) * (1 - z / D) + v * z / zplane
        assert (np.abs(x) <= half * (1 + 1e-4)).all()
    v = np.concatenate(vs)
    assert len(v) > 200
    assert inside_polygon(v, verts, a * np.sqrt(2) + 1e-6).all()
    inradius = abs(scale) * R * np.cos(np.pi / 6)
    assert (np.hypot(v[:, 0], v[:, 1]) > inradius + a * np.sqrt(2)).any()
