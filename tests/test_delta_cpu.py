"""Delta lights (include/gpuspectral_pt.h "Delta lights") on the CPU: the product's shade_vertex<.., DLT = true> compiled for the host
(tests/emu/delta_emu.cpp) against closed forms -- a diffuse plane under one delta light has no Monte-Carlo noise --, the selection
probabilities, the bits a context without delta lights keeps, and the small functions of pt_deltalight.h against float64."""
import copy
import math

import numpy as np
import pytest

import delta_util as du
from gpuspectral_amd import abi, scenes

W, H = du.PLANE_W, du.PLANE_H
POINT_POS, POINT_I = (0.4, -0.3, 1.5), (6.0, 9.0, 12.0)
SUN_DIR, SUN_E = (0.3, -0.2, -0.9327379053088815), (2.0, 3.0, 1.0)  # unit
# a spot close above the plane that looks sideways: both cone boundaries cross the frame as gently curved lines
SPOT_POS, SPOT_DIR = (-0.3, 0.1, 1.2), (0.97590007, 0.09759001, -0.19518001)
SPOT_CUTOFF_DEG, SPOT_BEAM_DEG = 65.0, 45.0
SPOT_W, SPOT_H = 64, 48


@pytest.fixture(scope="module")
def emu():
    return du.DeltaEmu()


@pytest.fixture(scope="module")
def plane(emu):
    sc = du.plane_scene()
    return sc, emu.scene(sc), du.plane_points(sc)


def check_point(img, P, position, intensity, sel=None):
    """every selected pixel is (albedo / pi) I cos / d^2 within closed_form_bound"""
    want = du.point_radiance(P, position, intensity)
    sel = np.ones(len(P), bool) if sel is None else sel
    d = np.linalg.norm(np.asarray(position)[None, :] - P, axis=1)
    bound = du.closed_form_bound(d.min(), abs(position[2]))
    assert bound <= 1e-4
    rel = np.abs(img[sel, :3].astype(np.float64) / want[sel] - 1.0)
    print("point light: largest relative deviation %.3g (bound %.3g) over %d pixels" % (rel.max(), bound, sel.sum()))
    assert rel.max() <= bound
    return bound


def test_point_light_closed_form(plane):
    sc, es, P = plane
    img, st, per = es.render(W, H, 1, delta=[abi.point_light(POINT_POS, POINT_I)], samples=True, **du.PLANE_PARAMS)
    check_point(img, P, POINT_POS, POINT_I)
    assert (img[:, 3] == 1.0).all() and st["shadow_rays"] == W * H
    # the same for every sample: no variate enters the value
    img4, _, per4 = es.render(W, H, 4, delta=[abi.point_light(POINT_POS, POINT_I)], samples=True, **du.PLANE_PARAMS)
    assert all(du.same(per4[:, k, :3], per[:, 0, :3]) for k in range(4))


def test_directional_light_closed_form(plane):
    sc, es, P = plane
    img, st = es.render(W, H, 1, delta=[abi.directional_light(SUN_DIR, SUN_E, 10.0)], **du.PLANE_PARAMS)
    want = du.albedo_over_pi() * np.float64(SUN_E) * abs(SUN_DIR[2])
    # no distance enters: the vertex's operations alone (closed_form_bound's second term) and the float32 statement of the direction (3)
    bound = 43 * du.EPS
    rel = np.abs(img[:, :3].astype(np.float64) / want[None, :] - 1.0)
    print("directional light: largest relative deviation %.3g (bound %.3g)" % (rel.max(), bound))
    assert bound <= 1e-4 and rel.max() <= bound
    assert st["shadow_rays"] == W * H


def spot_parts(P):
    cc, cb = math.cos(math.radians(SPOT_CUTOFF_DEG)), math.cos(math.radians(SPOT_BEAM_DEG))
    light = abi.spot_light(SPOT_POS, SPOT_DIR, POINT_I, cc, cb)
    c = du.spot_cosine(P, SPOT_POS, SPOT_DIR)
    cc32, cb32 = float(np.float32(cc)), float(np.float32(cb))
    return light, c, cc32, cb32


def check_spot(img, P):
    light, c, cc, cb = spot_parts(P)
    inside, outside = c >= cb, c <= cc
    keep = du.away_from(inside, outside, SPOT_W, SPOT_H)
    assert keep.mean() >= 0.8, keep.mean()
    assert (inside & keep).any() and (outside & keep).any() and (~inside & ~outside & keep).any()  # the cone edge crosses the quad
    full = du.point_radiance(P, SPOT_POS, POINT_I)
    bound = check_point(img, P, SPOT_POS, POINT_I, sel=inside & keep)
    assert (img[outside & keep, :3] == 0.0).all()
    # the ramp: s = smoothstep(t).  |ds| <= 1.5 |dt|, dt = dc / (cos_beam - cos_cutoff), dc <= |dP| / d (the shading point) + 8 EPS
    # (dot, negation, the float32 direction), + 6 EPS relative for the subtraction, division, clamp and polynomial
    ramp = ~inside & ~outside & keep
    s, _ = du.smoothstep_ref(c, cc, cb)
    d = np.linalg.norm(np.asarray(SPOT_POS)[None, :] - P, axis=1)
    ds = 1.5 * (32 * 8 * du.EPS / d.min() + 8 * du.EPS) / (cb - cc) + 6 * du.EPS
    assert ds <= 1e-4
    got_s = img[ramp, :3].astype(np.float64) / full[ramp]
    dev = np.abs(got_s - s[ramp, None])
    print("spot: %d ramp pixels, largest |s - smoothstep| %.3g (bound %.3g)" % (ramp.sum(), dev.max(), ds + bound))
    assert dev.max() <= ds + bound


def test_spot_light_closed_form(plane):
    sc, es, _ = plane
    P = du.plane_points(sc, SPOT_W, SPOT_H)
    img, _ = es.render(SPOT_W, SPOT_H, 1, delta=[spot_parts(P)[0]], **du.PLANE_PARAMS)
    check_spot(img, P)


# ---- hard shadows ---------------------------------------------------------------------------------------------------------------------
# 64 x 48 and small occluders: a square of s pixels costs the band of 16 s pixels around its edge, and all bands together may take a
# tenth of the frame.  The point light doubles the occluder (it sits at half the light's height): a shadow of 8 pixels; the
# directional light's two shadows have the occluders' own size, 6 pixels.
SH_W, SH_H = 64, 48
OCC_CENTRE = (0.1, 0.0, 0.75)
FAR = 1e4


def shadow_of(P, centre, half, light_pos=None, light_dir=None):
    """the plane points whose segment towards the light crosses the occluder's plane z = centre.z inside its square"""
    if light_pos is not None:
        toL = np.asarray(light_pos, np.float64)[None, :] - P
    else:
        toL = np.tile(-np.asarray(light_dir, np.float64), (len(P), 1))
    t = centre[2] / toL[:, 2]
    q = P + toL * t[:, None]
    return (np.abs(q[:, 0] - centre[0]) < half) & (np.abs(q[:, 1] - centre[1]) < half)


def sees_occluder(P, centre, half):
    """pixels whose camera ray meets the occluder itself (black, and unlit from below) before the plane"""
    eye = np.asarray(du.PLANE_EYE)
    t = (centre[2] - eye[2]) / (P[:, 2] - eye[2])
    q = eye[None, :] + (P - eye[None, :]) * t[:, None]
    return (np.abs(q[:, 0] - centre[0]) < half) & (np.abs(q[:, 1] - centre[1]) < half)


def check_shadow(img, umbras, seen, want_lit, bound):
    """umbras: one mask per occluder.  Pixels in an umbra are exactly 0, pixels outside keep the closed form; left out: pixels within
    two pixels of a projected edge or of the occluder's own silhouette, and at least 90 % of the plane's pixels remain."""
    umbra = np.zeros(len(seen), bool)
    for u in umbras:
        umbra |= u
    keep = du.away_from(umbra, seen, SH_W, SH_H) & ~seen
    share = keep.sum() / (~seen).sum()
    print("hard shadow: %.1f %% of the plane's pixels kept, %s umbra pixels" % (100 * share, [int((u & keep).sum()) for u in umbras]))
    assert share >= 0.9
    assert all((u & keep).sum() >= 4 for u in umbras)
    assert (img[umbra & keep, :3] == 0.0).all()
    lit = ~umbra & keep
    assert (img[lit, :3] > 0.0).all()
    rel = np.abs(img[lit, :3].astype(np.float64) / want_lit[lit] - 1.0)
    assert rel.max() <= bound, rel.max()


def point_shadow_case():
    half = 0.09
    sc = du.plane_scene(occluder=(OCC_CENTRE, half))
    P = du.plane_points(sc, SH_W, SH_H)
    d = np.linalg.norm(np.asarray(POINT_POS)[None, :] - P, axis=1)
    return sc, [abi.point_light(POINT_POS, POINT_I)], dict(umbras=[shadow_of(P, OCC_CENTRE, half, light_pos=POINT_POS)], seen=sees_occluder(P, OCC_CENTRE, half),
                                                          want_lit=du.point_radiance(P, POINT_POS, POINT_I), bound=du.closed_form_bound(d.min(), POINT_POS[2]))


def sun_shadow_case():
    """... and a second square FAR units up the light direction from the plane point (-0.9, 0.6, 0): it shades a square of its own size
    around that point.  FAR units of a float32 direction move the shadow by up to 3 * FAR * 2^-24 = 2e-3 units, a twentieth of a pixel."""
    half = 0.135
    far_c = tuple(np.float64([-0.9, 0.6, 0.0]) - FAR * np.float64(SUN_DIR))
    near_c = (-0.5, -0.4, 0.75)  # (its shadow falls beside its own silhouette)
    sc = du.plane_scene(occluder=(near_c, half), far_occluder=(far_c, half))
    P = du.plane_points(sc, SH_W, SH_H)
    want = np.tile(du.albedo_over_pi() * np.float64(SUN_E) * abs(SUN_DIR[2]), (len(P), 1))
    return sc, [abi.directional_light(SUN_DIR, SUN_E, 10.0)], dict(
        umbras=[shadow_of(P, near_c, half, light_dir=SUN_DIR), shadow_of(P, far_c, half, light_dir=SUN_DIR)], seen=sees_occluder(P, near_c, half),
        want_lit=want, bound=43 * du.EPS)


@pytest.mark.parametrize("case", [point_shadow_case, sun_shadow_case])
def test_hard_shadows(emu, case):
    sc, lights, expect = case()
    img, _ = emu.scene(sc).render(SH_W, SH_H, 1, delta=lights, **du.PLANE_PARAMS)
    check_shadow(img, **expect)


# ---- selection --------------------------------------------------------------------------------------------------------------------------
def test_two_point_lights_uniform_pick(plane):
    sc, es, P = plane
    p2, i2 = (-0.8, 0.5, 1.0), (3.0, 2.0, 1.0)
    lights = [abi.point_light(POINT_POS, POINT_I), abi.point_light(p2, i2)]
    c1, c2 = du.point_radiance(P, POINT_POS, POINT_I), du.point_radiance(P, p2, i2)
    d = min(np.linalg.norm(np.asarray(q)[None, :] - P, axis=1).min() for q in (POINT_POS, p2))
    bound = du.closed_form_bound(d, 1.0) + 2 * du.EPS  # (+ pmf = 0.5f and the running mean's weight)
    assert bound <= 1e-4
    n = 256
    total = np.zeros((W * H, 3))
    picked1 = 0
    for ts in range(n):
        img, _, per = es.render(W, H, 1, delta=lights, first_timestamp=ts, samples=True, **du.PLANE_PARAMS)
        s = per[:, 0, :3].astype(np.float64)
        is1 = np.abs(s / (2 * c1) - 1.0).max(1) <= bound
        is2 = np.abs(s / (2 * c2) - 1.0).max(1) <= bound
        assert (is1 | is2).all()
        picked1 += int(is1.sum())
        total += s
    mean = total / n
    # a two-point distribution per pixel: variance (c1 - c2)^2 per channel at p = 1 / 2
    se = np.abs(c1 - c2) / math.sqrt(n)
    assert (np.abs(mean - (c1 + c2)) <= 5 * se + bound * (c1 + c2)).all()
    assert abs(picked1 / (n * W * H) - 0.5) < 5 * 0.5 / math.sqrt(n * W * H)


def test_power_pick_table_against_float64_weights(emu):
    sc = scenes.cornell_materials(8)
    cc, cb = math.cos(math.radians(30.0)), math.cos(math.radians(10.0))
    lights = [abi.point_light((0, 1, 0), (1, 2, 3)), abi.spot_light((0, 1.5, 0), (0, -1, 0), (40, 30, 20), cc, cb),
              abi.directional_light((0, -1, 0), (0.5, 0.5, 0.5), 3.0), abi.point_light((0, 1, 0), (0, 0, 0))]
    err, accepted = emu.check(lights)
    assert err is None
    table, inv_sum = emu.light_pick(sc.lights, accepted)
    n = len(sc.lights) + len(lights)
    assert len(table) == n
    w = np.concatenate([du.triangle_weight_ref(sc.lights), [du.pick_weight_ref(l) for l in accepted]])
    assert w[-1] == 0.0 and (w[:-1] > 0).all()
    p = du.pick_pmf(table)
    aliased = np.bincount(table["alias"][table["alias"] != np.arange(n)], minlength=n)
    # the header's bound for the alias table ("Light selection"): |p_i - w_i / sum(w)| <= (1 + d_i) / (n 2^32)
    assert (np.abs(p - w / w.sum()) <= (1 + aliased) / (n * 2.0 ** 32) + 1e-15).all()
    assert abs(float(inv_sum) * w.sum() - 1.0) <= 2 * du.EPS
    assert np.array_equal(table["pmf_self"], p.astype(np.float32))
    # ... and the frame under it: one point light and a dark one, power pick: the bright one is always picked, pmf 1
    plane_sc = du.plane_scene()
    img, _ = emu.scene(plane_sc).render(W, H, 1, delta=[abi.point_light(POINT_POS, POINT_I), abi.point_light((0, 0, 1), (0, 0, 0))], light_mode=du.POWER,
                                        **du.PLANE_PARAMS)
    check_point(img, du.plane_points(plane_sc), POINT_POS, POINT_I)


# ---- the selection probability of an emitter that is hit ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [du.UNIFORM, du.POWER])
def test_a_dark_delta_light_keeps_the_expected_image_under_the_textbook_estimator(emu, mode):
    """Cornell box with its area light, textbook estimator.  One delta light of intensity 0 changes every selection probability (uniform:
    1 / 2 -> 1 / 3 per triangle; power: unchanged weights, a longer table) but not the expected image: its own term is 0, and an emitter
    that is hit is weighted with the p_sel of the longer table.  A p_sel that forgot the delta record would weigh emitter hits against a
    light pdf 3 / 2 too large under the uniform pick and darken the frame."""
    sc = scenes.cornell_materials(8, full=False)
    es = emu.scene(sc)
    w, h, spp = 24, 18, 192
    dark = [abi.point_light((0.0, 1.0, 0.0), (0.0, 0.0, 0.0))]
    frames = []
    for delta in (None, dark):
        _, _, per = es.render(w, h, spp, delta=delta, estimator=du.TEXTBOOK, light_mode=mode, samples=True)
        frames.append(per[:, :, :3].astype(np.float64).mean(2))  # [pixel, sample]: the mean over the channels
    means = [f.mean() for f in frames]
    ses = [f.mean(0).std(ddof=1) / math.sqrt(spp) for f in frames]  # the frame mean of sample k, over k
    print("mode %d: frame mean %.5f +- %.5f without, %.5f +- %.5f with the dark light" % (mode, means[0], ses[0], means[1], ses[1]))
    assert ses[0] < 0.01 * means[0] and ses[1] < 0.01 * means[1]
    assert abs(means[0] - means[1]) <= 5 * math.hypot(ses[0], ses[1])
    if mode == du.UNIFORM:
        assert not du.same(frames[0].astype(np.float32), frames[1].astype(np.float32))


# ---- bits kept ----------------------------------------------------------------------------------------------------------------------------
def test_no_delta_lights_is_the_emulation_without_them(emu):
    sc = scenes.cornell_materials(8)
    es = emu.scene(sc)
    import scatter_util as su

    ref, st_ref = su.ScatterEmu().scene(sc).render(24, 18, 2)
    img, st = es.render(24, 18, 2, delta=[])
    assert du.same(img, ref) and st["shadow_rays"] == st_ref["shadow_rays"]


def test_triangle_picks_in_a_mixed_table_keep_their_bits(emu):
    """Textbook estimator, uniform pick: a table of the scene's 2 triangle lights + 2 delta lights of intensity 0 against a table of 4
    TRIANGLE lights whose last two are black: the same pick, the same pmf 1 / 4, and a black light adds nothing either way (under the
    textbook estimator the path's lastPdf does not depend on the shadow ray) -- so the frames agree bit for bit exactly when the <DLT>
    vertex forms a triangle sample with the operations of the vertex without delta lights."""
    sc = scenes.cornell_materials(8)
    assert len(sc.lights) == 2
    black = copy.copy(sc)
    extra = sc.lights.copy()
    extra["positions"][:, :, :3] += np.float32(50.0)
    extra["radiance"][:, :3] = 0.0
    black.lights = np.concatenate([sc.lights, extra])
    ref, _ = emu.scene(black).render(24, 18, 4, estimator=du.TEXTBOOK)
    dark = [abi.point_light((0.0, 1.0, 0.0), (0.0, 0.0, 0.0)), abi.directional_light((0.0, -1.0, 0.0), (0.0, 0.0, 0.0), 1.0)]
    img, _ = emu.scene(sc).render(24, 18, 4, delta=dark, estimator=du.TEXTBOOK)
    assert du.same(img, ref)
    assert not du.same(img, emu.scene(sc).render(24, 18, 4, estimator=du.TEXTBOOK)[0])  # (the table's length matters: 1 / 4 against 1 / 2)


def mixed_lights():
    cc, cb = math.cos(math.radians(40.0)), math.cos(math.radians(25.0))
    return [abi.point_light((0.3, 1.2, 0.4), (1.5, 1.2, 0.9)), abi.spot_light((-0.5, 1.8, 0.5), (0.2, -0.9591663046625439, -0.2), (6.0, 6.0, 8.0), cc, cb),
            abi.directional_light((-0.4, -0.8, -0.4472135954999579), (0.4, 0.35, 0.3), 2.5)]


@pytest.mark.parametrize("mode", [du.UNIFORM, du.POWER])
@pytest.mark.parametrize("est", [du.REFERENCE, du.TEXTBOOK])
def test_the_scattering_kernel_is_the_narrow_one_for_every_media_class(emu, mode, est):
    """The library builds <DLT> for MED = SCT = true only.  A context without media, and one whose media only absorb, get from it the bits
    of the <DLT> instantiation of their own class (which only this emulation compiles)."""
    import scatter_util as su

    sc = scenes.cornell_materials(8)
    es = emu.scene(sc)
    a, _ = es.render(24, 18, 2, delta=mixed_lights(), estimator=est, light_mode=mode)
    b, _ = es.render(24, 18, 2, delta=mixed_lights(), estimator=est, light_mode=mode, narrow=True)
    assert du.same(a, b) and np.isfinite(a).all() and (a >= 0).all()
    glass = su.mu.glass_instances(sc)
    med = su.mu.with_medium(sc, [int(glass[0])], 1)
    ems = emu.scene(med)
    a, _ = ems.render(24, 18, 2, delta=mixed_lights(), media=[su.SIGMA_A], estimator=est, light_mode=mode)
    b, _ = ems.render(24, 18, 2, delta=mixed_lights(), media=[su.SIGMA_A], estimator=est, light_mode=mode, narrow=True)
    c, _ = ems.render(24, 18, 2, delta=mixed_lights(), media=[su.SIGMA_A], scatter=[((0.0, 0.0, 0.0), 0.3)], estimator=est, light_mode=mode)
    assert du.same(a, b) and du.same(a, c)
    assert not du.same(a, es.render(24, 18, 2, delta=mixed_lights(), estimator=est, light_mode=mode)[0])  # (the medium absorbs)


def test_disable_nee_leaves_delta_lights_dark(plane):
    sc, es, P = plane
    img, st = es.render(W, H, 1, delta=[abi.point_light(POINT_POS, POINT_I)], disable_nee=1, **du.PLANE_PARAMS)
    assert (img[:, :3] == 0.0).all() and st["shadow_rays"] == 0


# ---- the small functions ----------------------------------------------------------------------------------------------------------------
def test_spot_falloff_against_float64(emu):
    c, cc, cb = du.falloff_vectors()
    got = emu.spot_falloff(c, cc, cb).astype(np.float64)
    want, t = du.smoothstep_ref(c, cc, cb)
    # t: two subtractions whose results carry EPS each relative to their OPERANDS' difference (exact inputs: Sterbenz or one rounding), the
    # division: dt <= 3 EPS t; the polynomial: 4 more on values <= 3
    assert (np.abs(got - want) <= 1.5 * 3 * du.EPS * t + 8 * du.EPS).all()
    assert (got[c <= cc] == 0.0).all() and (got[c >= cb] == 1.0).all()
    assert ((got > 0) & (got < 1)).sum() > 1000


def test_sample_delta_light_against_float64(emu):
    rec, pos, pmf = du.sample_vectors()
    out = emu.sample_delta_light(rec, pos, pmf)
    kind = rec[:, 3].view(np.uint32)
    L, Ldist, emission, pdf = out[:, 0:3].astype(np.float64), out[:, 3].astype(np.float64), out[:, 4:7].astype(np.float64), out[:, 7].astype(np.float64)
    inten, direction = rec[:, 8:11].astype(np.float64), rec[:, 4:7].astype(np.float64)
    sun = kind == abi.LIGHT_DIRECTIONAL
    assert du.same(out[sun, 0:3], -rec[sun, 4:7]) and (out[sun, 3] == np.float32(1e30)).all() and du.same(out[sun, 7], pmf[sun]) and du.same(out[sun, 4:7], rec[sun, 8:11])
    toL = rec[:, 0:3].astype(np.float64) - pos.astype(np.float64)
    d2 = (toL * toL).sum(1)
    zero = ~sun & (pdf == 0.0)
    assert (d2[zero] < 2.0 ** -126).all() and (Ldist[zero] == 0.0).all() and zero.sum() >= len(pmf) // 20  # pos == position, or d2 underflowed
    ok = ~sun & ~zero & np.isfinite(out[:, 7]) & (d2 > 1e-30) & (d2 < 1e30)
    assert ok.sum() > 5000
    assert (np.abs(pdf[ok] / (d2[ok] * pmf[ok].astype(np.float64)) - 1.0) <= 7 * du.EPS).all()
    assert (np.abs(Ldist[ok] / np.sqrt(d2[ok]) - 1.0) <= 5 * du.EPS).all()
    assert (np.abs(L[ok] - toL[ok] / np.sqrt(d2[ok])[:, None]) <= 6 * du.EPS).all()
    pt = ok & (kind == abi.LIGHT_POINT)
    assert du.same(out[pt, 4:7], rec[pt, 8:11])
    sp = ok & (kind == abi.LIGHT_SPOT)
    c = -((toL[sp] / np.sqrt(d2[sp])[:, None]) * direction[sp]).sum(1)
    s, t = du.smoothstep_ref(c, rec[sp, 7], rec[sp, 11])
    width = (rec[sp, 11] - rec[sp, 7]).astype(np.float64)
    ds = 1.5 * (12 * du.EPS / width) + 8 * du.EPS  # c carries L's error (6 EPS per component) and its own dot product
    assert (np.abs(emission[sp] - inten[sp] * s[:, None]) <= (ds[:, None] + 2 * du.EPS) * inten[sp] + 1e-30).all()
    huge = ~sun & ~np.isfinite(out[:, 7])
    assert huge.sum() > 100 and (d2[huge] > 3e38).all()  # d2 beyond float32: pdf = +inf, the NEE term 0


def test_validation_leaves_nothing_accepted(emu):
    good = abi.point_light((0, 1, 0), (1, 1, 1))
    assert emu.check([good])[0] is None
    cc, cb = 0.8, 0.9
    bad = []
    l = abi.point_light((0, 1, 0), (1, 1, 1)); l.kind = 0; bad.append(l)
    l = abi.point_light((0, 1, 0), (1, 1, 1)); l.kind = 4; bad.append(l)
    bad.append(abi.point_light((0, float("nan"), 0), (1, 1, 1)))
    bad.append(abi.point_light((0, 1, 0), (1, float("inf"), 1)))
    bad.append(abi.point_light((0, 1, 0), (1, -1e-6, 1)))
    bad.append(abi.spot_light((0, 1, 0), (0, -1.002, 0), (1, 1, 1), cc, cb))
    bad.append(abi.spot_light((0, 1, 0), (0, 0, 0), (1, 1, 1), cc, cb))
    bad.append(abi.spot_light((0, 1, 0), (0, -1, 0), (1, 1, 1), cb, cb))
    bad.append(abi.spot_light((0, 1, 0), (0, -1, 0), (1, 1, 1), cb, cc))
    bad.append(abi.directional_light((0, -1, 0), (1, 1, 1), 0.0))
    bad.append(abi.directional_light((0, -1, 0), (1, 1, 1), -1.0))
    bad.append(abi.directional_light((0.6, -0.6, 0.6), (1, 1, 1), 1.0))
    l = abi.point_light((0, 1, 0), (1, 1, 1)); l.reserved[1] = 1.0; bad.append(l)
    l = abi.point_light((0, 1, 0), (1, 1, 1)); l.extent = float("nan"); bad.append(l)
    for k, l in enumerate(bad):
        err, acc = emu.check([good, l])
        assert err is not None and acc is None, k
    # accepted: a direction within 1e-3 of unit is renormalised in double
    err, acc = emu.check([abi.spot_light((0, 1, 0), (0.0, -1.0009, 0.0), (1, 1, 1), cc, cb), abi.directional_light((0.6004, 0.0, -0.8), (1, 1, 1), 2.0)])
    assert err is None
    assert list(acc[0].direction) == [0.0, -1.0, 0.0]
    want = np.float64([np.float32(0.6004), 0.0, np.float32(-0.8)])
    want = (want / np.linalg.norm(want)).astype(np.float32)
    assert np.array_equal(np.float32(list(acc[1].direction)), want)
