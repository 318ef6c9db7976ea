"""Scattering media (include/gpuspectral_pt.h, "Scattering media") on the CPU: the device functions of pt_medium.h against float64
restatements; the bits a context keeps when nothing scatters; the furnace, on the product's stage headers compiled for the host
(tests/emu/scatter_emu.cpp); the validation of gsp_set_media_scattering and the layout of its struct."""
import ctypes as C
import math

import numpy as np
import pytest

import media_util as mu
import scatter_util as su

EPS = su.EPS
W = H = 48
SPP = 4


@pytest.fixture(scope="module")
def emu():
    return su.ScatterEmu()


# ---- 1: the device functions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", su.HG_GS)
def test_sample_hg_is_unit_length_has_mean_cosine_g_and_its_pdf_integrates_to_one(emu, g):
    """1e5 stratified (u1, u2).  The mean cosine and the integral of the pdf are estimated from the samples: the tolerance is 5 times
    the stratified estimator's own standard error, computed here from the spread inside the strata of u1 (cos and the pdf depend
    on u1 alone), plus 32 half-ulps for the float32 values that are averaged.
    Unit length: the frame of make_frame is orthonormal to a few roundings and (sin, cos) of theta and phi are each a rounding or
    two from unit: 16 half-ulps bound the norm's error, and the error of the cosine read back off the direction.
    Against float64: the operation-by-operation bounds of scatter_util.hg_cos_bound / hg_pdf_bound."""
    d, gg, u1, u2 = su.hg_vectors(g)
    dirs, pdf = emu.sample_hg(d, gg, u1, u2)
    n1, n2 = su.HG_GRID
    dirs64 = dirs.astype(np.float64)
    assert np.abs(np.linalg.norm(dirs64, axis=1) - 1.0).max() <= 16 * EPS
    cos = (dirs64 * d.astype(np.float64)).sum(1)
    want_cos = su.hg_cos_ref(gg, u1)
    bound = su.hg_cos_bound(gg, u1) + 16 * EPS
    print("g %g: largest |cos - float64| = %.3g, %.2f of its bound" % (g, np.abs(cos - want_cos).max(), (np.abs(cos - want_cos) / bound).max()))
    assert (np.abs(cos - want_cos) <= bound).all()
    # mean cosine = g: stratified estimator, its standard error from the within-stratum spread
    per = cos.reshape(n1, n2)
    se = math.sqrt((per.var(axis=1, ddof=1) / n2).sum()) / n1
    print("g %g: mean cosine %.6f, standard error %.2e" % (g, cos.mean(), se))
    g_eff = 0.0 if abs(g) < 1e-3 else float(np.float32(g))
    assert abs(cos.mean() - g_eff) <= 5 * se + 32 * EPS
    # the pdf the function reports is hg_pdf of the sampled cosine, and equals the float64 formula
    c32 = su.hg_cos_ref(gg, u1).astype(np.float32)
    again = emu.hg_pdf(gg, c32)
    ref = su.hg_pdf_ref(gg, c32)
    tol = su.hg_pdf_bound(gg, c32)
    print("g %g: largest |pdf / float64 - 1| = %.3g, %.2f of its bound" % (g, np.abs(again / ref - 1.0).max(), (np.abs(again / ref - 1.0) / tol).max()))
    assert (np.abs(again / ref - 1.0) <= tol).all()
    assert su.same(emu.hg_pdf(gg, su.hg_cos_ref(gg, u1).astype(np.float32) * 0 + np.float32(0.25)), emu.hg_pdf(gg, np.full(len(gg), 0.25, np.float32)))
    # the pdf integrates to 1 over the sphere: int pdf dw = E_uniform[4 pi pdf], uniform directions by stratified cos in [-1, 1]
    cu = (1.0 - 2.0 * u1.astype(np.float64)).astype(np.float32)
    f = 4.0 * math.pi * emu.hg_pdf(gg, cu).astype(np.float64)
    per = f.reshape(n1, n2)
    se = math.sqrt((per.var(axis=1, ddof=1) / n2).sum()) / n1
    print("g %g: integral of the pdf %.6f, standard error %.2e" % (g, f.mean(), se))
    assert abs(f.mean() - 1.0) <= 5 * se + 32 * EPS
    # ... and the pdf at the samples is the density of the samples: E_hg[1 / (4 pi pdf)] = 1
    h = 1.0 / (4.0 * math.pi * pdf.astype(np.float64))
    per = h.reshape(n1, n2)
    se = math.sqrt((per.var(axis=1, ddof=1) / n2).sum()) / n1
    assert abs(h.mean() - 1.0) <= 5 * se + 32 * EPS


def test_hg_below_the_threshold_is_the_isotropic_form(emu):
    d, _, u1, u2 = su.hg_vectors(0.0)
    a = emu.sample_hg(d, np.zeros(len(u1), np.float32), u1, u2)
    b = emu.sample_hg(d, np.full(len(u1), 1e-4, np.float32), u1, u2)
    assert su.same(a[0], b[0]) and su.same(a[1], b[1])
    assert (a[1] == np.float32(1.0) / (np.float32(4.0) * np.float32(math.pi))).all()


def test_free_path_decision_and_weights_equal_the_float64_restatement(emu):
    """The decision (which event) must agree wherever float64 is not within rounding of the boundary s = t; the weight then agrees to
        |w - w64| <= (12 + 5 x_c + sum_j term_j (5 x_j + 4) / sum_j term_j) half-ulps of w64   + one float32 denormal step,
    x_c = sigma_t_c * distance.  Count: s carries the log's error (2 half-ulps: det_logf is good to ~1 ulp), the division (1) and the
    product sigma_t * s (1), the exponential's own argument reduction (1): 5 half-ulps of the EXPONENT x, which exp turns into 5 x
    half-ulps of Tr; Tr itself 2 more (det_expf ~1 ulp), each summand of p one more product and the sum and / 3 three more -- p's
    error is the term-weighted mean of (5 x_j + 4), bounded through the float64 terms; the numerator (weight * sigma_s) * Tr two
    products and the final division one: 12 covers the fixed part (2 + 2 + 3 + 3 + 2 spare)."""
    v = su.event_vectors()
    out = emu.medium_event(*v)
    scatter, valid, s, w, x, terms = su.medium_event_ref(*v)
    t64 = v[2].astype(np.float64)
    near = np.abs(s - t64) <= 8 * EPS * np.maximum(np.abs(t64), 1e-30)  # the boundary itself: either side is right
    assert ((out[:, 0] != 0) == scatter)[~near].all()
    assert near.mean() < 0.01
    assert ((out[:, 1] != 0) == valid).all()
    ok = ~near & valid
    # s where there is a medium event
    m = ok & scatter
    assert (np.abs(out[m, 2] - s[m]) <= 4 * EPS * s[m] + 1e-45).all()
    with np.errstate(all="ignore"):
        pterm = (terms * (5.0 * x + 4.0)).sum(1) / terms.sum(1)
    tol = (12.0 + 5.0 * x + pterm[:, None]) * EPS * np.abs(w)
    err = np.abs(out[:, 3:].astype(np.float64) - w)
    # a channel whose exponent x is beyond 60 has a transmittance under 1e-26: towards x = 87.34 det_expf's result goes denormal and
    # beyond it is 0 by definition (pt_math.h) where float64 still holds a number.  Those channels are held to: exactly 0 beyond
    # the cut, never above the float64 value by more than the bound, never negative or non-finite
    big = x <= 60.0
    sel = ok[:, None] & big
    print("free-path weights: largest error %.2f of the bound, %.1f half-ulps; %d vectors, %d medium events, %d with an underflowed channel"
          % ((err[sel] / np.maximum(tol[sel], 1e-300)).max(), (err[sel] / np.maximum(EPS * np.abs(w[sel]), 1e-300)).max(), ok.sum(), m.sum(),
             (ok[:, None] & ~big).any(1).sum()))
    assert (err[sel] <= tol[sel]).all()
    tail = ok[:, None] & ~big
    got = out[:, 3:].astype(np.float64)
    assert np.isfinite(got[tail]).all() and (got[tail] >= 0).all() and (got[tail] <= w[tail] + tol[tail] + 1e-30).all()
    assert (got[ok[:, None] & (x > 87.4)] == 0).all() and (ok[:, None] & (x > 87.4)).any()
    # the cases the vectors were built for are all there
    st = v[0] + v[1]
    assert ((st == 0).all(1) & ok).any() and ((st == 0).any(1) & ~(st == 0).all(1) & ok).any() and ((v[2] == 0) & ok).any()
    assert (ok[:, None] & ~big).any() and m.any() and (ok & ~scatter).any()
    # sigma_t = 0 everywhere: the surface, weight untouched; t = 0: the surface, weight within 5 half-ulps (Tr = 1, p = 1)
    z = (st == 0).all(1)
    assert (out[z, 0] == 0).all() and su.same(out[z, 3:], v[5][z])
    z = v[2] == 0
    assert (out[z, 0] == 0).all() and su.same(out[z, 3:], v[5][z])


# ---- 2: bits kept --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tinted(materials_scene):
    return mu.with_medium(materials_scene, mu.glass_instances(materials_scene), 1)


def test_all_zero_scattering_table_keeps_every_bit_and_ray(emu, tinted):
    for sc, media, n in ((tinted, [su.SIGMA_A], W), (mu.slab_scene(1), [mu.SLAB_SIGMA], 32)):
        s = emu.scene(sc)
        ref, rst = s.render(n, n, SPP, media=media)
        img, st = s.render(n, n, SPP, media=media, scatter=[((0.0, 0.0, 0.0), 0.5)])
        assert su.same(img, ref) and st == rst
        # ... and both are the frame of the media emulation (the code of the parent)
        old, ost = mu.MediaEmu().scene(sc).render(n, n, SPP, media=media)
        assert su.same(ref, old) and all(rst[k] == ost[k] for k in ost)


def test_mixed_context_keeps_the_pixels_that_met_no_scatterer(emu, materials_scene):
    """Medium 1 absorbs, medium 2 scatters.  A pixel whose paths met no back face of the scatterer (the emulation's log) has the bits
    of the context without a scattering table: the absorber takes the deterministic line and draws nothing."""
    sc, _, _ = su.two_glass_scene(materials_scene)
    media = [su.SIGMA_A, (0.5, 0.25, 0.125)]
    s = emu.scene(sc)
    ref, _ = s.render(W, H, SPP, media=media)
    img, st, back, events = s.render(W, H, SPP, media=media, scatter=[((0.0, 0.0, 0.0), 0.0), (su.SIGMA_S, su.G)], log=True)
    met = (back & 2) != 0
    assert 0.02 < met.mean() < 0.9 and ((back & 1) != 0).mean() > met.mean()  # (some pixels met the absorber alone)
    assert su.same(img[~met], ref[~met])
    assert not su.same(img[met], ref[met]) and st["medium_events"] > 0 and (events[~met] == 0).all()
    assert np.isfinite(img).all()


# ---- 3: the furnace ------------------------------------------------------------------------------------------------------------------
def furnace(emu, n, spp, sigma_a, sigma_s, g=0.0, ts0=0, pixel_ids=None, **over):
    params = dict(su.FURNACE_PARAMS, **over)
    return emu.scene(su.furnace_scene()).render(n, n, spp, media=[sigma_a], scatter=[(sigma_s, g)], first_timestamp=ts0, log=True, pixel_ids=pixel_ids,
                                                **params)


@pytest.mark.parametrize("rr", ["off", "on"])
def test_furnace_grey_albedo_one_is_L_everywhere(emu, rr):
    img, st, back, events = furnace(emu, 32, 2, (0, 0, 0), (2.0, 2.0, 2.0), **({} if rr == "off" else dict(rr_start_depth=3)))
    assert events.max() <= su.FURNACE_MAX_EVENTS and st["medium_events"] > 300
    su.check_furnace_white(img, spp=2, rr=rr == "on")


def test_furnace_grey_half_albedo_samples_are_powers_and_follow_the_free_path_law(emu):
    n = 32
    frames = [furnace(emu, n, 1, (1.0, 1.0, 1.0), (1.0, 1.0, 1.0), ts0=ts) for ts in range(16)]
    k = su.check_furnace_half([f[0] for f in frames], n, sigma_a=1.0, sigma_t=2.0, albedo=0.5, timestamps=range(16))
    # the image's k is the emulation's event count, sample by sample
    _, inside, outside = mu.slab_reference(n, n)
    for f, kk in zip(frames, k):
        assert (f[3][:, 0][inside | outside] == kk[inside | outside]).all()


def test_furnace_chromatic_albedo_one_has_mean_L(emu):
    """sigma_s = (1, 2, 4), albedo 1: the single-channel free path with the three-channel average density is unbiased, so the mean
    over the inside pixels is L within 5 standard errors -- the error estimated from those pixels' own spread, and required to be
    under 1 % of L so that the check has teeth."""
    n, spp = 64, 64
    _, inside, _ = mu.slab_reference(n, n)
    img = furnace(emu, n, spp, (0, 0, 0), (1.0, 2.0, 4.0), pixel_ids=np.flatnonzero(inside))[0]
    px = img[:, :3].astype(np.float64)
    mean, se = px.mean(0), px.std(0, ddof=1) / math.sqrt(len(px))
    print("chromatic furnace: mean", mean, "standard error", se, "over", len(px), "pixels at", spp, "spp")
    assert (se < 0.01 * su.FURNACE_L).all()
    assert (np.abs(mean - su.FURNACE_L) <= 5 * se).all()


@pytest.mark.parametrize("albedo,g", [(0.25, 0.0), (0.9, 0.6), (1.0, -0.5)])
def test_furnace_no_channel_exceeds_L(emu, albedo, g):
    st = 3.0
    img, _, _, events = furnace(emu, 32, 4, (st * (1 - albedo),) * 3, (st * albedo,) * 3, g=g)
    su.check_furnace_bounded(img, events.max())


# ---- 4: validation, layout -----------------------------------------------------------------------------------------------------------
def test_validation(emu):
    ok = [(su.SIGMA_S, su.G)]
    assert emu.check(ok, 1) is None and emu.check(None, 3) is None and emu.check(ok, 1, count=0) is None
    assert emu.check([((0, 0, 0), -0.999)], 1) is None and emu.check([((0, 0, 0), 0.0)] * 2, 2) is None
    for bad in ((-1.0, 0, 0), (0, float("nan"), 0), (0, 0, float("inf"))):
        assert "finite and >= 0" in emu.check([(bad, 0.0)], 1)
    for g in (1.0, -1.0, 1.5, float("nan"), float("inf")):
        assert "|g| < 1" in emu.check([((1, 1, 1), g)], 1)
    for have in (0, 2):
        assert "media count" in emu.check(ok, have)


def test_struct_layout_and_exports():
    import os

    from conftest import ROOT
    from gpuspectral_amd import abi, pt

    assert C.sizeof(abi.MediumScatter) == 16 and abi.MediumScatter.g.offset == 12 and C.sizeof(abi.Medium) == 16
    text = open(os.path.join(ROOT, "include", "gpuspectral_pt.h")).read()
    assert "#define GSP_ABI_VERSION 9 " in text
    for name in ("gsp_set_media_scattering", "gsp_multi_set_media_scattering"):
        assert ("int %s(" % name) in text and name in pt.EXPORTS
    arr = abi.media_scatter_array([(1, 2, 3), ((4, 5, 6), 0.5)])
    assert [tuple(a.sigma_s) + (a.g,) for a in arr] == [(1.0, 2.0, 3.0, 0.0), (4.0, 5.0, 6.0, 0.5)]
    assert abi.media_scatter_array([]) is None and abi.media_scatter_array(None) is None
