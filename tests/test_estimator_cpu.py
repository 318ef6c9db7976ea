"""The textbook estimator (include/gpuspectral_pt.h "Estimator") without a GPU: the product's shade_vertex<.., EST> and path loop
compiled for the host (tests/emu/estimator_emu.cpp) against the CPU oracle under its test-only mask oracle_set_quirks_off(1 | 2 | 8),
bit for bit; the occluded-shadow-ray paths that make that equality say something about the commit; mode 0 and disable_nee; the
frame means of textbook + uniform, textbook + power and plain path tracing where the reference's two light selection modes
disagree; and p_sel against the pmf of the integer alias table."""
import math

import numpy as np
import pytest

import estimator_util as eu
import lights_util as lu


@pytest.fixture(scope="module")
def emu():
    return eu.EstimatorEmu()


@pytest.fixture(scope="module")
def textbook_frames(emu):
    """The emulation's textbook frames of eu.FRAMES (uniform pick), rendered once."""
    out = {}
    for name, (w, h, spp) in eu.FRAMES.items():
        img, st = emu.scene(eu.frame_scene(name)).render(w, h, spp, estimator=eu.TEXTBOOK)
        img.setflags(write=False)
        out[name] = (img, st)
    return out


@pytest.mark.parametrize("name", sorted(eu.FRAMES))
def test_emulation_equals_the_oracle_with_the_three_quirks_off(textbook_frames, name):
    """shade_vertex<.., EST = true> is oracle_pt.cpp:499, :509-516, :540 and oracle_bsdf.h:447-450, operation for operation: image and
    ray counts.  `materials` has rough plastic (the floor of the eval pdf) and glass / mirror paths (wasDelta)."""
    try:
        want, wst = eu.oracle_frame(name)
    finally:
        assert eu.oracle_quirks_off() == 0  # the mask is process state: never left set
    got, gst = textbook_frames[name]
    bad = int((got.view(np.uint32) != want.view(np.uint32)).any(axis=1).sum())
    assert bad == 0, (name, bad)
    assert eu.counts_of(gst) == eu.counts_of(wst)
    if name == "materials":
        assert gst["emitter_hits_after_delta"] > 0  # wasDelta is exercised


def test_the_mask_is_zero_after_a_failure_inside_the_block():
    with pytest.raises(RuntimeError):
        with eu.oracle_textbook():
            assert eu.oracle_quirks_off() == eu.ORACLE_TEXTBOOK_MASK == 11
            raise RuntimeError("inside")
    assert eu.oracle_quirks_off() == 0


def test_cornell_frame_has_paths_that_hit_the_light_behind_an_occluded_shadow_ray(textbook_frames):
    """Without a path whose shadow ray was occluded at vertex k and that hit an emitter at vertex k + 1 (NEE on, countEmitted == 0,
    wasDelta == 0), the bit-equality above says nothing about the commit of an occluded ray: the reference's commit writes 1 over
    the field that carries lastPdf in textbook mode."""
    _, st = textbook_frames["cornell"]
    assert st["emitter_hits_after_occluded"] >= 1, st
    assert st["emitter_hits_after_clear"] >= 1, st


def test_textbook_differs_from_the_reference_and_mode_0_is_the_reference(emu, textbook_frames):
    """Mode 0 rendered after mode 1 is the frame of the emulation that never heard of the mode (pt_emu.cpp emu_render =
    shade_vertex<TEX> with its defaults) and of the unmasked oracle, bit for bit."""
    from oracle import oracle as orc

    import ctypes as C

    w, h, spp = eu.FRAMES["materials"]
    sc = eu.frame_scene("materials")
    s = emu.scene(sc)
    tb, _ = textbook_frames["materials"]
    ref, rst = s.render(w, h, spp, estimator=eu.REFERENCE)
    assert not eu.same(ref, tb)
    p = emu.abi.default_render_params(spp, 0)
    plain = np.zeros((w * h, 4), np.float32)
    emu.L.emu_render.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(emu.abi.RenderParams), C.c_void_p]
    assert emu.L.emu_render(s.h, w, h, None, w * h, C.byref(p), plain.ctypes.data) == 0
    assert eu.same(ref, plain)
    o = orc.Oracle(sc)
    want, wst = o.render(w, h, spp=spp)
    o.close()
    assert eu.same(ref, want) and eu.counts_of(rst) == eu.counts_of(wst)


@pytest.mark.parametrize("light_mode", [eu.UNIFORM, eu.POWER])
def test_disable_nee_renders_the_same_bits_in_both_modes(emu, light_mode):
    s = emu.scene(eu.frame_scene("materials"))
    a, ast = s.render(48, 40, 2, estimator=eu.REFERENCE, light_mode=light_mode, disable_nee=1)
    b, bst = s.render(48, 40, 2, estimator=eu.TEXTBOOK, light_mode=light_mode, disable_nee=1)
    assert eu.same(a, b) and eu.counts_of(ast) == eu.counts_of(bst) and ast["shadow_rays"] == 0


def test_ray_counts_do_not_depend_on_the_estimator(emu, textbook_frames):
    """The weights do not steer the path: extension rays, shadow rays and shaded vertices are the reference mode's."""
    w, h, spp = eu.FRAMES["cornell"]
    _, rst = emu.scene(eu.frame_scene("cornell")).render(w, h, spp, estimator=eu.REFERENCE)
    assert eu.counts_of(rst) == eu.counts_of(textbook_frames["cornell"][1])


# ---- unbiased where the reference is not ---------------------------------------------------------------------------------------
# The fan and the quad (lights_util.fan_and_quad_scene: 64 fan triangles hold 1 % of sum(w), 2 quad triangles 99 %), 1 across and 2 above
# the floor, radiance 5 (the power of the 0.2-wide lights of radiance 125): the setting of DESIGN section 26 (0.0466 uniform, 0.0812 power).
# The reference's emitter-hit weight reads the pdf of the light the previous vertex SAMPLED: under the uniform pick that is almost
# always a fan triangle, under the power pick almost always the quad, and the two modes converge to frame means 0.0346 apart.
FAN_W = FAN_H = 16
FAN_SPP = 1024  # chosen on the CPU: combined standard errors of 0.0008 .. 0.0013 (printed below), under a tenth of the gap 0.0346
REFERENCE_GAP = 0.0346


@pytest.fixture(scope="module")
def fan_frames(emu):
    s = emu.scene(lu.fan_and_quad_scene(height=2.0, side=1.0, le=5.0))
    kw = dict(clamp=1e30, rr_start_depth=1000000, moments=True)
    out = {}
    for key, est, lm, nee_off in (("textbook_uniform", eu.TEXTBOOK, eu.UNIFORM, 0), ("textbook_power", eu.TEXTBOOK, eu.POWER, 0),
                                  ("plain", eu.REFERENCE, eu.UNIFORM, 1), ("reference_uniform", eu.REFERENCE, eu.UNIFORM, 0),
                                  ("reference_power", eu.REFERENCE, eu.POWER, 0)):
        _, _, mom = s.render(FAN_W, FAN_H, FAN_SPP, estimator=est, light_mode=lm, disable_nee=nee_off, **kw)
        out[key] = eu.frame_mean_and_se(mom, FAN_SPP)
    return out


def test_textbook_modes_agree_with_plain_path_tracing_where_the_reference_modes_do_not(fan_frames):
    """Frame means (red channel) of textbook + uniform, textbook + power and plain path tracing (disable_nee) agree pairwise within 4
    combined standard errors (a false-failure rate below 1e-4 per comparison; the seeds are fixed, so it is decided once, here),
    with the combined standard error below a tenth of the gap between the two reference-mode means -- and the reference mode still
    shows that gap.  Without the feature the textbook renders are the reference's and the first assertion fails."""
    for k, (m, se) in sorted(fan_frames.items()):
        print("%-18s mean %.5f +- %.5f" % (k, m, se))
    names = ("textbook_uniform", "textbook_power", "plain")
    for i in range(3):
        for j in range(i + 1, 3):
            (ma, sa), (mb, sb) = fan_frames[names[i]], fan_frames[names[j]]
            se = math.hypot(sa, sb)
            print("%s - %s: %.5f = %.2f combined standard errors (%.5f)" % (names[i], names[j], ma - mb, (ma - mb) / se, se))
            assert se < REFERENCE_GAP / 10.0, (names[i], names[j], se)
            assert abs(ma - mb) <= 4.0 * se, (names[i], names[j], ma, mb, se)
    (mu, su), (mp, sp) = fan_frames["reference_uniform"], fan_frames["reference_power"]
    gap, se = mp - mu, math.hypot(su, sp)
    print("reference power - uniform: %.5f (+- %.5f)" % (gap, se))
    assert se < REFERENCE_GAP / 10.0
    # the gap of DESIGN section 26 was measured at 32 x 32; this frame is 16 x 16 (other pixel centres, the same camera), so it is held
    # to half of that figure, and to being a gap at all (4 combined standard errors)
    assert gap > 0.5 * REFERENCE_GAP and gap > 4.0 * se, (gap, se)
    # ... and the reference's uniform mode is not within 4 standard errors of plain path tracing's mean (its power mode, whose sampled
    # light is nearly always the quad that is then hit, happens to be close on this scene)
    mpl, spl = fan_frames["plain"]
    assert abs(mu - mpl) > 4.0 * math.hypot(su, spl)


# ---- p_sel ---------------------------------------------------------------------------------------------------------------------------
def _random_lights(abi, rng, n, zero=()):
    lt = np.zeros(n, abi.LIGHT_DT)
    for i in range(n):
        v0 = rng.uniform(-2, 2, 3)
        e1, e2 = rng.uniform(-1, 1, 3) * 10.0 ** rng.uniform(-2, 0), rng.uniform(-1, 1, 3) * 10.0 ** rng.uniform(-2, 0)
        lt["positions"][i, 0, :3], lt["positions"][i, 1, :3], lt["positions"][i, 2, :3] = v0, v0 + e1, v0 + e2
        lt["radiance"][i, :3] = 0.0 if i in zero else rng.uniform(0.1, 1.0, 3) * 10.0 ** rng.uniform(-1, 2)
    return lt


@pytest.mark.parametrize("n,seed", [(1, 0), (3, 1), (66, 2), (130, 3), (1000, 4)])
def test_p_sel_is_the_pmf_of_the_table_to_the_stated_bound(emu, n, seed):
    """|p_sel - pmf_table| <= (1 + d_i) / (n 2^32) plus float32 rounding: p_sel = fl(fl(fl(Y) * A) * fl(1 / sum)) carries the rounding of
    Y (three products, two sums), of A (a float32 cross product, length and halving: a few ulp), of the two products and of inv_sum_w --
    under 16 ulp in all, taken as 16 * 2^-24 relative."""
    rng = np.random.RandomState(seed)
    zero = (1,) if n > 2 else ()
    lt = _random_lights(emu.abi, rng, n, zero)
    p_sel, inv = emu.psel(lt)
    table = lu.LightsEmu().build(lt)
    pmf, d = lu.implied_pmf(table)
    w = lu.weights64(lt)
    assert inv == np.float32(1.0 / w.sum())
    bound = (1.0 + d) / (n * lu.TWO32) + 16.0 * 2.0 ** -24 * pmf
    assert (np.abs(p_sel.astype(np.float64) - pmf) <= bound).all(), float((np.abs(p_sel - pmf) - bound).max())
    assert abs(float(p_sel.astype(np.float64).sum()) - 1.0) < 1e-5
    for i in zero:  # a zero-weight emitter: p_sel 0, hitPdf 0, weight power_heuristic(lastPdf, 0) = 1
        assert p_sel[i] == 0.0
        assert emu.hit_weight(0.37, 2.5, (0.0, -1.0, 0.0), (0.0, 1.0, 0.0), 0.02, float(p_sel[i])) == 1.0


def test_p_sel_of_an_all_zero_table_is_one_over_n(emu):
    lt = _random_lights(emu.abi, np.random.RandomState(9), 7, zero=range(7))
    p_sel, inv = emu.psel(lt)
    assert inv == 0.0 and (p_sel == np.float32(1.0) / np.float32(7.0)).all()
    table = lu.LightsEmu().build(lt)
    assert (table["pmf_self"] == np.float32(1.0 / 7.0)).all()  # the table fell back to the uniform pick


def test_hit_weight_is_the_power_heuristic_of_the_two_pdfs(emu):
    """power_heuristic(lastPdf, ((t * t) / (|dot(-d, N)| * A)) * p_sel) in float32, in that order."""
    f = np.float32
    last, t, A, p = f(0.8), f(3.0), f(0.25), f(0.125)
    d, n = np.array([0.6, -0.8, 0.0], f), np.array([0.0, 1.0, 0.0], f)
    cos = abs(f(f(f(-d[0]) * n[0] + f(-d[1]) * n[1]) + f(-d[2]) * n[2]))
    g = f(f(f(t * t) / f(cos * A)) * p)
    want = f(f(last * last) / f(f(last * last) + f(g * g)))
    assert f(emu.hit_weight(float(last), float(t), d, n, float(A), float(p))) == want
