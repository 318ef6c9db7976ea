"""The illumination history on the CPU (include/gpuspectral_pt.h, "Illumination history"): the library's per-pixel text (csrc/pt_illum.h
through tests/emu/illum_emu.cpp) against the emulations of the sections it builds on (bit for bit where the feature is off), against
closed forms, and against the float64 restatement of tests/illum_util.py.  No GPU."""
import os

import numpy as np
import pytest

import illum_util as iu
import temporal_util as tu
from conftest import ROOT
from illum_util import IllumEmu
from motion_util import MotionEmu
from svgf_util import SvgfEmu
from temporal_util import U32, TemporalEmu, same

FOV = 0.05
W, H = 24, 10
MODES = ("plain", "moments", "moments+follow")
FRAGILE_CAP = 0.02
LINES = {}


@pytest.fixture(scope="module")
def emu():
    return IllumEmu()


@pytest.fixture(scope="module", autouse=True)
def record():
    """After the module's tests: profiles/illum_cpu_check.txt, written when every test that contributes a line has run."""
    yield
    want = ["off", "overflow", "feedback1", "feedback0"] + ["agree %s %d" % (m, s) for m in MODES for s in (1, 2)]
    if all(k in LINES for k in want):
        with open(os.path.join(ROOT, "profiles", "illum_cpu_check.txt"), "w") as fh:
            fh.write("tests/test_illum_cpu.py -- csrc/pt_illum.h on the host (tests/emu/illum_emu.cpp) against the emulations it builds on and against\n"
                     "the float64 restatement of tests/illum_util.py.  Golden Cornell box with a per-pixel textured albedo (2 % of it below the floor),\n"
                     "camera moves, one instance translating and rotating.\n\n" + "\n".join(LINES[k] for k in want) + "\n")


def textured(rng, f, floor_some=False):
    """The frame f with an albedo that differs from pixel to pixel (coverage stays 1: A = a' exactly in float32 and float64)."""
    c, a, g, i = (p.copy() for p in f)
    surf = i[..., 2] != tu.BACKGROUND
    a[..., :3] = np.where(surf[..., None], a[..., :3] * rng.uniform(0.3, 1.0, a.shape[:2] + (3,)), a[..., :3]).astype(np.float32)
    if floor_some:
        a[..., :3][rng.uniform(size=a.shape[:2]) < 0.02] = np.float32(0.001)  # below the floor of 0.01
    return c, a, g, i


def frames(cornell, seed, n=5):
    """tests/test_motion_cpu.py's Cornell frames (camera moves, one instance translating and rotating) with a textured albedo."""
    from test_motion_cpu import cornell_frames

    rng = np.random.default_rng(1000 + seed)
    return [(cam, xf, textured(rng, f, floor_some=True)) for cam, xf, f in cornell_frames(cornell, seed, n=n)]


_FRAMES = {}


def cached_frames(cornell, seed):
    if seed not in _FRAMES:
        _FRAMES[seed] = frames(cornell, seed)
    return _FRAMES[seed]


# ---- off: the emulations of the sections below, bit for bit -----------------------------------------------------------------------------
def test_demodulation_off_is_the_existing_emulations_bit_for_bit(emu, cornell):
    from gpuspectral_amd import abi

    temu, semu, memu = TemporalEmu(), SvgfEmu(), MotionEmu()
    fov = float(cornell.fov)
    h0 = h1 = h2 = g0 = g1 = g2 = None
    for cam, xf, f in cached_frames(cornell, 1)[:4]:
        g0 = emu.step(None, cam, fov, *f, hist=g0, demod=False)
        h0 = temu.step(None, cam, fov, *f, hist=h0)
        assert same(g0.H, h0.H) and same(g0.G, h0.G) and np.array_equal(g0.I, h0.I)
        g1 = emu.step(None, cam, fov, *f, hist=g1, moments=True, demod=False)
        h1 = semu.step(None, cam, fov, *f, hist=h1)
        assert same(g1.H, h1.H) and same(g1.M, h1.M) and same(g1.G, h1.G) and np.array_equal(g1.I, h1.I)
        g2 = emu.step(None, cam, fov, *f, xforms=xf, hist=g2, moments=True, demod=False)
        h2 = memu.step(None, cam, fov, *f, xf, hist=h2, moments=True)
        assert same(g2.H, h2.H) and same(g2.M, h2.M) and same(g2.V, h2.V) and np.array_equal(g2.I, h2.I)
    a, g = f[1], f[2]
    for dn, sv in ((None, None), (abi.denoise(iterations=3), abi.svgf(min_history=2, sigma_variance=1.0))):
        assert same(emu.svgf(dn, sv, g1.H, g1.M, a, g, demod=False), semu.run(dn, sv, h1.H, h1.M, a, g))
    assert same(emu.image(g1.H, a, demod=False), g1.H)
    from denoise_util import DenoiseEmu

    assert same(emu.denoise(None, g0.H, a, g, demod=False), DenoiseEmu().run(None, h0.H, a, g))
    LINES["off"] = "demodulation off, no feedback: H, G, I, M, V over four Cornell frames and the filters equal TemporalEmu / SvgfEmu / MotionEmu / DenoiseEmu bit for bit"


# ---- the first frame: closed forms on random planes ---------------------------------------------------------------------------------------
def random_frame(rng, h=H, w=W):
    cam = tu.camera()
    c, a, g, i = tu.plane_frame(rng, h, w, cam, FOV)
    a[..., :3] = rng.uniform(0.0, 1.0, (h, w, 3))
    a[..., 3] = rng.choice(np.float32([1.0, 1.0, 0.75, 0.5]), (h, w))
    a[..., :3] *= a[..., 3:4]  # (the feature pass accumulates albedo * coverage)
    g *= a[..., 3:4]
    bad = rng.uniform(size=(h, w))
    c[..., 0][bad < 0.05] = np.nan
    c[..., 1][(bad >= 0.05) & (bad < 0.1)] = np.inf
    a[..., :3][(bad >= 0.1) & (bad < 0.2)] = 0.0  # A at its floor
    return cam, (c, a, g, i)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_first_frame_on_random_planes(emu, seed):
    rng = np.random.default_rng(seed)
    cam, f = random_frame(rng)
    new = emu.step(None, cam, FOV, *f, moments=True)
    r = iu.illum64(*f, cam, FOV, moments=True)
    ok = ~r["fragile"]
    u = r["u"]
    assert (~u).sum() >= 3 and u.sum() > 100
    # not u: the raw record, nobody's history; u: {e, 1}
    assert same(new.H[~u][:, :3], f[0][~u][:, :3]) and np.all(new.H[..., 3][~u] == 0.0) and np.all(new.H[..., 3][u] == 1.0)
    assert np.all(new.M[~u] == np.float32([0, 0, 1, 0]))
    # e = c / A: miss, the sum and the quotient are one rounding each -- 3 u relative; L three products and two sums on top: 6 u;
    # l * l 13 u
    sel = u & ok
    e64, e32 = r["e"][sel], new.H[sel][:, :3].astype(np.float64)
    assert np.all(np.abs(e32 - e64) <= 3 * U32 * np.abs(e64))
    L64 = r["M"][sel][:, 0]
    Labs = iu.luma64(np.abs(e64))
    assert np.all(np.abs(new.M[sel][:, 0] - L64) <= 6 * U32 * Labs) and np.all(np.abs(new.M[sel][:, 1] - L64 * L64) <= 13 * U32 * Labs * Labs)
    assert np.all(new.M[sel][:, 2] == 1.0)
    # the image read-out gives the frame back: e * A = c up to the quotient's and the product's rounding
    img = emu.image(new.H, f[1])
    assert same(img[~u], new.H[~u]) and same(img[..., 3], new.H[..., 3])
    i64 = iu.image64(new.H, f[1])
    assert np.all(np.abs(img[sel][:, :3] - i64[sel][:, :3]) <= 3 * U32 * np.abs(i64[sel][:, :3]))
    assert np.all(np.abs(img[sel][:, :3] - f[0][sel][:, :3].astype(np.float64)) <= 6 * U32 * np.abs(f[0][sel][:, :3]))


def test_overflowing_quotient_takes_the_not_u_path(emu):
    """c finite and c / A not finite: without history the raw record with length 0, with history H' = prev and no growth."""
    rng = np.random.default_rng(5)
    cam, f = random_frame(rng)
    c, a, g, i = (p.copy() for p in f)
    c[..., :3] = rng.uniform(0.5, 1.5, c[..., :3].shape)
    a[..., :3], a[..., 3] = 0.5, 1.0
    g[..., :3], g[..., 3] = (0.0, 0.0, -1.0), f[2][..., 3] / f[1][..., 3]
    first = emu.step(None, cam, FOV, c, a, g, i, moments=True)
    assert np.all(first.H[..., 3] == 1.0)
    c2, a2 = c.copy(), a.copy()
    c2[2, 3, :3] = np.float32([1.0, 3.0e38, 1.0])
    a2[2, 3, :3] = np.float32([0.5, 0.02, 0.5])  # 3e38 / 0.02 overflows
    c2[4, 5, :3] = np.float32([1.0, 3.0e38, 1.0])  # ... and 3e38 / 0.5 overflows as well
    c2[6, 7, :3] = np.float32([1.0, 1.0e38, 1.0])  # ... while 1e38 / 0.5 = 2e38 does not
    assert np.isfinite(c2[..., :3]).all()
    fr = iu.frame64(c2, a2)
    assert not fr["u"][2, 3] and not fr["u"][4, 5] and fr["u"][6, 7] and (~fr["u"]).sum() == 2
    none = emu.step(None, cam, FOV, c2, a2, g, i, moments=True)
    for y, x in ((2, 3), (4, 5)):
        assert same(none.H[y, x], np.float32([c2[y, x, 0], c2[y, x, 1], c2[y, x, 2], 0.0])) and same(none.M[y, x], np.float32([0, 0, 1, 0]))
    assert none.H[6, 7, 3] == 1.0 and none.H[6, 7, 1] == np.float32(1.0e38) / np.float32(0.5)
    second = emu.step(None, cam, FOV, c2, a2, g, i, hist=first, moments=True)
    for y, x in ((2, 3), (4, 5)):  # an unmoved camera: one tap of weight 1, prev = the pixel's own record
        assert same(second.H[y, x], first.H[y, x]) and same(second.M[y, x], first.M[y, x])
    assert second.H[6, 7, 3] == 2.0 and np.all(second.H[..., 3][fr["u"]] == 2.0)
    LINES["overflow"] = "overflow: c finite with c / A not finite takes the not-u path (raw record and length 0 without history, H' = prev with it)"


# ---- feedback -----------------------------------------------------------------------------------------------------------------------------
def grown(emu, rng, demod, n=5, nan=True):
    cam = tu.camera()
    hist = None
    for k in range(n):
        f = textured(rng, tu.plane_frame(rng, H, W, cam, FOV))
        if nan and k == n - 1:
            f[0][1, 2, 0] = np.nan
            f[0][7, 20, 2] = np.inf
        hist = emu.step(None, cam, FOV, *f, hist=hist if k != n - 1 or not nan else None, moments=True, demod=demod)
        if nan and k == n - 1:  # a last frame without history: two invalid records, every other pixel of length 1 ...
            assert not np.isfinite(hist.H[1, 2, 0]) and hist.H[1, 2, 3] == 0.0
    return hist, f[1], f[2]


@pytest.mark.parametrize("demod", [True, False])
def test_feedback_output_and_what_it_leaves_alone(emu, demod):
    from gpuspectral_amd import abi

    rng = np.random.default_rng(21)
    for nan in (False, True):
        hist, a, g = grown(emu, rng, demod, nan=nan)
        valid = np.isfinite(hist.H[..., :3]).all(-1)
        assert nan == (not valid.all())
        for dn, sv, its in ((None, abi.svgf(min_history=2), 5), (abi.denoise(iterations=3), abi.svgf(min_history=2, sigma_variance=1.0), 3)):
            plain = emu.svgf(dn, sv, hist.H, hist.M, a, g, demod=demod)
            for levels in range(1, its + 1):
                before = hist.H.copy()
                out, fb = emu.svgf(dn, sv, hist.H, hist.M, a, g, demod=demod, levels=levels)
                assert same(out, plain)  # the call's output is the plain filter's, bit for bit
                assert same(hist.H, before)  # (the emulation returns the fed-back history, it does not write it)
                assert same(fb[..., 3], hist.H[..., 3]) and same(fb[~valid], hist.H[~valid])  # len and the invalid pixels keep their bits
                assert np.isfinite(fb[valid]).all() and not same(fb[valid], hist.H[valid])
            # feeding back every level of a filter whose output is not re-modulated gives that output: levels = iterations, demod off
            if not demod:
                assert same(emu.svgf(dn, sv, hist.H, hist.M, a, g, demod=False, levels=its)[1][valid], plain[valid])
            with pytest.raises(ValueError):
                emu.svgf(dn, sv, hist.H, hist.M, a, g, demod=demod, levels=its + 1)
    LINES["feedback%d" % demod] = ("feedback, demodulation %s: output == the plain filter bit for bit at every levels 1 .. iterations; len and invalid pixels keep "
                                   "their bits (G, I, M are not arguments of the store)" % ("on" if demod else "off"))


# ---- agreement with the restatement on histories grown over several frames ----------------------------------------------------------------
# Bounds.  H and M: what tests/test_motion_cpu.py and tests/test_svgf_cpu.py derive for anything pulled through the reprojection -- the
# position carries dp = 96 u * 128 of a pixel (64 u without the record; the larger is used for every mode), prev = s / sw moves by at
# most 2 * 8 dp / sw * max |H_q| -- plus the new value's own error and a few roundings of the blend on the larger of the two: there 16 u;
# here the new value is e = c / A (3 u, and the restatement is fed e rounded to float32: 1 u more) resp. l (6 u on top) and l^2
# (13 u), so 24 u and 32 u.  The image: A and the product, 3 u.  The filter and the feedback: svgf64's own running bound (illum_util.svgf_demod64).
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seed", [1, 2])
def test_emulation_agrees_with_the_restatement(emu, cornell, mode, seed):
    from gpuspectral_amd import abi

    moments, follow = mode != "plain", mode == "moments+follow"
    fov = float(cornell.fov)
    hist = None
    worst_left = worst_h = worst_m = 0.0
    for k, (cam, xf, f) in enumerate(cached_frames(cornell, seed)):
        xforms = xf if follow else None
        new = emu.step(abi.temporal(), cam, fov, *f, xforms=xforms, hist=hist, moments=moments)
        r = iu.illum64(*f, cam, fov, xforms=xforms, hist=hist, moments=moments)
        assert same(r["G"], new.G) and np.array_equal(r["I"], new.I)
        fragile = r["fragile"]  # the restatement alone decides what is left out
        left = float(fragile.mean())
        ok = ~fragile
        dp = 96 * U32 * 128
        big = float(np.abs(hist.H[..., :3]).max()) if hist is not None else 0.0
        emax = float(np.abs(r["e"][r["u"]]).max())
        bound = 2 * 8 * dp / np.maximum(r["sw"], 0.01) * big + 24 * U32 * max(big, emax)
        dev = np.abs(new.H.astype(np.float64) - r["H"]).max(-1)
        assert left <= FRAGILE_CAP
        assert np.all(dev[ok] <= bound[ok])
        worst_left, worst_h = max(worst_left, left), max(worst_h, float((dev[ok] / bound[ok]).max()))
        if moments:
            bigm = np.abs(hist.M[..., :3]).max((0, 1)).astype(np.float64) if hist is not None else np.zeros(3)
            lmax = float(iu.luma64(np.abs(r["e"][r["u"]])).max())
            bm = 2 * 8 * dp / np.maximum(r["sw"], 0.01)[..., None] * bigm + 32 * U32 * np.maximum(bigm, [lmax, lmax * lmax, 1.0])
            dm = np.abs(new.M[..., :3].astype(np.float64) - r["M"][..., :3])
            assert np.all(dm[ok] <= bm[ok])
            worst_m = max(worst_m, float((dm[ok] / bm[ok]).max()))
        if follow:
            assert np.array_equal(r["V"][..., 3][ok], new.V[..., 3][ok])
        print("%s seed %d frame %d: %.3f %% of the pixels left out as fragile, largest |H - H64| / bound %.3f" % (mode, seed, k, 100 * left, (dev[ok] / bound[ok]).max()))
        hist = new
    a, g = f[1], f[2]
    img = emu.image(hist.H, a)
    i64 = iu.image64(hist.H, a)
    assert same(img[..., 3], hist.H[..., 3]) and np.all(np.abs(img[..., :3] - i64[..., :3]) <= 3 * U32 * np.abs(i64[..., :3]))
    assert not same(img[..., :3], hist.H[..., :3])  # a textured albedo: the image is not the illumination
    line = "%s, seed %d: five Cornell frames 128 x 128, largest fragile share %.3f %% (cap %.0f %%), largest |H - H64| / bound %.3f" % (
        mode, seed, 100 * worst_left, 100 * FRAGILE_CAP, worst_h)
    if moments:
        line += ", largest |M - M64| / bound %.3f" % worst_m
        for dn_kw, sv_kw, levels in ((dict(), dict(), 1), (dict(iterations=3), dict(min_history=2, sigma_variance=1.0), 3)):
            out, fb = emu.svgf(abi.denoise(**dn_kw), abi.svgf(**sv_kw), hist.H, hist.M, a, g, levels=levels)
            q = iu.svgf_demod64(hist.H, hist.M, a, g, levels=levels, **dn_kw, **sv_kw)
            v = q["valid"]
            assert v.all() and same(out[..., 3], hist.H[..., 3])
            d_out = np.abs(out[..., :3].astype(np.float64) - q["out"][..., :3]).max(-1)
            d_fb = np.abs(fb[..., :3].astype(np.float64) - q["fb"]["e"]).max(-1)
            assert np.all(d_out <= q["err"]) and np.all(d_fb <= q["fb"]["err"])
            line += "; filter %s levels=%d: largest deviation / bound %.3f (output), %.3f (fed-back H)" % (
                dn_kw.get("iterations", 5), levels, (d_out / q["err"]).max(), (d_fb / q["fb"]["err"]).max())
    else:
        got = emu.denoise(None, hist.H, a, g)
        assert same(got[..., 3], hist.H[..., 3]) and np.isfinite(got).all()
    print(line)
    LINES["agree %s %d" % (mode, seed)] = line
