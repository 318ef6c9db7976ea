"""The variance-guided filter on the CPU (include/gpuspectral_pt.h, "Variance-guided filter"): the library's per-pixel text
(csrc/pt_svgf.h through tests/emu/svgf_emu.cpp) against closed forms, against the existing emulations where the two must agree bit
for bit, and against the float64 restatement of tests/svgf_util.py with its running error bound.  No GPU."""
import os

import numpy as np
import pytest

import denoise_util as du
import svgf_util as su
import temporal_util as tu
from conftest import GOLDEN
from svgf_util import INF, U32, SvgfEmu, same, svgf64
from temporal_util import FLT_MIN

ALL_OFF = dict(sigma_color=INF, sigma_normal=INF, sigma_depth=INF, sigma_albedo=INF)
W, H = 32, 16
FOV = 0.8


@pytest.fixture(scope="module")
def emu():
    return SvgfEmu()


@pytest.fixture(scope="module")
def temu():
    return tu.TemporalEmu()


@pytest.fixture(scope="module")
def demu():
    return du.DenoiseEmu()


def f32(x):
    return np.asarray(x, np.float32)


def variance_temporal32(M):
    """V0 of the temporal branch in numpy float32, operation for operation: bit for bit the library's."""
    m1, m2, r = f32(M[..., 0]), f32(M[..., 1]), f32(M[..., 2])
    d = m2 - m1 * m1
    with np.errstate(all="ignore"):
        return np.where(d > 0, d, np.float32(0)) * (r / (np.float32(1) - r))


def moving_frames(rng, n, nan=False):
    """n frames of a plane with a step in depth and instance under a camera that turns and steps, with a jump before the last frame
    that brings new surface into view; optionally with spoilt pixels."""
    depth = np.where(np.arange(W)[None, :] < W // 2, 5.0, 7.0) * np.ones((H, W))
    inst = np.where(np.arange(W)[None, :] < W // 2, 3, 4) * np.ones((H, W), np.uint32)
    out = []
    for k in range(n):
        cam = tu.camera(0.012 * k + (0.2 if k == n - 1 else 0.0), -0.004 * k, (0.02 * k, 0.0, -1.0))
        c, a, g, i = tu.plane_frame(rng, H, W, cam, FOV, depth=depth, inst=inst)
        if nan:
            for value in (np.nan, np.inf, -np.inf):
                c[rng.integers(0, H, 6), rng.integers(0, W, 6), rng.integers(0, 3, 6)] = value
        out.append((cam, (c, a, g, i)))
    return out


# ---- moments beside the history ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nan", [False, True], ids=["finite", "nan-inf"])
def test_history_is_bit_for_bit_the_untracked_one(emu, temu, nan):
    from gpuspectral_amd import abi

    rng = np.random.default_rng(7)
    for t in (None, abi.temporal(alpha=FLT_MIN, max_history=3), abi.temporal(alpha=0.6)):
        hist = plain = None
        for k, (cam, f) in enumerate(moving_frames(rng, 6, nan)):
            hist = emu.step(t, cam, FOV, *f, hist=hist)
            plain = temu.step(t, cam, FOV, *f, hist=plain)
            assert same(hist.H, plain.H) and same(hist.G, plain.G) and np.array_equal(hist.I, plain.I), k
            assert not hist.M[..., 3].any()
        assert hist.H[..., 3].max() > 2.0 and (hist.H[..., 3] <= 1.0).any()  # some pixels kept their history, some restarted


# Unmoved camera, the pure running mean: a = fl(1 / k) at frame k, every pixel reads its own history with weight exactly 1.
#   r:  r_k = fl(fl(fl(b b) r_{k-1}) + fl(a a)), b = fl(1 - a).  a carries u, b then <= 2 u (a <= 1/2), b b 5 u, its product with r 6 u;
#       a a 3 u; the sum one more u.  Both terms are <= r_k = 1 / k, and the error of step k - 1 enters with b^2 <= 1:
#       |r_k - 1 / k| <= 7 u sum_{j=2..k} 1 / j.
#   m1: the running mean of tests/test_temporal_cpu.py with range R = max l, sum_k (3 R / k + R) u, and the emulation's l is the
#       float64 l of the test to within 6 u R (three divisions, three products, two sums): + 6 u R.
#   m2: the same for l^2 (range R^2), whose float32 value carries 2 * 6 + 1 = 13 u.
#   V0 = max(m2 - m1^2, 0) (r / (1 - r)) against s^2 / k (s^2: the unbiased sample variance; (m2 - m1^2) = s^2 (k - 1) / k and
#       r / (1 - r) = 1 / (k - 1) in exact arithmetic): the difference carries dm2 + 2 R dm1 + dm1^2 + 3 u R^2, the ratio
#       dr k / (k - 1) relative from r, dr k from 1 - r >= 1/2, and 2 u.
def running_bounds(k, R):
    hsum = sum(3.0 / j + 1.0 for j in range(1, k + 1))
    dr = 7 * U32 * sum(1.0 / j for j in range(2, k + 1))
    dm1 = (hsum + 6) * U32 * R
    dm2 = (hsum + 13) * U32 * R * R
    dd = dm2 + 2 * R * dm1 + dm1 * dm1 + 3 * U32 * R * R
    ratio = 1.0 / (k - 1) if k > 1 else 0.0
    dv = dd * ratio + R * R * ratio * (dr * k / (k - 1) + 2 * dr * k + 2 * U32) if k > 1 else 0.0
    return dr, dm1, dm2, dv


def test_unmoved_camera_running_moments_and_variance(emu):
    from gpuspectral_amd import abi

    rng = np.random.default_rng(3)
    cam = tu.camera(0.1, -0.05, (0.3, 0.2, -1.0))
    t = abi.temporal(alpha=FLT_MIN, max_history=64)
    hist, ls = None, []
    worst = np.zeros(4)
    for k in range(1, 9):
        c, a, g, i = tu.plane_frame(rng, H, W, cam, FOV)
        hist = emu.step(t, cam, FOV, c, a, g, i, hist)
        ls.append(su.frame_luminance64(c, a))
        R = float(np.max(ls))
        dr, dm1, dm2, dv = running_bounds(k, R)
        assert np.all(hist.H[..., 3] == np.float32(k))
        dev = [float(np.abs(hist.M[..., 2] - 1.0 / k).max()), float(np.abs(hist.M[..., 0] - np.mean(ls, 0)).max()),
               float(np.abs(hist.M[..., 1] - np.mean(np.square(ls), 0)).max())]
        assert dev[0] <= dr and dev[1] <= dm1 and dev[2] <= dm2, (k, dev, dr, dm1, dm2)
        if k >= 2:
            _, v0, _ = emu.run(abi.denoise(iterations=1), abi.svgf(min_history=2), hist.H, hist.M, a, g, with_variance=True)
            assert same(v0, variance_temporal32(hist.M))
            dev.append(float(np.abs(v0 - np.var(ls, 0, ddof=1) / k).max()))
            assert dev[3] <= dv, (k, dev[3], dv)
            worst = np.maximum(worst, np.array(dev) / np.array([dr, dm1, dm2, dv]))
    print("unmoved camera, 8 frames: largest deviation / bound for r, m1, m2, V0: %.3f %.3f %.3f %.3f" % tuple(worst))


# ---- the filter -------------------------------------------------------------------------------------------------------------------
def history_of(emu, rng, n=5, temporal=None, nan=False):
    hist = None
    for cam, f in moving_frames(rng, n, nan):
        hist = emu.step(temporal, cam, FOV, *f, hist=hist)
    return hist, f[1], f[2]


def test_term_off_is_the_denoiser_without_its_colour_term(emu, demu):
    from gpuspectral_amd import abi

    hist, a, g = history_of(emu, np.random.default_rng(11))
    for it in (1, 3, 5, 8):
        for kw in ({}, dict(sigma_normal=1.0, sigma_depth=0.5, sigma_albedo=0.02), dict(sigma_normal=INF, sigma_depth=INF, sigma_albedo=INF)):
            got = emu.run(abi.denoise(iterations=it, **kw), abi.svgf(sigma_variance=INF), hist.H, hist.M, a, g)
            assert same(got, demu.run(abi.denoise(iterations=it, sigma_color=INF, **kw), hist.H, a, g)), (it, kw)
    # ... and sigma_color itself is validated and not used
    assert same(emu.run(abi.denoise(sigma_color=0.01), None, hist.H, hist.M, a, g), emu.run(abi.denoise(sigma_color=INF), None, hist.H, hist.M, a, g))


def planes(rng, h, w, L=None):
    E = np.zeros((h, w, 4), np.float32)
    E[..., :3] = rng.uniform(0.5, 1.5, (h, w, 3)) if L is None else L[..., None]
    E[..., 3] = du.luma64(E[..., :3].astype(np.float64)).astype(np.float32) if L is None else L
    A = np.ones((h, w, 4), np.float32)
    G = np.zeros((h, w, 4), np.float32)
    G[..., 2], G[..., 3] = -1.0, 5.0
    return E, A, G


def test_constant_variance_shrinks_by_the_kernel_energy(emu):
    """Every edge-stop off: w = h exactly, sum_w = 1 exactly in the interior, so V' = sum(h^2 v) / 1: 25 products of the exact h^2
    with v (u each) and 24 additions of positive terms: <= 49 u relative to v (70/256)^2, the sum of h^2."""
    from gpuspectral_amd import abi

    rng = np.random.default_rng(5)
    E, A, G = planes(rng, 12, 20)
    for v in (1.0, 0.3, 7.7e-5):
        _, v2 = emu.level(abi.denoise(**ALL_OFF), abi.svgf(sigma_variance=INF), 0, E, A, G, np.full((12, 20), v, np.float32))
        want = float(np.float32(v)) * (70.0 / 256.0) ** 2
        dev = float(np.abs(v2[2:-2, 2:-2] / want - 1.0).max())
        print("constant V = %g: interior V' / (v (70/256)^2) - 1 = %.2f u" % (v, dev / U32))
        assert dev <= 49 * U32
        assert np.all(v2 >= want * (1 - 49 * U32))  # at the border the same mass over a smaller sum_w^2: not smaller


def test_a_luminance_step_isolates_under_a_small_variance_and_mixes_under_a_large_one(emu):
    """L = 1 | 2 with V = 1e-8: inv_l = 1 / (4e-4 + 1e-4) = 2000, so a tap across the step has x = 2000 > 87.34 and w = 0 exactly:
    each side is what it would be with ANY other side.  Under V = 1 the same tap has x = 1 / 4.0001 and the sides mix."""
    from gpuspectral_amd import abi

    rng = np.random.default_rng(9)
    h, w = 10, 24
    left = np.arange(w)[None, :] < w // 2

    def run(right, v):
        L = np.where(left, 1.0, right).astype(np.float32) * np.ones((h, w), np.float32)
        E, A, G = planes(rng, h, w, L)
        return emu.level(abi.denoise(**ALL_OFF), None, 0, E, A, G, np.full((h, w), v, np.float32))

    e_a, v_a = run(2.0, 1e-8)
    e_b, v_b = run(3.0, 1e-8)
    assert same(e_a[:, : w // 2], e_b[:, : w // 2]) and same(v_a[:, : w // 2], v_b[:, : w // 2])
    assert np.all(e_a[:, : w // 2, :3] == 1.0) and np.all(e_a[:, w // 2:, :3] == 2.0)
    e_c, _ = run(2.0, 1.0)
    near = e_c[:, w // 2 - 2: w // 2, :3]
    assert np.all(near > 1.0) and np.all(near < 2.0)  # it mixed
    assert np.all(e_c[:, : w // 2 - 2, :3] == 1.0)  # out of the 5 x 5 kernel's reach


def test_spatial_fallback_is_chosen_per_pixel(emu):
    from gpuspectral_amd import abi

    rng = np.random.default_rng(13)
    dn = abi.denoise(iterations=1)
    hist, a, g = history_of(emu, rng, n=3, temporal=abi.temporal(alpha=FLT_MIN))
    _, v_spatial, _ = emu.run(dn, abi.svgf(min_history=65536), hist.H, hist.M, a, g, with_variance=True)
    r = svgf64(hist.H, hist.M, a, g, iterations=1, min_history=65536)
    assert not r["temporal"].any()
    _, v_mixed, _ = emu.run(dn, abi.svgf(min_history=2), hist.H, hist.M, a, g, with_variance=True)
    t = (hist.H[..., 3] >= 2.0) & (hist.M[..., 2] < 1.0)
    assert t.any() and (~t).any()  # the camera's step disoccluded some pixels: they are in their first frame
    assert same(v_mixed[t], variance_temporal32(hist.M)[t]) and same(v_mixed[~t], v_spatial[~t])
    assert not same(v_mixed[t], v_spatial[t])
    # three frames of an unmoved camera: every pixel has len = 3 >= 2
    cam = tu.camera()
    still = None
    for _ in range(3):
        f = tu.plane_frame(rng, H, W, cam, FOV)
        still = emu.step(abi.temporal(alpha=FLT_MIN), cam, FOV, *f, hist=still)
    _, v_all, _ = emu.run(dn, abi.svgf(min_history=2), still.H, still.M, f[1], f[2], with_variance=True)
    assert same(v_all, variance_temporal32(still.M))
    _, v_none, _ = emu.run(dn, None, still.H, still.M, f[1], f[2], with_variance=True)  # the default asks for 4 frames
    assert same(v_none, emu.run(dn, abi.svgf(min_history=65536), still.H, still.M, f[1], f[2], with_variance=True)[1])


def agree(emu, denoise_kw, svgf_kw, Hh, M, a, g, what):
    """The emulation against the restatement, pixel by pixel within the restatement's own error bound.  Returns (largest
    deviation, largest deviation / bound)."""
    from gpuspectral_amd import abi

    kw = {k: v for k, v in denoise_kw.items() if k != "sigma_color"}
    got, v0, _ = emu.run(abi.denoise(**denoise_kw), abi.svgf(**svgf_kw), Hh, M, a, g, with_variance=True)
    r = svgf64(Hh, M, a, g, **kw, **svgf_kw)
    valid = np.isfinite(np.asarray(Hh, np.float32)[..., :3]).all(-1)
    assert same(got[..., 3], np.asarray(Hh, np.float32)[..., 3]) and same(got[~valid], np.asarray(Hh, np.float32)[~valid])
    assert np.all(v0[~valid] == 0.0)
    dev = np.abs(got[valid][:, :3].astype(np.float64) - r["out"][valid][:, :3]).max(-1)
    assert np.isfinite(got[valid]).all()
    if dev.size == 0:
        return 0.0, 0.0
    ratio = float((dev / r["err"][valid]).max())
    print("%s: largest deviation %.3e, largest deviation / bound %.3f, largest bound %.3e" % (what, dev.max(), ratio, r["err"][valid].max()))
    assert np.all(dev <= r["err"][valid]), what
    return float(dev.max()), ratio


def test_non_finite_pixels(emu):
    rng = np.random.default_rng(17)
    hist, a, g = history_of(emu, rng, n=5, nan=True)
    bad = ~np.isfinite(hist.H[..., :3]).all(-1)
    assert bad.any() and np.all(hist.H[..., 3][bad] == 0.0)  # only a pixel without history can hold a non-finite record
    assert np.all(hist.M[bad] == np.float32([0, 0, 1, 0]))
    assert np.isfinite(hist.M).all()
    for it in (1, 5):
        agree(emu, dict(iterations=it), {}, hist.H, hist.M, a, g, "NaN / Inf pixels, %d iterations" % it)
        agree(emu, dict(iterations=it), dict(min_history=2, sigma_variance=1.0), hist.H, hist.M, a, g, "NaN / Inf pixels, %d iterations, min_history 2" % it)


@pytest.mark.parametrize("size", [(1, 1), (5, 3)])
def test_small_frames_and_steps_beyond_the_frame(emu, size):
    from gpuspectral_amd import abi

    w, h = size
    rng = np.random.default_rng(19)
    cam = tu.camera()
    hist = None
    for _ in range(5):
        f = tu.plane_frame(rng, h, w, cam, FOV)
        hist = emu.step(abi.temporal(alpha=FLT_MIN), cam, FOV, *f, hist=hist)
    for it in (1, 3, 8):  # steps 1 .. 128: every tap but the centre leaves the frame soon
        for kw in ({}, dict(min_history=65536), dict(sigma_variance=0.5)):
            agree(emu, dict(iterations=it), kw, hist.H, hist.M, f[1], f[2], "%dx%d, %d iterations, %s" % (w, h, it, kw or "defaults"))
    if size == (1, 1):  # one pixel: the spatial estimate is 0, the filter is the identity up to the division and the product
        out = emu.run(None, abi.svgf(min_history=65536), hist.H, hist.M, f[1], f[2])
        assert np.all(np.abs(out[..., :3] / hist.H[..., :3] - 1.0) <= 2 * U32 * 1.01)


# ---- agreement with the restatement on the Cornell box ----------------------------------------------------------------------------
# The moments: what tests/test_temporal_cpu.py derives for H holds for anything pulled through the same reprojection -- the
# position carries dp = 64 u * 128 of a pixel, prev = s / sw moves by at most 2 * 8 dp / sw * max |M_q| -- plus a few u of the
# larger of the reprojected and the new value; the new values l and l^2 carry 6 u and 13 u themselves (see running_bounds).
# The filter: svgf64 carries its own running error bound (tests/svgf_util.py), pixel by pixel, and is fed the emulation's
# float32 H and M, so no decision of the filter can fall differently: no pixel is left out there.
AGREE_SEEDS = (1, 2, 3, 4)
LEFT_OUT_CAP = 0.01


def cornell_frames(cornell, seed, n, size=128):
    """The frames and camera moves of tests/test_temporal_cpu.py (the same random sequence), n of them."""
    from test_temporal_cpu import cornell_frames as frames

    return frames(cornell, seed, n=n, size=size)


@pytest.mark.parametrize("seed", AGREE_SEEDS)
def test_emulation_agrees_with_the_restatement_on_cornell(emu, cornell, seed):
    from gpuspectral_amd import abi

    fov = float(cornell.fov)
    hist = None
    for k, (cam, f) in enumerate(cornell_frames(cornell, seed, 5)):
        new = emu.step(abi.temporal(), cam, fov, *f, hist=hist)
        r = su.moments64(*f, cam, fov, hist=hist)
        fragile = r["fragile"] | (np.abs(r["H"][..., 3] - new.H[..., 3]) > 1e-3)  # (a tap kept by one and dropped by the other)
        left_out = float(fragile.mean())
        dp = 64 * U32 * 128
        big = np.abs(hist.M[..., :3]).max((0, 1)).astype(np.float64) if hist is not None else np.zeros(3)  # per channel: m1, m2, r
        lmax = float(np.nanmax(su.frame_luminance64(f[0], f[1])))
        bound = 2 * 8 * dp / np.maximum(r["sw"], 0.01)[..., None] * big + 16 * U32 * np.maximum(big, [lmax, lmax * lmax, 1.0])
        dev = np.abs(new.M[..., :3].astype(np.float64) - r["M"][..., :3])
        print("seed %d frame %d: moments: %.3f %% of the pixels left out, largest deviation / bound of m1, m2, r: %s; largest deviation %s"
              % (seed, k, 100 * left_out, (dev / bound)[~fragile].max(0).round(4), dev[~fragile].max(0)))
        assert left_out <= LEFT_OUT_CAP
        assert np.all(dev[~fragile] <= bound[~fragile])
        hist = new
    t = (hist.H[..., 3] >= 4.0) & (hist.M[..., 2] < 1.0)
    assert 0.5 < t.mean() < 1.0  # both estimates of the initial variance are in play
    for it, kw in ((5, {}), (1, {}), (3, dict(min_history=2, sigma_variance=1.0))):
        agree(emu, dict(iterations=it), kw, hist.H, hist.M, f[1], f[2], "seed %d, filter, %d iterations, %s" % (seed, it, kw or "defaults"))


# ---- quality ---------------------------------------------------------------------------------------------------------------------------
REFERENCE = os.path.join(GOLDEN, "cornell_64_4096spp.npy")  # the oracle, 64 x 64, timestamps 8 .. 4103 (make_reference below)


def make_reference(cornell, oracle_mod):
    orc = oracle_mod.Oracle(cornell)
    try:
        ref = np.zeros((64 * 64, 4), np.float32)
        for done in range(0, 4096, 256):
            ref, _ = orc.render(64, 64, 256, 8 + done, accum=ref)  # (sample 8 + j is folded with weight 1 / (8 + j + 1) ...)
    finally:
        orc.close()
    ref[:, :3] *= np.float32((8 + 4096) / 4096.0)  # ... so the cleared buffer holds sum / (8 + 4096)
    return ref


def test_svgf_is_closer_to_the_reference_than_the_history(emu, demu, cornell, oracle_mod):
    """Cornell box 64 x 64, unmoved camera: eight 1-spp frames (frame k = the oracle's sample of timestamp k alone, as
    gsp_frame_sample_base(k) makes it), default temporal parameters, guides from the features emulation.  MSE over RGB against the
    committed 4096-spp oracle image of other timestamps, for H, the plain filter of H and the variance-guided filter of H.
    Asserted: SVGF below H.  Measured: profiles/svgf_quality.txt."""
    import features_util as fu
    from gpuspectral_amd import abi

    W_ = H_ = 64
    ref = np.load(REFERENCE).astype(np.float64)
    a, g, i = fu.full(fu.FeaturesEmu().scene(cornell).render(W_, H_, 1), W_, H_)
    orc = oracle_mod.Oracle(cornell)
    hist = None
    try:
        for k in range(8):
            c, _ = orc.render(W_, H_, 1, k)
            c = c.reshape(H_, W_, 4).copy()
            c[..., :3] *= np.float32(k + 1)  # the fold weighs sample k by 1 / (k + 1) on the cleared buffer; the base undoes that
            hist = emu.step(None, cornell.to_world, float(cornell.fov), c, a, g, i, hist=hist)
    finally:
        orc.close()
    mse = lambda img: float(((np.asarray(img, np.float64)[..., :3] - ref) ** 2).mean())
    m_h = mse(hist.H)
    m_plain = mse(demu.run(None, hist.H, a, g))
    m_svgf = mse(emu.run(None, None, hist.H, hist.M, a, g))
    print("MSE against 4096 spp: H %.6g, plain a-trous of H %.6g (ratio %.3f), SVGF of H %.6g (ratio %.3f)"
          % (m_h, m_plain, m_plain / m_h, m_svgf, m_svgf / m_h))
    for s in (1.0, 2.0, 8.0):
        for mh in (2, 4):
            m = mse(emu.run(None, abi.svgf(sigma_variance=s, min_history=mh), hist.H, hist.M, a, g))
            print("  sigma_variance %g, min_history %d: MSE %.6g (ratio %.3f)" % (s, mh, m, m / m_h))
    assert m_svgf < m_h


if __name__ == "__main__":  # python tests/test_svgf_cpu.py: renders the committed reference again (minutes of CPU)
    from oracle import mitsuba_loader as ml
    from oracle import oracle as orc_mod
    from conftest import CORNELL_XML

    img = make_reference(ml.load_scene(CORNELL_XML), orc_mod).reshape(64, 64, 4)[..., :3]
    np.save(REFERENCE, img.astype(np.float32))
    print("wrote", REFERENCE)
