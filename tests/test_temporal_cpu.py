"""Temporal accumulation on the CPU (include/gpuspectral_pt.h, "Temporal accumulation"): the library's per-pixel text
(csrc/pt_temporal.h through tests/emu/temporal_emu.cpp) against closed forms and against the float64 restatement of
tests/temporal_util.py.  No GPU."""
import copy
import os

import numpy as np
import pytest

import temporal_util as tu
from conftest import GOLDEN
from temporal_util import BACKGROUND, FLT_MIN, U32, TemporalEmu, same, temporal64

FOV = 0.05  # a narrow camera: a turn by atan(k / zplane) then shifts every pixel by k to within 0.01 of a pixel (see test_pure_shift)
W, H = 32, 16


@pytest.fixture(scope="module")
def emu():
    return TemporalEmu()


def pure_mean(**kw):
    from gpuspectral_amd import abi

    return abi.temporal(alpha=FLT_MIN, **kw)


# ---- unmoved camera ----------------------------------------------------------------------------------------------------------------
# Bound on |H_k - mean64| after K frames of a running mean with colours in [0, R), R = 2.  With the snap every pixel reads its
# own pixel with weight exactly 1, so prev = (1 * H) / 1 = H and len = (1 * len) / 1 = len without rounding.  Step k computes
# fl(prev + fl(fl(c - prev) * fl(1 / k))): three roundings on the correction term, each at most u relative, and |c - prev| < R, so
# the term carries at most 3 u R / k (first order); the sum's rounding adds at most u |H_k| < u R.  The error of step k - 1 enters
# with factor (1 - 1/k) <= 1.  So e_K <= sum_{k=1..K} (3 R / k + R) u, which is 32.3 u for K = 8, R = 2 (step 1 is in fact exact).
K_FRAMES = 8
RANGE = 2.0
MEAN_BOUND = sum(3.0 * RANGE / k + RANGE for k in range(1, K_FRAMES + 1)) * U32


def test_unmoved_camera_is_an_exact_running_mean(emu):
    rng = np.random.default_rng(3)
    cam = tu.camera(0.1, -0.05, (0.3, 0.2, -1.0))
    hist, frames, worst = None, [], 0.0
    for k in range(1, K_FRAMES + 1):
        c, a, g, i = tu.plane_frame(rng, H, W, cam, 0.8)
        frames.append(c[..., :3].astype(np.float64))
        hist, kept = emu.step(pure_mean(max_history=64), cam, 0.8, c, a, g, i, hist, with_kept=True)
        assert np.all(hist.H[..., 3] == np.float32(k))
        if k > 1:
            assert np.all(kept == 0x81)  # the projection lands in the frame and tap 0 alone (weight 1) is kept
        dev = float(np.abs(hist.H[..., :3] - np.mean(frames, 0)).max())
        worst = max(worst, dev)
    print("unmoved camera, %d frames: largest |H - float64 mean| = %.3f u (bound %.1f u)" % (K_FRAMES, worst / U32, MEAN_BOUND / U32))
    assert 4.0 * worst <= MEAN_BOUND


# ---- a pure image-plane shift -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, -3])
def test_pure_shift(emu, k):
    """The camera turns by atan(k / zplane) about its up axis in front of a fronto-parallel plane.  A turn moves image column x to
    zplane * tan(atan(x / zplane) + theta): k * (1 + (x / zplane)^2) / (1 - k x / zplane^2) pixels away.  With fov 0.05 rad, x / zplane
    <= 0.025 and the shift is k to within 0.003 of a pixel (rows move by less than 0.003): columns whose predecessor lies in the
    frame take it (bilinear weights, sw ~ 1) and have len == 2 exactly (sl and sw are the same float sums, so sl / sw == 1), the |k|
    columns that entered the frame have no tap of weight >= 0.01."""
    from gpuspectral_amd import abi

    rng = np.random.default_rng(5)
    zp = tu.zplane64(W, H, FOV)
    cam0, cam1 = tu.camera(), tu.camera(np.arctan(k / zp))
    f0 = tu.plane_frame(rng, H, W, cam0, FOV)
    f1 = tu.plane_frame(rng, H, W, cam1, FOV)
    h0 = emu.step(abi.temporal(), cam0, FOV, *f0)
    assert np.all(h0.H[..., 3] == 1.0) and same(h0.H[..., :3], f0[0][..., :3])
    h1 = emu.step(abi.temporal(), cam1, FOV, *f1, hist=h0)
    fresh = h1.H[..., 3] == 1.0
    cols = np.flatnonzero(fresh.all(0))
    assert len(cols) == abs(k) and (np.array_equal(cols, np.arange(abs(k))) or np.array_equal(cols, np.arange(W - abs(k), W))), cols
    assert np.all(h1.H[..., 3][~fresh] == 2.0) and not fresh[:, [c for c in range(W) if c not in cols]].any()
    assert same(h1.H[..., :3][fresh], f1[0][..., :3][fresh])  # bit for bit
    # ... and the history came from the column k away: against the restatement
    r = temporal64(*f1, cam1, FOV, hist=h0)
    assert np.array_equal(r["H"][..., 3], h1.H[..., 3]) and np.abs(r["H"][..., :3] - h1.H[..., :3]).max() < 1e-3


# ---- rejection -----------------------------------------------------------------------------------------------------------------------
def two_regions(rng, cam, split, what):
    """A frame whose columns >= split are region B: another instance, a depth step of 2.5 x the tolerance, or a flipped normal."""
    b = (np.mgrid[0:H, 0:W][1] >= split)
    depth = np.where(b, 5.0 * (1.0 + 2.5 * 0.02), 5.0) if what == "depth" else 5.0
    inst = np.where(b, 7, 3).astype(np.uint32) if what == "instance" else 3
    normal = np.where(b[..., None], (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)) if what == "normal" else (0.0, 0.0, -1.0)
    return tu.plane_frame(rng, H, W, cam, FOV, depth=depth, inst=inst, normal=normal)


@pytest.mark.parametrize("what", ["instance", "depth", "normal"])
def test_history_never_crosses_an_edge(emu, what):
    """Frame 0 is split at column 16, frame 1 -- the camera half a pixel further in both directions, so every pixel has four taps --
    at column 11: columns 11 .. 14 of frame 1 are region B and all their taps (columns x - 1 .. x + 1) were region A."""
    from gpuspectral_amd import abi

    rng = np.random.default_rng(9)
    zp = tu.zplane64(W, H, FOV)
    cam0, cam1 = tu.camera(), tu.camera(np.arctan(0.5 / zp), np.arctan(0.5 / zp))
    f0, f1 = two_regions(rng, cam0, 16, what), two_regions(rng, cam1, 11, what)
    h0 = emu.step(abi.temporal(), cam0, FOV, *f0)
    h1, kept = emu.step(abi.temporal(), cam1, FOV, *f1, hist=h0, with_kept=True)
    inner = (slice(1, H - 1), slice(11, 15))
    assert np.all(kept[inner] == 0x80) and np.all(h1.H[inner][..., 3] == 1.0) and same(h1.H[inner][..., :3], f1[0][inner][..., :3])
    for cols in (slice(1, 9), slice(18, W - 1)):  # far from both edges: four taps kept
        assert np.all(kept[1:H - 1, cols] == 0x8F) and np.all(h1.H[1:H - 1, cols, 3] == 2.0)
    # the same frames with one region everywhere: history everywhere
    g0, g1 = two_regions(rng, cam0, W, what), two_regions(rng, cam1, W, what)
    h1 = emu.step(abi.temporal(), cam1, FOV, *g1, hist=emu.step(abi.temporal(), cam0, FOV, *g0))
    assert np.all(h1.H[1:H - 1, 1:W - 1, 3] == 2.0)


# ---- background ----------------------------------------------------------------------------------------------------------------------
def test_background_ignores_translation_and_follows_rotation(emu):
    from gpuspectral_amd import abi

    rng = np.random.default_rng(13)
    zp = tu.zplane64(W, H, FOV)
    f0, f1 = tu.background_frame(rng, H, W), tu.background_frame(rng, H, W)
    h0 = emu.step(abi.temporal(), tu.camera(), FOV, *f0)
    assert np.all(h0.I == BACKGROUND) and not h0.G.any()
    h1, kept = emu.step(pure_mean(), tu.camera(eye=(3.0, -2.0, 40.0)), FOV, *f1, hist=h0, with_kept=True)
    assert np.all(kept == 0x81) and np.all(h1.H[..., 3] == 2.0)
    want = 0.5 * (f0[0][..., :3].astype(np.float64) + f1[0][..., :3])
    assert np.abs(h1.H[..., :3] - want).max() <= 4 * U32 * RANGE
    cam = tu.camera(np.arctan(3 / zp))
    h2 = emu.step(pure_mean(), cam, FOV, *f1, hist=h0)
    fresh = h2.H[..., 3] == 1.0
    assert fresh.all(0).sum() == 3 and fresh.sum() == 3 * H
    r = temporal64(*f1, cam, FOV, hist=h0, alpha=FLT_MIN)
    assert np.array_equal(r["H"][..., 3], h2.H[..., 3]) and np.abs(r["H"][..., :3] - h2.H[..., :3]).max() < 1e-3
    assert np.abs(h2.H[..., :3] - h1.H[..., :3]).max() > 0.1  # not the unshifted blend
    # a surface where the history is background, and the reverse: no history
    s1 = tu.plane_frame(rng, H, W, tu.camera(), FOV)
    assert np.all(emu.step(abi.temporal(), tu.camera(), FOV, *s1, hist=h0).H[..., 3] == 1.0)
    hs = emu.step(abi.temporal(), tu.camera(), FOV, *s1)
    assert np.all(emu.step(abi.temporal(), tu.camera(), FOV, *f1, hist=hs).H[..., 3] == 1.0)


# ---- edge cases ----------------------------------------------------------------------------------------------------------------------
def test_non_finite_pixels(emu):
    from gpuspectral_amd import abi

    rng = np.random.default_rng(17)
    cam = tu.camera()
    f0, f1, f2 = (tu.plane_frame(rng, H, W, cam, FOV) for _ in range(3))
    bad = [(2, 3, np.nan), (4, 5, np.inf), (6, 7, -np.inf)]
    h0 = emu.step(pure_mean(), cam, FOV, *f0)
    for y, x, v in bad:
        f1[0][y, x, y % 3] = v
    h1 = emu.step(pure_mean(), cam, FOV, *f1, hist=h0)
    for y, x, _ in bad:  # with history: prev and len kept
        assert same(h1.H[y, x], h0.H[y, x])
    assert np.all(np.delete(h1.H[..., 3].reshape(-1), [y * W + x for y, x, _ in bad]) == 2.0)
    n0 = emu.step(pure_mean(), cam, FOV, *f1)  # without history: len 0, the record itself
    for y, x, _ in bad:
        assert n0.H[y, x, 3] == 0.0 and same(n0.H[y, x, :3], f1[0][y, x, :3])
    n1 = emu.step(pure_mean(), cam, FOV, *f2, hist=n0)  # ... and it is nobody's history
    for y, x, _ in bad:
        assert n1.H[y, x, 3] == 1.0 and same(n1.H[y, x, :3], f2[0][y, x, :3])
    assert np.isfinite(n1.H).all()


def test_behind_the_previous_camera_is_no_history(emu):
    from gpuspectral_amd import abi

    rng = np.random.default_rng(19)
    f0 = tu.plane_frame(rng, H, W, tu.camera(), FOV)
    back = tu.camera(np.pi)
    f1 = tu.plane_frame(rng, H, W, back, FOV, depth=-5.0, normal=(0.0, 0.0, 1.0))
    h1, kept = emu.step(abi.temporal(), back, FOV, *f1, hist=emu.step(abi.temporal(), tu.camera(), FOV, *f0), with_kept=True)
    assert not kept.any() and np.all(h1.H[..., 3] == 1.0) and same(h1.H[..., :3], f1[0][..., :3])


@pytest.mark.parametrize("size", [(1, 1), (5, 3)])
def test_small_frames(emu, size):
    from gpuspectral_amd import abi

    w, h = size
    rng = np.random.default_rng(23)
    zp = tu.zplane64(w, h, FOV)
    cam0, cam1 = tu.camera(), tu.camera(np.arctan(0.25 / zp), np.arctan(-0.25 / zp))
    f0, f1 = tu.plane_frame(rng, h, w, cam0, FOV), tu.plane_frame(rng, h, w, cam1, FOV)
    h0 = emu.step(abi.temporal(), cam0, FOV, *f0)
    h1 = emu.step(abi.temporal(), cam1, FOV, *f1, hist=h0)
    r = temporal64(*f1, cam1, FOV, hist=h0)
    assert np.array_equal(r["H"][..., 3], h1.H[..., 3]) and np.all(h1.H[..., 3] == 2.0)
    assert np.abs(r["H"][..., :3] - h1.H[..., :3]).max() < 1e-3 and same(r["G"], h1.G) and np.array_equal(r["I"], h1.I)
    h2 = emu.step(abi.temporal(), cam0, FOV, *f0, hist=h0)
    assert np.all(h2.H[..., 3] == 2.0)


@pytest.mark.parametrize("fields", [dict(alpha=1.0), dict(max_history=1)], ids=["alpha-1", "max-history-1"])
def test_alpha_1_and_max_history_1_equal_no_history(emu, fields):
    """a = 1: H' = prev + (c - prev) * 1, which is c up to the roundings of the difference and of the sum (u (|c| + |prev|) in all)."""
    from gpuspectral_amd import abi

    rng = np.random.default_rng(29)
    cam = tu.camera()
    f0, f1 = tu.plane_frame(rng, H, W, cam, FOV), tu.plane_frame(rng, H, W, cam, FOV)
    h1 = emu.step(abi.temporal(**fields), cam, FOV, *f1, hist=emu.step(abi.temporal(**fields), cam, FOV, *f0))
    assert np.abs(h1.H[..., :3].astype(np.float64) - f1[0][..., :3]).max() <= 2 * U32 * (2 * RANGE)
    assert np.all(h1.H[..., 3] == (1.0 if "max_history" in fields else 2.0))


def test_singular_previous_camera(emu):
    from gpuspectral_amd import abi

    rng = np.random.default_rng(31)
    flat = tu.camera().copy()
    flat[10] = 0.0  # a to_world whose z column is zero
    f = tu.plane_frame(rng, H, W, tu.camera(), FOV)
    h0 = emu.step(abi.temporal(), tu.camera(), FOV, *f)
    h0.to_world = flat
    with pytest.raises(ValueError, match="singular"):
        emu.step(abi.temporal(), tu.camera(), FOV, *f, hist=h0)


# ---- agreement with the restatement on the Cornell box ---------------------------------------------------------------------------------
# Bound.  The reprojected position goes through ~20 float32 operations on numbers up to max(W, H) (pixels) and up to the scene's
# extent (world units, mapped to pixels by zplane / l.z <= a few hundred here), so it carries at most ~64 u * max(W, H) of a pixel:
# dp = 64 u * 128 = 4.9e-4.  A bilinear weight moves by at most 2 dp, the four of them by 8 dp in sum, and prev = s / sw moves by at
# most 8 dp / sw * max |H_q| (numerator) plus the same again (denominator).  The blend and the sums add a few u of max(|c|, |H_q|).
AGREE_SEEDS = (1, 2, 3, 4)  # checked on the build machine: the share of pixels left out stays under 0.5 % for each


def cornell_frames(cornell, seed, n=3, size=128):
    import features_util as fu

    rng = np.random.default_rng(seed)
    img = np.load(os.path.join(GOLDEN, "cornell_128_1spp.npy")).reshape(128, 128, 3)
    femu = fu.FeaturesEmu()
    out = []
    to_world = np.asarray(cornell.to_world, np.float32).copy()
    for _ in range(n):
        sc = copy.copy(cornell)
        sc.to_world = to_world.copy()
        a, g, i = fu.full(femu.scene(sc).render(size, size, 1), size, size)
        c = np.ones((size, size, 4), np.float32)
        c[..., :3] = img * rng.uniform(0.5, 1.5, (size, size, 1))
        out.append((to_world.copy(), (c, a, g, i)))
        # a smooth move: a degree or two about y through the room's middle, a small step of the eye
        to_world = tu.rotated_about_y(to_world, rng.uniform(-2.5, 2.5), pivot=(0.0, 1.0, 0.0))
        to_world[12:15] += rng.uniform(-0.05, 0.05, 3).astype(np.float32)
    return out


@pytest.mark.parametrize("seed", AGREE_SEEDS)
def test_emulation_agrees_with_the_restatement_on_cornell(emu, cornell, seed):
    from gpuspectral_amd import abi

    fov = float(cornell.fov)
    frames = cornell_frames(cornell, seed)
    hist = None
    for k, (cam, f) in enumerate(frames):
        new, kept = emu.step(abi.temporal(), cam, fov, *f, hist=hist, with_kept=True)
        r = temporal64(*f, cam, fov, hist=hist)
        assert same(r["G"], new.G) and np.array_equal(r["I"], new.I)
        agree = (r["kept"] == kept) & ~r["fragile"]
        left_out = 1.0 - agree.mean()
        dp = 64 * U32 * 128
        big = float(np.abs(hist.H).max()) if hist is not None else 0.0
        bound = 2 * 8 * dp / np.maximum(r["sw"], 0.01) * big + 16 * U32 * max(big, float(np.abs(f[0][..., :3]).max()))
        dev = np.abs(new.H.astype(np.float64) - r["H"]).max(-1)
        print("seed %d frame %d: %.3f %% of the pixels left out, largest deviation %.3e (bound there %.3e), mean history length %.2f"
              % (seed, k, 100 * left_out, dev[agree].max(), bound[agree][np.argmax(dev[agree])], new.H[..., 3].mean()))
        assert left_out <= 0.005
        assert np.all(dev[agree] <= bound[agree])
        if k:
            assert new.H[..., 3].mean() > 1.5  # most of the frame found its history
        hist = new
