"""Temporal anti-aliasing on the CPU (include/gpuspectral_pt.h, "Temporal anti-aliasing"): the library's per-pixel text
(csrc/pt_taa.h through tests/emu/taa_emu.cpp) against the float32 restatement of tests/taa_util.py bit for bit, against known
answers, its containment in the neighbourhood box, what it does to a shimmering edge and to a disocclusion, its validation, and
the emulation as a program of its own under the sanitizers.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import taa_util as tu
from display_util import DisplayEmu
from illum_util import IllumEmu
from taa_util import TaaEmu
from temporal_util import same
from test_antilag_cpu import FRAMES, H, W, cornell_frames

TONEMAPS = {
    "clamp": dict(tonemap=0),
    "aces": dict(tonemap=2, exposure=0.5),
    "reinhard-measured": dict(tonemap=1),
    "reinhard-fixed": dict(tonemap=1, log_avg_luminance=0.21, max_luminance=3.5, key=0.3, burn=0.2),
}
GAMMAS = {"srgb": 0.0, "gamma2.2": 2.2}
PARAMS = {"defaults": (0.0, 0.0), "a0.2-s2": (0.2, 2.0), "a1-s0.5": (1.0, 0.5)}


@pytest.fixture(scope="module")
def emu():
    return TaaEmu()


@pytest.fixture(scope="module")
def demu():
    return DisplayEmu()


def make_display(tonemap, gamma):
    from gpuspectral_amd import abi

    return abi.display(gamma=GAMMAS[gamma], **TONEMAPS[tonemap])


_SEQ = {}


def cornell_sources(cornell, kind):
    """The golden Cornell sequence of tests/test_antilag_cpu.py through the accumulate's emulation with following on: per frame
    (src, V).  kind "colour": the frame's raw noisy colour; "image": the image read-out of the demodulated history."""
    if kind not in _SEQ:
        acc = IllumEmu()
        fov = float(cornell.fov)
        demod = kind == "image"
        hist, out = None, []
        for cam, xf, f in cornell_frames(cornell):
            new = acc.step(None, cam, fov, *f, xforms=xf, hist=hist, moments=False, demod=demod)
            out.append((acc.image(new.H, f[1], demod=True) if demod else f[0], new.V))
            hist = new
        _SEQ[kind] = out
    return _SEQ[kind]


# ---- the emulation against the restatement, bit for bit ----------------------------------------------------------------------------------
@pytest.mark.parametrize("params", PARAMS)
@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("tonemap", TONEMAPS)
@pytest.mark.parametrize("kind", ["colour", "image"])
def test_emulation_equals_the_restatement(emu, demu, cornell, kind, tonemap, gamma, params):
    from gpuspectral_amd import abi

    alpha, sigma = PARAMS[params]
    taa = abi.taa(alpha, sigma) if alpha else None
    disp = make_display(tonemap, gamma)
    prev = prev_ref = None
    used = clipped = 0
    seq = cornell_sources(cornell, kind)
    assert len(seq) == FRAMES
    for k, (src, V) in enumerate(seq):
        assert src.shape == (H, W, 4) and (k == 0 or (V[..., 3] != 0).mean() > 0.5)
        D, words = emu.step(taa, disp, src, V, prev)
        r = tu.taa_ref(src, V, prev_ref, alpha, sigma, disp, demu)
        assert same(D, r["D"]), "frame %d: %d pixels differ" % (k, (D.view(np.uint32) != r["D"].view(np.uint32)).any(-1).sum())
        assert np.array_equal(words, r["words"])
        assert np.array_equal(D[..., 3] == 1.0, r["history"]) and (k > 0 or not r["history"].any())
        used += int(r["history"].sum())
        clipped += int((r["history"][..., None] & ((r["Hc"] < r["lo"]) | (r["Hc"] > r["hi"]))).any(-1).sum())
        prev, prev_ref = D, r["D"]
    assert used > 0.5 * (FRAMES - 1) * W * H and clipped > 20  # (the history is used, and the box acts)


# ---- known answers ------------------------------------------------------------------------------------------------------------------------
def still(h, w, sw=1.0, cls=1.0):
    V = np.zeros((h, w, 4), np.float32)
    V[..., 2], V[..., 3] = sw, cls
    return V


def test_first_resolve_is_the_toned_frame(emu, demu):
    rng = np.random.default_rng(5)
    src = rng.uniform(-0.2, 2.5, (9, 13, 4)).astype(np.float32)
    src[2, 3, 0], src[4, 5, 1] = np.nan, np.inf
    disp = make_display("aces", "srgb")
    D, words = emu.step(None, disp, src, still(9, 13), None)
    r, g, b = tu.tone(src, demu.consts(disp, src))
    expect = np.stack([tu.clamp01(c) for c in tu.rgb(*tu.ycocg(r, g, b))] + [np.zeros((9, 13), np.float32)], -1)
    assert same(D, expect) and not D[..., 3].any()
    assert np.isfinite(D).all() and D[..., :3].min() >= 0.0 and D[..., :3].max() <= 1.0


def test_unmoved_constant_source_is_a_fixed_point(emu):
    """The constant is dyadic -- (0.25, 0.5, 0.75), tests/test_antilag_cpu.py's -- so that its YCoCg (0.5, -0.25, 0), the nine-term
    sums, their mean and the variance 0 are exact in float32 and the answer is known to the bit: the box is the point X, the
    history is X, frame 2 is frame 1.  A constant that is not exactly representable leaves roundings of the sums in the box: it
    comes back within a few ulp, held here to 1e-6."""
    src = np.tile(np.float32([0.25, 0.5, 0.75, 1.0]), (7, 11, 1))
    D1, w1 = emu.step(None, None, src, still(7, 11), None)
    D2, w2 = emu.step(None, None, src, still(7, 11), D1)
    assert same(D1[..., :3], src[..., :3])
    assert same(D2[..., :3], D1[..., :3]) and (D2[..., 3] == 1.0).all() and not D1[..., 3].any()
    assert np.array_equal(w1, w2)
    src = np.tile(np.float32([0.3, 0.55, 0.2, 1.0]), (7, 11, 1))
    D1, _ = emu.step(None, None, src, still(7, 11), None)
    D2, _ = emu.step(None, None, src, still(7, 11), D1)
    assert np.abs(D2[..., :3].astype(np.float64) - D1[..., :3]).max() <= 1e-6 and (D2[..., 3] == 1.0).all()


def test_alpha_one_is_the_frame(emu):
    from gpuspectral_amd import abi

    rng = np.random.default_rng(6)
    src = rng.uniform(0.0, 1.5, (8, 12, 4)).astype(np.float32)
    prev = rng.uniform(0.0, 1.0, (8, 12, 4)).astype(np.float32)
    V = still(8, 12)
    V[..., :2] = rng.uniform(-1.5, 1.5, (8, 12, 2))
    none, _ = emu.step(None, None, src, V, None)
    one, _ = emu.step(abi.taa(alpha=1.0), None, src, V, prev)
    assert same(one[..., :3], none[..., :3]) and (one[..., 3] == 1.0).mean() > 0.8


def test_pixels_without_a_history(emu):
    rng = np.random.default_rng(7)
    h, w = 6, 10
    src = rng.uniform(0.0, 1.0, (h, w, 4)).astype(np.float32)
    prev = rng.uniform(0.0, 1.0, (h, w, 4)).astype(np.float32)
    V = still(h, w)
    V[1, 1, 3] = 0.0  # cls == 0
    V[2, 2, 2] = 0.009  # sw < 0.01
    V[3, 3, :2] = (-5.0, 0.0)  # all four taps left of the frame
    V[4, 9, :2] = (1.0, 0.0)  # x0 = W: right of it
    V[0, 4, :2] = (0.0, -1.0)  # y0 = -1 with wy = 0: both kept taps would lie above the frame
    V[5, 5, :2] = (0.25, 0.5)
    D, _ = emu.step(None, None, src, V, prev)
    none, _ = emu.step(None, None, src, V, None)
    gone = np.zeros((h, w), bool)
    for y, x in ((1, 1), (2, 2), (3, 3), (4, 9), (0, 4)):
        gone[y, x] = True
    assert np.array_equal(D[..., 3] == 0.0, gone)
    assert same(D[gone], none[gone])
    # a tap of weight 0 is skipped, not multiplied: a NaN next to an integer fetch position does not reach the pixel
    prev[2, 6] = np.nan
    D, _ = emu.step(None, None, src, V, prev)
    assert np.isfinite(D[2, 5]).all() and D[2, 5, 3] == 1.0 and np.isfinite(D[1, 6]).all()


# ---- containment ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", PARAMS)
def test_blend_stays_between_the_box_and_the_frame(emu, demu, cornell, params):
    """Before the final clamp every YCoCg channel of o lies in [min(lo, X_p), max(hi, X_p)] up to 1e-6, in float64.  o is read off
    the emulation's D' where the final clamp did not act (every channel strictly inside (0, 1): rgb -> YCoCg of a float32 triple
    adds at most a few 1e-7) and the box off the restatement, which the test above holds to the emulation bit for bit."""
    from gpuspectral_amd import abi

    alpha, sigma = PARAMS[params]
    taa = abi.taa(alpha, sigma) if alpha else None
    disp = make_display("aces", "srgb")
    prev, checked = None, 0
    for src, V in cornell_sources(cornell, "colour"):
        D, _ = emu.step(taa, disp, src, V, prev)
        r = tu.taa_ref(src, V, prev, alpha, sigma, disp, demu)
        d = D[..., :3].astype(np.float64)
        o = np.stack([0.25 * d[..., 0] + 0.5 * d[..., 1] + 0.25 * d[..., 2], 0.5 * d[..., 0] - 0.5 * d[..., 2], -0.25 * d[..., 0] + 0.5 * d[..., 1] - 0.25 * d[..., 2]], -1)
        inside = r["history"] & ((D[..., :3] > 0.0) & (D[..., :3] < 1.0)).all(-1)
        X, lo, hi = (r[n].astype(np.float64) for n in ("X", "lo", "hi"))
        assert np.all(o[inside] >= np.minimum(lo, X)[inside] - 1e-6) and np.all(o[inside] <= np.maximum(hi, X)[inside] + 1e-6)
        checked += int(inside.sum())
        prev = D
    assert checked > 2 * W * H


# ---- it anti-aliases and it does not ghost ------------------------------------------------------------------------------------------------------
LEFT, RIGHT = np.float32([0.9, 0.7, 0.5]), np.float32([0.1, 0.1, 0.2])


def edge_frame(rng, edge, noise=True):
    """A vertical edge at x = edge, every pixel evaluated at x + u, u uniform in [0, 1) per pixel and frame (u = 0.5 without noise),
    every channel times 1 + 0.05 uniform(-1, 1)."""
    x = np.arange(W)[None, :] + (rng.uniform(0.0, 1.0, (H, W)) if noise else 0.5)
    c = np.where((x < edge)[..., None], LEFT, RIGHT).astype(np.float64)
    if noise:
        c = c * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, (H, W, 3)))
    out = np.ones((H, W, 4), np.float32)
    out[..., :3] = c
    return out


def test_it_settles_an_edge_and_does_not_ghost(emu):
    rng = np.random.default_rng(2024)
    V = still(H, W)
    prev = None
    srcs, outs = [], []
    for k in range(40):
        src = edge_frame(rng, 20.37)
        prev, _ = emu.step(None, None, src, V, prev)
        srcs.append(src[..., 1])
        outs.append(prev[..., 1])
    srcs, outs = np.asarray(srcs[12:], np.float64), np.asarray(outs[12:], np.float64)
    sd_src, sd_out = srcs[:, :, 20].std(0).mean(), outs[:, :, 20].std(0).mean()
    mean = outs[:, :, 20].mean()
    print("column 20, green: temporal sd %.4f of the source's %.4f (ratio %.3f), resolved mean %.4f (coverage value 0.322)" % (sd_out, sd_src, sd_out / sd_src, mean))
    assert sd_out < 0.30 * sd_src  # (a)
    assert abs(mean - (0.6 * 0.37 + 0.1)) < 0.02  # (b)
    # (c) after ten frames the edge jumps to x = 10.0 with the noise off: columns 12..18 were lit and are dark at once
    prev = None
    for k in range(10):
        prev, _ = emu.step(None, None, edge_frame(rng, 20.37), V, prev)
    src = edge_frame(rng, 10.0, noise=False)
    D, _ = emu.step(None, None, src, V, prev)
    dev = np.abs(D[:, 12:19, :3].astype(np.float64) - src[:, 12:19, :3]).max()
    print("disocclusion: largest |D' - source| over columns 12..18 on the next frame %.3g" % dev)
    assert (D[:, 12:19, 3] == 1.0).all() and dev <= 1e-6


# ---- validation ------------------------------------------------------------------------------------------------------------------------------
def test_resolve_taa(emu):
    from gpuspectral_amd import abi

    assert emu.resolve(None) == (dict(alpha=float(np.float32(0.1)), sigma_clip=1.0), None)
    assert emu.resolve(abi.Taa()) == (dict(alpha=float(np.float32(0.1)), sigma_clip=1.0), None)  # struct_size 0: every default
    assert emu.resolve(abi.taa(1.0, 0.5)) == (dict(alpha=1.0, sigma_clip=0.5), None)
    short = abi.taa(0.5, -1.0)
    short.struct_size = 8  # (a host whose header ends after alpha: sigma_clip is not read)
    assert emu.resolve(short) == (dict(alpha=0.5, sigma_clip=1.0), None)
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        assert emu.resolve(abi.taa(alpha=bad)) == (None, "gsp_taa.alpha must be 0 (the default, 0.1) or within (0, 1]")
    for bad in (-1.0, float("nan"), float("inf")):
        assert emu.resolve(abi.taa(sigma_clip=bad)) == (None, "gsp_taa.sigma_clip must be 0 (the default, 1.0) or positive and finite")
    with pytest.raises(ValueError, match="gsp_display.tonemap"):
        emu.step(None, abi.display(tonemap=7), np.zeros((2, 2, 4), np.float32), np.zeros((2, 2, 4), np.float32))


# ---- the emulation as a program of its own, under the sanitizers -----------------------------------------------------------------------------------
def test_standalone_program_is_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "taa_main")
    tu.build_main(exe)
    for seed in ("1", "7"):
        p = subprocess.run([exe, seed], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
        assert p.returncode == 0, p.stdout + p.stderr
        assert "pixels blended with their history" in p.stdout and "runtime error" not in p.stderr
