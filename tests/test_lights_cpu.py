"""Light selection without a GPU (include/gpuspectral_pt.h, "Light selection"): the product's table builder (pt_lightpick.h) and
shade_vertex<.., LSEL = true> compiled for the host (tests/emu/lights_emu.cpp) against a float64 restatement of the definition,
against the uniform mode's frames, against an analytic direct-light integral, and the variance the power pick removes."""
import os
import subprocess

import numpy as np
import pytest

import lights_util as lu
from conftest import ROOT


@pytest.fixture(scope="module")
def emu():
    return lu.LightsEmu()


def _weight_vectors():
    rng = np.random.RandomState(11)
    out = {}
    for n in (1, 2, 3, 66, 336, 4096):
        w = 10.0 ** rng.uniform(-6.0, 4.0, n)
        if n >= 3:
            w[rng.choice(n, max(1, n // 7), replace=False)] = 0.0  # zeros among them
        out[n] = w
    out["weak+strong"] = lu.weak_and_strong_weights()
    return out


WEIGHTS = _weight_vectors()


# ---- the table against the definition ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(WEIGHTS), ids=[str(k) for k in WEIGHTS])
def test_table_implies_the_weights(emu, key):
    """sum p = 1 to 1e-12; p_i = 0 exactly where w_i = 0; |p_i - w_i / sum(w)| <= (1 + d_i) / (n 2^32): each threshold is rounded by
    at most half a unit of 2^-32 / n, and entry i collects its own and those of the d_i entries aliased to it; the bound leaves
    twice that for the double arithmetic.  The stored pmfs are float32 of p, p computed HERE from the integer table."""
    w = WEIGHTS[key]
    n = len(w)
    t = emu.build_weights(w)
    p, d = lu.implied_pmf(t)
    want = w / w.sum()
    err = np.abs(p - want) * n * lu.TWO32
    print("n = %d: sum p - 1 = %.2e, largest error %.2f units of 2^-32 / n, largest d %d" % (n, p.sum() - 1.0, err.max(), d.max()))
    assert abs(p.sum() - 1.0) <= 1e-12
    assert (p[w == 0.0] == 0.0).all() and (t["threshold"][w == 0.0] == 0).all()
    assert not np.isin(np.flatnonzero(w == 0.0), t["alias"][t["alias"] != np.arange(n)]).any()  # nobody's alias
    assert (err <= 1.0 + d).all()
    assert (t["alias"] < n).all()
    sat = t["threshold"] == 0xFFFFFFFF
    assert (t["alias"][sat] == np.flatnonzero(sat)).all()
    assert np.array_equal(t["pmf_self"], p.astype(np.float32))
    assert np.array_equal(t["pmf_alias"], p[t["alias"]].astype(np.float32))


def test_weights_from_records(emu):
    """w = max(Y, 0) * area from the caller's records, in double; non-finite -> 0."""
    sc = lu.room_scene(130)
    lt = sc.lights.copy()
    lt["radiance"][5, :3] = (-1.0, -2.0, -3.0)  # negative luminance -> 0
    lt["radiance"][6, 0] = np.inf
    lt["radiance"][7, 1] = np.nan
    lt["positions"][8, 1, :3] = lt["positions"][8, 0, :3]  # degenerate: area 0
    want = lu.weights64(lt)
    got = emu.weights(lt)
    assert (want[[5, 6, 7, 8]] == 0.0).all() and (want > 0).sum() == 126
    assert np.allclose(got, want, rtol=1e-14, atol=0.0)
    t = emu.build(lt)
    p, d = lu.implied_pmf(t)
    assert (p[[5, 6, 7, 8]] == 0.0).all()
    assert (np.abs(p - want / want.sum()) * 130 * lu.TWO32 <= 1.0 + d).all()


def test_table_is_deterministic(emu):
    for w in WEIGHTS.values():
        assert emu.build_weights(w).tobytes() == emu.build_weights(w.copy()).tobytes()


def test_all_zero_and_non_finite_weights(emu):
    for w in (np.zeros(5), np.array([np.nan, np.inf, -np.inf, -1.0, 0.0])):
        t = emu.build_weights(w)
        p, _ = lu.implied_pmf(t)
        assert np.array_equal(p, np.full(5, 0.2))  # every weight became 1
        assert (t["threshold"] == 0xFFFFFFFF).all() and np.array_equal(t["alias"], np.arange(5))
    t = emu.build_weights(np.array([np.nan, 2.0, np.inf, 6.0]))
    p, _ = lu.implied_pmf(t)
    assert p[0] == 0.0 and p[2] == 0.0 and abs(p[1] - 0.25) <= 2.0 / (4 * lu.TWO32) and abs(p[3] - 0.75) <= 4.0 / (4 * lu.TWO32)


def test_one_light(emu):
    t = emu.build_weights(np.array([3.5]))
    assert (int(t["threshold"][0]), int(t["alias"][0]), float(t["pmf_self"][0]), float(t["pmf_alias"][0])) == (0xFFFFFFFF, 0, 1.0, 1.0)


def test_very_weak_light_is_dropped(emu):
    """A share below about 2^-33 / n rounds to threshold 0: the documented loss."""
    t = emu.build_weights(np.array([1.0, 1e-12, 1.0]))
    p, _ = lu.implied_pmf(t)
    assert t["threshold"][1] == 0 and p[1] == 0.0


# ---- the pick rule -----------------------------------------------------------------------------------------------------------------
def test_pick_rule_counts(emu):
    """M = 2^22 evenly spaced draws over 66 lights (64 weak + 2 strong): the product's counts are those of the rule restated in numpy
    integers, exactly; and lie within 2 n / M of the table's p (each slot's interval of r has two borders, each border misplaces at
    most one draw)."""
    w = lu.weak_and_strong_weights()
    t = emu.build_weights(w)
    M = 1 << 22
    r = (np.arange(M, dtype=np.uint64) << np.uint64(10)).astype(np.uint32)
    counts, pmf = emu.pick(t, r)
    k = lu.pick64(t, r)
    assert np.array_equal(counts.astype(np.int64), np.bincount(k, minlength=len(t)))
    p, _ = lu.implied_pmf(t)
    dev = np.abs(counts / M - p).max()
    print("largest |count / M - p| = %.2e, bound %.2e" % (dev, 2 * len(t) / M))
    assert dev <= 2 * len(t) / M
    assert np.array_equal(pmf, p.astype(np.float32)[k])  # the pdf handed back is the picked light's


# ---- structure ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rooms(emu):
    """{lights: (scene, emulation, uniform (frame, stats), power (frame, stats))}: 3 lights (table image within LDS reach on the
    device), 130 (beyond it), rendered once."""
    out = {}
    for n in (1, 3, 130):
        sc = lu.room_scene(n)
        es = emu.scene(sc)
        out[n] = (sc, es, es.render(40, 32, 4, mode=lu.UNIFORM), es.render(40, 32, 4, mode=lu.POWER))
    return out


def test_uniform_mode_is_the_emulation_of_old(emu, rooms):
    """lights_emu_render in uniform mode is emu_render (the harness adds nothing of its own)."""
    import ctypes as C

    sc, es, (uni, _), _ = rooms[130]
    p = emu.abi.default_render_params()
    p.spp = 4
    ref = np.zeros((40 * 32, 4), np.float32)
    emu.L.emu_render.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(emu.abi.RenderParams), C.c_void_p]
    assert emu.L.emu_render(es.h, 40, 32, None, 40 * 32, C.byref(p), ref.ctypes.data) == 0
    assert lu.same(ref, uni)


def test_one_light_modes_coincide(rooms):
    """pmf = 1.0f = inv_num_lights and j = 0: bit for bit."""
    _, _, (uni, su), (pw, sp) = rooms[1]
    assert lu.same(uni, pw) and su["shadow_rays"] == sp["shadow_rays"] and uni[:, :3].max() > 0.0


@pytest.mark.parametrize("n", [3, 130])
def test_without_nee_modes_coincide(rooms, n):
    _, es, _, _ = rooms[n]
    a, sa = es.render(40, 32, 2, mode=lu.UNIFORM, disable_nee=1)
    b, sb = es.render(40, 32, 2, mode=lu.POWER, disable_nee=1)
    assert lu.same(a, b) and sa["shadow_rays"] == sb["shadow_rays"] == 0


@pytest.mark.parametrize("n", [3, 130])
def test_only_the_shadow_rays_differ(rooms, n):
    _, _, (uni, su), (pw, sp) = rooms[n]
    assert su["extension_rays"] == sp["extension_rays"] and su["shaded_vertices"] == sp["shaded_vertices"]
    assert not lu.same(uni, pw)  # (the pick does change the frame)
    assert np.isfinite(pw).all() and pw[:, :3].min() >= 0.0


# ---- expectation -------------------------------------------------------------------------------------------------------------------
def test_both_modes_estimate_the_analytic_direct_light(emu):
    """A diffuse floor under 16 small lights at height h = 10 (areas A 1e-4 .. 1e-1, luminances 100 .. 1), clamp 1e30, no Russian
    roulette.  A floor vertex continues along a cosine-distributed direction; it meets a light with probability
    sum_i A_i cos cos' / (pi d^2) <= sum(A) / (pi h^2) = 0.271 / 314 = 8.6e-4, and the emission it then collects carries the
    emitter-hit weight power_heuristic(bsdf pdf, pdf of the floor vertex's NEE sample) <= (bsdf pdf / light pdf)^2 with
    bsdf pdf <= 1 / pi and light pdf = d^2 / (cos' A_k) * pmf_k >= h^2 pmf_k / A_k: uniform, pmf = 1 / 16 and A <= 0.1 give
    >= 62.5, so the weight is <= (0.318 / 62.5)^2 = 2.6e-5; power, pmf_k / A_k = Y_k / sum(Y A) >= 1 / 0.643 gives >= 155 and
    4.2e-6.  The emitter-hit term is the direct light times a weight below 3e-5, and NEE carries the rest with an MIS weight above
    1 - 3e-5: both modes estimate rho / pi sum Le integral cos cos' / d^2 dA to 3e-5, far below the standard error here (about 1 %).
    The per-pixel means over 4096 timestamps agree with the float64 quadrature and with each other within 4 standard errors of the
    mean, the errors estimated from the samples themselves."""
    W = H = 16
    N = 4096
    sc = lu.expectation_scene()
    ref = lu.direct_light64(sc, W, H)
    assert (ref > 0.0).all()
    es = emu.scene(sc)
    means, ses = [], []
    for mode in (lu.UNIFORM, lu.POWER):
        _, st, m = es.render(W, H, N, mode=mode, moments=True, clamp=1e30, rr_start_depth=255)
        mean = m[:, :3] / N
        se = np.sqrt(np.maximum(m[:, 3:] / N - mean * mean, 0.0) / (N - 1))
        z = np.abs(mean - ref) / se
        print("mode %d: largest |mean - analytic| = %.2f standard errors; frame mean / analytic = %s" % (mode, z.max(), mean.mean(0) / ref.mean(0)))
        assert st["nee_cut"] == 0 and (se > 0.0).all()
        assert z.max() <= 4.0
        means.append(mean)
        ses.append(se)
    z = np.abs(means[0] - means[1]) / np.sqrt(ses[0] ** 2 + ses[1] ** 2)
    print("uniform against power: %.2f standard errors" % z.max())
    assert z.max() <= 4.0


# ---- variance ----------------------------------------------------------------------------------------------------------------------
# measured on the emulation (32 x 32, 64 spp, clamp 1e30): summed per-pixel sample variance 144.74 (uniform) / 0.004863 (power)
MEASURED_VARIANCE_RATIO = 29762.0


def test_power_pick_removes_the_selection_variance(emu):
    """The fan and quad: 64 fan triangles hold 1 % of sum(w), 2 quad triangles 99 %, n sum(p^2) = 32.3 (the factor between the
    second moments of the light choice).  Summed per-pixel sample variance of the uniform frame over that of the power frame at
    equal spp.  The VARIANCE ratio is far above the second-moment factor: with the power pick nearly every sample of a pixel lands on
    the quad with the same pdf, so what is left is the variation of the integrand over the quad (the lights are 0.2 across, 4 away)
    and the 1 % of samples on the fan.  The test asks for half the measured ratio (a ratio of two noisy sums)."""
    sc = lu.fan_and_quad_scene()
    w = lu.weights64(sc.lights)
    p = w / w.sum()
    assert abs(len(p) * (p * p).sum() - 32.3) < 0.1 and abs(p[:64].sum() - 0.01) < 1e-6
    es = emu.scene(sc)
    var, second = [], []
    for mode in (lu.UNIFORM, lu.POWER):
        _, st, m = es.render(32, 32, 64, mode=mode, moments=True, clamp=1e30)
        mean = m[:, :3] / 64
        var.append(float((m[:, 3:] / 64 - mean * mean).sum()))
        second.append(float((m[:, 3:] / 64).sum()))
    ratio = var[0] / var[1]
    print("summed sample variance: uniform %.4g, power %.4g, ratio %.1f; second moments %.4g / %.4g = %.1f" % (var[0], var[1], ratio, second[0], second[1], second[0] / second[1]))
    assert ratio >= 0.5 * MEASURED_VARIANCE_RATIO


# ---- the builder under the sanitizers ----------------------------------------------------------------------------------------------
def test_builder_standalone_under_asan_ubsan(tmp_path):
    """tests/emu/lightpick_main.cpp (its own main): the builder over random and degenerate weight vectors, n = 1 .. 4096, compiled
    with -fsanitize=address,undefined and run on the CPU; it re-checks every table's invariants itself."""
    exe = tmp_path / "lightpick_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "emu", "lightpick_main.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "tables ok" in out.stdout
