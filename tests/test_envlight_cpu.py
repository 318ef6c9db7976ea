"""The environment light (include/gpuspectral_pt.h, "Environment light") without a GPU: the host builder of the cell table and the
product's stage headers compiled for the host (tests/emu/envlight_emu.cpp).

1. the table: pmfs, the density's integral over the sphere, positivity under the bilinear footprint;
2. the round trip: the shared function called on the sampled direction finds the cell that was picked;
3. the independent value: a diffuse plane under a dim sky with a sun against (albedo / pi) * integral of L cos, from numpy;
4. on against off with an occluder;  5. the gain in RMSE at equal spp;  6. off is the parent, bit for bit."""
import math

import numpy as np
import pytest

import delta_util as du
import envlight_util as eu
import textured

W, H = 32, 24
PLANE = dict(max_depth=0, rr_start_depth=250, clamp=1e30)   # direct light only: the vertex behind the first bounce is never shaded
DEEP = dict(max_depth=50, rr_start_depth=250, clamp=1e30)   # every bounce that matters, no roulette, no firefly cut-off
EXTENT = 4.0


@pytest.fixture(scope="module")
def emu():
    return eu.EnvEmu()


# ---- 1. the table ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", eu.MAP_SIZES, ids=lambda s: "%dx%d" % s)
def test_pmfs_sum_to_one_and_the_density_integrates_to_one(emu, size):
    w, h = size
    env = np.random.RandomState(w).uniform(0.5, 1.5, (h, w, 4)).astype(np.float32)  # (no sun: the bound below is linear in the peak of the density)
    cw, ch, table, weights = emu.cells(env)
    assert (cw, ch) == (min(w, 512), min(h, 256)) and len(table) == cw * ch
    mass = du.pick_pmf(table)                       # what the integer table implies, float64
    assert abs(mass.sum() - 1.0) < 1e-12
    assert np.array_equal(table["pmf_self"], mass.astype(np.float32))  # pmf(cell) is that mass, rounded once
    assert abs(float(table["pmf_self"].astype(np.float64).sum()) - 1.0) <= 2.0 ** -23  # (each rounded by at most 2^-24 relative)
    assert np.allclose(mass, weights / weights.sum(), rtol=0, atol=2.0 / (cw * ch * 2.0 ** 32) * cw * ch)  # the table carries the weights
    # the density of the product's function over a (theta, phi) grid that is NOT aligned with the cells, midpoint rule.  The integrand
    # p sin(theta) is constant inside a cell, so only quadrature boxes cut by a cell border err, each by at most its area times the
    # largest integrand:  (ch + 1) n_phi + (cw + 1) n_theta boxes of (pi / n_theta) (2 pi / n_phi)  ->  the bound below; + float32 rounding
    n_theta, n_phi = min(100 * ch + 1, 2001), min(100 * cw + 3, 20483)
    theta, phi = np.meshgrid((np.arange(n_theta) + 0.5) * math.pi / n_theta, (np.arange(n_phi) + 0.5) * 2.0 * math.pi / n_phi - math.pi, indexing="ij")
    local = np.stack([np.sin(theta) * np.sin(phi), np.cos(theta), -np.sin(theta) * np.cos(phi)], -1).reshape(-1, 3)
    dirs = (local @ eu.rot3(eu.TO_LOCAL)).astype(np.float32)
    rec = emu.record(eu.TO_LOCAL, cw, ch)
    _, density, _ = emu.env_eval(env, eu.TO_LOCAL, table, rec, dirs)
    integral = float((density.astype(np.float64) * np.sin(theta).ravel()).sum() * (math.pi / n_theta) * (2.0 * math.pi / n_phi))
    peak = mass.max() * cw * ch / (2.0 * math.pi ** 2)
    bound = peak * ((ch + 1) * n_phi + (cw + 1) * n_theta) * (math.pi / n_theta) * (2.0 * math.pi / n_phi) + 1e-5
    print("%dx%d: integral %.6f, bound %.3g" % (w, h, integral, bound))
    assert abs(integral - 1.0) <= bound


def test_density_is_positive_wherever_the_lookup_is_not_zero(emu):
    env = np.zeros((8, 16, 4), np.float32)
    env[5, 15, :3] = (3.0, 2.0, 1.0)  # in the last column: its footprint wraps into column 0
    cw, ch, table, _ = emu.cells(env)
    v, u = np.meshgrid((np.arange(256) + 0.5) / 256, (np.arange(512) + 0.5) / 512, indexing="ij")
    lit = (eu.lookup(env, u, v) != 0.0).any(-1).ravel()
    dirs = (eu.local_dirs(u, v).reshape(-1, 3) @ eu.rot3(eu.TO_LOCAL)).astype(np.float32)
    radiance, density, _ = emu.env_eval(env, eu.TO_LOCAL, table, emu.record(eu.TO_LOCAL, cw, ch), dirs)
    assert lit.sum() > 1000 and (~lit).sum() > 1000
    assert (density[lit] > 0.0).all()
    assert (density[(radiance != 0.0).any(1)] > 0.0).all()  # ... and wherever the product's own lookup is not zero


def test_cell_weights_take_the_maximum_over_the_bilinear_footprint(emu):
    env = np.zeros((7, 13, 4), np.float32)
    env[3, 0, :3] = 1.0
    cw, ch, _, weights = emu.cells(env)
    wgt = weights.reshape(ch, cw)
    lit = np.argwhere(wgt > 0)
    assert sorted(map(tuple, lit)) == sorted((j, i) for j in (2, 3, 4) for i in (12, 0, 1))  # the neighbours the filter reaches: wrap in u
    assert np.allclose(wgt[3, 0], math.sin(math.pi * 3.5 / 7) * 0.2126 + math.sin(math.pi * 3.5 / 7) * (0.7152 + 0.0722))
    env[:] = 0.0
    env[0, 4, :3] = 1.0  # bottom row: clamp in v
    wgt = emu.cells(env)[3].reshape(ch, cw)
    assert sorted(map(tuple, np.argwhere(wgt > 0))) == sorted((j, i) for j in (0, 1) for i in (3, 4, 5))


def test_power_weight_is_pi_extent2_times_the_radiant_sum(emu):
    env = eu.random_map(13, 7)
    e64 = env.astype(np.float64)
    y = np.maximum(0.2126 * e64[..., 0] + 0.7152 * e64[..., 1] + 0.0722 * e64[..., 2], 0.0)
    sa = (2 * math.pi / 13) * (math.pi / 7) * np.sin(math.pi * (np.arange(7) + 0.5) / 7)
    want = math.pi * 2.5 ** 2 * (y * sa[:, None]).sum()
    assert abs(emu.power_weight(env, 2.5) / want - 1.0) < 1e-12
    assert abs(sa.sum() * 13 / (4 * math.pi) - 1.0) < 0.02  # (the texels' solid angles tile the sphere)


def test_validation_of_the_switch_and_the_frame(emu):
    assert emu.check(1, 2.0) is None and emu.check(0, -1.0) is None  # (off: the extent is not read)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert "extent" in emu.check(1, bad)
    assert "reserved" in emu.check(1, 1.0, (0, 7))
    assert emu.is_rotation(eu.TO_LOCAL) and emu.is_rotation(np.eye(4).ravel())
    scaled = np.asarray(eu.TO_LOCAL).copy()
    scaled[:3] *= 1.001
    sheared = np.eye(4, dtype=np.float32).ravel()
    sheared[4] = 0.01
    assert not emu.is_rotation(scaled) and not emu.is_rotation(sheared)


# ---- 2. the round trip -------------------------------------------------------------------------------------------------------------
ROUND_TRIP_CAP = 2e-3  # the share of draws that may sit within float rounding of a cell border (and only those may name another cell)


@pytest.mark.parametrize("size", [(16, 8), (13, 7), (1030, 3)], ids=lambda s: "%dx%d" % s)
def test_the_sampled_direction_evaluates_in_the_cell_that_was_picked(emu, size):
    w, h = size
    env = eu.random_map(w, h)
    cw, ch, table, _ = emu.cells(env)
    rec = emu.record(eu.TO_LOCAL, cw, ch, 0.5)
    rng = np.random.RandomState(11)
    n = 100000
    r2 = rng.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    e1, e2 = (rng.randint(0, 2 ** 24, n) / np.float32(2 ** 24)).astype(np.float32), (rng.randint(0, 2 ** 24, n) / np.float32(2 ** 24)).astype(np.float32)
    L, emission, pdf, picked, found = emu.sample_env_light(env, eu.TO_LOCAL, table, rec, (r2, e1, e2))
    # every cell is drawn in proportion to its mass
    assert (picked < cw * ch).all()
    freq = np.bincount(picked, minlength=cw * ch) / n
    mass = du.pick_pmf(table)
    assert np.abs(freq - mass).max() < 5.0 * np.sqrt(mass.max() / n) + 1e-4
    # within float rounding of a border: the (u, v) the direction was built from, against the error of the way there and back -- two
    # sincos, a rotation and its inverse, two atan2: 4e-7 absolute in (u, v), and in u 2e-7 / sin(theta) more (the azimuth of a short vector)
    u = ((picked % cw) + e1.astype(np.float64)) / cw
    v = ((picked // cw) + e2.astype(np.float64)) / ch
    err_u = 4e-7 + 2e-7 / np.maximum(np.sin((1.0 - v) * math.pi), 1e-30)
    near = (np.abs(u * cw - np.round(u * cw)) < err_u * cw) | (np.abs(v * ch - np.round(v * ch)) < 4e-7 * ch)
    print("%dx%d: %d of %d draws near a border, %d name another cell" % (w, h, int(near.sum()), n, int((found != picked).sum())))
    assert near.mean() <= ROUND_TRIP_CAP                 # the condition on the inputs
    assert (found[~near] == picked[~near]).all()         # everywhere else the two sides name the same cell
    # the direction is unit and the pdf is the density of the cell that was FOUND times p_sel
    assert np.abs(np.linalg.norm(L.astype(np.float64), axis=1) - 1.0).max() < 1e-5
    sin_t = np.hypot(*(L.astype(np.float64) @ eu.rot3(eu.TO_LOCAL).T)[:, [0, 2]].T)
    want = mass[found] * cw * ch / (2.0 * math.pi ** 2 * sin_t) * 0.5
    assert (np.abs(pdf / want - 1.0) <= 1e-5 + 5e-7 / sin_t).all()  # (sin(theta) of the float32 direction: absolute error of a few 1e-7)
    # one function for both sides: called on L it returns what the sample carries, and its radiance is the escape's lookup, bit for bit
    radiance, density, cell = emu.env_eval(env, eu.TO_LOCAL, table, rec, L)
    assert eu.same(radiance, emission) and eu.same(density * np.float32(0.5), pdf) and np.array_equal(cell, found)
    assert eu.same(radiance, emu.sample_envmap(env, eu.TO_LOCAL, L))
    away = sin_t > 0.2  # (the azimuth of a direction near a pole is ill-conditioned: there the float64 restatement reads other texels)
    ref = eu.lookup(env, *eu.uv_of(L.astype(np.float64) @ eu.rot3(eu.TO_LOCAL).T))
    assert np.abs(emission[away] - ref[away]).max() <= 60.0 * max(w, h) * 4e-6 + 1e-4  # slope of the map (its sun is 60) times the error in (u, v), in texels


# ---- 3. the independent value ---------------------------------------------------------------------------------------------------------
def run_frame(scene, spp, ts0, **kw):
    """The frame of the spp samples with timestamps ts0 .. ts0 + spp - 1 alone, float64[n, 3].  The running mean folds sample t with
    1 / (t + 1): started from a zero frame at ts0 it leaves sum / (ts0 + spp)."""
    return scene.render(W, H, spp, first_timestamp=ts0, **kw)[0][:, :3].astype(np.float64) * ((ts0 + spp) / spp)


def eight_runs(scene, spp, **kw):
    """frame means (RGB) of 8 independent runs with distinct first_timestamp: float64[8, 3]"""
    return np.array([run_frame(scene, spp, 1000 * k, **kw).mean(0) for k in range(8)])


def within_four_standard_errors(means, expected, what):
    se = means.std(0, ddof=1) / math.sqrt(len(means))
    dev = np.abs(means.mean(0) - expected) / se
    print("%s: mean %s expected %s, standard error %s, deviation %s standard errors" % (what, means.mean(0), expected, se, dev))
    assert (se > 0).all() and (dev <= 4.0).all(), (what, dev)


@pytest.fixture(scope="module")
def plane(emu):
    return emu.scene(eu.sky_plane())


@pytest.fixture(scope="module")
def plane_value():
    env = eu.sun_map()
    coarse, fine = eu.plane_irradiance_value(env, nu=2048, nv=1024), eu.plane_irradiance_value(env)
    assert np.abs(coarse / fine - 1.0).max() < 1e-4  # the quadrature has converged far below the standard errors of the test
    return fine


@pytest.mark.parametrize("light_mode", [eu.UNIFORM, eu.POWER], ids=["uniform", "power"])
def test_a_plane_under_a_sun_gets_albedo_over_pi_times_the_irradiance(plane, plane_value, light_mode):
    means = eight_runs(plane, 16, env=EXTENT, light_mode=light_mode, **PLANE)
    within_four_standard_errors(means, plane_value, "sampling on")


def test_the_sun_carries_most_of_the_irradiance():
    """(the scene is the case the feature exists for: without the sun texel the value is less than half)"""
    env = eu.sun_map()
    dim = env.copy()
    dim[..., :3] = np.float32(eu.SKY)
    assert (eu.plane_irradiance_value(dim, nu=1024, nv=512) < 0.5 * eu.plane_irradiance_value(env, nu=1024, nv=512)).all()


# ---- 4. on against off ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def boxed(emu):
    return emu.scene(eu.sky_plane(box=True))


def test_on_and_off_agree_on_a_scene_with_a_shadow(boxed):
    on = eight_runs(boxed, 32, env=EXTENT, **DEEP)
    off = eight_runs(boxed, 128, **DEEP)
    se = np.sqrt(on.var(0, ddof=1) / 8 + off.var(0, ddof=1) / 8)
    dev = np.abs(on.mean(0) - off.mean(0)) / se
    print("on %s off %s combined standard error %s deviation %s" % (on.mean(0), off.mean(0), se, dev))
    assert (dev <= 4.0).all()


# ---- 5. the gain ------------------------------------------------------------------------------------------------------------------------
MEASURED_GAIN = 6.4  # RMSE(off) / RMSE(on) at equal spp (8), measured on the emulation: off 1.653, on 0.257
GAIN_BAR = MEASURED_GAIN / 2.0  # half of it: the margin is for seed-to-seed spread


def test_sampling_the_sun_lowers_the_error_at_equal_spp(boxed):
    converged = 0.5 * (run_frame(boxed, 2048, 50000, env=EXTENT, **DEEP) + run_frame(boxed, 2048, 90000, **DEEP))
    rmse = lambda img: math.sqrt(((img - converged) ** 2).mean())
    on = np.mean([rmse(run_frame(boxed, 8, 100 * k, env=EXTENT, **DEEP)) for k in range(4)])
    off = np.mean([rmse(run_frame(boxed, 8, 100 * k, **DEEP)) for k in range(4)])
    print("RMSE at 8 spp: off %.5f on %.5f gain %.2f" % (off, on, off / on))
    assert off / on >= GAIN_BAR


# ---- 6. off is the parent ------------------------------------------------------------------------------------------------------------------
def test_off_is_the_delta_emulation_bit_for_bit_and_disable_nee_ignores_the_switch(emu):
    sc = textured.decorate(textured.open_scene(8), seed=2)
    parent = du.DeltaEmu().scene(sc)
    mine = emu.scene(sc)
    lights = [__import__("gpuspectral_amd").abi.point_light((0.0, 2.0, 0.5), (3.0, 3.0, 3.0))]
    for kw in (dict(estimator=eu.REFERENCE), dict(estimator=eu.TEXTBOOK, light_mode=eu.POWER), dict(estimator=eu.TEXTBOOK, delta=lights)):
        a, ca = parent.render(W, H, 2, **kw)
        b, cb = mine.render(W, H, 2, **kw)
        assert eu.same(a, b) and ca == cb, kw
    # disable_nee: every escape takes the full weight and no vertex samples a light -- the frame of the switch off
    off, _ = mine.render(W, H, 2, disable_nee=1)
    on, c = mine.render(W, H, 2, env=EXTENT, disable_nee=1)
    assert eu.same(on, off) and c["shadow_rays"] == 0
    lit, c = mine.render(W, H, 2, env=EXTENT)
    assert not eu.same(lit, mine.render(W, H, 2)[0]) and c["shadow_rays"] > 0
    # a scene without a map: the switch is inert
    bare = emu.scene(textured.decorate(textured.open_scene(8), seed=2, envmap=False))
    assert eu.same(bare.render(W, H, 2, env=EXTENT)[0], bare.render(W, H, 2)[0])
    # the reference estimator does not take the switch
    with pytest.raises(ValueError):
        mine.render(W, H, 1, env=EXTENT, estimator=eu.REFERENCE)


# ---- the host-side builder under the sanitizers -------------------------------------------------------------------------------------------
def test_builder_standalone_under_asan_ubsan(tmp_path):
    """tests/emu/envlight_builder_main.cpp (its own main): the cell weights, the alias table over them, the radiant sum, the record, and
    the sampler and the shared function on the host, over maps from 1 x 1 to beyond both cell caps with NaN, infinite and negative
    texels, compiled with -fsanitize=address,undefined and run on the CPU."""
    import os
    import subprocess

    from conftest import ROOT

    exe = tmp_path / "envlight_builder_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-mfma", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emu", "envlight_builder_main.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "40 maps ok" in out.stdout
