"""The light grid without a GPU (include/gpuspectral_pt.h, "Light grid"): the product's builder and device functions
(pt_lightgrid.h) and shade_vertex<.., GRD = true> compiled for the host (tests/emu/lightgrid_emu.cpp) against a float64 restatement
of the header, against an analytic direct-light integral, and the variance the grid removes."""
import numpy as np
import pytest

import lightgrid_util as gu
import lights_util as lu


@pytest.fixture(scope="module")
def emu():
    return gu.GridEmu()


def _scenes():
    return {"room 3": lu.room_scene(3), "room 40": lu.room_scene(40), "floor": gu.floor_under_lights(equal=True, area=1e-2)}


@pytest.fixture(scope="module")
def grids(emu):
    """{name: (scene, bounds, Grid at 4 x 2 x 4)}"""
    out = {}
    for name, sc in _scenes().items():
        b = emu.scene(sc).bounds()
        out[name] = (sc, b, emu.build(b, (4, 2, 4), sc.lights))
    return out


# ---- the builder -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(_scenes()))
def test_every_cell_table_implies_its_weights(grids, name):
    """Per cell: sum p = 1 to 1e-12 and |p_i - w_i * inv_sum_w| within (1 + d_i) / (n 2^32) ("Light selection") plus the float32
    rounding of inv_sum_w (2^-24 relative); the weights are the float32 values of the one weight function, and agree with the
    float64 restatement of the header to float32 rounding (a dozen operations: 1e-5 relative)."""
    sc, _, g = grids[name]
    n = g.n
    worst = 0.0
    for c in range(g.cells):
        w = g.weights[c]
        assert (w >= 0.0).all() and np.isfinite(w).all() and w.sum() > 0.0
        p, d = lu.implied_pmf(g.tables[c])
        assert abs(p.sum() - 1.0) <= 1e-12
        assert abs(float(g.tails[c]) * w.sum() - 1.0) <= 2.0 ** -23
        err = np.abs(p - w * float(g.tails[c]))
        bound = (1.0 + d) / (n * lu.TWO32) + 2.0 ** -23 * p
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all()
        assert (p[w == 0.0] == 0.0).all()
    print("%s: %d cells x %d lights, largest error %.2f of its bound" % (name, g.cells, n, worst))
    for ix, iy, iz in ((0, 0, 0), (3, 1, 2), (1, 0, 3)):
        c = g.number(ix, iy, iz)
        want = np.array([gu.tri_weight64(g.header, g.centre(ix, iy, iz), L) for L in sc.lights])
        assert np.allclose(g.weights[c], want, rtol=1e-5, atol=0.0), (ix, iy, iz)


@pytest.mark.parametrize("name", list(_scenes()))
def test_fallback_is_the_power_table(emu, grids, name):
    """The fallback table and its trailing record are those of lights_emu's builder (a context without the grid), byte for byte."""
    sc, _, g = grids[name]
    le = lu.LightsEmu()
    assert g.fallback.tobytes() == le.build(sc.lights).tobytes()
    w = le.weights(sc.lights)
    assert g.fallback_tail[0] == np.float32(1.0 / w.sum()) and (g.fallback_tail[1:] == 0.0).all()


def test_cull_behind_a_down_facing_light(emu):
    """One light facing down at y = 1 in a box that reaches up to y = 2, three cells in y -- [0, 2/3), [2/3, 4/3), [4/3, 2]: the top
    cell lies wholly behind the light (weight 0), the middle one is cut by its plane (not 0), the bottom one sees it.  A second light
    at the ceiling keeps the top cell's table its own."""
    from gpuspectral_amd import abi

    lt = np.zeros(2, abi.LIGHT_DT)
    lt["positions"][0, :, :3] = lu.down_triangle(0.5, 0.5, 1.0, 0.01)
    lt["positions"][1, :, :3] = lu.down_triangle(0.5, 0.5, 2.0, 0.01)
    lt["radiance"][:, :3] = 5.0
    bounds = (0, 0, 0, 1, 2, 1)
    g = emu.build(bounds, (1, 3, 1), lt)
    w = g.weights  # [cell = iy, light]
    assert w[2, 0] == 0.0 and w[1, 0] > 0.0 and w[0, 0] > 0.0
    assert (w[:, 1] > 0.0).all()  # the ceiling light faces every cell
    p, _ = lu.implied_pmf(g.tables[2])
    assert p[0] == 0.0 and p[1] == 1.0
    # a cell whose weights are ALL zero: only the light at y = 1 -> the top cell copies the fallback and stores tail 0
    g1 = emu.build(bounds, (1, 3, 1), lt[:1])
    assert g1.weights[2, 0] == 0.0 and g1.tails[2] == 0.0 and g1.tables[2].tobytes() == g1.fallback.tobytes()
    assert g1.tails[0] != 0.0


def test_all_zero_and_non_finite_weights(emu):
    """A light of NaN radiance and one of negative luminance count as 0 in every cell."""
    sc = lu.room_scene(3)
    lt = sc.lights.copy()
    lt["radiance"][0, 1] = np.nan
    lt["radiance"][1, :3] = (-1.0, -2.0, -3.0)
    g = emu.build(emu.scene(sc).bounds(), (2, 2, 2), lt)
    assert (g.weights[:, :2] == 0.0).all() and (g.weights[:, 2] > 0.0).all()


def test_delta_weights(emu):
    """Point and spot: Y / max(D^2, Rcell^2); directional: Y, in every cell."""
    from gpuspectral_amd import abi

    sc = lu.room_scene(3)
    b = emu.scene(sc).bounds()
    delta = [abi.point_light((0.2, 1.0, 0.1), (3.0, 2.0, 1.0)), abi.directional_light((0.0, -1.0, 0.0), (0.5, 0.5, 0.5), 2.0)]
    g = emu.build(b, (3, 2, 3), sc.lights, delta)
    assert g.n == 5
    rc2 = float(g.header["half_diag"]) ** 2
    for ix, iy, iz in ((0, 0, 0), (2, 1, 1)):
        c = g.centre(ix, iy, iz)
        d2 = ((np.array([0.2, 1.0, 0.1]) - c) ** 2).sum()
        w = g.weights[g.number(ix, iy, iz)]
        assert abs(w[3] / (gu.luminance(np.array([3.0, 2.0, 1.0])) / max(d2, rc2)) - 1.0) < 1e-5
        assert abs(w[4] / 0.5 - 1.0) < 1e-6


# ---- resolution --------------------------------------------------------------------------------------------------------------------
def test_auto_resolution_respects_the_cap(emu):
    cube = (0, 0, 0, 1, 1, 1)
    assert emu.resolve(cube, 3) == (32, 32, 32)  # 98304 entries
    assert emu.resolve(cube, 40) == (29, 29, 29)  # 29^3 * 40 = 975560 <= 2^20 < 30^3 * 40
    slab = (0, 0, 0, 4, 1, 2)
    r = emu.resolve(slab, 16)
    assert r == (32, 8, 16)
    # a synthetic table of 5000 lights: 209 cells at most
    r = emu.resolve(cube, 5000)
    assert r == (5, 5, 5) and 125 * 5000 <= gu.MAX_ENTRIES < 216 * 5000
    r = emu.resolve(slab, 5000)
    assert r[0] * r[1] * r[2] * 5000 <= gu.MAX_ENTRIES and r[0] >= r[2] >= r[1] >= 1
    assert emu.resolve((0, 0, 0, 1, 0, 1), 16) == (32, 1, 32)  # a degenerate extent: 1 cell on that axis
    assert emu.resolve((0, 0, 0, 0, 0, 0), 16) == (1, 1, 1)
    assert emu.resolve(cube, gu.MAX_ENTRIES + 1) is None  # even 1 x 1 x 1 is beyond the cap
    # explicit
    assert emu.resolve(cube, 16, (8, 2, 8)) == (8, 2, 8)
    assert emu.resolve((0, 0, 0, 1, 0, 1), 16, (8, 2, 8)) == (8, 1, 8)
    assert emu.resolve(cube, 5000, (8, 8, 8)) is None
    assert emu.resolve(cube, 4, (64, 64, 64)) == (64, 64, 64)  # 2^18 cells * 4 = 2^20 exactly


def test_validation(emu):
    assert emu.check(0, (99, 0, 1), (1, 2, 3, 4)) is None  # off: nothing else is read
    assert emu.check(1) is None and emu.check(1, (64, 1, 64)) is None
    assert "reserved" in emu.check(1, (0, 0, 0), (0, 0, 1, 0))
    assert "64" in emu.check(1, (65, 1, 1))
    assert "auto" in emu.check(1, (4, 0, 4)) and "auto" in emu.check(1, (0, 0, 1))


# ---- the cell of a point -------------------------------------------------------------------------------------------------------------
def test_cell_lookup(emu, grids):
    """A point on a cell's lower face belongs to that cell; a point outside the box on any axis, on the box's upper face, or not
    finite takes the fallback.  All positions of gu.probe_positions against floor((p - lo) * inv_cell) restated in float32 numpy."""
    _, b, g = grids["room 40"]
    h = g.header
    pos = gu.probe_positions(b, g.res)
    cell, ixyz = emu.cell(g, pos)
    with np.errstate(all="ignore"):
        f = np.floor((pos - h["lo"][None, :]) * h["inv_cell"][None, :])
        inside = ((f >= 0) & (f < np.array(g.res, np.float32)[None, :])).all(1)
    assert inside.sum() > 300 and (~inside).sum() > 300
    assert (cell[~inside] == gu.NO_CELL).all()
    fi = f[inside].astype(np.int64)
    assert np.array_equal(ixyz[inside], fi.astype(np.uint32))
    assert np.array_equal(cell[inside], ((fi[:, 2] * g.res[1] + fi[:, 1]) * g.res[0] + fi[:, 0]).astype(np.uint32))
    # by name: the lower corner is cell 0, the upper corner and every non-finite point the fallback; the face between x cells 1 and 2 is cell 2's
    lo, hi = b[:3], b[3:]
    mid = 0.5 * (lo + hi)
    face = mid.copy()
    face[0] = h["lo"][0] + np.float32(2.0) / h["inv_cell"][0]
    named = np.array([lo, hi, face, [np.nan, mid[1], mid[2]], [mid[0], np.inf, mid[2]], [lo[0] - 1e-3, mid[1], mid[2]]], np.float32)
    c, xyz = emu.cell(g, named)
    assert c[0] == 0 and c[1] == gu.NO_CELL and c[3] == c[4] == c[5] == gu.NO_CELL
    assert xyz[2, 0] in (1, 2) and xyz[2, 0] == int(np.floor((named[2, 0] - h["lo"][0]) * h["inv_cell"][0]))


def test_pick_and_hit_pmf_follow_the_cell(emu, grids):
    """The pick of a draw is light_pick_index on the table of the point's cell (lu.pick64 on that table) or on the fallback; the hit
    pdf of a light record's own triangle is its weight times the cell's inv_sum_w, or the fallback rule."""
    sc, b, g = grids["room 40"]
    pos = gu.probe_positions(b, g.res, random=600)
    rng = np.random.RandomState(2)
    r = rng.randint(0, 2 ** 32, len(pos), dtype=np.uint64).astype(np.uint32)
    cell, _ = emu.cell(g, pos)
    k, pmf = emu.pick(g, pos, r)
    li = rng.randint(0, g.n, len(pos))
    tris = np.concatenate([sc.lights["positions"][li][:, :, :3].reshape(-1, 9), sc.lights["radiance"][li][:, :3]], 1)
    ps = emu.hit_pmf(g, pos, tris)
    wf = lu.LightsEmu().weights(sc.lights)
    for i in range(len(pos)):
        t = g.fallback if cell[i] == gu.NO_CELL else g.tables[cell[i]]
        ki = int(lu.pick64(t, r[i : i + 1])[0])
        assert k[i] == ki
        assert pmf[i] == t["pmf_self"][ki]  # (the stored pmf of the light that was picked, whichever slot named it)
        if cell[i] == gu.NO_CELL:
            assert abs(ps[i] / (wf[li[i]] / wf.sum()) - 1.0) < 1e-5
        else:
            assert abs(ps[i] - g.weights[cell[i], li[i]] * float(g.tails[cell[i]])) <= 1e-6 * ps[i] + 1e-30


# ---- structure of the frames -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def room(emu):
    sc = lu.room_scene(3)
    es = emu.scene(sc)
    return sc, es, es.render(40, 32, 2, grid=False), es.render(40, 32, 2, grid=(8, 2, 8))


def test_off_is_the_power_textbook_frame(emu, room):
    """The switch off: the frame of lights_emu / estimator_emu's power + textbook context (delta_emu's dispatch), bit for bit."""
    import delta_util as du

    sc, _, (off, so), _ = room
    ref, sr = du.DeltaEmu().scene(sc).render(40, 32, 2, light_mode=du.POWER, estimator=du.TEXTBOOK)
    assert gu.same(off, ref) and so["shadow_rays"] == sr["shadow_rays"] and so["resolution"] == (0, 0, 0)


def test_only_the_light_samples_differ(room):
    """Extension rays and shaded vertices are those of the power pick (the continuation does not read the light sample); the frame
    differs, is finite and not negative."""
    _, _, (off, so), (on, sn) = room
    assert so["extension_rays"] == sn["extension_rays"] and so["shaded_vertices"] == sn["shaded_vertices"]
    assert sn["resolution"] == (8, 2, 8)
    assert not gu.same(off, on) and np.isfinite(on).all() and on[:, :3].min() >= 0.0


def test_without_nee_the_grid_changes_nothing(room):
    _, es, _, _ = room
    a, sa = es.render(40, 32, 2, grid=False, disable_nee=1)
    b, sb = es.render(40, 32, 2, grid=(8, 2, 8), disable_nee=1)
    assert gu.same(a, b) and sa["shadow_rays"] == sb["shadow_rays"] == 0


def test_prerequisites_in_the_emulation(emu, room):
    _, es, _, _ = room
    for kw in (dict(light_mode=gu.UNIFORM), dict(estimator=gu.REFERENCE)):
        with pytest.raises(ValueError, match="returned 1"):
            es.render(8, 8, 1, grid=None, **kw)
    with pytest.raises(ValueError, match="returned 3"):
        emu.scene(lu.room_scene(40)).render(8, 8, 1, grid=(64, 64, 64))  # 2^18 cells * 40 lights > 2^20: explicit, so refused


# ---- unbiased ----------------------------------------------------------------------------------------------------------------------
UNBIASED_W = UNBIASED_H = 16
UNBIASED_N = 4096  # tests/test_lights_cpu.py test_both_modes_estimate_the_analytic_direct_light: the same N and the same 4 standard errors
UNBIASED_GRID = (6, 2, 6)


def unbiased_case(emu):
    """(the scene as rendered, its emulation, the bounds as uploaded, the analytic direct light, the mask of fallback pixels)"""
    up = gu.unbiased_scene()
    bounds = emu.scene(up).bounds()
    sc = gu.moved(up, 0, dx=gu.UNBIASED_SHIFT)
    ref = lu.direct_light64(sc, UNBIASED_W, UNBIASED_H)
    x = gu.floor_points64(sc, UNBIASED_W, UNBIASED_H)
    outside = (x[:, 0] > bounds[3]) | (x[:, 0] < bounds[0]) | (x[:, 2] > bounds[5]) | (x[:, 2] < bounds[2])
    return sc, emu.scene(sc), bounds, ref, outside


def z_scores(m, n, ref):
    mean = m[:, :3] / n
    se = np.sqrt(np.maximum(m[:, 3:] / n - mean * mean, 0.0) / (n - 1))
    assert (se > 0.0).all()
    return np.abs(mean - ref) / se


def test_grid_estimates_the_analytic_direct_light(emu):
    """The floor under the 16 lights of lu.expectation_scene, moved behind the upload so that the right part of the view lies
    outside the grid's box (fallback table) and the rest inside (cell tables), max_depth = 1 (the floor is flat and the lights do not
    reflect: only direct light arrives, as in test_lights_cpu.py).  The per-pixel mean over N = 4096 timestamps agrees with the
    float64 quadrature within 4 standard errors of the mean, the errors from the rendered moments -- the rule and the N of
    test_both_modes_estimate_the_analytic_direct_light.  First the uniform pick alone on this scene, then the power pick, then the grid."""
    sc, es, bounds, ref, outside = unbiased_case(emu)
    assert (ref > 0.0).all() and 20 <= outside.sum() <= outside.size - 20, outside.sum()
    common = dict(moments=True, clamp=1e30, rr_start_depth=255, max_depth=1, bounds=bounds)
    for name, kw in (("uniform", dict(light_mode=gu.UNIFORM)), ("power", dict()), ("grid", dict(grid=UNBIASED_GRID))):
        _, st, m = es.render(UNBIASED_W, UNBIASED_H, UNBIASED_N, **common, **kw)
        z = z_scores(m, UNBIASED_N, ref)
        print("%s: largest |mean - analytic| = %.2f standard errors (inside the box %.2f, fallback pixels %.2f)" % (name, z.max(), z[~outside].max(), z[outside].max()))
        assert z.max() <= 4.0
    assert st["resolution"] == UNBIASED_GRID


# ---- it helps ----------------------------------------------------------------------------------------------------------------------
HELP_W, HELP_H, HELP_SPP = 48, 32, 4
# measured on the emulation (48 x 32, 4 spp, clamp 1e30, the pixels within 1 unit of a light's foot): see the test's output and DESIGN.md section 31
def help_case():
    sc = gu.help_scene()
    ref = lu.direct_light64(sc, HELP_W, HELP_H, levels=5)
    x = gu.floor_points64(sc, HELP_W, HELP_H)
    feet = np.array([(8.0 * (i % 4 - 1.5), 0.0, 8.0 * (i // 4 - 1.5)) for i in range(16)])
    near = (np.linalg.norm(x[:, None, :] - feet[None, :, :], axis=2) <= 1.0).any(1)
    return sc, ref, near


def mse(img, ref, mask):
    return float(((img[mask, :3].astype(np.float64) - ref[mask]) ** 2).mean())


def test_grid_halves_the_error_under_the_lights(emu):
    """16 equal lights, every one the dominant light of the floor under it: the power pick gives each probability 1 / 16, the grid
    gives the light above a cell roughly 0.7.  Mean squared error against the analytic direct light over the pixels within 1 unit of
    a light's foot, 4 spp: the grid's is at most half of the power pick's (measured ratio: printed)."""
    sc, ref, near = help_case()
    assert near.sum() >= 48, near.sum()  # (every one of the 16 feet is in view: at least 3 pixels each)
    es = emu.scene(sc)
    common = dict(clamp=1e30, rr_start_depth=255, max_depth=1)
    power, _ = es.render(HELP_W, HELP_H, HELP_SPP, **common)
    grid, st = es.render(HELP_W, HELP_H, HELP_SPP, grid=gu.HELP_RES, **common)
    assert st["resolution"] == gu.HELP_RES
    a, b = mse(power, ref, near), mse(grid, ref, near)
    print("MSE over %d pixels: power %.4g, grid %.4g, ratio %.2f" % (near.sum(), a, b, a / b))
    assert b <= 0.5 * a


# ---- the builder under the sanitizers ------------------------------------------------------------------------------------------------
def test_builder_standalone_under_asan_ubsan(tmp_path):
    """tests/emu/lightgrid_builder_main.cpp (its own main): validation, resolution, header and builder over random and degenerate
    light tables and boxes, every image in a buffer of exactly lightgrid_bytes(), then lookup, pick and hit pdf over it with positions
    inside, outside and not finite; compiled with -fsanitize=address,undefined and run on the CPU."""
    import os
    import subprocess

    from conftest import ROOT

    exe = tmp_path / "lightgrid_builder_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-mfma", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emu", "lightgrid_builder_main.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "grids ok" in out.stdout
