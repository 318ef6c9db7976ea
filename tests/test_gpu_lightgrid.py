"""The light grid (include/gpuspectral_pt.h, "Light grid") on the GPU.

The wavefront pipeline with the <GRD> kernels against the same stage headers run in scalar on the host (tests/emu/lightgrid_emu.cpp),
bit for bit, image and ray counts: 3 and 40 lights (the tables in front of the grid are staged into LDS, the grid never is; the
versioned kernels of the table edit read everything from global memory), both contexts and two first timestamps, with textures, with a scattering medium, with two delta lights, across an undrained
table edit (<VER, GRD>: every version carries its own grid), on two shares; the switch on and off again; the statistical tests of
tests/test_lightgrid_cpu.py on the GPU's own frames.  Frames of at most 48 x 32 pixels, grids of at most 8 x 2 x 8 cells (the
16 x 2 x 16 grid of the gain test aside, which the issue fixes)."""
import copy
import json
import os

import numpy as np
import pytest

import lightgrid_util as gu
import lights_util as lu
import test_lightgrid_cpu as cpu  # the statistical cases and their checks
import textured
from conftest import ROOT

pytestmark = pytest.mark.gpu

COUNTS = ("extension_rays", "shadow_rays", "shaded_vertices")
W, H = 48, 32
SPP = 4
GRID = (8, 2, 8)
LIGHTS = (3, 40)


@pytest.fixture(scope="module")
def emu():
    return gu.GridEmu()


@pytest.fixture(scope="module")
def rooms():
    return {n: lu.room_scene(n) for n in LIGHTS}


@pytest.fixture(scope="module")
def references(emu, rooms):
    """The emulation's frames, rendered once: {(lights, first timestamp): (image, counts)} with the grid, {(lights, first timestamp,
    "off")} the power pick's without."""
    out = {(n, ts0): emu.scene(rooms[n]).render(W, H, SPP, grid=GRID, first_timestamp=ts0) for n in LIGHTS for ts0 in (0, 5)}
    out.update({(n, ts0, "off"): emu.scene(rooms[n]).render(W, H, SPP, grid=False, first_timestamp=ts0) for n in LIGHTS for ts0 in (0, 5)})
    return out


def make_ctx(kind="default", grid=GRID):
    import gpuspectral_amd as g

    ctx = g.Context(0) if kind == "default" else g.Context(0, finish_paths=0xFFFFFFFF)
    ctx.set_light_sampling("power")
    ctx.set_estimator("textbook")
    if grid is not False:
        ctx.set_light_grid(True, grid)
    return ctx


def frame(ctx, sc=None, ts0=0, w=W, h=H, spp=SPP, **params):
    if sc is not None:
        ctx.upload_scene(sc)
    ctx.frame_begin(w, h)
    ctx.reset_stats()
    ctx.render(spp=spp, first_timestamp=ts0, **params)
    return ctx.download().reshape(-1, 4).copy(), ctx.stats()


def agree(img, st, ref):
    rimg, rst = ref
    assert gu.same(img, rimg), "%d pixels differ" % int((img != rimg).any(1).sum())
    for k in COUNTS:
        assert st[k] == rst[k], (k, st[k], rst[k])


# ---- GPU == emulation, bit for bit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["default", "wavefront-only"])
@pytest.mark.parametrize("ts0", [0, 5])
@pytest.mark.parametrize("n", LIGHTS)
def test_gpu_equals_emu(rooms, references, kind, ts0, n):
    with make_ctx(kind) as ctx:
        img, st = frame(ctx, rooms[n], ts0=ts0)
        assert ctx.light_grid()[:2] == (True, GRID)
    agree(img, st, references[(n, ts0)])
    assert not gu.same(img, references[(n, ts0, "off")][0])
    # the continuation does not read the light sample: the extension rays are the power pick's
    assert st["extension_rays"] == references[(n, ts0, "off")][1]["extension_rays"]


def test_gpu_equals_emu_with_textures(emu, rooms):
    sc = textured.decorate(copy.deepcopy(rooms[3]), seed=5, envmap=False)
    ref = emu.scene(sc).render(W, H, SPP, grid=GRID)
    for kind in ("default", "wavefront-only"):
        with make_ctx(kind) as ctx:
            img, st = frame(ctx, sc)
        agree(img, st, ref)


def test_gpu_equals_emu_with_a_scattering_medium(emu, rooms):
    import media_util as mu
    import scatter_util as su

    sc = mu.with_medium(rooms[3], mu.glass_instances(rooms[3]), 1)
    es = emu.scene(sc)
    ref = es.render(W, H, SPP, grid=GRID, media=[su.SIGMA_A], scatter=[(su.SIGMA_S, su.G)])
    absorber = es.render(W, H, SPP, grid=GRID, media=[su.SIGMA_A])
    assert not gu.same(ref[0], absorber[0])
    with make_ctx() as ctx:
        ctx.set_media([su.SIGMA_A])
        ctx.set_media_scattering([(su.SIGMA_S, su.G)])
        img, st = frame(ctx, sc)
        agree(img, st, ref)
        ctx.set_media_scattering(None)  # the table of zeros takes its place: the absorber's bits
        img, st = frame(ctx)
        agree(img, st, absorber)


def test_gpu_equals_emu_with_two_delta_lights(emu, rooms):
    from gpuspectral_amd import abi

    delta = [abi.point_light((0.3, 1.2, 0.2), (0.8, 0.7, 0.5)), abi.directional_light((0.0, -0.8, 0.6), (0.3, 0.3, 0.4), 2.0)]
    for n in LIGHTS:
        ref = emu.scene(rooms[n]).render(W, H, SPP, grid=GRID, delta=delta)
        with make_ctx() as ctx:
            ctx.set_delta_lights(delta)
            img, st = frame(ctx, rooms[n])
        agree(img, st, ref)
        assert st["shadow_rays"] != 0


@pytest.mark.parametrize("n", LIGHTS)
def test_gpu_equals_emu_across_a_table_edit(emu, rooms, n):
    """<VER, GRD>: gsp_update_tables dims a light between two gsp_render calls of the frame, neither drained.  The samples of the
    first call finish on their version of the tables -- lights, fallback table AND grid -- next to those of the second."""
    sc = copy.copy(rooms[n])
    with make_ctx() as ctx:
        ctx.upload_scene(sc)
        ctx.frame_begin(W, H)
        ctx.reset_stats()
        ctx.render(spp=2)
        acc, c1 = emu.scene(sc).render(W, H, 2, grid=GRID)
        lights = sc.lights.copy()
        lights["radiance"][int(np.argmax(lu.weights64(lights))), :3] *= np.float32(0.02)  # the strongest light is dimmed: other tables in every cell
        sc.lights = lights
        ctx.update_tables(sc)
        ctx.render(spp=2, first_timestamp=2)
        acc, c2 = emu.scene(sc).render(W, H, 2, grid=GRID, first_timestamp=2, accum=acc)
        img = ctx.download().reshape(-1, 4)
        st = ctx.stats()
        assert ctx.light_grid()[:2] == (True, GRID)
    assert st["scene_updates"] == 1 and st["scene_drains"] == 0, st  # (the first call's samples were in flight at the edit)
    agree(img, st, (acc, {k: c1[k] + c2[k] for k in COUNTS}))


@pytest.mark.parametrize("n", LIGHTS)
def test_two_shares_of_a_multi_context(rooms, references, n):
    from gpuspectral_amd import pt

    with pt.MultiContext([0, 0]) as m:
        m.set_light_sampling("power")
        m.set_estimator("textbook")
        m.set_light_grid(True, GRID)
        m.upload_scene(rooms[n])
        m.frame_begin(W, H)
        m.render(spp=SPP)
        m.gather()
        img = m.download().reshape(-1, 4)
    assert gu.same(img, references[(n, 0)][0])


# ---- off ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LIGHTS)
def test_on_then_off_is_a_context_that_never_heard_of_it(rooms, references, n):
    """Frame, gsp_stats and the resident pick table, bit for bit, against a context that was never told of the grid."""
    with make_ctx(grid=False) as ctx:
        ref, rst = frame(ctx, rooms[n])
        table = ctx.download_light_pick()
    agree(ref, rst, references[(n, 0, "off")])
    with make_ctx() as ctx:
        ctx.upload_scene(rooms[n])
        ctx.frame_begin(W, H)
        ctx.render(spp=1)
        ctx.set_light_grid(False)  # (under the resident scene: the tables are packed again without the grid)
        assert ctx.light_grid()[0] is False
        img, st = frame(ctx)
        assert ctx.download_light_pick().tobytes() == table.tobytes()
    assert gu.same(img, ref)
    timed = [k for k in rst if k.endswith("_ms") or k.endswith("_seconds") or "time" in k]
    for k in rst:
        if k not in timed and k != "scene_drains":
            assert st[k] == rst[k], (k, st[k], rst[k])


def test_switched_on_under_a_resident_scene(rooms, references):
    """The setter behind the upload: repacked from the host copy, the frame of a context that had the switch first."""
    with make_ctx(grid=False) as ctx:
        ctx.upload_scene(rooms[40])
        ctx.set_light_grid(True, GRID)
        img, st = frame(ctx)
    agree(img, st, references[(40, 0)])


# ---- unbiased, and it helps: the GPU's own frames under the rules of tests/test_lightgrid_cpu.py -------------------------------------------
def test_grid_estimates_the_analytic_direct_light_on_the_gpu(emu):
    """The floor moved behind the upload (gsp_update_instances): part of the view picks from cell tables, part from the fallback.
    The GPU's mean over N = 4096 timestamps against the float64 quadrature, within 4 standard errors from the emulation's rendered
    moments of the same samples (the GPU's frame is their float32 running mean: N * 2^-24 = 2.4e-4 relative at worst, checked to 1e-3)."""
    up = gu.unbiased_scene()
    sc, es, bounds, ref, outside = cpu.unbiased_case(emu)
    params = dict(clamp=1e30, rr_start_depth=255, max_depth=1)
    _, _, m = es.render(cpu.UNBIASED_W, cpu.UNBIASED_H, cpu.UNBIASED_N, grid=cpu.UNBIASED_GRID, bounds=bounds, moments=True, **params)
    with make_ctx(grid=cpu.UNBIASED_GRID) as ctx:
        ctx.upload_scene(up)
        ctx.update_instances(sc.instances)
        got_bounds = ctx.light_grid()[2]
        img, _ = frame(ctx, w=cpu.UNBIASED_W, h=cpu.UNBIASED_H, spp=cpu.UNBIASED_N, **params)
    assert np.array_equal(np.float32(got_bounds[0] + got_bounds[1]), bounds)  # the bounds as uploaded: the move did not shift them
    mean = m[:, :3] / cpu.UNBIASED_N
    assert np.allclose(img[:, :3], mean, rtol=1e-3, atol=0.0)
    se = np.sqrt(np.maximum(m[:, 3:] / cpu.UNBIASED_N - mean * mean, 0.0) / (cpu.UNBIASED_N - 1))
    z = np.abs(img[:, :3].astype(np.float64) - ref) / se
    print("GPU: largest |mean - analytic| = %.2f standard errors (inside the box %.2f, fallback pixels %.2f)" % (z.max(), z[~outside].max(), z[outside].max()))
    assert z.max() <= 4.0


def test_moved_floor_frame_equals_emu(emu):
    """... and at 4 spp that frame is the emulation's bit for bit: the moved scene, the bounds of the upload."""
    up = gu.unbiased_scene()
    sc, es, bounds, _, _ = cpu.unbiased_case(emu)
    ref = es.render(cpu.UNBIASED_W, cpu.UNBIASED_H, SPP, grid=cpu.UNBIASED_GRID, bounds=bounds)
    with make_ctx(grid=cpu.UNBIASED_GRID) as ctx:
        ctx.upload_scene(up)
        ctx.update_instances(sc.instances)
        img, st = frame(ctx, w=cpu.UNBIASED_W, h=cpu.UNBIASED_H)
    agree(img, st, ref)


def test_grid_halves_the_error_under_the_lights_on_the_gpu(emu):
    """test_lightgrid_cpu.test_grid_halves_the_error_under_the_lights on the GPU's frames (which are the emulation's)."""
    sc, ref, near = cpu.help_case()
    params = dict(clamp=1e30, rr_start_depth=255, max_depth=1)
    with make_ctx(grid=False) as ctx:
        power, _ = frame(ctx, sc, w=cpu.HELP_W, h=cpu.HELP_H, spp=cpu.HELP_SPP, **params)
        ctx.set_light_grid(True, gu.HELP_RES)
        grid, _ = frame(ctx, w=cpu.HELP_W, h=cpu.HELP_H, spp=cpu.HELP_SPP, **params)
    a, b = cpu.mse(power, ref, near), cpu.mse(grid, ref, near)
    print("GPU: MSE over %d pixels: power %.4g, grid %.4g, ratio %.2f" % (near.sum(), a, b, a / b))
    assert b <= 0.5 * a
    es = emu.scene(sc)
    assert gu.same(grid, es.render(cpu.HELP_W, cpu.HELP_H, cpu.HELP_SPP, grid=gu.HELP_RES, **params)[0])


# ---- nothing else moved --------------------------------------------------------------------------------------------------------------
def test_kernel_digest_is_unchanged():
    """kernel_digest (sha256 of the instruction streams of k_trace<ExtendIO>, k_trace<ConnectIO> and k_shade<0, 0, 0, 0, 0>) is what it
    was before the grid existed: a context without it runs the same code."""
    with open(os.path.join(ROOT, "gpuspectral_amd", "lib", "valu_mix.json")) as fh:
        vm = json.load(fh)
    from gpuspectral_amd import pt

    assert vm["library_digest"] == pt.source_digest()
    assert vm["kernel_digest"] == "46198066bb589355"


# ---- the C++ host and the CLI ------------------------------------------------------------------------------------------------------
def _run_cli(args):
    import subprocess

    lib = os.path.join(ROOT, "gpuspectral_amd", "lib")
    env = dict(os.environ, LD_LIBRARY_PATH=lib + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    return subprocess.run([os.path.join(lib, "gsp_render")] + args, env=env, capture_output=True, text=True, timeout=300)


def _pfm_equals(path, img, w, h):
    from oracle import mitsuba_loader as ml

    got = np.asarray(ml.read_pfm(path), np.float32).reshape(h, w, -1)[:, :, :3]
    rgb = img.reshape(h, w, 4)[:, :, :3]
    return gu.same(got, rgb) or gu.same(got[::-1], rgb)  # (PFM rows run bottom to top)


def test_host_and_cli_render_the_emulations_frame(emu, tmp_path):
    """PathTracer::setLightGrid and `gsp_render --light-sampling power --estimator textbook --light-grid 4,2,4` on a scene file."""
    from gpuspectral_amd import host
    from test_scatter_loader import write_scatter_xml

    xml = write_scatter_xml(tmp_path)
    w, h, spp = 48, 32, 4
    sc = host.Scene(xml)
    ref, _ = emu.scene(sc.arrays()).render(w, h, spp, grid=(4, 2, 4))
    off, _ = emu.scene(sc.arrays()).render(w, h, spp, grid=False)
    assert not gu.same(ref, off)
    pt = host.PathTracer(w, h)
    pt.set_light_sampling("power")
    pt.set_estimator("textbook")
    pt.set_light_grid(True, (4, 2, 4))
    pt.render(sc, spp)
    img = pt.download().reshape(-1, 4).copy()
    pt.set_light_grid(False)
    pt.reset()
    pt.render(sc, spp)
    img_off = pt.download().reshape(-1, 4).copy()
    pt.close()
    assert gu.same(img, ref) and gu.same(img_off, off)
    out = str(tmp_path / "g.pfm")
    r = _run_cli(["--light-sampling", "power", "--estimator", "textbook", "--light-grid", "4,2,4", xml, out, str(w), str(h), str(spp)])
    assert r.returncode == 0, r.stderr
    assert _pfm_equals(out, ref, w, h)
    r = _run_cli(["--light-sampling", "power", "--estimator", "textbook", "--light-grid", xml, out, str(w), str(h), "1"])  # no resolution: auto
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("flags, word", [(["--light-sampling", "power"], "GSP_ESTIMATOR_TEXTBOOK"), (["--estimator", "textbook"], "GSP_LIGHTS_POWER"),
                                         (["--light-sampling", "power", "--estimator", "textbook", "--light-grid", "65,1,1"], "at most 64")])
def test_cli_without_a_prerequisite_exits_2_with_the_librarys_message(tmp_path, flags, word):
    """--light-grid implies nothing else."""
    from test_scatter_loader import write_scatter_xml

    xml = write_scatter_xml(tmp_path)
    args = flags if "--light-grid" in flags else flags + ["--light-grid"]
    r = _run_cli(args + [xml, str(tmp_path / "x.pfm"), "16", "16", "1"])
    assert r.returncode == 2 and "gsp_set_light_grid" in r.stderr and word in r.stderr, r.stderr
    assert not os.path.exists(str(tmp_path / "x.pfm"))
