"""The environment light (include/gpuspectral_pt.h, "Environment light") on the GPU.

The wavefront pipeline with the <ENV> kernels against the same stage headers run in scalar on the host (tests/emu/envlight_emu.cpp),
bit for bit, image and ray counts, at 32 x 24 pixels and 8 spp: the environment alone and beside a triangle light and a point light,
both picks, both drivers (k_shade and k_finish), across a table edit (<VER>), with an absorbing and a scattering medium, under maps
of 13 x 7 and 1030 x 3 texels; the narrower contexts through the widest instantiation; the independent value of
tests/test_envlight_cpu.py on the GPU frame itself."""
import copy

import numpy as np
import pytest

import envlight_util as eu
import media_util as mu
import scatter_util as su
import test_envlight_cpu as cpu
import textured

pytestmark = pytest.mark.gpu

COUNTS = ("extension_rays", "shadow_rays", "shaded_vertices")
W, H = 32, 24
SPP = 8
EXTENT = 3.0
PICKS = {"uniform": eu.UNIFORM, "power": eu.POWER}


def point_light():
    from gpuspectral_amd import abi

    return [abi.point_light((0.4, 1.6, 0.8), (4.0, 3.0, 2.0))]


@pytest.fixture(scope="module")
def emu():
    return eu.EnvEmu()


@pytest.fixture(scope="module")
def sky_scene():
    """textured.open_scene with textures and its random sky with a sun: one triangle light (two triangles) beside the environment"""
    return textured.decorate(textured.open_scene(8), seed=3)


@pytest.fixture(scope="module")
def tinted(sky_scene):
    return mu.with_medium(sky_scene, mu.glass_instances(sky_scene), 1)


def make_ctx(mode="default"):
    import gpuspectral_amd as g

    ctx = g.Context(0) if mode == "default" else g.Context(0, finish_paths=0xFFFFFFFF)
    ctx.set_estimator("textbook")
    return ctx


def frame(ctx, sc=None, ts0=0, spp=SPP, **params):
    if sc is not None:
        ctx.upload_scene(sc)
    ctx.frame_begin(W, H)
    ctx.reset_stats()
    ctx.render(spp=spp, first_timestamp=ts0, **params)
    return ctx.download().reshape(-1, 4).copy(), ctx.stats()


def agree(img, st, ref):
    rimg, rst = ref
    assert eu.same(img, rimg), "%d pixels differ" % int((img != rimg).any(1).sum())
    for k in COUNTS:
        assert st[k] == rst[k], (k, st[k], rst[k])


# ---- GPU == emulation, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "wavefront-only"])
@pytest.mark.parametrize("pick", list(PICKS))
def test_environment_alone(emu, mode, pick):
    sc = eu.sky_plane(box=True)  # no triangle light, no delta light: every pick lands on the environment record
    ref = emu.scene(sc).render(W, H, SPP, env=EXTENT, light_mode=PICKS[pick])
    with make_ctx(mode) as ctx:
        ctx.set_light_sampling(pick)
        ctx.set_envmap_sampling(True, EXTENT)
        img, st = frame(ctx, sc)
    agree(img, st, ref)
    assert st["shadow_rays"] > 0


@pytest.mark.parametrize("mode", ["default", "wavefront-only"])
@pytest.mark.parametrize("pick", list(PICKS))
def test_environment_beside_a_triangle_light_and_a_point_light(emu, sky_scene, mode, pick):
    ref = emu.scene(sky_scene).render(W, H, SPP, env=EXTENT, delta=point_light(), light_mode=PICKS[pick], first_timestamp=5)
    off = emu.scene(sky_scene).render(W, H, SPP, delta=point_light(), light_mode=PICKS[pick], first_timestamp=5)
    with make_ctx(mode) as ctx:
        ctx.set_light_sampling(pick)
        ctx.set_delta_lights(point_light())
        img, st = frame(ctx, sky_scene, ts0=5)            # the switch never set: the kernels and the bits of before
        agree(img, st, off)
        ctx.set_envmap_sampling(True, EXTENT)              # set under the resident scene: the tables are packed again
        img, st = frame(ctx, ts0=5)
        agree(img, st, ref)
        assert not eu.same(img, off[0])
        ctx.set_envmap_sampling(False)                     # ... and cleared again
        img, st = frame(ctx, ts0=5)
        agree(img, st, off)


@pytest.mark.parametrize("pick", list(PICKS))
def test_across_a_table_edit(emu, sky_scene, pick):
    """<VER, ENV>: gsp_update_tables between two gsp_render calls of the frame, neither drained; the record rides in both versions."""
    sc = copy.copy(sky_scene)
    with make_ctx() as ctx:
        ctx.set_light_sampling(pick)
        ctx.set_envmap_sampling(True, EXTENT)
        ctx.upload_scene(sc)
        ctx.frame_begin(W, H)
        ctx.reset_stats()
        ctx.render(spp=SPP // 2)
        acc, c1 = emu.scene(sc).render(W, H, SPP // 2, env=EXTENT, light_mode=PICKS[pick])
        bs = [b.copy() for b in sc.bsdfs]
        bs[0]["reflectance"][0] = (0.1, 0.5, 0.9)
        sc.bsdfs = bs
        lights = sc.lights.copy()
        lights["radiance"][:, :3] = np.array([8.0, 12.0, 17.0], np.float32)
        sc.lights = lights
        ctx.update_tables(sc)
        ctx.render(spp=SPP // 2, first_timestamp=SPP // 2)
        acc, c2 = emu.scene(sc).render(W, H, SPP // 2, env=EXTENT, light_mode=PICKS[pick], first_timestamp=SPP // 2, accum=acc)
        img = ctx.download().reshape(-1, 4)
        st = ctx.stats()
    assert st["scene_updates"] == 1 and st["scene_drains"] == 0, st
    agree(img, st, (acc, {k: c1[k] + c2[k] for k in COUNTS}))


@pytest.mark.parametrize("which", ["absorber", "scatterer"])
def test_with_media(emu, tinted, which):
    scatter = [(su.SIGMA_S, su.G)] if which == "scatterer" else None
    ref = emu.scene(tinted).render(W, H, SPP, env=EXTENT, media=[su.SIGMA_A], scatter=scatter)
    with make_ctx() as ctx:
        ctx.set_media([su.SIGMA_A])
        if scatter:
            ctx.set_media_scattering(scatter)
        ctx.set_envmap_sampling(True, EXTENT)
        img, st = frame(ctx, tinted)
    agree(img, st, ref)


@pytest.mark.parametrize("size", [(13, 7), (1030, 3)], ids=lambda s: "%dx%d" % s)
def test_odd_maps(emu, sky_scene, size):
    sc = copy.copy(sky_scene)
    sc.env_texels = eu.random_map(*size)
    ref = emu.scene(sc).render(W, H, SPP, env=EXTENT, light_mode=eu.POWER)
    with make_ctx() as ctx:
        ctx.set_light_sampling("power")
        ctx.set_envmap_sampling(True, EXTENT)
        img, st = frame(ctx, sc)
    agree(img, st, ref)


# ---- the narrower contexts through the widest instantiation ------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["plain", "delta", "absorber"])
def test_disable_nee_through_the_env_kernels_gives_the_bits_of_the_contexts_own_kernels(sky_scene, tinted, which):
    """Under disable_nee no vertex uses its light sample and every escape takes the full weight, so the <TEX, MED, EST, SCT, DLT, ENV>
    kernels must return what the context's own, narrower kernels return with the switch off: <TEX, EST>, <.., DLT>, <.., MED>."""
    sc = tinted if which == "absorber" else sky_scene
    with make_ctx() as ctx:
        if which == "absorber":
            ctx.set_media([su.SIGMA_A])
        if which == "delta":
            ctx.set_delta_lights(point_light())
        own, st_own = frame(ctx, sc, disable_nee=1)
        ctx.set_envmap_sampling(True, EXTENT)
        wide, st_wide = frame(ctx, disable_nee=1)
    agree(wide, st_wide, (own, st_own))


# ---- the independent value, on the device ------------------------------------------------------------------------------------------------
def test_a_plane_under_a_sun_gets_albedo_over_pi_times_the_irradiance_on_the_device(plane_value):
    with make_ctx() as ctx:
        ctx.set_envmap_sampling(True, cpu.EXTENT)
        ctx.upload_scene(eu.sky_plane())
        means = []
        for k in range(8):
            img, _ = frame(ctx, ts0=1000 * k, spp=16, **cpu.PLANE)
            means.append(img[:, :3].astype(np.float64).mean(0) * ((1000 * k + 16) / 16))
    cpu.within_four_standard_errors(np.array(means), plane_value, "device")


plane_value = cpu.plane_value
