"""Delta lights (include/gpuspectral_pt.h, "Delta lights") on the GPU.

The wavefront pipeline with the <DLT> kernels against the same stage headers run in scalar on the host (tests/emu/delta_emu.cpp),
bit for bit, image and ray counts: on the materials scene with one point, one spot and one directional light beside its triangle
lights -- both contexts, two first timestamps, both picks and both estimators, with textures, across a table edit, with absorbing
and with scattering media, on two shares; the closed forms of tests/test_delta_cpu.py on the GPU frame itself, with its bounds;
and the table as context state."""
import copy

import numpy as np
import pytest

import delta_util as du
import media_util as mu
import scatter_util as su
import test_delta_cpu as cpu  # the closed-form cases and their checks
import textured

pytestmark = pytest.mark.gpu

COUNTS = ("extension_rays", "shadow_rays", "shaded_vertices")
W, H = 48, 36
SPP = 4
LIGHTS = cpu.mixed_lights()
MODES = {"uniform reference": (du.UNIFORM, du.REFERENCE), "power reference": (du.POWER, du.REFERENCE), "uniform textbook": (du.UNIFORM, du.TEXTBOOK),
         "power textbook": (du.POWER, du.TEXTBOOK)}


@pytest.fixture(scope="module")
def emu():
    return du.DeltaEmu()


@pytest.fixture(scope="module")
def tinted(materials_scene):
    return mu.with_medium(materials_scene, mu.glass_instances(materials_scene), 1)


@pytest.fixture(scope="module")
def references(emu, materials_scene, tinted):
    """The emulation's frames, rendered once: {key: (image, counts)}."""
    s, t = emu.scene(materials_scene), emu.scene(tinted)
    out = {(name, ts0): s.render(W, H, SPP, delta=LIGHTS, first_timestamp=ts0, light_mode=lm, estimator=est) for name, (lm, est) in MODES.items() for ts0 in (0, 5)}
    out["none"] = s.render(W, H, SPP)
    out["point only"] = s.render(W, H, SPP, delta=LIGHTS[:1])
    out["absorber"] = t.render(W, H, SPP, delta=LIGHTS, media=[su.SIGMA_A])
    out["scatterer"] = t.render(W, H, SPP, delta=LIGHTS, media=[su.SIGMA_A], scatter=[(su.SIGMA_S, su.G)])
    return out


def make_ctx(mode="default"):
    import gpuspectral_amd as g

    return g.Context(0) if mode == "default" else g.Context(0, finish_paths=0xFFFFFFFF)


def frame(ctx, sc=None, ts0=0, w=W, h=H, spp=SPP, **params):
    if sc is not None:
        ctx.upload_scene(sc)
    ctx.frame_begin(w, h)
    ctx.reset_stats()
    ctx.render(spp=spp, first_timestamp=ts0, **params)
    return ctx.download().reshape(-1, 4).copy(), ctx.stats()


def agree(img, st, ref):
    rimg, rst = ref
    assert du.same(img, rimg), "%d pixels differ" % int((img != rimg).any(1).sum())
    for k in COUNTS:
        assert st[k] == rst[k], (k, st[k], rst[k])


# ---- GPU == emulation, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "wavefront-only"])
@pytest.mark.parametrize("ts0", [0, 5])
@pytest.mark.parametrize("which", list(MODES))
def test_gpu_equals_emu(materials_scene, references, mode, ts0, which):
    lm, est = MODES[which]
    with make_ctx(mode) as ctx:
        ctx.set_light_sampling(lm)
        ctx.set_estimator(est)
        ctx.set_delta_lights(LIGHTS)
        img, st = frame(ctx, materials_scene, ts0=ts0)
    agree(img, st, references[(which, ts0)])
    assert not du.same(img, references["none"][0]) and st["shadow_rays"] > references["none"][1]["shadow_rays"] // 2


def test_gpu_equals_emu_with_textures(emu, materials_scene):
    sc = textured.decorate(copy.deepcopy(materials_scene), seed=5, envmap=False)
    ref = emu.scene(sc).render(W, H, SPP, delta=LIGHTS)
    for mode in ("default", "wavefront-only"):
        with make_ctx(mode) as ctx:
            ctx.set_delta_lights(LIGHTS)
            img, st = frame(ctx, sc)
        agree(img, st, ref)


def test_gpu_equals_emu_across_a_table_edit(emu, materials_scene):
    """<VER, DLT>: gsp_update_tables between two gsp_render calls of the frame, neither drained; the delta records ride in both versions."""
    sc = copy.copy(materials_scene)
    with make_ctx() as ctx:
        ctx.set_delta_lights(LIGHTS)
        ctx.upload_scene(sc)
        ctx.frame_begin(W, H)
        ctx.reset_stats()
        ctx.render(spp=2)
        acc, c1 = emu.scene(sc).render(W, H, 2, delta=LIGHTS)
        bs = [b.copy() for b in sc.bsdfs]
        bs[0]["reflectance"][0] = (0.1, 0.5, 0.9)
        sc.bsdfs = bs
        lights = sc.lights.copy()
        lights["radiance"][:, :3] = np.array([8.0, 12.0, 17.0], np.float32)
        sc.lights = lights
        ctx.update_tables(sc)
        ctx.render(spp=2, first_timestamp=2)
        acc, c2 = emu.scene(sc).render(W, H, 2, delta=LIGHTS, first_timestamp=2, accum=acc)
        img = ctx.download().reshape(-1, 4)
        st = ctx.stats()
    assert st["scene_updates"] == 1 and st["scene_drains"] == 0, st
    agree(img, st, (acc, {k: c1[k] + c2[k] for k in COUNTS}))


@pytest.mark.parametrize("which", ["absorber", "scatterer"])
def test_gpu_equals_emu_with_media(tinted, references, which):
    with make_ctx() as ctx:
        ctx.set_media([su.SIGMA_A])
        if which == "scatterer":
            ctx.set_media_scattering([(su.SIGMA_S, su.G)])
        ctx.set_delta_lights(LIGHTS)
        img, st = frame(ctx, tinted)
        agree(img, st, references[which])
        if which == "scatterer":  # the scattering table goes: the table of zeros takes its place, and the absorber's bits come back
            ctx.set_media_scattering(None)
            img, st = frame(ctx)
            agree(img, st, references["absorber"])


def test_multi_on_two_shares_of_one_device(materials_scene, references):
    from gpuspectral_amd import pt

    with pt.MultiContext([0, 0]) as m:
        m.set_delta_lights(LIGHTS)
        m.upload_scene(materials_scene)
        m.frame_begin(W, H)
        m.render(spp=SPP)
        m.gather()
        img = m.download().reshape(-1, 4)
    assert du.same(img, references[("uniform reference", 0)][0])


# ---- the closed forms on the GPU frame ----------------------------------------------------------------------------------------------
def test_closed_forms_on_the_gpu_frame():
    sc = du.plane_scene()
    P = du.plane_points(sc)
    with make_ctx() as ctx:
        ctx.set_delta_lights([cpu.abi.point_light(cpu.POINT_POS, cpu.POINT_I)])
        img, st = frame(ctx, sc, spp=1, **du.PLANE_PARAMS)
        cpu.check_point(img, P, cpu.POINT_POS, cpu.POINT_I)
        assert st["shadow_rays"] == W * H
        ctx.set_delta_lights([cpu.abi.directional_light(cpu.SUN_DIR, cpu.SUN_E, 10.0)])
        img, _ = frame(ctx, spp=1, **du.PLANE_PARAMS)
        want = du.albedo_over_pi() * np.float64(cpu.SUN_E) * abs(cpu.SUN_DIR[2])
        assert np.abs(img[:, :3].astype(np.float64) / want[None, :] - 1.0).max() <= 43 * du.EPS
        Ps = du.plane_points(sc, cpu.SPOT_W, cpu.SPOT_H)
        ctx.set_delta_lights([cpu.spot_parts(Ps)[0]])
        img, _ = frame(ctx, w=cpu.SPOT_W, h=cpu.SPOT_H, spp=1, **du.PLANE_PARAMS)
        cpu.check_spot(img, Ps)


@pytest.mark.parametrize("case", [cpu.point_shadow_case, cpu.sun_shadow_case])
def test_hard_shadows_on_the_gpu_frame(case):
    sc, lights, expect = case()
    with make_ctx() as ctx:
        ctx.set_delta_lights(lights)
        img, _ = frame(ctx, sc, w=cpu.SH_W, h=cpu.SH_H, spp=1, **du.PLANE_PARAMS)
    cpu.check_shadow(img, **expect)


# ---- the contract ---------------------------------------------------------------------------------------------------------------------
def test_the_table_is_context_state(emu, materials_scene, references):
    import gpuspectral_amd as g

    with make_ctx() as ctx:
        img, st = frame(ctx, materials_scene)
        agree(img, st, references["none"])
        ctx.set_delta_lights(LIGHTS)  # set between frames, with the scene resident: a fresh context's frame
        img, st = frame(ctx)
        agree(img, st, references[("uniform reference", 0)])
        ctx.upload_scene(materials_scene)  # ... it survives gsp_upload_scene
        img, st = frame(ctx)
        agree(img, st, references[("uniform reference", 0)])
        sc = copy.copy(materials_scene)  # ... and gsp_update_tables
        lights = sc.lights.copy()
        lights["radiance"][:, :3] = np.array([8.0, 12.0, 17.0], np.float32)
        sc.lights = lights
        ctx.update_tables(sc)
        img, st = frame(ctx)
        agree(img, st, emu.scene(sc).render(W, H, SPP, delta=LIGHTS))
        ctx.update_tables(materials_scene)
        ctx.set_light_sampling("power")  # gsp_download_light_pick counts both kinds; the table is the emulation's, byte for byte
        table = ctx.download_light_pick()
        want, _ = emu.light_pick(materials_scene.lights, emu.check(LIGHTS)[1])
        assert len(table) == len(materials_scene.lights) + len(LIGHTS) and table.tobytes() == want.tobytes()
        ctx.set_light_sampling("uniform")
        bad = cpu.abi.spot_light((0, 1, 0), (0, -1, 0), (1, 1, 1), 0.9, 0.8)  # a refused call leaves the table as it was
        with pytest.raises(g.GspError, match="cos_beam > cos_cutoff"):
            ctx.set_delta_lights(LIGHTS[:1] + [bad])
        img, st = frame(ctx)
        agree(img, st, references[("uniform reference", 0)])
        ctx.set_delta_lights(LIGHTS[:1])
        img, st = frame(ctx)
        agree(img, st, references["point only"])
        ctx.set_delta_lights(None)  # count 0 drops the table: the kernels and the bits of a context that never had one
        img, st = frame(ctx)
        agree(img, st, references["none"])


# ---- the CLI and the C++ host ------------------------------------------------------------------------------------------------------------
def _run_cli(args):
    import os
    import subprocess

    from conftest import ROOT

    lib = os.path.join(ROOT, "gpuspectral_amd", "lib")
    env = dict(os.environ, LD_LIBRARY_PATH=lib + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([os.path.join(lib, "gsp_render")] + args, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout


def _pfm_equals(path, img, w, h):
    from oracle import mitsuba_loader as ml

    got = np.asarray(ml.read_pfm(path), np.float32).reshape(h, w, -1)[:, :, :3]
    rgb = img.reshape(h, w, 4)[:, :, :3]
    return du.same(got, rgb) or du.same(got[::-1], rgb)  # (PFM rows run bottom to top)


def test_cli_route_equals_the_api_route(tmp_path):
    from gpuspectral_amd import host
    from test_delta_loader import DEFAULTS, write_xml

    xml = write_xml(tmp_path, DEFAULTS)
    w, h, spp = 48, 36, 4
    out, out2 = str(tmp_path / "e.pfm"), str(tmp_path / "p.pfm")
    _run_cli(["--scene-emitters", xml, out, str(w), str(h), str(spp)])
    _run_cli(["--point-light", "0.5,2,-1,10,20,30", "--point-light", "-1,1,0.5,3,2,1", xml, out2, str(w), str(h), str(spp)])
    sc = host.Scene(xml, read_emitters=True)
    assert len(sc.delta_lights) == 3
    with make_ctx() as ctx:
        ctx.set_delta_lights(sc.delta_lights)
        img, st = frame(ctx, sc.arrays(), w=w, h=h, spp=spp)
        assert st["shadow_rays"] > 0 and img[:, :3].max() > 0
        ctx.set_delta_lights([cpu.abi.point_light((0.5, 2, -1), (10, 20, 30)), cpu.abi.point_light((-1, 1, 0.5), (3, 2, 1))])
        img2, _ = frame(ctx, w=w, h=h, spp=spp)
    assert _pfm_equals(out, img, w, h) and _pfm_equals(out2, img2, w, h) and not du.same(img, img2)


def test_host_tracker_sends_the_table_only_when_it_changed(tmp_path):
    """PathTracer::prepareScene compares Scene::deltaLights by value: a second pass with the same table waits for nothing (no drain,
    no update), an edited table is sent."""
    from gpuspectral_amd import host
    from test_delta_loader import DEFAULTS, write_xml

    xml = write_xml(tmp_path, DEFAULTS)
    w, h, spp = 48, 36, 2
    sc = host.Scene(xml, read_emitters=True)
    pt = host.PathTracer(w, h)
    pt.render(sc, spp)
    before = pt.stats()
    pt.render(sc, spp)  # the same table: nothing is sent, so the samples still in flight are not waited for
    after = pt.stats()
    assert after["scene_drains"] == before["scene_drains"] and after["scene_updates"] == before["scene_updates"]
    first = pt.download().reshape(-1, 4).copy()  # two calls of spp samples: one frame of 2 spp
    lights = sc.delta_lights
    sc.set_delta_lights(lights[:1])
    pt.reset()
    pt.render(sc, spp)
    second = pt.download().reshape(-1, 4).copy()
    pt.close()
    for lt, got, n in ((lights, first, 2 * spp), (lights[:1], second, spp)):
        with make_ctx() as ctx:
            ctx.set_delta_lights(lt)
            img, _ = frame(ctx, sc.arrays(), w=w, h=h, spp=n)
        assert du.same(got, img)
    assert not du.same(first, second)
