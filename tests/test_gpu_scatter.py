"""Scattering media (include/gpuspectral_pt.h, "Scattering media") on the GPU.

The wavefront pipeline with the <MED, SCT> kernels against the same stage headers run in scalar on the host
(tests/emu/scatter_emu.cpp), bit for bit, image and ray counts: alone, with textures, across a table edit, under the power pick and
the textbook estimator, on two shares; the furnace on the GPU frame itself; the table as context state; the errors; the feature
buffers; the CLI and the C++ host."""
import copy

import numpy as np
import pytest

import media_util as mu
import scatter_util as su
import textured

pytestmark = pytest.mark.gpu

COUNTS = ("extension_rays", "shadow_rays", "shaded_vertices")
W = H = 48
SPP = 4
MEDIA = [su.SIGMA_A]
SCATTER = [(su.SIGMA_S, su.G)]
SCATTER2 = [((0.5, 1.0, 6.0), -0.3)]


@pytest.fixture(scope="module")
def emu():
    return su.ScatterEmu()


@pytest.fixture(scope="module")
def tinted(materials_scene):
    """cornell_materials(16) with medium 1 on the glass sphere."""
    return mu.with_medium(materials_scene, mu.glass_instances(materials_scene), 1)


@pytest.fixture(scope="module")
def references(emu, tinted):
    """The emulation's frames of `tinted`, rendered once: {key: (image, counts)}."""
    s = emu.scene(tinted)
    out = {("sct", ts0): s.render(W, H, SPP, media=MEDIA, scatter=SCATTER, first_timestamp=ts0) for ts0 in (0, 5)}
    out["sct2"] = s.render(W, H, SPP, media=MEDIA, scatter=SCATTER2)
    out["absorber"] = s.render(W, H, SPP, media=MEDIA)
    out["power"] = s.render(W, H, SPP, media=MEDIA, scatter=SCATTER, light_mode=su.POWER)
    out["textbook"] = s.render(W, H, SPP, media=MEDIA, scatter=SCATTER, estimator=su.TEXTBOOK)
    out["textbook power"] = s.render(W, H, SPP, media=MEDIA, scatter=SCATTER, estimator=su.TEXTBOOK, light_mode=su.POWER)
    return out


def make_ctx(mode="default"):
    import gpuspectral_amd as g

    return g.Context(0) if mode == "default" else g.Context(0, finish_paths=0xFFFFFFFF)


def frame(ctx, sc, media, scatter, calls=(SPP,), ts0=0, upload=True, w=W, h=H, **params):
    if upload:
        ctx.set_media(media)
        ctx.set_media_scattering(scatter)
        ctx.upload_scene(sc)
    ctx.frame_begin(w, h)
    ctx.reset_stats()
    t = ts0
    for spp in calls:
        ctx.render(spp=spp, first_timestamp=t, **params)
        t += spp
    return ctx.download().reshape(-1, 4).copy(), ctx.stats()


def agree(img, st, ref):
    rimg, rst = ref
    assert su.same(img, rimg), "%d pixels differ" % int((img != rimg).any(1).sum())
    for k in COUNTS:
        assert st[k] == rst[k], (k, st[k], rst[k])


# ---- 6: GPU == emulation, bit for bit --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "wavefront-only"])
@pytest.mark.parametrize("ts0", [0, 5])
def test_gpu_equals_emu(tinted, references, mode, ts0):
    with make_ctx(mode) as ctx:
        img, st = frame(ctx, tinted, MEDIA, SCATTER, ts0=ts0)
    agree(img, st, references[("sct", ts0)])
    assert not su.same(img, references["absorber"][0]) and references[("sct", ts0)][1]["medium_events"] > 100


def test_gpu_equals_emu_with_textures(emu, materials_scene):
    """<TEX, MED, SCT>: the textured room of test_gpu_textures.py with the medium on its glass sphere."""
    sc = textured.decorate(copy.deepcopy(materials_scene), seed=5, envmap=False)
    sc = mu.with_medium(sc, mu.glass_instances(sc), 1)
    ref = emu.scene(sc).render(W, H, SPP, media=MEDIA, scatter=SCATTER)
    for mode in ("default", "wavefront-only"):
        with make_ctx(mode) as ctx:
            img, st = frame(ctx, sc, MEDIA, SCATTER)
        agree(img, st, ref)


def test_gpu_equals_emu_across_a_table_edit(emu, tinted):
    """<VER, MED, SCT>: gsp_update_tables between two gsp_render calls of the frame, neither drained."""
    sc = copy.copy(tinted)
    with make_ctx() as ctx:
        ctx.set_media(MEDIA)
        ctx.set_media_scattering(SCATTER)
        ctx.upload_scene(sc)
        ctx.frame_begin(W, H)
        ctx.reset_stats()
        ctx.render(spp=2)
        acc, c1 = emu.scene(sc).render(W, H, 2, media=MEDIA, scatter=SCATTER)
        bs = [b.copy() for b in sc.bsdfs]
        bs[0]["reflectance"][0] = (0.1, 0.5, 0.9)
        sc.bsdfs = bs
        lights = sc.lights.copy()
        lights["radiance"][:, :3] = np.array([8.0, 12.0, 17.0], np.float32)
        sc.lights = lights
        ctx.update_tables(sc)
        ctx.render(spp=2, first_timestamp=2)
        acc, c2 = emu.scene(sc).render(W, H, 2, media=MEDIA, scatter=SCATTER, first_timestamp=2, accum=acc)
        img = ctx.download().reshape(-1, 4)
        st = ctx.stats()
    assert st["scene_updates"] == 1 and st["scene_drains"] == 0, st
    agree(img, st, (acc, {k: c1[k] + c2[k] for k in COUNTS}))


@pytest.mark.parametrize("mode", ["default", "wavefront-only"])
@pytest.mark.parametrize("which", ["power", "textbook", "textbook power"])
def test_gpu_equals_emu_under_the_power_pick_and_the_textbook_estimator(tinted, references, mode, which):
    with make_ctx(mode) as ctx:
        if "power" in which:
            ctx.set_light_sampling("power")
        if "textbook" in which:
            ctx.set_estimator("textbook")
        img, st = frame(ctx, tinted, MEDIA, SCATTER)
    agree(img, st, references[which])
    assert not su.same(img, references[("sct", 0)][0])


def test_multi_on_two_shares_of_one_device(tinted, references):
    from gpuspectral_amd import pt

    with pt.MultiContext([0, 0]) as m:
        m.set_media(MEDIA)
        m.set_media_scattering(SCATTER)
        m.upload_scene(tinted)
        m.frame_begin(W, H)
        m.render(spp=SPP)
        m.gather()
        img = m.download().reshape(-1, 4)
    assert su.same(img, references[("sct", 0)][0])


# ---- 7: the furnace on the GPU frame ---------------------------------------------------------------------------------------------
def gpu_furnace(ctx, n, spp, sigma_a, sigma_s, g=0.0, ts0=0, upload=True, **over):
    params = dict(su.FURNACE_PARAMS, **over)
    return frame(ctx, su.furnace_scene(), [sigma_a], [(sigma_s, g)], calls=(spp,), ts0=ts0, w=n, h=n, upload=upload, **params)[0]


@pytest.mark.parametrize("rr", ["off", "on"])
def test_furnace_grey_albedo_one_is_L_everywhere(emu, rr):
    over = {} if rr == "off" else dict(rr_start_depth=3)
    with make_ctx() as ctx:
        img = gpu_furnace(ctx, 32, 2, (0, 0, 0), (2.0, 2.0, 2.0), **over)
    su.check_furnace_white(img, spp=2, rr=rr == "on")
    ref = emu.scene(su.furnace_scene()).render(32, 32, 2, media=[(0, 0, 0)], scatter=[((2.0, 2.0, 2.0), 0.0)], **dict(su.FURNACE_PARAMS, **over))[0]
    assert su.same(img, ref)


def test_furnace_grey_half_albedo_samples_are_powers_and_follow_the_free_path_law():
    n = 32
    with make_ctx() as ctx:
        frames = [gpu_furnace(ctx, n, 1, (1.0, 1.0, 1.0), (1.0, 1.0, 1.0), ts0=ts, upload=ts == 0) for ts in range(16)]
    su.check_furnace_half(frames, n, sigma_a=1.0, sigma_t=2.0, albedo=0.5, timestamps=range(16))


@pytest.mark.parametrize("albedo,g", [(0.25, 0.0), (0.9, 0.6), (1.0, -0.5)])
def test_furnace_no_channel_exceeds_L(albedo, g):
    st = 3.0
    with make_ctx() as ctx:
        img = gpu_furnace(ctx, 32, 4, (st * (1 - albedo),) * 3, (st * albedo,) * 3, g=g)
    su.check_furnace_bounded(img)


# ---- 9: the contract -------------------------------------------------------------------------------------------------------------
def test_set_media_scattering_between_frames_equals_a_fresh_context(tinted, references):
    with make_ctx() as ctx:
        img, st = frame(ctx, tinted, MEDIA, SCATTER)
        agree(img, st, references[("sct", 0)])
        ctx.set_media_scattering(SCATTER2)
        img2, st2 = frame(ctx, tinted, MEDIA, SCATTER2, upload=False)
        agree(img2, st2, references["sct2"])
        ctx.set_media_scattering(None)  # back to the absorber: the <MED> kernels and their bits
        img3, st3 = frame(ctx, tinted, MEDIA, None, upload=False)
        agree(img3, st3, references["absorber"])
        ctx.set_media_scattering([((0.0, 0.0, 0.0), 0.9)])  # a table that scatters nowhere: the same
        img4, st4 = frame(ctx, tinted, MEDIA, None, upload=False)
        agree(img4, st4, references["absorber"])


def test_errors_and_the_dropped_table(materials_scene, tinted, references):
    import gpuspectral_amd as g

    with make_ctx() as ctx:
        with pytest.raises(g.GspError, match="media count"):
            ctx.set_media_scattering(SCATTER)  # no media yet
        ctx.set_media(MEDIA)
        for bad in ((-1.0, 0.0, 0.0), (0.0, float("nan"), 0.0), (0.0, 0.0, float("inf"))):
            with pytest.raises(g.GspError, match="finite and >= 0"):
                ctx.set_media_scattering([(bad, 0.0)])
        for gg in (1.0, -1.0, float("nan")):
            with pytest.raises(g.GspError, match=r"\|g\| < 1"):
                ctx.set_media_scattering([((1.0, 1.0, 1.0), gg)])
        with pytest.raises(g.GspError, match="media count"):
            ctx.set_media_scattering(SCATTER * 2)
        ctx.set_media_scattering(SCATTER)
        img, st = frame(ctx, tinted, MEDIA, SCATTER)
        agree(img, st, references[("sct", 0)])
        with pytest.raises(g.GspError, match="media count"):  # a refused call leaves the table as it was
            ctx.set_media_scattering(SCATTER * 2)
        img, st = frame(ctx, tinted, MEDIA, SCATTER, upload=False)
        agree(img, st, references[("sct", 0)])
        ctx.set_media(MEDIA)  # the same count keeps the scattering table
        img, st = frame(ctx, tinted, MEDIA, SCATTER, upload=False)
        agree(img, st, references[("sct", 0)])
        ctx.set_media(MEDIA + [mu.SLAB_SIGMA])  # another count drops it
        img, st = frame(ctx, tinted, MEDIA, None, upload=False)
        agree(img, st, references["absorber"])
        with pytest.raises(g.GspError, match="media count"):
            ctx.set_media_scattering(SCATTER)
        ctx.set_media_scattering(SCATTER + [((0.0, 0.0, 0.0), 0.0)])
        img, st = frame(ctx, tinted, MEDIA, SCATTER, upload=False)
        agree(img, st, references[("sct", 0)])


def test_features_are_unchanged(tinted):
    planes = []
    with make_ctx() as ctx:
        for scatter in (None, SCATTER):
            frame(ctx, tinted, MEDIA, scatter, calls=(1,))
            ctx.render_features(spp=2)
            planes.append(ctx.download_features())
    (a0, g0, i0), (a1, g1, i1) = planes
    assert np.array_equal(i0, i1) and su.same(a0, a1) and su.same(g0, g1)


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
    return su.same(got, rgb) or su.same(got[::-1], rgb)  # (PFM rows run bottom to top)


def _tables(sc):
    return [tuple(m) for m in sc.media.tolist()], [(tuple(m[:3]), float(m[3])) for m in sc.media_scattering.tolist()]


def test_cli_scene_scattering_equals_the_api_route(tmp_path):
    from gpuspectral_amd import host
    from test_scatter_loader import write_scatter_xml

    xml = write_scatter_xml(tmp_path)
    w, h, spp = 64, 48, 4
    out, out0 = str(tmp_path / "s.pfm"), str(tmp_path / "m.pfm")
    _run_cli(["--scene-scattering", xml, out, str(w), str(h), str(spp)])
    _run_cli(["--scene-media", xml, out0, str(w), str(h), str(spp)])
    sc, sc0 = host.Scene(xml, read_scattering=True), host.Scene(xml, read_media=True)
    with make_ctx() as ctx:
        img, _ = frame(ctx, sc.arrays(), *_tables(sc), calls=(spp,), w=w, h=h)
    with make_ctx() as ctx:
        absorbers, _ = frame(ctx, sc0.arrays(), _tables(sc0)[0], None, calls=(spp,), w=w, h=h)
    assert _pfm_equals(out, img, w, h) and _pfm_equals(out0, absorbers, w, h)
    assert not su.same(img, absorbers)


def test_host_tracker_sends_and_updates_the_table(tmp_path):
    """PathTracer::prepareScene: the scattering table goes behind the media table, and an edit (another scatterer on another
    object) is noticed by value."""
    from gpuspectral_amd import host
    from test_scatter_loader import write_scatter_xml

    xml = write_scatter_xml(tmp_path)
    w, h, spp = 64, 48, 4
    sc = host.Scene(xml, read_scattering=True)
    pt = host.PathTracer(w, h)
    frames, arrays, tables = [], [], []
    for step in range(2):
        if step == 1:
            sc.set_object_medium(6, sc.add_scattering_medium((0.5, 0.5, 0.5), (9.0, 0.5, 7.0), -0.4))
            pt.reset()
        pt.render(sc, spp)
        frames.append(pt.download().reshape(-1, 4).copy())
        arrays.append(sc.arrays())
        tables.append(_tables(sc))
    pt.close()
    assert len(tables[1][1]) == 4 and not su.same(frames[0], frames[1])
    for k in range(2):
        with make_ctx() as ctx:
            img, _ = frame(ctx, arrays[k], *tables[k], calls=(spp,), w=w, h=h)
        assert su.same(frames[k], img), k
