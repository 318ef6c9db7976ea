"""Interior media (include/gpuspectral_pt.h, "Interior media") on the GPU.

The wavefront pipeline with the <MED> kernels against the same stage headers run in scalar on the host (tests/emu/media_emu.cpp),
bit for bit, image and ray counts: alone, with textures (<TEX, MED>), across a table edit (<VER, MED>), on a split scene; the
analytic slab; zero absorption; the media as context state; the errors; the feature buffers; every share of a multi context."""
import copy

import numpy as np
import pytest

import media_util as mu
import textured

pytestmark = pytest.mark.gpu

COUNTS = ("extension_rays", "shadow_rays", "shaded_vertices")
W = H = 48
SPP = 4
SIGMA = (1.0, 3.0, 5.0)
SIGMA2 = (4.0, 0.5, 0.25)


@pytest.fixture(scope="module")
def emu():
    return mu.MediaEmu()


@pytest.fixture(scope="module")
def tinted(materials_scene):
    """cornell_materials(16) with medium 1 on the glass sphere."""
    return mu.with_medium(materials_scene, mu.glass_instances(materials_scene), 1)


@pytest.fixture(scope="module")
def references(emu, tinted):
    """The emulation's frames of `tinted`, rendered once: {(sigma, first timestamp): (image, counts)}."""
    s = emu.scene(tinted)
    return {(sig, ts0): s.render(W, H, SPP, media=[sig], first_timestamp=ts0) for sig, ts0 in ((SIGMA, 0), (SIGMA, 5), (SIGMA2, 0))}


def make_ctx(mode):
    import gpuspectral_amd as g

    return g.Context(0) if mode == "default" else g.Context(0, finish_paths=0xFFFFFFFF)


def frame(ctx, sc, media, calls=(SPP,), ts0=0, upload=True, w=W, h=H):
    if upload:  # (a scene that names medium k wants the table first; a table can only shrink once no resident scene names its end)
        if int(((sc.instances["bsdf"] >> 19) & 0xFFF).max()) > 0:
            ctx.set_media(media)
            ctx.upload_scene(sc)
        else:
            ctx.upload_scene(sc)
            ctx.set_media(media)
    ctx.frame_begin(w, h)
    ctx.reset_stats()
    t = ts0
    for spp in calls:
        ctx.render(spp=spp, first_timestamp=t)
        t += spp
    return ctx.download().reshape(-1, 4).copy(), ctx.stats()


def agree(img, st, ref):
    rimg, rst = ref
    assert mu.same(img, rimg), "%d pixels differ" % int((img != rimg).any(1).sum())
    for k in COUNTS:
        assert st[k] == rst[k], (k, st[k], rst[k])


# ---- 7: GPU == emu, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "wavefront-only"])
@pytest.mark.parametrize("ts0", [0, 5])
def test_gpu_equals_emu(tinted, references, mode, ts0):
    with make_ctx(mode) as ctx:
        img, st = frame(ctx, tinted, [SIGMA], ts0=ts0)
    agree(img, st, references[(SIGMA, ts0)])


def test_gpu_equals_emu_with_textures(emu, materials_scene):
    """<TEX, MED>: the textured room of test_gpu_textures.py with the medium on its glass sphere."""
    sc = textured.decorate(copy.deepcopy(materials_scene), seed=5, envmap=False)
    sc = mu.with_medium(sc, mu.glass_instances(sc), 1)
    ref = emu.scene(sc).render(W, H, SPP, media=[SIGMA])
    plain, _ = emu.scene(sc).render(W, H, SPP, media=[(0.0, 0.0, 0.0)])
    assert not mu.same(ref[0], plain)
    for mode in ("default", "wavefront-only"):
        with make_ctx(mode) as ctx:
            img, st = frame(ctx, sc, [SIGMA])
        agree(img, st, ref)


def test_gpu_equals_emu_across_a_table_edit(emu, tinted):
    """<VER, MED>: gsp_update_tables between two gsp_render calls of the frame, neither drained: the samples of the first call
    finish on their version of the tables next to those of the second.  The frame is the running mean over the two scenes."""
    import gpuspectral_amd as g

    sc = copy.copy(tinted)
    with g.Context(0) as ctx:
        ctx.set_media([SIGMA])
        ctx.upload_scene(sc)
        ctx.frame_begin(W, H)
        ctx.reset_stats()
        ctx.render(spp=2)
        acc, c1 = emu.scene(sc).render(W, H, 2, media=[SIGMA])
        bs = [b.copy() for b in sc.bsdfs]
        bs[0]["reflectance"][0] = (0.1, 0.5, 0.9)
        sc.bsdfs = bs
        lights = sc.lights.copy()
        lights["radiance"][:, :3] = np.array([8.0, 12.0, 17.0], np.float32)
        sc.lights = lights
        ctx.update_tables(sc)
        ctx.render(spp=2, first_timestamp=2)
        acc, c2 = emu.scene(sc).render(W, H, 2, media=[SIGMA], first_timestamp=2, accum=acc)
        img = ctx.download().reshape(-1, 4)
        st = ctx.stats()
    assert st["scene_updates"] == 1 and st["scene_drains"] == 0, st  # (the first call's samples were in flight at the edit)
    agree(img, st, (acc, {k: c1[k] + c2[k] for k in COUNTS}))


# ---- 8: the analytic slab --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def slab_frames(emu):
    """(GPU frame without media, GPU frame with the medium, emu frame with the medium) of the slab, 32 x 32 at 8 spp."""
    n = 32
    with make_ctx("default") as ctx:
        plain, _ = frame(ctx, mu.slab_scene(), None, calls=(8,), w=n, h=n)
        img, _ = frame(ctx, mu.slab_scene(1), [mu.SLAB_SIGMA], calls=(8,), w=n, h=n)
    ref, _ = emu.scene(mu.slab_scene(1)).render(n, n, 8, media=[mu.SLAB_SIGMA])
    return plain, img, ref


def test_slab_equals_emu_and_keeps_the_pixels_outside(slab_frames):
    plain, img, ref = slab_frames
    _, inside, outside = mu.slab_reference(32, 32)
    assert (~(inside | outside)).mean() <= 0.08
    assert mu.same(img, ref)
    assert mu.same(img[outside], plain[outside])
    assert np.abs(plain[:, :3] - np.float32(mu.SLAB_EMISSION)).max() <= 1e-6


def test_slab_matches_beer_lambert(slab_frames):
    """L_c * exp(-sigma_c * 0.5 / cos(theta)), float64, relative tolerance 1e-5, as tests/test_media_cpu.py asks of the emulation
    (the GPU frame is the emulation's bit for bit: 4.7e-7 / 1.8e-6 / 3.9e-6 in r / g / b)."""
    plain, img, ref = slab_frames
    expected, inside, outside = mu.slab_reference(32, 32)
    rel = np.abs(img[inside, :3].astype(np.float64) - expected[inside]) / expected[inside]
    print("slab on the GPU: largest relative error per channel against L exp(-sigma 0.5 / cos):", rel.max(0))
    assert rel.max() <= 1e-5


# ---- 9: zero sigma ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "wavefront-only"])
def test_zero_sigma_equals_no_media(materials_scene, tinted, mode):
    with make_ctx(mode) as ctx:
        ref, rst = frame(ctx, materials_scene, None)
        img, st = frame(ctx, tinted, [(0.0, 0.0, 0.0)])
    agree(img, st, (ref, rst))


# ---- 10: edits -------------------------------------------------------------------------------------------------------------------
def moved(sc):
    inst = sc.instances.copy()
    k = int(mu.glass_instances(sc)[0])
    t = inst["transform"][k].copy()
    t[12:15] += np.float32([0.12, 0.05, 0.2])
    inst["transform"][k] = t
    out = copy.copy(sc)
    out.instances = inst
    return out


@pytest.mark.parametrize("when", ["in flight", "idle"])
def test_moved_sphere_equals_a_fresh_upload(tinted, when):
    """gsp_update_instances moves the glass sphere: with samples in flight (the split arm: the edited instance gets a tree of its
    own and the <VER, MED> kernels run from then on) and on an idle context (a refit of the whole tree)."""
    import gpuspectral_amd as g

    sc2 = moved(tinted)
    with g.Context(0) as ctx:
        fresh, fst = frame(ctx, sc2, [SIGMA])
    with g.Context(0) as ctx:
        frame(ctx, tinted, [SIGMA], calls=(2,))
        if when == "in flight":
            ctx.frame_begin(W, H)
            ctx.render(spp=2)  # queued, not waited for
        ctx.update_instances(sc2.instances)
        st = ctx.stats()
        assert st["scene_updates"] == 1
        assert (st["scene_splits"] == 1) if when == "in flight" else (st["scene_refits"] == 1), st
        img, ist = frame(ctx, sc2, [SIGMA], upload=False)
    agree(img, ist, (fresh, fst))
    assert not mu.same(img, frame_of_unmoved(tinted))


_unmoved = {}


def frame_of_unmoved(tinted):
    import gpuspectral_amd as g

    if "img" not in _unmoved:
        with g.Context(0) as ctx:
            _unmoved["img"] = frame(ctx, tinted, [SIGMA])[0]
    return _unmoved["img"]


def test_set_media_between_frames_equals_a_fresh_context(tinted, references):
    import gpuspectral_amd as g

    with g.Context(0) as ctx:
        img, st = frame(ctx, tinted, [SIGMA])
        agree(img, st, references[(SIGMA, 0)])
        ctx.set_media([SIGMA2])
        img2, st2 = frame(ctx, tinted, [SIGMA2], upload=False)
    agree(img2, st2, references[(SIGMA2, 0)])
    assert not mu.same(img, img2)


def test_set_media_between_the_calls_of_one_frame(emu, tinted):
    """The samples in flight finish on the table they started with (the wait of every scene edit)."""
    import gpuspectral_amd as g

    s = emu.scene(tinted)
    acc, _ = s.render(W, H, 2, media=[SIGMA])
    acc, _ = s.render(W, H, 2, media=[SIGMA2], first_timestamp=2, accum=acc)
    with g.Context(0) as ctx:
        ctx.set_media([SIGMA])
        ctx.upload_scene(tinted)
        ctx.frame_begin(W, H)
        ctx.render(spp=2)
        ctx.set_media([SIGMA2])
        ctx.render(spp=2, first_timestamp=2)
        img = ctx.download().reshape(-1, 4)
    assert mu.same(img, acc)


# ---- 11: errors ------------------------------------------------------------------------------------------------------------------
def test_set_media_contract(materials_scene, tinted, references):
    import gpuspectral_amd as g

    with g.Context(0) as ctx:
        for bad in ([(-1.0, 0.0, 0.0)], [(0.0, float("nan"), 0.0)], [(0.0, 0.0, float("inf"))]):
            with pytest.raises(g.GspError, match="finite and >= 0"):
                ctx.set_media(bad)
        with pytest.raises(g.GspError, match="4095"):
            ctx.set_media([(1.0, 1.0, 1.0)] * 4096)
        ctx.set_media([(1.0, 1.0, 1.0)] * 4095)
        ctx.set_media(None)
        # a medium number above the count: at upload ...
        with pytest.raises(g.GspError, match="BSDF handle out of range"):
            ctx.upload_scene(tinted)
        ctx.set_media([SIGMA])
        two = mu.with_medium(materials_scene, mu.glass_instances(materials_scene), 2)
        with pytest.raises(g.GspError, match="BSDF handle out of range"):
            ctx.upload_scene(two)
        ctx.upload_scene(tinted)
        # ... and at gsp_update_instances
        with pytest.raises(g.GspError, match="BSDF handle out of range"):
            ctx.update_instances(two.instances)
        # shrinking the table under the resident scene: refused, and the scene still renders with the table it had
        with pytest.raises(g.GspError, match="medium number above the new count"):
            ctx.set_media(None)
        img, st = frame(ctx, tinted, [SIGMA], upload=False)
        agree(img, st, references[(SIGMA, 0)])
        ctx.set_media([SIGMA, SIGMA2])  # growing it is fine
        ctx.update_instances(two.instances)
        img2, st2 = frame(ctx, two, [SIGMA, SIGMA2], upload=False)
        agree(img2, st2, references[(SIGMA2, 0)])


# ---- 12: feature buffers ---------------------------------------------------------------------------------------------------------
def test_features_report_the_handle_without_the_medium(materials_scene, tinted):
    import gpuspectral_amd as g

    planes = []
    with g.Context(0) as ctx:
        for sc, media in ((materials_scene, None), (tinted, [SIGMA])):
            frame(ctx, sc, media, calls=(1,))
            ctx.render_features(spp=2)
            planes.append(ctx.download_features())
    (a0, g0, i0), (a1, g1, i1) = planes
    assert np.array_equal(i0, i1) and mu.same(a0, a1) and mu.same(g0, g1)
    glass = int(materials_scene.instances["bsdf"][mu.glass_instances(materials_scene)[0]])
    assert (i1[..., 1] == glass).any() and int(i1[..., 1][i1[..., 1] != 0xFFFFFFFF].max()) < (1 << 19)


# ---- 13: gsp_multi_set_media -----------------------------------------------------------------------------------------------------
def _gpus():
    import gpuspectral_amd as g

    return g.device_count()


def multi_frame(devices, tinted):
    from gpuspectral_amd import pt

    with pt.MultiContext(devices) as m:
        m.set_media([SIGMA])
        m.upload_scene(tinted)
        m.frame_begin(W, H)
        m.render(spp=SPP)
        m.gather()
        return m.download().reshape(-1, 4)


def test_multi_set_media_on_two_shares_of_one_device(tinted, references):
    assert mu.same(multi_frame([0, 0], tinted), references[(SIGMA, 0)][0])


@pytest.mark.skipif("_gpus() < 2", reason="needs >= 2 physical GPUs (the test pool has one)")
def test_multi_set_media_on_every_visible_device(tinted, references):
    assert mu.same(multi_frame(list(range(_gpus())), tinted), references[(SIGMA, 0)][0])


# ---- 14: the C++ host and the CLI ------------------------------------------------------------------------------------------------
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
    return mu.same(got, rgb) or mu.same(got[::-1], rgb)  # (PFM rows run bottom to top)


def test_cli_scene_media_equals_the_api_route(tmp_path):
    import gpuspectral_amd as g
    from gpuspectral_amd import host
    from test_media_loader import write_media_xml

    xml = write_media_xml(tmp_path)
    w, h, spp = 64, 48, 4
    out, out0 = str(tmp_path / "m.pfm"), str(tmp_path / "p.pfm")
    _run_cli(["--scene-media", xml, out, str(w), str(h), str(spp)])
    _run_cli([xml, out0, str(w), str(h), str(spp)])  # without the flag: the reference's clear glass
    sc = host.Scene(xml, read_media=True)
    with g.Context(0) as ctx:
        img, _ = frame(ctx, sc.arrays(), [tuple(m) for m in sc.media.tolist()], calls=(spp,), w=w, h=h)
        clear, _ = frame(ctx, host.Scene(xml).arrays(), None, calls=(spp,), w=w, h=h)
    assert _pfm_equals(out, img, w, h) and _pfm_equals(out0, clear, w, h)
    assert not mu.same(img, clear)


def test_host_tracker_sends_the_media_and_notices_a_change(tmp_path):
    """PathTracer::prepareScene: the media table goes before the scene that names it, and a medium edited between two passes
    (another entry on another object) is noticed by value."""
    import gpuspectral_amd as g
    from gpuspectral_amd import host
    from test_media_loader import write_media_xml

    xml = write_media_xml(tmp_path)
    w, h, spp = 64, 48, 4
    sc = host.Scene(xml, read_media=True)
    pt = host.PathTracer(w, h)
    frames = []
    pt.render(sc, spp)
    frames.append(pt.download().reshape(-1, 4).copy())
    arrays = [sc.arrays()]
    tables = [[tuple(m) for m in sc.media.tolist()]]
    sc.set_object_medium(5, sc.add_medium((9.0, 0.5, 7.0)))
    pt.reset()
    pt.render(sc, spp)
    frames.append(pt.download().reshape(-1, 4).copy())
    arrays.append(sc.arrays())
    tables.append([tuple(m) for m in sc.media.tolist()])
    pt.close()
    assert len(tables[1]) == 3 and not mu.same(frames[0], frames[1])
    for k in range(2):
        with g.Context(0) as ctx:
            img, _ = frame(ctx, arrays[k], tables[k], calls=(spp,), w=w, h=h)
        assert mu.same(frames[k], img), k
