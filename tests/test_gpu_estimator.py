"""The textbook estimator (include/gpuspectral_pt.h, "Estimator") on the GPU.

The wavefront pipeline with the <EST> kernels and the textbook any-hit sources against the CPU oracle under its test-only mask
(oracle_set_quirks_off(1 | 2 | 8)), bit for bit, image and ray counts; and against the same stage headers run in scalar on the
host (tests/emu/estimator_emu.cpp) where the oracle cannot follow: textures (<TEX, EST>), media (<MED, EST>), the power pick with
the tables in LDS and in global memory (<LSEL, EST>), an undrained table edit (<VER, EST>), a sphere moved with samples in flight (the
split-scene any-hit source) and a scene edited whole (the ring source), adaptive sampling, two shares of a multi context, the mode
switched between frames and between the calls of a frame; the occluded-commit case; the interface; and the kernel digest."""
import copy
import json
import os
import subprocess

import numpy as np
import pytest

import estimator_util as eu
import lights_util as lu
import textured
from conftest import ROOT

pytestmark = pytest.mark.gpu

W, H = 56, 40  # (2240 pixels: several 256-thread tiles, no multiple of the tile)
SPP = 4
LIGHTS = (3, 130)  # the table image fits the 8192 bytes of LDS / stays in global memory
MODES = {"uniform": eu.UNIFORM, "power": eu.POWER}


@pytest.fixture(scope="module")
def emu():
    return eu.EstimatorEmu()


@pytest.fixture(scope="module")
def rooms():
    return {n: lu.room_scene(n) for n in LIGHTS}


@pytest.fixture(scope="module")
def references(emu, rooms):
    """The emulation's textbook frames of the rooms, rendered once: {(lights, light mode): (image, counts)}."""
    return {(n, lm): emu.scene(rooms[n]).render(W, H, SPP, estimator=eu.TEXTBOOK, light_mode=MODES[lm]) for n in LIGHTS for lm in MODES}


def make_ctx(kind):
    import gpuspectral_amd as g

    return g.Context(0) if kind == "default" else g.Context(0, finish_paths=0xFFFFFFFF)


def frame(ctx, sc, estimator="textbook", light_mode=None, calls=(SPP,), ts0=0, upload=True, media=None, size=(W, H), **params):
    if estimator is not None:
        ctx.set_estimator(estimator)
    if light_mode is not None:
        ctx.set_light_sampling(light_mode)
    if upload:
        if media is not None:
            ctx.set_media(media)
        ctx.upload_scene(sc)
    ctx.frame_begin(*size)
    ctx.reset_stats()
    t = ts0
    for spp in calls:
        ctx.render(spp=spp, first_timestamp=t, **params)
        t += spp
    return ctx.download().reshape(-1, 4).copy(), ctx.stats()


def agree(img, st, ref):
    rimg, rst = ref
    assert eu.same(img, rimg), "%d pixels differ" % int((np.asarray(img).reshape(-1, 4) != np.asarray(rimg).reshape(-1, 4)).any(1).sum())
    for k in eu.COUNT_KEYS:
        assert st[k] == rst[k], (k, st[k], rst[k])


# ---- GPU == the oracle with the three quirks off -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["default", "wavefront-only"])
@pytest.mark.parametrize("ts0", [0, 5])
@pytest.mark.parametrize("name", sorted(eu.FRAMES))
def test_gpu_equals_the_textbook_oracle(name, ts0, kind):
    """Image and ray counts.  The default context ends its frame in k_finish<.., EST>; the wavefront-only one runs k_shade<.., EST> and the
    textbook any-hit source to the last path."""
    w, h, spp = eu.FRAMES[name]
    try:
        ref = eu.oracle_frame(name, ts0)
    finally:
        assert eu.oracle_quirks_off() == 0
    with make_ctx(kind) as ctx:
        img, st = frame(ctx, eu.frame_scene(name), calls=(spp,), ts0=ts0, size=(w, h))
    agree(img, st, ref)


# ---- GPU == emulation where the oracle cannot follow ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["default", "wavefront-only"])
@pytest.mark.parametrize("n", LIGHTS)
def test_gpu_equals_emu_under_the_power_pick(rooms, references, kind, n):
    """<LSEL, EST>: p_sel of the light that was hit through the trailing record behind the alias table, in LDS (3 lights) and in
    global memory (130)."""
    with make_ctx(kind) as ctx:
        img, st = frame(ctx, rooms[n], light_mode="power")
    agree(img, st, references[(n, "power")])
    assert not eu.same(img, references[(n, "uniform")][0])


def test_light_pick_table_keeps_its_count_and_bytes_in_textbook_mode(rooms):
    """The trailing record sits BEHIND the table: gsp_download_light_pick returns what it returned."""
    import gpuspectral_amd as g

    want = lu.LightsEmu().build(rooms[130].lights)
    with g.Context(0) as ctx:
        ctx.set_light_sampling("power")
        ctx.upload_scene(rooms[130])
        ctx.set_estimator("textbook")  # under the resident scene: repacked with the record
        got = ctx.download_light_pick()
        assert len(got) == 130 and got.tobytes() == want.tobytes()
        ctx.set_estimator("reference")
        assert ctx.download_light_pick().tobytes() == want.tobytes()


@pytest.mark.parametrize("light_mode", sorted(MODES))
def test_gpu_equals_emu_with_textures(emu, rooms, light_mode):
    """<TEX, EST> and <TEX, LSEL, EST>."""
    sc = textured.decorate(copy.deepcopy(rooms[3]), seed=5, envmap=False)
    ref = emu.scene(sc).render(W, H, SPP, estimator=eu.TEXTBOOK, light_mode=MODES[light_mode])
    for kind in ("default", "wavefront-only"):
        with make_ctx(kind) as ctx:
            img, st = frame(ctx, sc, light_mode=light_mode)
        agree(img, st, ref)


def test_gpu_equals_emu_with_media(emu, rooms):
    """<MED, EST>: the glass sphere of the room absorbs."""
    import media_util as mu

    sigma = (1.0, 3.0, 5.0)
    sc = mu.with_medium(rooms[3], mu.glass_instances(rooms[3]), 1)
    ref = emu.scene(sc).render(W, H, SPP, estimator=eu.TEXTBOOK, media=[sigma])
    assert not eu.same(ref[0], emu.scene(sc).render(W, H, SPP, estimator=eu.TEXTBOOK, media=[(0.0, 0.0, 0.0)])[0])
    for kind in ("default", "wavefront-only"):
        with make_ctx(kind) as ctx:
            img, st = frame(ctx, sc, media=[sigma])
        agree(img, st, ref)


@pytest.mark.parametrize("light_mode", sorted(MODES))
def test_gpu_equals_emu_across_a_table_edit(emu, rooms, light_mode):
    """<VER, EST>: gsp_update_tables changes a light's radiance between two gsp_render calls of the frame, neither drained.  Under the
    power pick every version of the tables has its own alias table AND its own trailing record (another sum of weights)."""
    import gpuspectral_amd as g

    sc = copy.copy(rooms[3])
    lm = MODES[light_mode]
    with g.Context(0) as ctx:
        ctx.set_estimator("textbook")
        ctx.set_light_sampling(light_mode)
        ctx.upload_scene(sc)
        ctx.frame_begin(W, H)
        ctx.reset_stats()
        ctx.render(spp=2)
        acc, c1 = emu.scene(sc).render(W, H, 2, estimator=eu.TEXTBOOK, light_mode=lm)
        lights = sc.lights.copy()
        lights["radiance"][0, :3] *= np.float32(40.0)
        sc.lights = lights
        ctx.update_tables(sc)
        ctx.render(spp=2, first_timestamp=2)
        acc, c2 = emu.scene(sc).render(W, H, 2, estimator=eu.TEXTBOOK, light_mode=lm, first_timestamp=2, accum=acc)
        img = ctx.download().reshape(-1, 4)
        st = ctx.stats()
    assert st["scene_updates"] == 1 and st["scene_drains"] == 0, st  # (the first call's samples were in flight at the edit)
    agree(img, st, (acc, {k: c1[k] + c2[k] for k in eu.COUNT_KEYS}))


def _moved(sc, which, delta):
    inst = sc.instances.copy()
    for k in which:
        t = inst["transform"][k].copy()
        t[12:15] += np.float32(delta)
        inst["transform"][k] = t
    out = copy.copy(sc)
    out.instances = inst
    return out


def test_moved_sphere_with_samples_in_flight_equals_a_fresh_upload():
    """The split-scene any-hit source: the edited instance gets a tree of its own, and the shadow rays of the samples in flight
    walk both trees and commit through the textbook source of the split form."""
    import gpuspectral_amd as g
    import media_util as mu

    from gpuspectral_amd import scenes

    sc = scenes.cornell_materials(16)  # (the glass sphere holds under a quarter of the triangles: an edit of it alone splits the scene)
    sc2 = _moved(sc, [int(mu.glass_instances(sc)[0])], (0.12, 0.05, 0.2))
    with g.Context(0) as ctx:
        fresh = frame(ctx, sc2)
    with g.Context(0) as ctx:
        frame(ctx, sc, calls=(2,))
        ctx.frame_begin(W, H)
        ctx.render(spp=2)  # queued, not waited for
        ctx.update_instances(sc2.instances)
        st = ctx.stats()
        assert st["scene_updates"] == 1 and st["scene_splits"] == 1, st
        img, ist = frame(ctx, sc2, estimator=None, upload=False)
    agree(img, ist, fresh)


def test_scene_edited_whole_with_samples_in_flight_equals_a_fresh_upload(rooms):
    """The ring any-hit source: a scene whose every instance moves does not split; the first edit makes the ring of whole trees behind
    a wait, the second takes its next slot while samples are in flight.  Those samples finish on the geometry they started on (the
    frame of a fresh upload of the first edit), the next frame is that of a fresh upload of the second."""
    import gpuspectral_amd as g

    sc = rooms[3]
    every = range(len(sc.instances))
    sc1, sc2 = _moved(sc, every, (0.01, 0.0, 0.0)), _moved(sc, every, (0.02, 0.0, 0.0))
    with g.Context(0) as ctx:
        fresh1 = frame(ctx, sc1, calls=(2,))
    with g.Context(0) as ctx:
        fresh2 = frame(ctx, sc2, calls=(2,))
    with g.Context(0) as ctx:
        frame(ctx, sc, calls=(1,))
        ctx.frame_begin(W, H)
        ctx.render(spp=1)  # in flight at the first edit: it waits for them and makes the ring
        ctx.update_instances(sc1.instances)
        ctx.frame_begin(W, H)
        ctx.reset_stats()
        ctx.render(spp=2)  # in flight at the second edit: they finish on their slot of the ring ...
        ctx.update_instances(sc2.instances)
        st = ctx.stats()  # (completes the samples in flight)
        assert st["scene_splits"] == 0 and st["scene_updates"] == 2, st
        img1 = ctx.download().reshape(-1, 4).copy()
        img2, st2 = frame(ctx, sc2, estimator=None, upload=False, calls=(2,))  # ... and these start on the next
    agree(img1, st, fresh1)
    agree(img2, st2, fresh2)
    assert not eu.same(img1, img2)


def test_adaptive_sampling_in_textbook_mode(emu, rooms):
    """Every pixel is the emulation's textbook render of that pixel at the count the device stopped it at."""
    import gpuspectral_amd as g

    sc = rooms[130]
    es = emu.scene(sc)
    with g.Context(0) as ctx:
        ctx.set_estimator("textbook")
        ctx.set_light_sampling("power")
        ctx.upload_scene(sc)
        ctx.frame_begin(W, H)
        ctx.reset_stats()
        ctx.render(spp=16, adaptive_threshold=0.3, adaptive_min_spp=4, adaptive_step=4)
        img = ctx.download_compact()
        _, spp = ctx.pixel_stats()
        st = ctx.stats()
    assert len(np.unique(spp)) >= 2 and set(np.unique(spp)) <= {4, 8, 12, 16}
    ext = 0
    for k in np.unique(spp):
        sel = np.flatnonzero(spp == k).astype(np.uint32)
        ref, rst = es.render(W, H, int(k), estimator=eu.TEXTBOOK, light_mode=eu.POWER, pixel_ids=sel)
        ext += rst["extension_rays"]
        assert eu.same(img[sel], ref), "count %d" % k
    assert st["samples"] == int(spp.astype(np.int64).sum()) and st["extension_rays"] == ext


@pytest.mark.parametrize("light_mode", sorted(MODES))
def test_two_shares_of_a_multi_context(rooms, references, light_mode):
    from gpuspectral_amd import pt

    with pt.MultiContext([0, 0]) as m:
        with pytest.raises(pt.GspError):
            m.set_estimator(2)
        m.set_estimator("textbook")
        m.set_light_sampling(light_mode)
        m.upload_scene(rooms[3])
        m.frame_begin(W, H)
        m.render(spp=SPP)
        m.gather()
        img = m.download().reshape(-1, 4)
    assert eu.same(img, references[(3, light_mode)][0])


def test_mode_switched_between_frames_and_between_the_calls_of_a_frame(emu, rooms, references):
    """The samples in flight finish under the mode they were generated in (the wait of every scene edit); under the power pick every
    switch repacks the tables with or without the trailing record."""
    import gpuspectral_amd as g

    es = emu.scene(rooms[130])
    acc, _ = es.render(W, H, 2, estimator=eu.TEXTBOOK, light_mode=eu.POWER)
    acc, _ = es.render(W, H, 2, estimator=eu.REFERENCE, light_mode=eu.POWER, first_timestamp=2, accum=acc)
    acc, _ = es.render(W, H, 2, estimator=eu.TEXTBOOK, light_mode=eu.POWER, first_timestamp=4, accum=acc)
    with g.Context(0) as ctx:
        ctx.set_light_sampling("power")
        ctx.set_estimator("textbook")
        ctx.upload_scene(rooms[130])
        ctx.frame_begin(W, H)
        ctx.render(spp=2)
        ctx.set_estimator("reference")
        ctx.render(spp=2, first_timestamp=2)
        ctx.set_estimator("textbook")
        ctx.render(spp=2, first_timestamp=4)
        img = ctx.download().reshape(-1, 4)
        st = ctx.stats()
        assert eu.same(img, acc) and st["scene_drains"] == 2
        # ... and between frames: the next frame of the same context, under the other light selection
        img2, st2 = frame(ctx, rooms[130], light_mode="uniform", upload=False)
        agree(img2, st2, references[(130, "uniform")])


def test_mode_0_after_mode_1_is_a_context_that_never_heard_of_it(rooms):
    """Frame and gsp_stats, bit for bit (the timings aside), under both light selection modes."""
    import gpuspectral_amd as g

    for light_mode in sorted(MODES):
        with g.Context(0) as ctx:
            ref, rst = frame(ctx, rooms[130], estimator=None, light_mode=light_mode)
        with g.Context(0) as ctx:
            ctx.set_estimator("textbook")
            ctx.set_light_sampling(light_mode)
            ctx.upload_scene(rooms[130])
            ctx.frame_begin(W, H)
            ctx.render(spp=1)
            ctx.set_estimator("reference")  # under the resident scene
            img, st = frame(ctx, rooms[130], estimator=None, upload=False)
        assert eu.same(img, ref), light_mode
        timed = [k for k in rst if k.endswith("_ms") or k.endswith("_seconds") or "time" in k]
        assert st["scene_drains"] == 1 and rst["scene_drains"] == 0
        for k in rst:
            if k not in timed and k != "scene_drains":
                assert st[k] == rst[k], (light_mode, k, st[k], rst[k])


def test_disable_nee_renders_the_same_bits_in_both_modes(rooms):
    import gpuspectral_amd as g

    with g.Context(0) as ctx:
        a, ast = frame(ctx, rooms[3], estimator="reference", disable_nee=1)
        b, bst = frame(ctx, rooms[3], estimator="textbook", upload=False, disable_nee=1)
    agree(a, ast, (b, bst))
    assert ast["shadow_rays"] == 0


# ---- the occluded commit ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["default", "wavefront-only"])
def test_emitter_hit_behind_an_occluded_shadow_ray(emu, kind):
    """A light behind a plate, the continuing path aimed at a second emitter: the any-hit commit of the occluded ray must leave P2.w
    (lastPdf) alone.  With the reference's commit (P2.w = 1) the weight of the emitter hit is power_heuristic(1, hitPdf) and the frame
    differs."""
    sc = eu.occluded_light_scene()
    ref = emu.scene(sc).render(16, 16, 4, estimator=eu.TEXTBOOK)
    assert ref[1]["emitter_hits_after_occluded"] >= 16  # the frame has the paths the case is about
    with make_ctx(kind) as ctx:
        img, st = frame(ctx, sc, size=(16, 16))
    agree(img, st, ref)


# ---- interface -----------------------------------------------------------------------------------------------------------------------
def test_unknown_mode_is_refused_and_changes_nothing(rooms, references):
    import gpuspectral_amd as g

    with g.Context(0) as ctx:
        ctx.set_estimator("textbook")
        for bad in (2, 0xFFFFFFFF):
            with pytest.raises(g.GspError, match="unknown mode"):
                ctx.set_estimator(bad)
        img, st = frame(ctx, rooms[3], estimator=None)
    agree(img, st, references[(3, "uniform")])


def test_mode_survives_upload_scene(rooms, references):
    import gpuspectral_amd as g

    with g.Context(0) as ctx:
        ctx.set_estimator("textbook")
        ctx.upload_scene(rooms[130])
        img, st = frame(ctx, rooms[3], estimator=None)
    agree(img, st, references[(3, "uniform")])


def test_cxx_host_and_cli_render_the_textbook_frame(tmp_path):
    """PathTracer::setEstimator through the host library, and gsp_render --estimator textbook: the C++ loader's Cornell box in textbook
    mode is the textbook oracle's frame of the Python loader's; without the flag the CLI writes another image."""
    from conftest import CORNELL_XML
    from gpuspectral_amd import host
    from gpuspectral_amd.pt import GspError
    from oracle import mitsuba_loader as ml

    w, h, spp = eu.FRAMES["cornell"]
    want, _ = eu.oracle_frame("cornell")
    want = want.reshape(h, w, 4)
    pt = host.PathTracer(w, h, 0)
    try:
        pt.set_estimator("textbook")
        with pytest.raises(GspError, match="unknown mode"):
            pt.set_estimator(5)
        pt.render(host.Scene(CORNELL_XML), spp)
        assert eu.same(pt.download(), want)
    finally:
        pt.close()
    lib = os.path.join(ROOT, "gpuspectral_amd", "lib")
    env = dict(os.environ, LD_LIBRARY_PATH=lib + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    args = ["--estimator", "textbook", CORNELL_XML, str(tmp_path / "t.pfm"), str(w), str(h), str(spp)]
    r = subprocess.run([os.path.join(lib, "gsp_render")] + args, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.asarray(ml.read_pfm(str(tmp_path / "t.pfm")), np.float32).reshape(h, w, -1)[:, :, :3]
    assert eu.same(got[::-1], want[:, :, :3])  # (writePfm: rows bottom to top)
    args[1], args[3] = "reference", str(tmp_path / "r.pfm")
    r = subprocess.run([os.path.join(lib, "gsp_render")] + args, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    plain = np.asarray(ml.read_pfm(str(tmp_path / "r.pfm")), np.float32).reshape(h, w, -1)[:, :, :3]
    assert not eu.same(plain, got)


# ---- the kernels of a reference-mode context are the parent's ---------------------------------------------------------------------------
def test_kernel_digest_of_the_reference_mode_kernels_is_unchanged():
    """kernel_digest (sha256 of the instruction streams of k_trace<ExtendIO>, k_trace<ConnectIO> and k_shade<0, 0, 0, 0, 0>, written next
    to the library by the build) is what it was before the estimator mode existed: a reference-mode context runs the same code."""
    with open(os.path.join(ROOT, "gpuspectral_amd", "lib", "valu_mix.json")) as fh:
        vm = json.load(fh)
    from gpuspectral_amd import pt

    assert vm["library_digest"] == pt.source_digest()  # (the file belongs to this tree's library)
    assert vm["kernel_digest"] == "46198066bb589355"
