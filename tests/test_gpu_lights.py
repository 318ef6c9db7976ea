"""Light selection (include/gpuspectral_pt.h, "Light selection") on the GPU.

The wavefront pipeline with the <LSEL> kernels against the same stage headers run in scalar on the host (tests/emu/lights_emu.cpp),
bit for bit, image and ray counts: 3 lights (the table image is staged into LDS) and 130 lights (it stays in global memory), with
textures (<TEX, LSEL>), media (<MED, LSEL>), across an undrained table edit (<VER, LSEL>: every version has its own pick table),
under adaptive sampling, on two shares of a multi context, with the mode switched inside a frame; the resident table against the
host builder's bytes; and the uniform mode of a context that has been to power mode and back."""
import copy

import numpy as np
import pytest

import lights_util as lu
import textured

pytestmark = pytest.mark.gpu

COUNTS = ("extension_rays", "shadow_rays", "shaded_vertices")
W, H = 56, 40  # (2240 pixels: several 256-thread tiles, no multiple of the tile)
SPP = 4
LIGHTS = (3, 130)


@pytest.fixture(scope="module")
def emu():
    return lu.LightsEmu()


@pytest.fixture(scope="module")
def rooms():
    return {n: lu.room_scene(n) for n in LIGHTS}


@pytest.fixture(scope="module")
def references(emu, rooms):
    """The emulation's power-mode frames, rendered once: {(lights, first timestamp): (image, counts)}."""
    return {(n, ts0): emu.scene(rooms[n]).render(W, H, SPP, mode=lu.POWER, first_timestamp=ts0) for n in LIGHTS for ts0 in (0, 5)}


def make_ctx(kind):
    import gpuspectral_amd as g

    return g.Context(0) if kind == "default" else g.Context(0, finish_paths=0xFFFFFFFF)


def frame(ctx, sc, mode="power", calls=(SPP,), ts0=0, upload=True, media=None):
    if mode is not None:
        ctx.set_light_sampling(mode)
    if upload:
        if media is not None:
            ctx.set_media(media)
        ctx.upload_scene(sc)
    ctx.frame_begin(W, H)
    ctx.reset_stats()
    t = ts0
    for spp in calls:
        ctx.render(spp=spp, first_timestamp=t)
        t += spp
    return ctx.download().reshape(-1, 4).copy(), ctx.stats()


def agree(img, st, ref):
    rimg, rst = ref
    assert lu.same(img, rimg), "%d pixels differ" % int((img != rimg).any(1).sum())
    for k in COUNTS:
        assert st[k] == rst[k], (k, st[k], rst[k])


# ---- GPU == emulation, bit for bit -------------------------------------------------------------------------------------------------
def test_the_two_scenes_sit_on_either_side_of_the_lds_limit(rooms):
    """The table image of the 3-light room fits the 8192 bytes k_shade stages into LDS, that of the 130-light room (130 x (64 + 16)
    bytes of lights and pick table alone) does not."""
    rec = sum(len(b) * (b.dtype.itemsize + 16) for b in rooms[3].bsdfs)
    assert rec + 3 * 80 + 9 * 16 <= 8192 < 130 * 80


@pytest.mark.parametrize("kind", ["default", "wavefront-only"])
@pytest.mark.parametrize("ts0", [0, 5])
@pytest.mark.parametrize("n", LIGHTS)
def test_gpu_equals_emu(rooms, references, kind, ts0, n):
    with make_ctx(kind) as ctx:
        img, st = frame(ctx, rooms[n], ts0=ts0)
    agree(img, st, references[(n, ts0)])


def test_download_light_pick_equals_the_host_builder(emu, rooms):
    import gpuspectral_amd as g

    with g.Context(0) as ctx:
        ctx.upload_scene(rooms[130])
        with pytest.raises(g.GspError, match="UNIFORM"):
            ctx.download_light_pick()
        ctx.set_light_sampling("power")  # (with the scene resident: re-packed from the host copy)
        got = ctx.download_light_pick()
        assert got.tobytes() == emu.build(rooms[130].lights).tobytes() and len(got) == 130
        ctx.upload_scene(rooms[3])  # the mode survives gsp_upload_scene
        assert ctx.download_light_pick().tobytes() == emu.build(rooms[3].lights).tobytes()


def test_gpu_equals_emu_with_textures(emu, rooms):
    """<TEX, LSEL>."""
    sc = textured.decorate(copy.deepcopy(rooms[3]), seed=5, envmap=False)
    ref = emu.scene(sc).render(W, H, SPP, mode=lu.POWER)
    for kind in ("default", "wavefront-only"):
        with make_ctx(kind) as ctx:
            img, st = frame(ctx, sc)
        agree(img, st, ref)


def test_gpu_equals_emu_with_media(emu, rooms):
    """<MED, LSEL>: the glass sphere of the room absorbs."""
    import media_util as mu

    sigma = (1.0, 3.0, 5.0)
    for n in LIGHTS:
        sc = mu.with_medium(rooms[n], mu.glass_instances(rooms[n]), 1)
        ref = emu.scene(sc).render(W, H, SPP, mode=lu.POWER, media=[sigma])
        assert not lu.same(ref[0], emu.scene(sc).render(W, H, SPP, mode=lu.POWER, media=[(0.0, 0.0, 0.0)])[0])
        with make_ctx("default") as ctx:
            img, st = frame(ctx, sc, media=[sigma])
        agree(img, st, ref)


@pytest.mark.parametrize("n", LIGHTS)
def test_gpu_equals_emu_across_a_table_edit(emu, rooms, n):
    """<VER, LSEL>: gsp_update_tables changes a light's radiance between two gsp_render calls of the frame, neither drained.  The
    samples of the first call finish on their version of the tables -- lights AND pick table -- next to those of the second."""
    import gpuspectral_amd as g

    sc = copy.copy(rooms[n])
    es = emu.scene(sc)
    with g.Context(0) as ctx:
        ctx.set_light_sampling("power")
        ctx.upload_scene(sc)
        ctx.frame_begin(W, H)
        ctx.reset_stats()
        ctx.render(spp=2)
        acc, c1 = es.render(W, H, 2, mode=lu.POWER)
        lights = sc.lights.copy()
        lights["radiance"][0, :3] *= np.float32(40.0)  # the weakest-looking light takes over: another table, not only another radiance
        sc.lights = lights
        ctx.update_tables(sc)
        table = ctx.download_light_pick()
        ctx.render(spp=2, first_timestamp=2)
        es2 = emu.scene(sc)
        acc, c2 = es2.render(W, H, 2, mode=lu.POWER, first_timestamp=2, accum=acc)
        img = ctx.download().reshape(-1, 4)
        st = ctx.stats()
    assert st["scene_updates"] == 1 and st["scene_drains"] == 0, st  # (the first call's samples were in flight at the edit)
    assert table.tobytes() == emu.build(lights).tobytes() != emu.build(rooms[n].lights).tobytes()  # the CURRENT version's table
    agree(img, st, (acc, {k: c1[k] + c2[k] for k in COUNTS}))


def test_adaptive_sampling_in_power_mode(emu, rooms):
    """Every pixel is the emulation's power-mode render of that pixel at the count the device stopped it at."""
    import gpuspectral_amd as g

    sc = rooms[130]
    es = emu.scene(sc)
    with g.Context(0) as ctx:
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
        ref, rst = es.render(W, H, int(k), mode=lu.POWER, pixel_ids=sel)
        ext += rst["extension_rays"]
        assert lu.same(img[sel], ref), "count %d" % k
    assert st["samples"] == int(spp.astype(np.int64).sum()) and st["extension_rays"] == ext


@pytest.mark.parametrize("n", LIGHTS)
def test_two_shares_of_a_multi_context(rooms, references, n):
    from gpuspectral_amd import pt

    with pt.MultiContext([0, 0]) as m:
        with pytest.raises(pt.GspError):
            m.set_light_sampling(2)
        m.set_light_sampling("power")
        m.upload_scene(rooms[n])
        m.frame_begin(W, H)
        m.render(spp=SPP)
        m.gather()
        img = m.download().reshape(-1, 4)
    assert lu.same(img, references[(n, 0)][0])


def test_mode_switched_between_the_calls_of_one_frame(emu, rooms):
    """The samples in flight finish under the mode they were generated in (the wait of every scene edit)."""
    import gpuspectral_amd as g

    es = emu.scene(rooms[130])
    acc, _ = es.render(W, H, 2, mode=lu.POWER)
    acc, _ = es.render(W, H, 2, mode=lu.UNIFORM, first_timestamp=2, accum=acc)
    acc, _ = es.render(W, H, 2, mode=lu.POWER, first_timestamp=4, accum=acc)
    with g.Context(0) as ctx:
        ctx.set_light_sampling("power")
        ctx.upload_scene(rooms[130])
        ctx.frame_begin(W, H)
        ctx.render(spp=2)
        ctx.set_light_sampling("uniform")
        ctx.render(spp=2, first_timestamp=2)
        ctx.set_light_sampling("power")
        ctx.render(spp=2, first_timestamp=4)
        img = ctx.download().reshape(-1, 4)
        st = ctx.stats()
    assert lu.same(img, acc) and st["scene_drains"] == 2


def test_unknown_mode_is_refused_and_changes_nothing(rooms, references):
    import gpuspectral_amd as g

    with g.Context(0) as ctx:
        ctx.set_light_sampling("power")
        for bad in (2, 0xFFFFFFFF):
            with pytest.raises(g.GspError, match="unknown mode"):
                ctx.set_light_sampling(bad)
        img, st = frame(ctx, rooms[3], mode=None)
    agree(img, st, references[(3, 0)])


# ---- uniform mode --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LIGHTS)
def test_uniform_after_power_is_a_context_that_never_heard_of_it(rooms, n):
    """Frame and gsp_stats, bit for bit, against a context that was never told of the mode (the timings aside, which no two runs
    share)."""
    import gpuspectral_amd as g

    with g.Context(0) as ctx:
        ref, rst = frame(ctx, rooms[n], mode=None)
    with g.Context(0) as ctx:
        ctx.set_light_sampling("power")
        ctx.upload_scene(rooms[n])
        ctx.frame_begin(W, H)
        ctx.render(spp=1)
        ctx.set_light_sampling("uniform")  # (under the resident scene: the tables are packed again without the pick table)
        img, st = frame(ctx, rooms[n], mode=None, upload=False)
    assert lu.same(img, ref)
    timed = [k for k in rst if k.endswith("_ms") or k.endswith("_seconds") or "time" in k]
    # scene_drains counts since the last gsp_upload_scene, across gsp_reset_stats: the switch back waited for the sample in flight,
    # which is this context's history, not its state
    assert st["scene_drains"] == 1 and rst["scene_drains"] == 0
    for k in rst:
        if k not in timed and k != "scene_drains":
            assert st[k] == rst[k], (k, st[k], rst[k])
