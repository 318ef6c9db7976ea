"""Per-frame scene semantics of the drop-in boundary (ABI 5, refit: 6): the reference's createRenderPass re-reads the camera, every
object's transform and material, the eight BSDF tables and the lights on EVERY call and only keeps the BLAS of a mesh
(S/renderer/PathTracer.cpp:10-19,58-93; Renderer.cpp:122-131).  The C++ PathTracer compares the scene by value each
frame (SceneTracker) and sends gsp_update_camera / _tables / _instances; every test compares the GPU frame bit for bit
with the oracle rendering the scene AS IT IS at that frame."""
import os

import numpy as np
import pytest

from conftest import CORNELL_XML

pytestmark = pytest.mark.gpu


def moved(to_world, dx=0.0, dy=0.0, dz=0.0):
    m = np.array(to_world, np.float32).copy()
    m[12] += np.float32(dx)
    m[13] += np.float32(dy)
    m[14] += np.float32(dz)
    return m


def test_host_pathtracer_follows_a_moving_camera(oracle_mod):
    """(a) the camera moves between createRenderPass calls.  No reset: like the reference, the running mean simply goes on
    (timestamps 0-2 through the first camera, 3-5 through the second); the oracle is driven the same way."""
    from gpuspectral_amd import host

    W = H = 64
    scene = host.Scene(CORNELL_XML)
    pt = host.PathTracer(W, H)
    a0 = scene.arrays()
    pt.render(scene, 3)
    ref, _ = oracle_mod.Oracle(a0).render(W, H, spp=3)
    assert np.array_equal(pt.download().reshape(-1, 4), ref)
    assert pt.stats()["scene_updates"] == 0
    build_ms = pt.stats()["bvh_build_ms"]
    scene.set_camera(moved(a0.to_world, dx=0.35, dy=-0.2), float(a0.fov) * 1.2)
    a1 = scene.arrays()
    for _ in range(3):
        pt.create_render_pass(scene)  # +1 spp each, timestamps 3, 4, 5
    ref, _ = oracle_mod.Oracle(a1).render(W, H, spp=3, first_timestamp=3, accum=ref)
    img = pt.download().reshape(-1, 4)
    assert np.array_equal(img, ref)
    st = pt.stats()
    assert st["scene_updates"] == 1 and st["bvh_build_ms"] == build_ms  # the camera path: no rebuild
    # and from a clean accumulate buffer: the frame IS the new view (a stale primary-hit memo would show the old one)
    pt.reset()
    pt.render(scene, 4)
    ref1, _ = oracle_mod.Oracle(a1).render(W, H, spp=4)
    ref0, _ = oracle_mod.Oracle(a0).render(W, H, spp=4)
    img = pt.download().reshape(-1, 4)
    assert np.array_equal(img, ref1) and not np.array_equal(img, ref0)
    pt.close()


def test_host_pathtracer_follows_transform_and_material_edits(oracle_mod):
    """(b) an object moves, a BSDF record changes colour, a box becomes a (new) rough conductor, the light dims: each frame
    equals the oracle on the scene as edited so far."""
    from gpuspectral_amd import host

    W = H = 72
    scene = host.Scene(CORNELL_XML)
    pt = host.PathTracer(W, H)

    def check(expect_updates):
        pt.reset()
        pt.render(scene, 3)
        ref, ost = oracle_mod.Oracle(scene.arrays()).render(W, H, spp=3)
        img = pt.download().reshape(-1, 4)
        assert np.array_equal(img, ref)
        st = pt.stats()
        assert st["scene_updates"] == expect_updates
        return img

    base = check(0)
    a = scene.arrays()
    # the tall box (object 6) slides and turns: gsp_update_instances (re-bake + BVH rebuild from the resident meshes)
    m = a.instances["transform"][6].copy()
    m[12] += 0.3
    m[14] += 0.2
    scene.set_transform(6, m)
    img1 = check(1)
    assert not np.array_equal(img1, base)
    # the left wall's BSDF record turns blue: gsp_update_tables only
    scene.set_diffuse_reflectance(0, [0.05, 0.1, 0.7])
    img2 = check(2)
    assert not np.array_equal(img2, img1)
    # the short box gets a BSDF that did not exist before: tables AND instances
    scene.make_object_rough_conductor(5, [0.2, 0.92, 1.1], [3.9, 2.45, 2.14], 0.14)
    img3 = check(4)
    assert not np.array_equal(img3, img2)
    # an edit that changes nothing sends nothing
    scene.set_diffuse_reflectance(0, [0.05, 0.1, 0.7])
    assert np.array_equal(check(4), img3)
    pt.close()


def test_two_scenes_in_the_same_stack_slot(oracle_mod, tmp_path):
    """(c) VERDICT r03 weak 6: a loop over scene files with a stack `Scene` puts different scenes of equal object count at
    the SAME address.  Each frame must be its own scene's."""
    from gpuspectral_amd import host
    from oracle import mitsuba_loader as ml

    xml = open(CORNELL_XML).read()
    other = xml.replace('value="0.63, 0.065, 0.05"', 'value="0.1, 0.2, 0.8"').replace(
        '<matrix value="-1 0 0 0 0 1 0 1 0 0 -1 6.8 0 0 0 1"/>', '<matrix value="-1 0 0 0.3 0 1 0 1.1 0 0 -1 6.2 0 0 0 1"/>').replace(
        'value="17, 12, 4"', 'value="6, 9, 14"')
    assert other != xml
    p2 = tmp_path / "cornell_variant.xml"
    p2.write_text(other)
    W = H = 56
    pt = host.PathTracer(W, H)
    paths = [CORNELL_XML, str(p2), CORNELL_XML, str(p2)]
    imgs, addr = pt.render_files_same_slot(paths, 3)
    assert len(set(addr.tolist())) == 1, "the test did not reproduce the hazard: the Scene objects did not share a slot"
    refs = [oracle_mod.Oracle(ml.load_scene(p)).render(W, H, spp=3)[0] for p in paths[:2]]
    assert not np.array_equal(refs[0], refs[1])
    for i, img in enumerate(imgs):
        assert np.array_equal(img.reshape(-1, 4), refs[i % 2]), "frame %d shows another scene" % i
    pt.close()


def test_c_abi_updates_equal_a_fresh_upload(oracle_mod):
    """gsp_update_camera / _instances / _tables through the C ABI on a scene of tens of thousands of triangles: the frame of
    an updated context == the frame of a fresh context that uploaded the edited scene == the oracle; and the error
    contract (another object list, a handle out of range, before any upload)."""
    import gpuspectral_amd as g
    from gpuspectral_amd import scenes

    W, H, SPP = 96, 54, 3
    sc = scenes.interior(40_000)
    with g.Context(0) as ctx:
        with pytest.raises(g.GspError, match="needs gsp_upload_scene first"):
            ctx.update_camera(sc.to_world, sc.fov)
        ctx.upload_scene(sc)
        ctx.frame_begin(W, H)
        ctx.render(spp=SPP)
        before = ctx.download().copy()
        # edits
        sc.to_world = moved(sc.to_world, dx=0.4, dz=-0.3)
        inst = sc.instances.copy()
        k = int(np.argmax(inst["vertex_count"]))  # move the largest object a little, make another one glow
        t = inst["transform"][k].copy()
        t[13] += 0.05
        inst["transform"][k] = t
        j = int(np.argmin(inst["vertex_count"]))
        sc.instances = inst
        bs = [b.copy() for b in sc.bsdfs]
        if len(bs[0]):
            bs[0]["reflectance"][0] = (0.9, 0.1, 0.1)
        sc.bsdfs = bs
        lights = sc.lights.copy()
        lights["radiance"][:, :3] *= np.float32(0.5)
        sc.lights = lights
        ctx.update_camera(sc.to_world, sc.fov)
        ctx.update_instances(sc.instances)
        ctx.update_tables(sc)
        assert ctx.stats()["scene_updates"] == 3
        ctx.frame_begin(W, H)
        ctx.render(spp=SPP)
        upd = ctx.download().copy()
        assert not np.array_equal(upd, before)
        # calls that change nothing do nothing (a host that mirrors the reference makes all three every frame)
        n0 = ctx.stats()["scene_updates"]
        ctx.update_tables(sc)
        ctx.update_instances(sc.instances)
        ctx.update_camera(sc.to_world, sc.fov)
        assert ctx.stats()["scene_updates"] == n0
        # pipelined: an update between two gsp_render calls without a sync in between drains the old samples first
        ctx.frame_begin(W, H)
        ctx.render(spp=2)
        ctx.update_camera(moved(sc.to_world, dy=0.1), sc.fov)
        ctx.render(spp=1, first_timestamp=2)
        mixed = ctx.download().reshape(-1, 4).copy()
        # errors leave the scene usable
        with pytest.raises(g.GspError, match="instances, the uploaded scene has"):
            ctx.update_instances(sc.instances[:-1])
        bad = sc.instances.copy()
        bad["bsdf"][0] = (7 << 16) | 0xFFFF
        with pytest.raises(g.GspError, match="BSDF handle out of range"):
            ctx.update_instances(bad)
        other = sc.instances.copy()
        other["first_vertex"][j] += 3
        with pytest.raises(g.GspError, match="another vertex range"):
            ctx.update_instances(other)
        ctx.update_camera(sc.to_world, sc.fov)
        ctx.frame_begin(W, H)
        ctx.render(spp=SPP)
        assert np.array_equal(ctx.download(), upd)
    with g.Context(0) as fresh:
        fresh.upload_scene(sc)
        fresh.frame_begin(W, H)
        fresh.render(spp=SPP)
        assert np.array_equal(fresh.download(), upd)
    o = oracle_mod.Oracle(sc)
    ref, _ = o.render(W, H, spp=SPP)
    assert np.array_equal(upd.reshape(-1, 4), ref)
    # the pipelined sequence: 2 samples through the first camera, the third through the moved one
    acc, _ = o.render(W, H, spp=2)
    cam2 = moved(sc.to_world, dy=0.1)
    keep = sc.to_world
    sc.to_world = cam2
    acc, _ = oracle_mod.Oracle(sc).render(W, H, spp=1, first_timestamp=2, accum=acc)
    sc.to_world = keep
    assert np.array_equal(mixed, acc)


def test_update_instances_refits_then_rebuilds(oracle_mod):
    """(ABI 6) gsp_update_instances keeps the tree's topology while its boxes stay within gsp_ctx_options.refit_growth of the
    built tree's (the reference rebuilds only its TLAS, PathTracer.cpp:10-19) and rebuilds beyond it.  Frames and ray counts
    equal the oracle's either way, and a context that always rebuilds renders the same bytes."""
    import gpuspectral_amd as g
    from gpuspectral_amd import abi, scenes

    W, H, SPP = 96, 54, 2
    sc = scenes.interior(40_000)
    base = sc.instances.copy()
    k = int(np.argmax(base["vertex_count"]))

    def edited(step, far=False):
        inst = base.copy()
        t = inst["transform"][k].copy()
        t[12:15] += (np.float32(60.0) if far else np.float32(0.02 * step)) * np.array([1.0, 0.3, -0.5], np.float32)
        inst["transform"][k] = t
        if step % 2:  # materials and emission travel with the instance record as well
            inst["twofaced"][(7 * step) % len(inst)] ^= 1
        return inst

    frames = {}
    for growth in (0.0, 1.0):  # default (refit) / always rebuild
        with g.Context(0, options=abi.CtxOptions(refit_growth=growth)) as ctx:
            ctx.upload_scene(sc)
            nodes = ctx.stats()["num_bvh_nodes"]
            out = []
            for step in range(1, 7):
                sc.instances = edited(step)
                ctx.update_instances(sc.instances)
                st = ctx.stats()
                assert st["scene_updates"] == step
                assert st["scene_refits"] == (step if growth == 0.0 else 0), (growth, step, st["scene_refits"])
                assert st["num_bvh_nodes"] == nodes or growth == 1.0
                ctx.frame_begin(W, H)
                ctx.render(spp=SPP)
                out.append(ctx.download().reshape(-1, 4).copy())
            # the object leaves the room: the refitted boxes outgrow the bound, the tree is rebuilt
            sc.instances = edited(7, far=True)
            ctx.update_instances(sc.instances)
            st = ctx.stats()
            assert st["scene_updates"] == 7 and st["scene_refits"] == (6 if growth == 0.0 else 0)
            ctx.frame_begin(W, H)
            ctx.render(spp=SPP)
            out.append(ctx.download().reshape(-1, 4).copy())
            # ... and comes back: a refit of the NEW tree (its measure is the rebuilt one's)
            sc.instances = edited(6)
            ctx.update_instances(sc.instances)
            ctx.frame_begin(W, H)
            ctx.render(spp=SPP)
            out.append(ctx.download().reshape(-1, 4).copy())
            frames[growth] = out
    for a, b in zip(frames[0.0], frames[1.0]):
        assert np.array_equal(a, b)
    assert np.array_equal(frames[0.0][5], frames[0.0][7])  # step 6 twice
    ref, _ = oracle_mod.Oracle(sc).render(W, H, spp=SPP)
    assert np.array_equal(frames[0.0][7], ref)
    sc.instances = edited(7, far=True)
    ref, _ = oracle_mod.Oracle(sc).render(W, H, spp=SPP)
    assert np.array_equal(frames[0.0][6], ref)
    sc.instances = base


def test_multi_updates_reach_every_share(oracle_mod, cornell):
    """gsp_multi_update_*: three shares on the one GPU, camera + tables + instances edited, frame == oracle."""
    import copy

    import gpuspectral_amd as g

    W = H = 80
    sc = copy.deepcopy(cornell)
    with g.MultiContext([0, 0, 0]) as m:
        m.upload_scene(sc)
        m.frame_begin(W, H)
        m.render(spp=2)
        first = m.download().copy()
        sc.to_world = moved(sc.to_world, dx=-0.3)
        inst = sc.instances.copy()
        t = inst["transform"][5].copy()
        t[12] -= 0.2
        inst["transform"][5] = t
        sc.instances = inst
        bs = [b.copy() for b in sc.bsdfs]
        bs[0]["reflectance"][1] = (0.2, 0.2, 0.9)
        sc.bsdfs = bs
        m.update_camera(sc.to_world, sc.fov)
        m.update_tables(sc)
        m.update_instances(sc.instances)
        m.frame_begin(W, H)
        m.render(spp=2)
        img = m.download()
        tot, each = m.stats(per_share=True)
        assert all(e["scene_updates"] == 3 for e in each)
    ref, _ = oracle_mod.Oracle(sc).render(W, H, spp=2)
    assert np.array_equal(img.reshape(-1, 4), ref) and not np.array_equal(img, first)


@pytest.mark.parametrize("which", ["materials", "cornell", "interior"])
def test_nee_off_matches_the_oracle(oracle_mod, cornell, materials_scene, which):
    """gsp_render_params.nee = 0 (RenderParams.nee, PathTracer.h:36-41; rayhit.rchit:733,763-768) on the GPU, with and
    without k_finish: bit-equal to the oracle, no shadow ray traced, same path segments as nee = 1."""
    import gpuspectral_amd as g
    from gpuspectral_amd import abi, scenes

    sc = {"materials": materials_scene, "cornell": cornell}.get(which) or scenes.interior(20_000)
    W, H, SPP = 80, 60, 5
    p = abi.default_render_params()
    p.disable_nee = 1
    ref, ost = oracle_mod.Oracle(sc).render(W, H, spp=SPP, params=p)
    for finish in (0, 0xFFFFFFFF):
        with g.Context(0, finish_paths=finish) as ctx:
            ctx.upload_scene(sc)
            ctx.frame_begin(W, H)
            ctx.render(spp=SPP, params=p)
            img = ctx.download().reshape(-1, 4)
            st = ctx.stats()
            assert np.array_equal(img, ref)
            assert st["shadow_rays"] == 0 == ost["shadow_rays"]
            assert st["extension_rays"] == ost["extension_rays"] and st["shaded_vertices"] == ost["shaded_vertices"]
            # switching the estimator between two calls drains the pipeline first (paths in flight carry no copy of it)
            ctx.frame_begin(W, H)
            ctx.render(spp=2)
            ctx.render(spp=3, first_timestamp=2, params=p)
            mix = ctx.download().reshape(-1, 4)
        acc, _ = oracle_mod.Oracle(sc).render(W, H, spp=2)
        p.spp, p.first_timestamp = 3, 2
        acc, _ = oracle_mod.Oracle(sc).render(W, H, spp=3, first_timestamp=2, accum=acc, params=p)
        assert np.array_equal(mix, acc)


def test_ctx_options_change_no_result(oracle_mod, materials_scene):
    """gsp_ctx_options: pool size, ring size, memory share, lanes, primary memo, k_finish threshold,
    reinsertion rounds are resources and schedules -- every setting renders the same frame and traces the same rays."""
    import gpuspectral_amd as g
    from gpuspectral_amd import abi

    W, H, SPP = 128, 96, 6
    ref, ost = oracle_mod.Oracle(materials_scene).render(W, H, spp=SPP)
    settings = [dict(), dict(pool_paths=1 << 16), dict(ring_bytes=1 << 24, pool_paths=1 << 18), dict(memory_share=0.02),
                dict(lanes=2), dict(primary_memo=2), dict(finish_paths=0xFFFFFFFF), dict(finish_paths=1 << 12),
                dict(reinsert_rounds=1), dict(reinsert_rounds=21), dict(lanes=2, primary_memo=2, pool_paths=1 << 17, finish_paths=0xFFFFFFFF)]
    for kw in settings:
        with g.Context(0, options=abi.CtxOptions(**kw)) as ctx:
            ctx.upload_scene(materials_scene)
            ctx.frame_begin(W, H)
            ctx.render(spp=4)
            ctx.render(spp=SPP - 4, first_timestamp=4)
            img = ctx.download().reshape(-1, 4)
            st = ctx.stats()
        assert np.array_equal(img, ref), kw
        assert (st["extension_rays"], st["shadow_rays"]) == (ost["extension_rays"], ost["shadow_rays"]), kw
        assert (st["memoised_rays"] == 0) == (kw.get("primary_memo") == 2), kw
    bad = abi.CtxOptions()
    bad.struct_size = 0
    with pytest.raises(g.GspError, match="struct_size"):
        g.Context(0, options=bad)


def test_random_edits_fuzz(oracle_mod):
    """tests/tools/fuzz_parity.py check_updates: random scenes edited twice through the update calls (random transforms incl.
    mirrored ones, swapped material handles, twofaced flips, emission, rescaled tables and lights, moved cameras), and 10
    seeds with nee = 0: every frame and every ray count equals the oracle's."""
    import sys

    import gpuspectral_amd as g
    from conftest import ROOT

    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import fuzz_parity

    with g.Context(0) as ctx:
        for seed in range(7000, 7016):
            ok, nbad, tris = fuzz_parity.check_updates(ctx, oracle_mod, seed)
            assert ok, "seed %d: %d of 3 frames differ (%d triangles)" % (seed, nbad, tris)
        for seed in range(7100, 7110):
            ok, ndiff, tris = fuzz_parity.check(ctx, oracle_mod, seed, nee=0)
            assert ok, "seed %d with nee = 0: %d pixels differ (%d triangles)" % (seed, ndiff, tris)


@pytest.mark.parametrize("which", ["cornell", "materials"])
def test_table_edits_every_frame_without_a_drain(oracle_mod, cornell, materials_scene, which):
    """(r05) gsp_update_tables with samples IN FLIGHT keeps them in flight: a sample carries the version of
    the BSDF / light tables it was generated under and finishes on it (a ring of 64 versions; an edit that changes the record
    counts, or the 64th edit within the life of one sample, still drains).  One sample per frame, a reflectance and the light's
    radiance edited before EVERY frame, 150 frames without a sync: more than two rounds of the ring, paths of a dozen versions in
    one launch.  The accumulate buffer must equal the oracle's running mean over the same sequence of scenes, bit for bit --
    and after the edits stop, the frames of the single surviving version too (the <VER = false> kernels again)."""
    import copy

    import gpuspectral_amd as g

    sc = copy.deepcopy(cornell if which == "cornell" else materials_scene)
    W, H = (48, 40) if which == "cornell" else (40, 32)
    frames = 150 if which == "cornell" else 70

    def edit(k):
        bs = [b.copy() for b in sc.bsdfs]
        n = len(bs[0])
        bs[0]["reflectance"][k % n] = (0.1 + 0.8 * ((k * 7) % 11) / 11.0, 0.2 + 0.6 * ((k * 3) % 5) / 5.0, 0.9 - 0.7 * ((k * 5) % 7) / 7.0)
        if which == "materials" and len(bs[4]):
            bs[4]["alpha"][k % len(bs[4])] = np.float32(0.05 + 0.02 * (k % 9))
        sc.bsdfs = bs
        lights = sc.lights.copy()
        lights["radiance"][:, :3] = np.array([17.0, 12.0, 4.0], np.float32) * np.float32(0.5 + 0.1 * (k % 6))
        sc.lights = lights

    acc = None
    with g.Context(0) as ctx:
        ctx.upload_scene(sc)
        ctx.frame_begin(W, H)
        for k in range(frames):
            edit(k)
            ctx.update_tables(sc)  # no sync anywhere in this loop
            ctx.render(spp=1, first_timestamp=k)
            acc, _ = oracle_mod.Oracle(sc).render(W, H, spp=1, first_timestamp=k, accum=acc)
        img = ctx.download().reshape(-1, 4)
        assert np.array_equal(img, acc), "%d pixels differ" % int((img != acc).any(1).sum())
        assert ctx.stats()["scene_updates"] == frames
        assert ctx.stats()["scene_drains"] == 0
        # the edits are over: more samples of the last version (the pipeline goes back to one version in slot 0), then one more
        # edit with nothing but that version in flight
        ctx.render(spp=3, first_timestamp=frames)
        acc, _ = oracle_mod.Oracle(sc).render(W, H, spp=3, first_timestamp=frames, accum=acc)
        edit(frames + 1)
        ctx.update_tables(sc)
        ctx.render(spp=2, first_timestamp=frames + 3)
        acc, _ = oracle_mod.Oracle(sc).render(W, H, spp=2, first_timestamp=frames + 3, accum=acc)
        assert np.array_equal(ctx.download().reshape(-1, 4), acc)
        # a layout change (one more diffuse record) with samples in flight takes the old road: drain, then upload
        ctx.render(spp=1, first_timestamp=frames + 5)
        acc, _ = oracle_mod.Oracle(sc).render(W, H, spp=1, first_timestamp=frames + 5, accum=acc)
        bs = [b.copy() for b in sc.bsdfs]
        extra = bs[0][:1].copy()
        extra["reflectance"][0] = (0.3, 0.3, 0.3)
        bs[0] = np.concatenate([bs[0], extra])
        sc.bsdfs = bs
        ctx.update_tables(sc)
        ctx.render(spp=2, first_timestamp=frames + 6)
        acc, _ = oracle_mod.Oracle(sc).render(W, H, spp=2, first_timestamp=frames + 6, accum=acc)
        assert np.array_equal(ctx.download().reshape(-1, 4), acc)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["cornell", "interior", "cornell-two-lanes"])
def test_transform_edits_every_frame_without_a_drain(oracle_mod, cornell, which):
    """(r05, VERDICT r04 item 6, second half) gsp_update_instances with samples IN FLIGHT keeps them in flight: the refit goes
    into the next slot of the geometry ring (8 versions of node records, intersection triangles and shading packets), a sample
    carries the slot it was generated under and finishes in it.  One sample per frame, an object moved (and a material flag
    flipped, a BSDF record and the light's radiance edited: both rings at once) before EVERY frame, no sync in the loop: several
    rounds of the ring, rays of up to eight trees in one launch.  The accumulate buffer must equal the oracle's running mean
    over the same sequence of scenes, bit for bit; then the edits stop (one version again, the <VER = false> kernels), an object
    leaves the room (the refit is abandoned, the samples in flight finish, the tree is rebuilt) and comes back."""
    import copy

    import gpuspectral_amd as g
    from gpuspectral_amd import scenes

    from gpuspectral_amd import abi

    if which.startswith("cornell"):
        sc, (W, H), frames = copy.deepcopy(cornell), (48, 40), 60
    else:
        sc, (W, H), frames = scenes.interior(20_000), (64, 36), 30
    options = abi.CtxOptions(lanes=2) if which.endswith("two-lanes") else None  # two pipelines, one ring
    base = sc.instances.copy()
    big = int(np.argmax(base["vertex_count"])) if which == "interior" else len(base) - 1
    emissive = {int(i) for i in np.nonzero(np.asarray(base["emission"]).reshape(len(base), -1)[:, :3].any(1))[0]}

    def edit(k, far=False):
        inst = base.copy()
        t = inst["transform"][big].copy()
        t[12:15] += (np.float32(80.0) if far else np.float32(0.01 * (k % 13))) * np.array([1.0, 0.25, -0.5], np.float32)
        inst["transform"][big] = t
        j = (5 * k) % len(inst)
        if j not in emissive and j != big:
            inst["twofaced"][j] ^= 1
        sc.instances = inst
        if k % 3 == 0:  # the tables now and then as well
            bs = [b.copy() for b in sc.bsdfs]
            bs[0]["reflectance"][k % len(bs[0])] = (0.15 + 0.7 * ((k * 7) % 11) / 11.0, 0.5, 0.85 - 0.6 * ((k * 5) % 7) / 7.0)
            sc.bsdfs = bs

    acc = None
    with g.Context(0, options=options) as ctx:
        ctx.upload_scene(sc)
        ctx.frame_begin(W, H)
        for k in range(frames):
            edit(k + 1)
            ctx.update_instances(sc.instances)  # (the first one drains and makes the ring; no sync after that)
            ctx.update_tables(sc)
            ctx.render(spp=1, first_timestamp=k)
            acc, _ = oracle_mod.Oracle(sc).render(W, H, spp=1, first_timestamp=k, accum=acc)
        img = ctx.download().reshape(-1, 4)
        assert np.array_equal(img, acc), "%d pixels differ" % int((img != acc).any(1).sum())
        st = ctx.stats()
        # every edit either refitted a tree or -- when it touched an instance no edit had touched before -- built the scene as two
        # trees (the edited instances / the rest); only those, and one attempt that found too much of the scene edited, waited
        # (... or, once, went back to one tree when more than a quarter of the scene had become "edited")
        assert frames - 1 <= st["scene_refits"] + st["scene_splits"] <= frames, st
        assert st["scene_drains"] <= st["scene_splits"] + 2, st  # (+ the attempt that said no, + the ring of whole trees made after it)
        if which == "interior":
            assert 1 <= st["scene_splits"] <= 12, st
        # the edits are over: more samples of the last version, then one edit with nothing but that version in flight
        ctx.render(spp=3, first_timestamp=frames)
        acc, _ = oracle_mod.Oracle(sc).render(W, H, spp=3, first_timestamp=frames, accum=acc)
        edit(frames + 2)
        ctx.update_instances(sc.instances)
        ctx.update_tables(sc)
        ctx.render(spp=2, first_timestamp=frames + 3)
        acc, _ = oracle_mod.Oracle(sc).render(W, H, spp=2, first_timestamp=frames + 3, accum=acc)
        assert np.array_equal(ctx.download().reshape(-1, 4), acc)
        # an object leaves the room while samples are in flight: refit abandoned, drain, rebuild -- and back (a new ring)
        ctx.render(spp=1, first_timestamp=frames + 5)
        acc, _ = oracle_mod.Oracle(sc).render(W, H, spp=1, first_timestamp=frames + 5, accum=acc)
        before = st["scene_refits"] + 1, st["scene_drains"]
        edit(frames + 3, far=True)
        ctx.update_instances(sc.instances)
        ctx.update_tables(sc)
        if which == "interior":  # the refit is abandoned, the samples in flight finish, the trees are built again
            st = ctx.stats()
            assert st["scene_refits"] == before[0] and st["scene_drains"] == before[1] + 1, (st, before)
        ctx.render(spp=1, first_timestamp=frames + 6)
        acc, _ = oracle_mod.Oracle(sc).render(W, H, spp=1, first_timestamp=frames + 6, accum=acc)
        for k in range(frames + 7, frames + 12):
            edit(k)
            ctx.update_instances(sc.instances)
            ctx.update_tables(sc)
            ctx.render(spp=1, first_timestamp=k)
            acc, _ = oracle_mod.Oracle(sc).render(W, H, spp=1, first_timestamp=k, accum=acc)
        assert np.array_equal(ctx.download().reshape(-1, 4), acc)


@pytest.mark.gpu
@pytest.mark.parametrize("versions", [1, 4])
def test_geometry_versions_option(oracle_mod, cornell, versions):
    """gsp_ctx_options.geometry_versions bounds the geometry ring (176 B per triangle and slot): 1 = no ring, every transform
    edit first completes the samples in flight (what r04 did); 4 = a ring that a path of a dozen bounces outlives, so some edits
    wait and some do not.  Same images either way."""
    import copy

    import gpuspectral_amd as g
    from gpuspectral_amd import abi

    sc = copy.deepcopy(cornell)
    W, H, frames = 48, 40, 24
    base = sc.instances.copy()
    acc = None
    with g.Context(0, options=abi.CtxOptions(geometry_versions=versions)) as ctx:
        ctx.upload_scene(sc)
        ctx.frame_begin(W, H)
        for k in range(frames):
            inst = base.copy()
            t = inst["transform"][len(inst) - 1].copy()
            t[12] += np.float32(0.01 * (k % 7))
            inst["transform"][len(inst) - 1] = t
            sc.instances = inst
            ctx.update_instances(sc.instances)
            ctx.render(spp=1, first_timestamp=k)
            acc, _ = oracle_mod.Oracle(sc).render(W, H, spp=1, first_timestamp=k, accum=acc)
        assert np.array_equal(ctx.download().reshape(-1, 4), acc)
        st = ctx.stats()
        changed = sum(1 for k in range(frames) if k % 7 != (k - 1) % 7 or k == 0) - (1 if 0 % 7 == 0 else 0)  # frame 0 leaves the transform as uploaded
        assert st["scene_updates"] == changed, st
        if versions == 1:
            assert st["scene_drains"] == changed, st  # (frame 0 was in flight when the first edit came)
        else:
            assert 0 < st["scene_drains"] < changed, st


@pytest.mark.gpu
def test_ring_and_drain_paths_agree_at_scale():
    """The oracle cannot follow a 200 k-triangle scene at 960x540 for 40 frames -- but the two roads of the library can check each
    other there: a context with both version rings (no edit waits) against one with `geometry_versions = 1` whose transform edits
    first complete the samples in flight (r04's behaviour), same sequence of transform + material + light edits, one sample per
    frame, no sync: the accumulate buffers must be equal bit for bit (millions of paths of up to 40 scene versions in one launch
    on the first road)."""
    import gpuspectral_amd as g
    from gpuspectral_amd import abi, scenes

    W, H, frames = 960, 540, 40
    sc = scenes.interior(200_000, seed=3)
    base = sc.instances.copy()
    big = int(np.argmax(base["vertex_count"]))
    images, drains = [], []
    for versions in (0, 1):
        sc.instances = base.copy()
        bs0 = [b.copy() for b in sc.bsdfs]
        with g.Context(0, options=abi.CtxOptions(geometry_versions=versions)) as ctx:
            ctx.upload_scene(sc)
            ctx.frame_begin(W, H)
            for k in range(frames):
                inst = base.copy()
                for j in (big, (big + 1 + k % 5) % len(inst)):
                    t = inst["transform"][j].copy()
                    t[12:15] += np.float32(0.004 * (1 + k % 9)) * np.array([1.0, 0.2, -0.6], np.float32)
                    inst["transform"][j] = t
                sc.instances = inst
                ctx.update_instances(inst)
                if k % 4 == 1:
                    bs = [b.copy() for b in bs0]
                    bs[0]["reflectance"][k % len(bs[0])] = (0.2 + 0.01 * k, 0.5, 0.7 - 0.01 * k)
                    sc.bsdfs = bs
                    ctx.update_tables(sc)
                ctx.render(spp=1, first_timestamp=k)
            images.append(ctx.download().copy())
            drains.append(ctx.stats()["scene_drains"])
        sc.bsdfs = bs0
    sc.instances = base
    assert drains[0] <= 6 and drains[1] >= frames - 2, drains  # (first road: only the edits that touched a new instance waited)
    assert np.array_equal(images[0], images[1]), "%d pixels differ" % int((images[0] != images[1]).any(-1).sum())
    assert np.isfinite(images[0]).all() and images[0][..., :3].max() > 0


@pytest.mark.gpu
def test_split_scene_trace_hook_and_statistics(oracle_mod, materials_scene):
    """A viewer's edits split the scene into two trees (the edited instances / the rest: `scene_splits`).  gsp_trace on a split scene
    walks both and reports scene-wide triangle indices, t, u, v equal to the oracle's bit for bit (closest and any hit); a statistics
    run puts the scene back into one tree; frames stay equal to the oracle's throughout."""
    import copy

    import gpuspectral_amd as g

    sc = copy.deepcopy(materials_scene)
    W, H = 64, 48
    base = sc.instances.copy()
    small = int(np.argsort(base["vertex_count"])[len(base) // 2])
    rng = np.random.RandomState(9)
    lo = np.array([-1.2, 0.0, -1.2], np.float32)
    hi = np.array([1.2, 2.2, 1.2], np.float32)
    o_ = (lo + rng.rand(20000, 3).astype(np.float32) * (hi - lo)).astype(np.float32)
    d_ = rng.normal(size=(20000, 3)).astype(np.float32)
    d_ /= np.linalg.norm(d_, axis=1, keepdims=True)
    rays = np.zeros((20000, 8), np.float32)
    rays[:, :3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o_, 0.0, d_, 1e10
    acc = None
    with g.Context(0) as ctx:
        ctx.upload_scene(sc)
        ctx.frame_begin(W, H)
        for k in range(6):
            inst = base.copy()
            t = inst["transform"][small].copy()
            t[12:15] += np.float32(0.02 * (k + 1)) * np.array([0.5, 0.1, -0.3], np.float32)
            inst["transform"][small] = t
            sc.instances = inst
            ctx.update_instances(inst)
            ctx.render(spp=1, first_timestamp=k)
            acc, _ = oracle_mod.Oracle(sc).render(W, H, spp=1, first_timestamp=k, accum=acc)
            if k == 3:  # with samples in flight
                o = oracle_mod.Oracle(sc)
                got, ref = ctx.trace(rays), o.trace(rays)
                assert (got["prim"] == ref["prim"]).all(), int((got["prim"] != ref["prim"]).sum())
                hit = ref["prim"] >= 0
                assert hit.sum() > 5000
                for f in ("t", "u", "v"):
                    assert np.array_equal(np.ascontiguousarray(got[f][hit]).view(np.uint32), np.ascontiguousarray(ref[f][hit]).view(np.uint32)), f
                sh = rays.copy()
                sh[:, 3], sh[:, 7] = 0.01, rng.uniform(0.05, 3.0, len(sh))
                assert (ctx.trace(sh, any_hit=True)["prim"] == o.trace(sh, any_hit=True)["prim"]).all()
        assert np.array_equal(ctx.download().reshape(-1, 4), acc)
        st = ctx.stats()
        assert st["scene_splits"] == 1 and st["scene_refits"] == 5 and st["scene_drains"] == 0, st  # (the first split needs no wait)
        nodes_split = st["num_bvh_nodes"]
        # a statistics run: one tree again, counters as the oracle's
        ctx.reset_stats()
        ctx.frame_begin(W, H)
        ctx.render(spp=2, collect_traversal_stats=1)
        st = ctx.stats()
        ref, so = oracle_mod.Oracle(sc).render(W, H, spp=2)
        assert np.array_equal(ctx.download().reshape(-1, 4), ref)
        assert st["extension_rays"] == so["extension_rays"] and st["shadow_rays"] == so["shadow_rays"] and st["stat_rays"] > 0
        assert st["num_bvh_nodes"] != nodes_split and st["num_triangles"] == sc.num_triangles


@pytest.mark.gpu
def test_split_scene_ring_wraps(oracle_mod, materials_scene):
    """90 one-sample frames with one object moved before each, no sync: the ring of the edited instances' tree (64 slots) goes round
    once and a half while paths of up to 52 frames ago are still in flight; every frame on the scene it was generated under."""
    import copy

    import gpuspectral_amd as g

    sc = copy.deepcopy(materials_scene)
    W, H, frames = 40, 30, 90
    base = sc.instances.copy()
    small = int(np.argsort(base["vertex_count"])[len(base) // 2])
    acc = None
    with g.Context(0) as ctx:
        ctx.upload_scene(sc)
        ctx.frame_begin(W, H)
        for k in range(frames):
            inst = base.copy()
            t = inst["transform"][small].copy()
            t[12:15] += np.float32(0.004 * (1 + k % 23)) * np.array([0.6, 0.1, -0.4], np.float32)
            inst["transform"][small] = t
            sc.instances = inst
            ctx.update_instances(inst)
            ctx.render(spp=1, first_timestamp=k)
            acc, _ = oracle_mod.Oracle(sc).render(W, H, spp=1, first_timestamp=k, accum=acc)
        img = ctx.download().reshape(-1, 4)
        assert np.array_equal(img, acc), "%d pixels differ" % int((img != acc).any(1).sum())
        st = ctx.stats()
        assert st["scene_splits"] == 1 and st["scene_drains"] == 0 and st["scene_refits"] == frames - 1, st


@pytest.mark.gpu
def test_reference_frame_loop_against_the_c_abi(oracle_mod, materials_scene):
    """INTEGRATION.md's frame loop -- the reference's Renderer::run: re-read camera, objects and tables, trace one sample, show the
    accumulate buffer from device memory -- 40 frames with all three edited before each and no call that waits: what is shown is
    always the running mean of a prefix of the samples, the final image equals the oracle's, bit for bit."""
    import copy
    import ctypes as C

    import gpuspectral_amd as g

    sc = copy.deepcopy(materials_scene)
    W, H, frames = 48, 36, 40
    base = sc.instances.copy()
    small = int(np.argsort(base["vertex_count"])[len(base) // 2])
    cam0 = np.array(sc.to_world, np.float32).copy()
    hip = C.CDLL("libamdhip64.so")
    dptr = C.c_void_p()
    nbytes = W * H * 16
    means = {0: np.zeros((W * H, 4), np.float32)}
    acc = None
    with g.Context(0) as ctx:
        ctx.upload_scene(sc)
        ctx.frame_begin(W, H)
        assert hip.hipMalloc(C.byref(dptr), C.c_size_t(nbytes)) == 0
        try:
            shown_before = 0
            for k in range(frames):
                sc.to_world = moved(cam0, dx=0.004 * (k % 7), dy=0.002 * (k % 3))
                inst = base.copy()
                t = inst["transform"][small].copy()
                t[12:15] += np.float32(0.01 * (1 + k % 11)) * np.array([0.5, 0.1, -0.4], np.float32)
                inst["transform"][small] = t
                sc.instances = inst
                bs = [b.copy() for b in sc.bsdfs]
                bs[0]["reflectance"][k % len(bs[0])] = (0.2 + 0.015 * k, 0.45, 0.8 - 0.015 * k)
                sc.bsdfs = bs
                ctx.update_camera(sc.to_world, sc.fov)
                ctx.update_instances(inst)
                ctx.update_tables(sc)
                ctx.render(spp=1, first_timestamp=k)
                acc, _ = oracle_mod.Oracle(sc).render(W, H, spp=1, first_timestamp=k, accum=acc)
                means[k + 1] = acc.copy()
                shown = ctx.peek_to_device(dptr.value, nbytes)
                assert shown_before <= shown <= k + 1
                shown_before = shown
                back = np.zeros((W * H, 4), np.float32)
                assert hip.hipMemcpy(C.c_void_p(back.ctypes.data), dptr, C.c_size_t(nbytes), 2) == 0
                assert np.array_equal(back, means[shown]), (k, shown)
            st = ctx.stats()  # (waits for the rest)
            assert st["scene_drains"] == 0 and st["scene_splits"] == 1, st
            assert np.array_equal(ctx.download().reshape(-1, 4), acc)
        finally:
            hip.hipFree(dptr)


def test_table_ring_is_made_lazily_and_capped_by_bytes():
    """(r06) gsp_upload_scene holds ONE copy of the BSDF / light tables; the version ring behind per-frame
    gsp_update_tables is made by the first edit that arrives with samples in flight, and its size is capped by bytes (a
    sixteenth of the free memory, at most 1 GiB).  A mesh emitter of a million triangles = 64 MB of light records: r05 allocated
    64 slots = 4 GB at upload; now the upload holds 64 MB and the ring gets 16 slots.  With 16 slots and paths that live for
    dozens of one-sample frames some edits must wait (scene_drains > 0) -- and the frames equal those of a context that waits
    before EVERY edit, bit for bit."""
    import copy

    import gpuspectral_amd as g
    from gpuspectral_amd import scenes

    b = scenes.SceneBuilder()
    room = b.add_mesh(*scenes.box_mesh())
    ball = b.add_mesh(*scenes.sphere_mesh(1024, 512))
    b.add_object(room, scenes.trs((0, 1, 0), (2.0, 1.2, 2.0)), b.diffuse((0.7, 0.6, 0.5)), twofaced=True)
    b.add_object(ball, scenes.trs((0.3, 1.4, -0.2), (0.3, 0.3, 0.3)), b.diffuse((0, 0, 0)), emission=(60.0, 50.0, 30.0))
    b.camera_lookat((1.6, 1.1, 1.7), (0, 0.9, 0), fov_deg=60)
    sc0 = b.build()
    slot_bytes = len(sc0.lights) * 64
    assert slot_bytes > 60e6
    W, H, frames = 40, 32, 24

    def edit(sc, k):
        lights = sc.lights.copy()
        lights["radiance"][:, :3] = np.array([60.0, 50.0, 30.0], np.float32) * np.float32(0.5 + 0.1 * (k % 6))
        sc.lights = lights

    def run(sync_every_frame):
        sc = copy.deepcopy(sc0)
        with g.Context(0) as ctx:
            ctx.upload_scene(sc)
            ctx.frame_begin(W, H)
            ctx.render(spp=1, first_timestamp=0)
            for k in range(1, frames):  # (no gsp_get_stats in this loop: it completes the queued samples, like gsp_sync)
                edit(sc, k)
                if sync_every_frame:
                    ctx.sync()
                ctx.update_tables(sc)
                ctx.render(spp=1, first_timestamp=k)
            return ctx.download().reshape(-1, 4), ctx.stats()

    img, st = run(False)
    ref, st_ref = run(True)
    assert np.array_equal(img, ref), "%d pixels differ" % int((img != ref).any(1).sum())
    # the context that waits before every edit never needs a ring (nothing is in flight when an edit arrives): what the other one
    # holds beyond it IS the ring -- made by its first in-flight edit, within the byte budget
    ring = int(st["device_bytes"]) - int(st_ref["device_bytes"])
    assert 7 * slot_bytes <= ring <= (1 << 30), (ring, slot_bytes)
    assert abs(ring / slot_bytes - 15.0) < 0.01, ring / slot_bytes  # 15 more slots (a slot = the light records + the few BSDF records): 16 = floor(1 GiB / 64 MB)
    assert st["scene_updates"] == frames - 1 == st_ref["scene_updates"]
    assert st["scene_drains"] > 0  # (16 slots, paths of up to 52 bounces in one-sample frames: some edits wait)


# ---- the arms of gsp_update_instances, one segment each ----------------------------------------------------------------------
# (pt_versions.h: (1) refit of the edited tree, (2) split / re-split, (3) the whole tree.)  Two small instances of the materials
# scene, A and B, are edited between one-sample frames with samples in flight; every frame is accumulated against the oracle
# rendering the scene as it is at that frame, and the counters are read once, at the end (gsp_get_stats completes the samples).
_SEGMENT_1 = [{"A": "small"}, {"A": "small"}, {"B": "small"}, {"A": "small", "B": "small"}]
_EDIT_SEGMENTS = {
    # steps, then scene_updates, scene_splits, scene_refits, scene_drains
    "refit-and-resplit": (_SEGMENT_1, 4, 2, 2, 1),  # no-wait split, in-slot refit, re-split behind a wait (B is new), in-slot refit
    "edited-tree-degrades": ([{"A": "small"}, {"A": "far"}], 2, 2, 0, 1),  # no-wait split; the small tree grows fourfold: both trees again
    "first-edit-moves-far": ([{"A": "far"}], 1, 1, 0, 1),  # the no-wait split's refit grows fourfold: the small tree is built where it is
}


def _two_small_instances(sc):
    """The two boxes of the materials scene: together at most a quarter of the triangles (what a split accepts)."""
    vc = sc.instances["vertex_count"]
    a, b = [int(i) for i in np.flatnonzero(vc == 36)[:2]]
    assert (int(vc[a]) + int(vc[b])) * 4 <= int(vc.sum()), (vc[a], vc[b], vc.sum())
    return {"A": a, "B": b}


def _edit_instance(sc, inst, i, how):
    t = inst["transform"][i].copy()  # column-major: t[12:15] is the translation
    if how == "small":
        t[12:15] += np.float32(0.03) * np.array([0.5, 0.1, -0.3], np.float32)
    else:  # "far": scaled by 2 about its own centre -- four times the box area of a single-instance tree
        first, count = int(inst["first_vertex"][i]), int(inst["vertex_count"][i])
        p = np.asarray(sc.positions, np.float32).reshape(-1, 3)[first:first + count]
        c = (p.min(0) + p.max(0)) * np.float32(0.5)
        centre = c[0] * t[0:3] + c[1] * t[4:7] + c[2] * t[8:11] + t[12:15]
        for col in (0, 4, 8):
            t[col:col + 3] *= np.float32(2.0)
        t[12:15] = centre + np.float32(2.0) * (t[12:15] - centre)
    inst["transform"][i] = t


def _run_edit_segment(ctx, sc, steps, oracle_mod=None, W=40, H=30):
    """render; then per step: edit, gsp_update_instances, render (one sample each, nothing waits).  -> the oracle's accumulation"""
    who = _two_small_instances(sc)
    inst = sc.instances.copy()
    acc = None
    for k in range(len(steps) + 1):
        if k:
            inst = inst.copy()
            for name, how in steps[k - 1].items():
                _edit_instance(sc, inst, who[name], how)
            sc.instances = inst
            ctx.update_instances(inst)
        ctx.render(spp=1, first_timestamp=k)
        if oracle_mod is not None:
            acc, _ = oracle_mod.Oracle(sc).render(W, H, spp=1, first_timestamp=k, accum=acc)
    return acc


@pytest.mark.gpu
@pytest.mark.parametrize("segment", sorted(_EDIT_SEGMENTS))
def test_update_instances_arms(oracle_mod, materials_scene, segment):
    """One segment per arm that had no exact counter check: the re-split, the edited tree that degrades, the first edit that moves
    too far.  Frames equal the oracle's bit for bit; the four scene counters are exactly what the arms taken add up to."""
    import copy

    import gpuspectral_amd as g

    steps, updates, splits, refits, drains = _EDIT_SEGMENTS[segment]
    sc = copy.deepcopy(materials_scene)
    W, H = 40, 30
    with g.Context(0) as ctx:
        ctx.upload_scene(sc)
        ctx.frame_begin(W, H)
        acc = _run_edit_segment(ctx, sc, steps, oracle_mod, W, H)
        img = ctx.download().reshape(-1, 4)
        st = ctx.stats()
    got = tuple(int(st[k]) for k in ("scene_updates", "scene_splits", "scene_refits", "scene_drains"))
    print("segment %s: updates, splits, refits, drains = %s" % (segment, got))
    assert np.array_equal(img, acc), "%d pixels differ" % int((img != acc).any(1).sum())
    assert got == (updates, splits, refits, drains), st


@pytest.mark.gpu
def test_device_bytes_settle_over_scene_cycles(materials_scene):
    """One context, three cycles of upload + frame + the edits of the first segment + sync: nothing shrinks, so from the second
    cycle on every buffer has its size and gsp_stats.device_bytes repeats."""
    import copy

    import gpuspectral_amd as g

    held = []
    with g.Context(0) as ctx:
        for _ in range(3):
            sc = copy.deepcopy(materials_scene)
            ctx.upload_scene(sc)
            ctx.frame_begin(40, 30)
            _run_edit_segment(ctx, sc, _SEGMENT_1)
            ctx.sync()
            held.append(int(ctx.stats()["device_bytes"]))
    print("device_bytes after each cycle:", held)
    assert held[1] == held[2], held
