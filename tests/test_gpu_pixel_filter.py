"""Pixel filter (include/gpuspectral_pt.h, "Pixel filter") on the GPU.

The wavefront pipeline against the same stage headers run in scalar on the host (tests/emu/filter_emu.cpp), bit for bit, for
every filter; an emitter-only scene whose expected image is composed from the emu's rays, the ORACLE's traversal and a numpy
running mean; the primary-hit memo across filtered / unfiltered calls; and the invariances every feature of the tracer keeps:
call splits, timestamps in flight, lanes, k_finish, adaptive sampling, tile shares, scene edits, struct_size."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import CORNELL_XML, ROOT
from test_pixel_filter_cpu import BOX, GAUSSIAN, NONE, TENT, FilterEmu

pytestmark = pytest.mark.gpu

FILTERS = [(BOX, 0.0), (TENT, 0.0), (TENT, 1.5), (GAUSSIAN, 0.0)]
COUNTS = ("extension_rays", "shadow_rays", "shaded_vertices")


@pytest.fixture(scope="module")
def femu():
    return FilterEmu()


@pytest.fixture(scope="module")
def ctx():
    import gpuspectral_amd as g

    c = g.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def wctx():
    """A context that never hands the last paths to k_finish (finish_paths = never): on frames as small as a test's, the default
    context lets k_finish trace every path of the drain itself, camera ray included, and the primary-hit memo -- which only the
    wavefront extend launch consults -- answers nothing, filter or not.  The memo tests need the path the bench runs."""
    import gpuspectral_amd as g

    c = g.Context(0, finish_paths=0xFFFFFFFF)
    yield c
    c.close()


def frame(ctx, sc, W, H, calls, upload=True, pixel_ids=None, **kw):
    """One frame of gsp_render calls [(spp, params...)]; returns (compact image, stats of the frame)."""
    if upload:
        ctx.upload_scene(sc)
    ctx.frame_begin(W, H, pixel_ids=pixel_ids)
    ctx.reset_stats()
    t = 0
    for spp in calls:
        ctx.render(spp=spp, first_timestamp=t, **kw)
        t += spp
    return ctx.download_compact().copy(), ctx.stats()


def same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


# ---- GPU == emu, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,W,spp", [("cornell", 64, 8), ("materials", 48, 4)])
@pytest.mark.parametrize("filt,param", FILTERS)
@pytest.mark.parametrize("ts0", [0, 5])
def test_gpu_equals_emu(ctx, femu, cornell, which, W, spp, filt, param, ts0):
    from gpuspectral_amd import scenes

    sc = cornell if which == "cornell" else scenes.cornell_materials(16)
    es = femu.scene(sc)
    ref, rst = es.render(W, W, spp, first_timestamp=ts0, pixel_filter=filt, pixel_filter_param=param)
    ctx.upload_scene(sc)
    ctx.frame_begin(W, W)
    ctx.reset_stats()
    ctx.render(spp=spp, first_timestamp=ts0, pixel_filter=filt, pixel_filter_param=param)
    img = ctx.download_compact()
    st = ctx.stats()
    bad = np.nonzero(np.any(img.view(np.uint32) != ref.view(np.uint32), axis=1))[0]
    assert len(bad) == 0, "%d of %d pixels differ from the emu (first: %d)" % (len(bad), W * W, bad[0])
    for k in COUNTS:
        assert st[k] == rst[k], k
    assert st["samples"] == W * W * spp


# ---- exact composition with the oracle ------------------------------------------------------------------------------------
def emitter_scene(n=200, seed=4):
    """n single-triangle instances at varied depths, each with its own emission below the clamp, on a black diffuse BSDF:
    nothing after the first hit contributes.  Every triangle faces the camera by a clear margin."""
    from gpuspectral_amd import scenes

    rng = np.random.RandomState(seed)
    b = scenes.SceneBuilder()
    black = b.diffuse((0.0, 0.0, 0.0))
    b.camera_lookat((0, 0, 5), (0, 0, 0), fov_deg=40.0)
    ident = np.eye(4, dtype=np.float32).reshape(16)
    for _ in range(n):
        c = np.array([rng.uniform(-1.6, 1.6), rng.uniform(-1.6, 1.6), rng.uniform(-3.0, 2.0)])
        a = rng.uniform(0, 2 * np.pi)
        r = rng.uniform(0.15, 0.45)
        tilt = rng.uniform(-0.5, 0.5, 3)
        p = [c + r * np.array([np.cos(a + k * 2.1), np.sin(a + k * 2.1), tilt[k]]) for k in range(3)]
        nrm = np.cross(p[1] - p[0], p[2] - p[0])
        if nrm[2] < 0:  # counter-clockwise as seen from +z, where the camera is
            p[1], p[2] = p[2], p[1]
            nrm = -nrm
        nrm /= np.linalg.norm(nrm)
        mesh = b.add_mesh(np.array(p, np.float32), np.tile(nrm.astype(np.float32), (3, 1)))
        b.add_object(mesh, ident, black, twofaced=False, emission=rng.uniform(0.5, 15.0, 3).astype(np.float32))
    return b.build()


def test_emitter_scene_composes_with_the_oracle(ctx, femu, oracle_mod):
    """Expected image: the emu's filtered camera rays -> Oracle.trace -> the hit primitive's emission (front-facing by
    construction) -> the float32 running mean restated in numpy.  The GPU frame with BOX at 16 spp equals it bit for bit."""
    W = H = 48
    SPP = 16
    sc = emitter_scene()
    orc = oracle_mod.Oracle(sc)
    gids = np.arange(W * H, dtype=np.uint32)
    pos = np.asarray(sc.positions, np.float64).reshape(-1, 3, 3)
    nrm = np.cross(pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    acc = np.zeros((W * H, 4), np.float32)
    hits_any = 0
    for ts in range(SPP):
        o, d, _, _ = femu.generate(sc, W, H, BOX, 0.0, gids, np.full(W * H, ts, np.uint32))
        rays = np.zeros((W * H, 8), np.float32)
        rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, 0.0, d, 1e10
        prim = orc.trace(rays)["prim"]
        hit = prim >= 0
        hits_any += int(hit.sum())
        ndv = -(nrm[prim[hit]] * d[hit].astype(np.float64)).sum(1)
        assert ndv.min() > 1e-3  # every hit is front-facing, far from the float32 sign boundary
        c = np.zeros((W * H, 3), np.float32)
        c[hit] = sc.instances["emission"][prim[hit]]
        if ts > 0:  # resolve_sample: mix(prev, c, 1 / (ts + 1)) in float32, in this order
            a = np.float32(1.0) / np.float32(ts + 1)
            c = acc[:, :3] * (np.float32(1.0) - a) + c * a
        acc[:, :3] = c
        acc[:, 3] = 1.0
    assert hits_any > W * H * SPP // 10
    img, st = frame(ctx, sc, W, H, [SPP], pixel_filter=BOX)
    bad = np.nonzero(np.any(img.view(np.uint32) != acc.view(np.uint32), axis=1))[0]
    assert len(bad) == 0, "%d pixels differ (first: %d: %s vs %s)" % (len(bad), bad[0], img[bad[0]], acc[bad[0]])
    assert len(np.unique(img[:, 0])) > 100  # (a jittered frame of edges: many partial coverages)


# ---- the primary-hit memo -------------------------------------------------------------------------------------------------
def test_none_with_param_is_todays_image(ctx, wctx, oracle_mod, cornell):
    W = H = 64
    ref, ost = oracle_mod.Oracle(cornell).render(W, H, spp=6)
    img, st = frame(wctx, cornell, W, H, [6], pixel_filter=NONE, pixel_filter_param=2.5)
    assert same(img, ref)
    assert st["memoised_rays"] > 0 and st["extension_rays"] == ost["extension_rays"]
    img, st = frame(ctx, cornell, W, H, [6], pixel_filter=NONE, pixel_filter_param=2.5)  # the default context (k_finish drains)
    assert same(img, ref) and st["extension_rays"] == ost["extension_rays"]


@pytest.mark.parametrize("filt,param", FILTERS)
def test_filtered_call_does_not_use_the_memo(wctx, cornell, filt, param):
    ctx = wctx
    W = H = 64
    ctx.upload_scene(cornell)
    ctx.frame_begin(W, H)
    ctx.render(spp=2)  # unfiltered: builds the memo
    ctx.sync()
    s0 = ctx.stats()
    assert s0["memo_build_rays"] > 0 and s0["memoised_rays"] > 0
    ctx.reset_stats()
    ctx.render(spp=4, first_timestamp=2, pixel_filter=filt, pixel_filter_param=param)
    ctx.sync()
    s1 = ctx.stats()
    assert s1["memoised_rays"] == 0 and s1["memo_build_rays"] == 0
    assert s1["extension_rays"] >= W * H * 4  # every camera ray was traced
    ctx.frame_begin(W, H)
    ctx.reset_stats()
    ctx.render(spp=4, pixel_filter=filt, pixel_filter_param=param)  # a fresh frame, filtered from its first call: no memo at all
    ctx.sync()
    s2 = ctx.stats()
    assert s2["memoised_rays"] == 0 and s2["memo_build_rays"] == 0


def test_unfiltered_after_filtered_equals_oracle(wctx, oracle_mod, cornell, materials_scene):
    """Memo validity across a switch: filtered frame, then unfiltered frames on the same context (same scene: a memo that is
    still valid may be reused; another scene and another frame size: it must be rebuilt), all equal to the oracle."""
    ctx = wctx
    W = H = 64
    frame(ctx, cornell, W, H, [4], pixel_filter=TENT)
    img, st = frame(ctx, cornell, W, H, [4], upload=False)
    assert same(img, oracle_mod.Oracle(cornell).render(W, H, spp=4)[0]) and st["memoised_rays"] > 0
    # within ONE frame: unfiltered, filtered, unfiltered again -- the filtered call must not have spoilt the memo
    ctx.frame_begin(W, H)
    ctx.render(spp=2)
    ctx.render(spp=2, first_timestamp=2, pixel_filter=BOX)
    ctx.frame_begin(W, H)
    ctx.render(spp=3, pixel_filter=GAUSSIAN)
    ctx.frame_begin(W, H)
    ctx.render(spp=5)
    assert same(ctx.download_compact(), oracle_mod.Oracle(cornell).render(W, H, spp=5)[0])
    frame(ctx, materials_scene, 48, 40, [2], pixel_filter=BOX)
    img, _ = frame(ctx, materials_scene, 48, 40, [3], upload=False)
    assert same(img, oracle_mod.Oracle(materials_scene).render(48, 40, spp=3)[0])


# ---- invariances ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt,param", [(BOX, 0.0), (TENT, 0.0), (GAUSSIAN, 0.0)])
def test_progressive_and_pipeline_options(ctx, femu, cornell, filt, param):
    import gpuspectral_amd as g

    W = H = 64
    kw = dict(pixel_filter=filt, pixel_filter_param=param)
    one, _ = frame(ctx, cornell, W, H, [8], **kw)
    assert same(one, femu.scene(cornell).render(W, H, 8, **kw)[0])
    two, _ = frame(ctx, cornell, W, H, [4, 4], upload=False, **kw)
    assert same(one, two)  # 2 calls x 4 spp == 1 call x 8 spp
    tif, _ = frame(ctx, cornell, W, H, [8], upload=False, timestamps_in_flight=1, **kw)
    assert same(one, tif)
    for opts in (dict(lanes=1), dict(lanes=2), dict(finish_paths=0xFFFFFFFF), dict(lanes=2, finish_paths=0xFFFFFFFF)):
        with g.Context(0, **opts) as c:
            img, _ = frame(c, cornell, W, H, [3, 5], **kw)
            assert same(one, img), opts


def test_adaptive_with_filter(ctx, femu, cornell):
    """A pixel that stopped after N samples equals the uniform FILTERED frame at N spp for that pixel."""
    W = H = 64
    es = femu.scene(cornell)
    ctx.upload_scene(cornell)
    for thr in (0.02, 0.03, 0.05, 0.07, 0.1, 0.15, 0.2, 0.3, 0.5):
        ctx.frame_begin(W, H)
        ctx.render(spp=48, adaptive_threshold=thr, adaptive_min_spp=8, adaptive_step=8, pixel_filter=TENT)
        img = ctx.download_compact()
        _, spp = ctx.pixel_stats()
        if len(np.unique(spp)) >= 3:
            break
    assert len(np.unique(spp)) >= 3, "no threshold stops pixels at three different counts"
    ids = np.arange(W * H, dtype=np.uint32)
    for n in np.unique(spp):
        sel = np.nonzero(spp == n)[0]
        ref, _ = es.render(W, H, int(n), pixel_filter=TENT, pixel_ids=ids[sel])
        assert same(img[sel], ref), "N_p = %d" % n


@pytest.mark.parametrize("world", [2, 3])
def test_shares_equal_single_context(ctx, cornell, world):
    from gpuspectral_amd import pt

    W, H = 96, 80
    single, _ = frame(ctx, cornell, W, H, [2, 3], pixel_filter=TENT, pixel_filter_param=1.5)
    with pt.MultiContext([0] * world) as m:  # a repeated device: the copy route
        m.upload_scene(cornell)
        m.frame_begin(W, H)
        m.render(spp=2, pixel_filter=TENT, pixel_filter_param=1.5)
        m.render(spp=3, first_timestamp=2, pixel_filter=TENT, pixel_filter_param=1.5)
        m.gather()
        img = m.download()
        assert m.gather_route()[0] == "copy"
    assert same(img.reshape(-1, 4), single)


def test_scene_edits_between_filtered_calls(femu, materials_scene):
    """gsp_update_camera and gsp_update_instances between filtered calls (the versioned and split-scene kernels generate and
    trace the later samples): the frame after the edits equals a fresh context's."""
    import copy

    import gpuspectral_amd as g

    W, H = 64, 48
    sc = copy.copy(materials_scene)
    kw = dict(pixel_filter=BOX)
    with g.Context(0) as c:
        c.upload_scene(sc)
        c.frame_begin(W, H)
        c.render(spp=3, **kw)  # no sync: the edits arrive while samples may be in flight
        tw = np.asarray(sc.to_world, np.float32).copy()
        tw[12] += 0.2
        sc.to_world = tw
        inst = sc.instances.copy()
        t = inst["transform"][len(inst) - 1].copy()
        t[13] += 0.05
        inst["transform"][len(inst) - 1] = t
        sc.instances = inst
        c.update_camera(sc.to_world, sc.fov)
        c.update_instances(sc.instances)
        c.frame_begin(W, H)
        c.render(spp=2, **kw)
        c.update_instances(sc.instances)
        c.render(spp=2, first_timestamp=2, **kw)
        edited = c.download_compact().copy()
    with g.Context(0) as c:
        fresh, _ = frame(c, sc, W, H, [4], **kw)
    assert same(edited, fresh)
    assert same(fresh, femu.scene(sc).render(W, H, 4, **kw)[0])


# ---- the ABI's edges ------------------------------------------------------------------------------------------------------
def test_invalid_filter_is_refused(ctx, cornell):
    import gpuspectral_amd as g

    ctx.upload_scene(cornell)
    ctx.frame_begin(32, 32)
    with pytest.raises(g.GspError, match="pixel_filter") as e:
        ctx.render(spp=1, pixel_filter=4)
    assert "(1)" in str(e.value)  # GSP_ERR_INVALID
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(g.GspError, match="pixel_filter_param"):
            ctx.render(spp=1, pixel_filter=TENT, pixel_filter_param=bad)
    ctx.render(spp=1, pixel_filter=TENT)  # the context is still usable


def test_struct_size_before_the_new_fields_renders_unfiltered(ctx, oracle_mod, cornell):
    from gpuspectral_amd import abi

    W = H = 48
    ctx.upload_scene(cornell)
    ctx.frame_begin(W, H)
    p = abi.default_render_params(4, 0)
    p.pixel_filter, p.pixel_filter_param = BOX, 0.0
    p.struct_size = abi.RenderParams.pixel_filter.offset  # an older host of ABI 9: the struct ends behind adaptive_step
    ctx._check(ctx._L.gsp_render(ctx._h, C.byref(p)), "gsp_render")
    assert same(ctx.download_compact(), oracle_mod.Oracle(cornell).render(W, H, spp=4)[0])
    z = abi.RenderParams()  # zero-initialised (struct_size 0 = the ABI-8 layout) apart from what a render needs
    z.spp, z.max_depth, z.rr_start_depth, z.clamp = 4, 50, 10, 20.0
    z.pixel_filter = TENT  # beyond what struct_size 0 covers: not read
    ctx.frame_begin(W, H)
    ctx._check(ctx._L.gsp_render(ctx._h, C.byref(z)), "gsp_render")
    assert same(ctx.download_compact(), oracle_mod.Oracle(cornell).render(W, H, spp=4)[0])


def test_cli_scene_filter_equals_python_tent(ctx, cornell, tmp_path):
    from oracle import mitsuba_loader as ml

    lib = os.path.join(ROOT, "gpuspectral_amd", "lib")
    exe = os.path.join(lib, "gsp_render")
    env = dict(os.environ, LD_LIBRARY_PATH=lib + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    W, H, SPP = 64, 48, 4
    out = str(tmp_path / "f.pfm")
    r = subprocess.run([exe, "--scene-filter", CORNELL_XML, out, str(W), str(H), str(SPP)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    pfm = ml.read_pfm(out)
    img, _ = frame(ctx, cornell, W, H, [SPP], pixel_filter=TENT, pixel_filter_param=1.0)
    rgb = img.reshape(H, W, 4)[:, :, :3]
    got = np.asarray(pfm, np.float32).reshape(H, W, -1)[:, :, :3]
    assert same(got, rgb) or same(got[::-1], rgb)  # (PFM rows run bottom to top)
    out2 = str(tmp_path / "g.pfm")
    r = subprocess.run([exe, "--filter", "tent:1", CORNELL_XML, out2, str(W), str(H), str(SPP)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert same(np.asarray(ml.read_pfm(out2), np.float32), np.asarray(pfm, np.float32))
