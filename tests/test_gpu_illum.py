"""The illumination history on the GPU (include/gpuspectral_pt.h, "Illumination history"): k_temporal_reproject_illum, k_illum_prepare,
k_illum_image and k_svgf_atrous_feedback against the same text run on the host (csrc/pt_illum.h through tests/emu/illum_emu.cpp, itself
checked against a float64 restatement in tests/test_illum_cpu.py).  The history, its moments and motion plane, the image read-out, the
feedback's output and the history after the feedback equal the emulation applied to gsp_download + gsp_download_features + the previous
emulated history BIT FOR BIT, frame after frame; then parity with the feature off, state, bytes and refusals, two quality orderings,
the device-memory read-outs, the host layer and the CLI."""
import copy
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import temporal_util as tu
from conftest import GOLDEN, ROOT
from illum_util import IllumEmu
from temporal_util import FLT_MIN, refusals, same
from test_gpu_motion import MOVERS, ORBIT, moved_instances, orbit, words

pytestmark = pytest.mark.gpu

# demodulate x {plain, moments, moments + follow}; feedback of 1 and of 3 levels on the moments cases (level 2 is the first that reads
# its taps from global memory)
CASES = [(d, m, lv) for d in (False, True) for m, lv in (("plain", 0), ("moments", 1), ("moments", 3), ("moments+follow", 1), ("moments+follow", 3))]
CASE_IDS = ["%s-%s-fb%d" % ("demod" if d else "colour", m, lv) for d, m, lv in CASES]
# the feedback level by (levels, iterations): level 1 (the second step that stages its taps in LDS) and a last level of each kind --
# iterations None = the default of 5
FB_LEVELS = [(2, None), (1, 1), (2, 2), (3, 3)]


@pytest.fixture(scope="module")
def emu():
    return IllumEmu()


@pytest.fixture(scope="module")
def scenes_(cornell, materials_scene):
    import textured

    return {"cornell": cornell, "materials": materials_scene, "textured": textured.decorate(copy.deepcopy(materials_scene), seed=5, envmap=False)}


@pytest.fixture(scope="module")
def rigs(scenes_):
    """Per scene: one context with the scene uploaded, shared by the cases below and put into the case's state."""
    import gpuspectral_amd as g

    made = {}

    def get(name, demod, mode):
        if name not in made:
            made[name] = g.Context(0)
            made[name].upload_scene(scenes_[name])
        ctx = made[name]
        ctx.set_lens()
        ctx.update_camera(scenes_[name].to_world, scenes_[name].fov)
        ctx.update_instances(scenes_[name].instances)
        ctx.temporal_demodulate(demod)
        ctx.temporal_track_moments("moments" in mode)
        ctx.temporal_follow_instances("follow" in mode)
        ctx.temporal_reset()
        return ctx

    yield get
    for ctx in made.values():
        ctx.close()


def check(what, name, got, want):
    bad = int((words(got) != words(want)).sum())
    assert bad == 0, "%s: %d of %d words of %s differ" % (what, bad, got.size, name)


def begin(ctx, size, ts, cam=None, fov=None, inst=None):
    if inst is not None:
        ctx.update_instances(inst)  # (before the frame's feature pass, as following asks)
    if cam is not None:
        ctx.update_camera(cam, fov)
    ctx.frame_begin(*size)
    ctx.frame_sample_base(ts)
    ctx.render(1, ts)
    ctx.render_features(1, ts)


def frame(ctx, emu, hist, cam, fov, size, ts, inst, demod, mode, levels, what="", dn=None):
    """One frame of the viewer loop -- the edit, the camera, the frame, its feature pass, the accumulate, the image read-out and (levels)
    the feedback -- on the GPU and by the emulation from `hist`.  Returns the emulated history the next frame starts from."""
    from gpuspectral_amd import abi

    moments, follow = "moments" in mode, "follow" in mode
    begin(ctx, size, ts, cam, fov, inst)
    ctx.temporal_accumulate(None)
    c = ctx.download()
    a, g, i = ctx.download_features()
    new = emu.step(None, cam, fov, c, a, g, i, xforms=inst["transform"] if follow else None, hist=hist, moments=moments, demod=demod)
    check(what, "H", ctx.download_temporal(), new.H)
    if moments:
        check(what, "M", ctx.download_temporal_moments(), new.M)
    if follow:
        check(what, "V", ctx.download_temporal_motion(), new.V)
    check(what, "the image", ctx.download_temporal_image(), emu.image(new.H, a, demod))
    if levels:
        sv = abi.svgf(min_history=2)
        out, fb = emu.svgf(dn, sv, new.H, new.M, a, g, demod=demod, levels=levels)
        check(what, "the feedback's output", ctx.temporal_svgf_feedback(dn, sv, levels), out)
        check(what, "H after the feedback", ctx.download_temporal(), fb)
        check(what, "the image after the feedback", ctx.download_temporal_image(), emu.image(fb, a, demod))
        check(what, "M after the feedback", ctx.download_temporal_moments(), new.M)
        new.H = fb
    return new


def sequence(ctx, emu, sc, size, movers, demod, mode, levels, degrees=ORBIT, what="", dn=None):
    hist = None
    for k, cam in enumerate(orbit(sc, degrees)):
        hist = frame(ctx, emu, hist, cam, sc.fov, size, k, moved_instances(sc.instances, movers, k), demod, mode, levels, "%s frame %d" % (what, k), dn)
    return hist


# ---- bit for bit against the emulation -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("demod,mode,levels", CASES, ids=CASE_IDS)
def test_cornell_orbit_with_the_tall_box_moving(rigs, emu, scenes_, demod, mode, levels):
    hist = sequence(rigs("cornell", demod, mode), emu, scenes_["cornell"], (96, 64), MOVERS["cornell"], demod, mode, levels, what="cornell")
    assert hist.H[..., 3].max() >= 3.0  # (the last three frames of the orbit are 2 degrees apart)
    if mode == "moments+follow":
        assert (hist.V[..., 3] == 1.0).any()


@pytest.mark.parametrize("demod,mode,levels", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("size", [(33, 17), (5, 3), (1, 1)])
def test_materials_scene(rigs, emu, scenes_, size, demod, mode, levels):
    sequence(rigs("materials", demod, mode), emu, scenes_["materials"], size, MOVERS["materials"], demod, mode, levels, what="materials %dx%d" % size)


@pytest.mark.parametrize("demod", [False, True], ids=["colour", "demod"])
@pytest.mark.parametrize("levels,iterations", FB_LEVELS)
def test_materials_scene_feedback_levels(rigs, emu, scenes_, demod, levels, iterations):
    """33 x 17 (two tiles across, three down, ragged both ways): the feedback on the filter's second level and on its last one."""
    from gpuspectral_amd import abi

    dn = abi.denoise(iterations=iterations) if iterations else None
    sequence(rigs("materials", demod, "moments"), emu, scenes_["materials"], (33, 17), MOVERS["materials"], demod, "moments", levels, degrees=ORBIT[:4],
             what="materials 33x17, level %d of %s" % (levels, iterations), dn=dn)


@pytest.mark.parametrize("demod", [False, True], ids=["colour", "demod"])
def test_materials_scene_following_without_moments(rigs, emu, scenes_, demod):
    """The one state of the three switches that CASES leaves out, at 33 x 17: instances followed, no moments plane."""
    hist = sequence(rigs("materials", demod, "follow"), emu, scenes_["materials"], (33, 17), MOVERS["materials"], demod, "follow", 0, degrees=ORBIT[:4],
                    what="materials 33x17, following without moments")
    assert hist.M is None and hist.V is not None


@pytest.mark.parametrize("demod,mode,levels", CASES, ids=CASE_IDS)
def test_ragged_tiles(rigs, emu, scenes_, demod, mode, levels):
    """300 x 200: ten tiles of 32 across (the last one 12 wide), 25 of 8 down; four frames."""
    hist = sequence(rigs("materials", demod, mode), emu, scenes_["materials"], (300, 200), MOVERS["materials"], demod, mode, levels,
                    degrees=[0.0, 3.0, -4.0, 9.0], what="materials 300x200")
    assert hist.H[..., 3].max() > 3.0 and (hist.H[..., 3] == 1.0).any()


@pytest.mark.parametrize("demod,mode,levels", CASES, ids=CASE_IDS)
def test_textured_scene(rigs, emu, scenes_, demod, mode, levels):
    """An albedo that differs from pixel to pixel: what the division and the re-modulation are for."""
    ctx, sc = rigs("textured", demod, mode), scenes_["textured"]
    hist = sequence(ctx, emu, sc, (48, 32), MOVERS["materials"], demod, mode, levels, degrees=ORBIT[:6], what="textured 48x32")
    alb = ctx.download_features()[0]
    # the albedo plane is textured: more distinct albedos in the frame than the scene has BSDF records
    assert len(np.unique(words(alb[..., :3]).reshape(-1, 3), axis=0)) > sum(len(r) for r in sc.bsdfs)
    if demod:
        assert not same(ctx.download_temporal_image()[..., :3], hist.H[..., :3])


def test_the_filters_of_a_demodulated_history(rigs, emu, scenes_):
    """gsp_download_temporal_svgf and gsp_download_temporal_denoised on a demodulated history: Prepare takes H as e."""
    from gpuspectral_amd import abi

    ctx, sc = rigs("textured", True, "moments"), scenes_["textured"]
    hist = sequence(ctx, emu, sc, (48, 32), MOVERS["materials"], True, "moments", 0, degrees=ORBIT[:4], what="filters")
    a, g, _ = ctx.download_features()
    for dn, sv in ((None, None), (abi.denoise(iterations=3), abi.svgf(min_history=2, sigma_variance=1.0))):
        check("filters", "svgf", ctx.download_temporal_svgf(dn, sv), emu.svgf(dn, sv, hist.H, hist.M, a, g))
        check("filters", "denoised", ctx.download_temporal_denoised(dn), emu.denoise(dn, hist.H, a, g))


# ---- off parity ------------------------------------------------------------------------------------------------------------------------
def test_off_is_word_identical_to_a_context_that_never_heard_of_it(scenes_):
    import gpuspectral_amd as g

    sc = scenes_["cornell"]
    with g.Context(0) as a, g.Context(0) as b:
        for ctx in (a, b):
            ctx.upload_scene(sc)
            ctx.temporal_track_moments(True)
        a.temporal_demodulate(False)  # (the current value: nothing happens)
        for k, cam in enumerate(orbit(sc, ORBIT)):
            for ctx in (a, b):
                begin(ctx, (96, 64), k, cam, sc.fov)
                ctx.temporal_accumulate(None)
            assert same(a.download_temporal(), b.download_temporal()), k
            assert same(a.download_temporal_moments(), b.download_temporal_moments()), k
            assert same(a.download_temporal_svgf(), b.download_temporal_svgf()), k
            assert same(a.download_temporal_image(), b.download_temporal()), k
            assert same(b.download_temporal_image(), b.download_temporal()), k


# ---- feedback once ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("demod", [False, True], ids=["colour", "demod"])
def test_feedback_once_per_accumulate(scenes_, emu, demod):
    import gpuspectral_amd as g
    from gpuspectral_amd import abi

    sc = scenes_["cornell"]
    size = (96, 64)
    sv = abi.svgf(min_history=2)
    with g.Context(0) as ctx:
        ctx.upload_scene(sc)
        ctx.temporal_track_moments(True)
        ctx.temporal_demodulate(demod)
        for k in range(3):
            begin(ctx, size, k)
            ctx.temporal_accumulate(None)
            before = ctx.download_temporal_svgf(None, sv)
            h0, m0 = ctx.download_temporal(), ctx.download_temporal_moments()
            a, gm, _ = ctx.download_features()
            want_out, want_h = emu.svgf(None, sv, h0, m0, a, gm, demod=demod, levels=2)
            if k == 1:  # no output asked for: the history is fed back all the same
                assert ctx.temporal_svgf_feedback(None, sv, 2, out=False) is None
            else:
                out = ctx.temporal_svgf_feedback(None, sv, 2)
                assert same(out, before) and same(out, want_out)
            check("frame %d" % k, "H after the feedback", ctx.download_temporal(), want_h)
            assert same(ctx.download_temporal()[..., 3], h0[..., 3]) and not same(ctx.download_temporal(), h0)
            assert same(ctx.download_temporal_moments(), m0)
            with pytest.raises(g.GspError, match="fed back already"):
                ctx.temporal_svgf_feedback(None, sv, 1)
            check("frame %d" % k, "H after the refused call", ctx.download_temporal(), want_h)


# ---- state, bytes and refusals ------------------------------------------------------------------------------------------------------------
def test_state_bytes_and_refusals(scenes_):
    import gpuspectral_amd as g
    from gpuspectral_amd import abi

    sc = scenes_["cornell"]
    w, h = 96, 64
    size = (w, h)
    skip = ("render_seconds", "extend_kernel_ms", "shade_kernel_ms", "connect_kernel_ms", "bvh_build_ms", "device_bytes")

    def untouched(ctx, call):
        """The frame's state around a call: download, features, stats apart from times and bytes."""
        state = lambda: (ctx.download(), ctx.download_features(), ctx.stats())
        s0 = state()
        res = call()
        s1 = state()
        assert same(s0[0], s1[0]) and all(np.array_equal(words(p), words(q)) for p, q in zip(s0[1], s1[1]))
        assert all(s1[2][k] == v for k, v in s0[2].items() if k not in skip)
        return res

    buf = np.zeros((h, w, 4), np.float32).ctypes.data
    bads = C.byref(abi.svgf(min_history=1))
    names = ("gsp_download_temporal_image", "gsp_temporal_image_to_device", "gsp_temporal_svgf_feedback", "gsp_temporal_svgf_feedback_to_device")
    null, hist, track, full, done, fed = (dict((n, n + t) for n in names) for t in (
        ": null output pointer", " needs a gsp_temporal_accumulate call since the history was last invalidated",
        " needs gsp_temporal_track_moments(ctx, 1) before the history was accumulated",
        " needs a full frame (no pixel_ids) and a gsp_render_features call since gsp_frame_begin",
        " needs a gsp_temporal_accumulate call since gsp_frame_begin", ": the history has been fed back already (one call per gsp_temporal_accumulate)"))
    span = lambda n, k: "%s: levels must be within 1 .. %d (the filter's iterations)" % (n, k)
    n0, n1, n2, n3 = names
    with g.Context(0) as ctx:
        ctx.upload_scene(sc)
        # the order of the refusals, two broken conditions per call (temporal_util.refusals): without a frame and a history ...
        refusals(ctx, [(n0, (None,), null[n0]), (n0, (buf,), hist[n0]), (n1, (None, 0), null[n1]), (n1, (16, 0), hist[n1]),
                      (n2, (None, None, 0, None), hist[n2]), (n3, (None, None, 0, 16, 0), hist[n3])])
        # ... with a history without moments, in the next frame before its feature pass ...
        begin(ctx, size, 0)
        ctx.temporal_accumulate(None)
        ctx.frame_begin(*size)
        refusals(ctx, [(n0, (None,), null[n0]), (n0, (buf,), done[n0]), (n1, (None, 4), null[n1]), (n1, (16, 4), done[n1]), (n2, (None, None, 0, buf), track[n2]),
                      (n3, (None, None, 0, 16, 4), "destination too small"), (n3, (None, None, 0, 16, 1 << 30), track[n3])])
    with g.Context(0) as on, g.Context(0) as off:
        for ctx in (on, off):
            ctx.upload_scene(sc)
            ctx.temporal_track_moments(True)
        # the same sequence with the feature off and on costs the same bytes: H holds illumination in its own 16 bytes, the image
        # read-out uses the filter's output plane
        on.temporal_demodulate(True)
        for k in range(2):
            for ctx in (on, off):
                begin(ctx, size, k)
                ctx.temporal_accumulate(None)
            untouched(off, lambda: off.download_temporal_svgf())
            untouched(on, lambda: on.temporal_svgf_feedback(None, None, 1))
            untouched(off, off.download_temporal_image)
            untouched(on, on.download_temporal_image)
            assert on.stats()["device_bytes"] == off.stats()["device_bytes"], k
        # ... and an image read-out in front of any filter makes that one plane (the scratch the header names) and nothing else
        with g.Context(0) as fresh:
            fresh.upload_scene(sc)
            fresh.temporal_demodulate(True)
            begin(fresh, size, 0)
            fresh.temporal_accumulate(None)
            b0 = fresh.stats()["device_bytes"]
            fresh.download_temporal()
            assert fresh.stats()["device_bytes"] == b0
            fresh.download_temporal_image()
            assert fresh.stats()["device_bytes"] == b0 + 16 * w * h
            fresh.download_temporal_image()
            assert fresh.stats()["device_bytes"] == b0 + 16 * w * h
        ctx = on
        # the toggle drops the history; a call with the current value does not
        ctx.temporal_demodulate(True)
        assert np.all(ctx.download_temporal()[..., 3] == 2.0)
        ctx.temporal_demodulate(False)
        with pytest.raises(g.GspError, match="gsp_temporal_accumulate"):
            ctx.download_temporal()
        with pytest.raises(g.GspError, match="gsp_temporal_accumulate"):
            ctx.download_temporal_image()
        begin(ctx, size, 2)
        ctx.temporal_accumulate(None)
        assert np.all(ctx.download_temporal()[..., 3] == 1.0)
        ctx.temporal_demodulate(False)
        assert np.all(ctx.download_temporal()[..., 3] == 1.0)
        ctx.temporal_demodulate(True)
        with pytest.raises(g.GspError, match="gsp_temporal_accumulate"):
            ctx.download_temporal()
        begin(ctx, size, 3)
        ctx.temporal_accumulate(None)
        # an image read-out and a feedback before the frame's accumulate: the albedo plane would belong to another frame
        begin(ctx, size, 4)
        assert np.all(ctx.download_temporal()[..., 3] == 1.0)  # (the history itself is there)
        with pytest.raises(g.GspError, match="gsp_download_temporal_image needs a gsp_temporal_accumulate call since gsp_frame_begin"):
            ctx.download_temporal_image()
        assert ctx._L.gsp_temporal_image_to_device(ctx._h, 16, 1 << 30) == 1 and "since gsp_frame_begin" in ctx._L.gsp_last_error(ctx._h).decode()
        with pytest.raises(g.GspError, match="gsp_temporal_svgf_feedback needs a gsp_temporal_accumulate call since gsp_frame_begin"):
            ctx.temporal_svgf_feedback(None, None, 1)
        # ... with moments, in a frame before its accumulate: the filter's parameters, then the levels, then the accumulate ...
        refusals(ctx, [(n2, (None, bads, 0, buf), "gsp_svgf.min_history"), (n2, (None, None, 0, buf), span(n2, 5)), (n2, (None, None, 1, buf), done[n2]),
                       (n3, (None, bads, 0, 16, 1 << 30), "gsp_svgf.min_history"), (n3, (None, None, 6, 16, 1 << 30), span(n3, 5)),
                       (n3, (None, None, 0, 16, 4), "destination too small")])
        ctx.frame_begin(*size)  # ... and before its feature pass
        refusals(ctx, [(n2, (None, bads, 0, buf), full[n2]), (n3, (None, bads, 0, 16, 1 << 30), full[n3])])
        begin(ctx, size, 4)
        ctx.temporal_accumulate(None)
        # levels outside 1 .. iterations (those the call resolves: 5 by default)
        for dn, levels in ((None, 0), (None, 6), (abi.denoise(iterations=2), 3)):
            with pytest.raises(g.GspError, match="levels must be within 1 .. %d" % (2 if dn is not None else 5)):
                ctx.temporal_svgf_feedback(dn, None, levels)
        with pytest.raises(g.GspError, match="gsp_svgf.min_history"):
            ctx.temporal_svgf_feedback(None, abi.svgf(min_history=1), 1)
        # a NULL host pointer for the image, destinations that are too small
        need = 16 * w * h
        assert ctx._L.gsp_download_temporal_image(ctx._h, None) == 1 and "null output" in ctx._L.gsp_last_error(ctx._h).decode()
        assert ctx._L.gsp_temporal_image_to_device(ctx._h, None, need) == 1 and "null output" in ctx._L.gsp_last_error(ctx._h).decode()
        assert ctx._L.gsp_temporal_image_to_device(ctx._h, 16, need - 4) == 1 and "destination too small" in ctx._L.gsp_last_error(ctx._h).decode()
        assert ctx._L.gsp_temporal_svgf_feedback_to_device(ctx._h, None, None, 1, 16, need - 4) == 1
        assert "destination too small" in ctx._L.gsp_last_error(ctx._h).decode()
        assert np.all(ctx.download_temporal()[..., 3] == 2.0)
        untouched(ctx, lambda: ctx.temporal_svgf_feedback(None, None, 5))  # (none of the refused calls counted as the frame's feedback)
        refusals(ctx, [(n2, (None, None, 0, buf), span(n2, 5)), (n2, (None, None, 1, None), fed[n2]), (n3, (None, None, 6, 16, 1 << 30), span(n3, 5)),
                       (n3, (None, None, 1, 16, 4), "destination too small")])  # ... and after the frame's feedback
        # feedback with tracking off
        ctx.temporal_track_moments(False)
        begin(ctx, size, 5)
        ctx.temporal_accumulate(None)
        with pytest.raises(g.GspError, match="gsp_temporal_track_moments"):
            ctx.temporal_svgf_feedback(None, None, 1)
        untouched(ctx, ctx.download_temporal_image)


# ---- quality ------------------------------------------------------------------------------------------------------------------------------
def checker_scene():
    """test_gpu_motion's approach_scene with a checkerboard in place of the quad: a plane facing the camera at (0, 0, 5) under a large
    distant light, textured with 64 x 64 texels of 8 x 8 squares, repeated twice each way (a uscale-style repeat through the uv)."""
    from gpuspectral_amd import scenes

    b = scenes.SceneBuilder()
    rect = b.add_mesh(*scenes.rect_mesh())
    b.add_object(rect, scenes.trs((0.0, 0.0, 0.0), 2.5), b.diffuse((1.0, 1.0, 1.0)))
    b.add_object(rect, scenes.trs((0.0, 0.0, 400.0), 120.0, 180.0), b.diffuse((0, 0, 0)), twofaced=True, emission=(6, 6, 6))
    b.camera_lookat((0.0, 0.0, 5.0), (0.0, 0.0, 0.0), fov_deg=40.0)
    sc = b.build()
    sc.uvs = ((sc.positions[:, :2] + 1.0) * 0.5 * 2.0).astype(np.float32)
    y, x = np.mgrid[0:64, 0:64]
    v = np.where(((x // 8) + (y // 8)) % 2 == 0, 230, 40).astype(np.uint8)
    sc.bsdfs[0]["has_texture"][0] = sc.add_texture(np.stack([v, v, v, np.full_like(v, 255)], -1))
    return sc


def test_demodulation_keeps_texture_edges_under_sub_pixel_motion():
    """A checkerboard plane at 64 x 64, eight 1-spp frames, the camera translating parallel to the plane by about 0.37 pixel per frame,
    every default but alpha = FLT_MIN (both runs are plain running means).  Illumination is constant across the plane, so its bilinear
    blend loses nothing, while the blend of colour low-passes every texel edge once per frame: the MSE of the image read-out over the
    plane's pixels against a 1024-spp frame of the final camera is lower with demodulation on."""
    import gpuspectral_amd as g
    from gpuspectral_amd import abi

    sc = checker_scene()
    W = H = 64
    FRAMES = 8
    pixel = 5.0 / tu.zplane64(W, H, sc.fov)  # world units per pixel on the plane
    cams = []
    for k in range(FRAMES):
        cam = np.asarray(sc.to_world, np.float32).copy()
        cam[12] += np.float32(0.37 * pixel * k)
        cams.append(cam)
    img = {}
    with g.Context(0) as ctx:
        ctx.upload_scene(sc)
        for demod in (False, True):
            ctx.temporal_demodulate(demod)
            ctx.temporal_reset()
            for k in range(FRAMES):
                begin(ctx, (W, H), k, cams[k], sc.fov)
                ctx.temporal_accumulate(abi.temporal(alpha=FLT_MIN))
            img[demod] = ctx.download_temporal_image()
            plane = ctx.download_features()[2][..., 2] == 0
        ctx.frame_begin(W, H)
        ctx.render(1024, 0)
        ref = ctx.download()
    assert plane.sum() > 0.9 * W * H and img[True][..., 3][plane].mean() > 6.0
    mse = {d: float(((img[d][..., :3][plane].astype(np.float64) - ref[..., :3][plane]) ** 2).mean()) for d in (False, True)}
    write_quality("test_demodulation_keeps_texture_edges_under_sub_pixel_motion",
                  "test_demodulation_keeps_texture_edges_under_sub_pixel_motion -- a checkerboard plane (64 x 64 texels, 8 x 8 squares, repeated twice),\n"
                        "64 x 64, eight 1-spp frames, the camera moving 0.37 pixel per frame parallel to it, alpha = FLT_MIN; MSE of\n"
                        "gsp_download_temporal_image over the plane's %d pixels against a 1024-spp frame of the final camera.\n\n"
                  "demodulation off  %.6f\ndemodulation on   %.6f\nordering (on < off): %s\n" % (plane.sum(), mse[False], mse[True], mse[True] < mse[False]))
    print("MSE over the plane: demodulation off %.6f, on %.6f" % (mse[False], mse[True]))
    assert mse[True] < mse[False]


def test_feedback_lowers_the_error_of_the_history(scenes_):
    """Cornell box 64 x 64, unmoved camera, sixteen 1-spp frames, every default: the MSE of gsp_download_temporal_image against the
    committed 4096-spp image is lower with a feedback of one level on every frame than without.  The MSE of the final filtered output
    with and without is written beside it and not asserted: more smoothing against less noise can go either way there."""
    import gpuspectral_amd as g

    sc = scenes_["cornell"]
    W = H = 64
    FRAMES = 16
    ref = np.load(os.path.join(GOLDEN, "cornell_64_4096spp.npy")).astype(np.float64).reshape(H, W, 3)
    mse = lambda x: float(((np.asarray(x, np.float64)[..., :3] - ref) ** 2).mean())
    res = {}
    with g.Context(0) as ctx:
        ctx.upload_scene(sc)
        ctx.temporal_track_moments(True)
        for fb in (False, True):
            ctx.temporal_reset()
            for k in range(FRAMES):
                begin(ctx, (W, H), 5000 + k)  # (timestamps the reference did not use)
                ctx.temporal_accumulate(None)
                out = ctx.temporal_svgf_feedback(None, None, 1) if fb else ctx.download_temporal_svgf()
            res[fb] = (mse(ctx.download_temporal_image()), mse(out))
    write_quality("test_feedback_lowers_the_error_of_the_history",
                  "test_feedback_lowers_the_error_of_the_history -- Cornell box 64 x 64, unmoved camera, sixteen 1-spp frames, every default;\n"
                           "MSE against tests/golden/cornell_64_4096spp.npy of gsp_download_temporal_image and of the filter's final output.\n\n"
                           "no feedback           image %.6f   filtered %.6f\nfeedback of 1 level   image %.6f   filtered %.6f\n"
                  "ordering (image, feedback < none): %s\n" % (res[False] + res[True] + (res[True][0] < res[False][0],)))
    print("MSE image / filtered: no feedback %.6f / %.6f, feedback %.6f / %.6f" % (res[False] + res[True]))
    assert res[True][0] < res[False][0]


def write_quality(name, text):
    """profiles/illum_quality.txt holds one section per quality test, each headed by the test's id: a test replaces its own section
    and keeps the other's, so either may run alone."""
    path = os.path.join(ROOT, "profiles", "illum_quality.txt")
    head = "tests/test_gpu_illum.py::"
    order = ("test_demodulation_keeps_texture_edges_under_sub_pixel_motion", "test_feedback_lowers_the_error_of_the_history")
    sections = {}
    if os.path.exists(path):
        with open(path) as fh:
            for part in fh.read().split(head)[1:]:
                sections[part.split(" ", 1)[0]] = part.rstrip("\n") + "\n"
    sections[name] = text.rstrip("\n") + "\n"
    with open(path, "w") as fh:
        fh.write("\n".join(head + sections[k] for k in order if k in sections))


# ---- device memory, host layer, CLI -------------------------------------------------------------------------------------------------------
_TORCH_CHILD = """
import sys
import torch  # first: the tracer's library then binds to the HIP runtime torch has loaded (see bench.py)
import numpy as np
sys.path.insert(0, sys.argv[1])
import gpuspectral_amd as g
from gpuspectral_amd import scenes
W, H = 96, 64
N = W * H * 4
sc = scenes.cornell_materials(8)
with g.Context(0) as ctx:
    ctx.upload_scene(sc)
    ctx.temporal_demodulate(True)
    ctx.temporal_track_moments(True)
    for ts in range(4):
        ctx.frame_begin(W, H)
        ctx.frame_sample_base(ts)
        ctx.render(1, ts)
        ctx.render_features(1, ts)
        ctx.temporal_accumulate(None)
        if ts < 2:
            continue
        off = ts - 2  # floats: the second destination is not 16-byte aligned
        want = ctx.download_temporal_image().reshape(-1)
        assert not np.array_equal(want.view(np.uint32), ctx.download_temporal().reshape(-1).view(np.uint32))
        t = torch.zeros(N + 8, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        ctx.temporal_image_to_device(t[off:off + N])
        back = t.cpu().numpy()
        assert np.array_equal(back[off:off + N].view(np.uint32), want.view(np.uint32)) and not back[:off].any() and not back[off + N:].any()
        want = ctx.download_temporal_svgf().reshape(-1)
        t = torch.zeros(N + 8, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        try:
            ctx.temporal_svgf_feedback_to_device(t.data_ptr(), N * 4 - 4)
            raise SystemExit("a destination of the wrong size was accepted")
        except g.GspError as e:
            assert "destination too small" in str(e), e
        ctx.temporal_svgf_feedback_to_device(t[off:off + N], levels=1)
        back = t.cpu().numpy()
        assert np.array_equal(back[off:off + N].view(np.uint32), want.view(np.uint32)) and not back[:off].any() and not back[off + N:].any()
        fed = ctx.download_temporal().reshape(-1)
    ctx.frame_begin(W, H)
    ctx.render(1, 9)
    ctx.render_features(1, 9)
    ctx.temporal_accumulate(None)
    ctx.temporal_svgf_feedback_to_device(None, levels=2)  # no output
    assert not np.array_equal(ctx.download_temporal().reshape(-1), fed)
    t = torch.zeros(N, dtype=torch.float32, device="cuda:0")
    try:
        ctx.temporal_image_to_device(t.data_ptr(), N * 4 - 4)
        raise SystemExit("a destination of the wrong size was accepted")
    except g.GspError as e:
        assert "destination too small" in str(e), e
    assert not t.cpu().numpy().any()
print("torch tensor ok")
"""


def test_to_device_torch_tensor():
    """Into a torch tensor, in a process of its own: torch has to be imported before the library is loaded (bench.py does the same)."""
    r = subprocess.run([sys.executable, "-c", _TORCH_CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "torch tensor ok" in r.stdout, r.stdout + r.stderr


def test_host_layer():
    """The C++ host layer: PathTracer::temporalDemodulate / downloadTemporalImage / temporalSvgfFeedback."""
    from conftest import CORNELL_XML
    from gpuspectral_amd import host

    W, H = 48, 40
    sc = host.Scene(CORNELL_XML)
    pt = host.PathTracer(W, H)
    try:
        pt.temporal_demodulate(True)
        pt.temporal_track_moments(True)
        for k in range(3):
            if k:
                pt.next_frame()
            pt.render(sc, 1)
            pt.render_features(sc, 1)
            pt.temporal_accumulate(None)
            hist, img = pt.download_temporal(), pt.download_temporal_image()
            assert np.all(hist[..., 3] == float(k + 1)) and same(img[..., 3], hist[..., 3]) and not same(img, hist)
            plain = pt.download_temporal_svgf()
            out = pt.temporal_svgf_feedback(None, None, 1)
            assert same(out, plain) and not same(pt.download_temporal(), hist) and np.isfinite(pt.download_temporal_image()).all()
            with pytest.raises(Exception, match="fed back already"):
                pt.temporal_svgf_feedback(None, None, 1, out=False)
        pt.temporal_demodulate(False)
        pt.next_frame()
        pt.render(sc, 1)
        pt.render_features(sc, 1)
        with pytest.raises(Exception, match="gsp_temporal_accumulate"):
            pt.download_temporal_image()
        pt.temporal_accumulate(None)
        assert np.all(pt.download_temporal()[..., 3] == 1.0) and same(pt.download_temporal_image(), pt.download_temporal())  # the switch dropped the history
        assert pt.temporal_svgf_feedback(None, None, 2, out=False) is None
    finally:
        pt.close()


def test_cli(tmp_path):
    """--temporal-demodulate --svgf-feedback 1 on the Cornell XML at 64 x 48 for four frames: finite files and the log lines."""
    from oracle import mitsuba_loader as ml
    from conftest import CORNELL_XML

    lib = os.path.join(ROOT, "gpuspectral_amd", "lib")
    env = dict(os.environ, LD_LIBRARY_PATH=lib + ":" + os.environ.get("LD_LIBRARY_PATH", ""))

    def run(args, code=0):
        r = subprocess.run([os.path.join(lib, "gsp_render")] + args, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == code, r.stdout + r.stderr
        return r.stdout + r.stderr

    W, H = 64, 48
    t = tmp_path
    pfm = lambda path: np.asarray(ml.read_pfm(str(path)), np.float32).reshape(H, W, -1)[::-1, :, :3]
    tail = [CORNELL_XML, str(t / "frame.pfm"), str(W), str(H), "1"]
    out = run(["--temporal", str(t / "t.pfm"), "--temporal-frames", "4", "--temporal-demodulate", "--svgf", str(t / "s.pfm"), "--svgf-feedback", "1"] + tail)
    assert "temporal: 4 frames" in out and "the history holds illumination" in out and "svgf feedback: the first 1 level fed back" in out and "svgf: 5 levels" in out
    hist, filt, frame_ = pfm(t / "t.pfm"), pfm(t / "s.pfm"), pfm(t / "frame.pfm")
    assert hist.shape == filt.shape == (H, W, 3) and np.isfinite(hist).all() and np.isfinite(filt).all() and hist.max() > 0.1 and filt.max() > 0.1
    assert frame_.shape == (H, W, 3) and not np.array_equal(hist, frame_) and not np.array_equal(hist, filt)
    out = run(["--temporal", str(t / "x.pfm"), "--temporal-frames", "2", "--svgf-feedback", "1"] + tail, code=1)
    assert "--svgf-feedback needs --svgf" in out
    out = run(["--temporal", str(t / "y.pfm"), "--temporal-frames", "2", "--svgf", str(t / "ys.pfm"), "--denoise", str(t / "yd.pfm"), "--denoise-iterations", "2",
               "--svgf-feedback", "3"] + tail, code=1)
    assert "levels must be within 1 .. 2" in out
