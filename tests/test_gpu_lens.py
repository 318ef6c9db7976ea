"""Thin lens (include/gpuspectral_pt.h, "Thin lens") on the GPU.

The wavefront pipeline against the same stage headers run in scalar on the host (tests/emu/lens_emu.cpp), bit for bit, for a
circular and two polygonal apertures, alone and behind a pixel filter; an emitter-only scene whose expected image is composed
from the emu's rays, the ORACLE's traversal and a numpy running mean; the primary-hit memo across lens / pinhole calls; the
invariances every feature of the tracer keeps; the lens as context state; the autofocus; the CLI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import CORNELL_XML, ROOT
from lens_util import CIRCLE, HEXAGON_ROT, LENSES, PENTAGON, LensEmu, same
from test_gpu_pixel_filter import emitter_scene

pytestmark = pytest.mark.gpu

NONE, BOX, TENT = 0, 1, 2
COUNTS = ("extension_rays", "shadow_rays", "shaded_vertices")


@pytest.fixture(scope="module")
def lemu():
    return LensEmu()


@pytest.fixture()
def ctx():
    import gpuspectral_amd as g

    c = g.Context(0)
    yield c
    c.close()


@pytest.fixture()
def wctx():
    """finish_paths = never: the wavefront extend launch, which alone consults the primary-hit memo, traces every path (see the
    fixture of the same name in test_gpu_pixel_filter.py)."""
    import gpuspectral_amd as g

    c = g.Context(0, finish_paths=0xFFFFFFFF)
    yield c
    c.close()


def frame(ctx, sc, W, H, calls, upload=True, pixel_ids=None, **kw):
    if upload:
        ctx.upload_scene(sc)
    ctx.frame_begin(W, H, pixel_ids=pixel_ids)
    ctx.reset_stats()
    t = 0
    for spp in calls:
        ctx.render(spp=spp, first_timestamp=t, **kw)
        t += spp
    return ctx.download_compact().copy(), ctx.stats()


# ---- GPU == emu, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,W,spp", [("cornell", 64, 8), ("materials", 48, 4)])
@pytest.mark.parametrize("lens", list(LENSES), ids=lambda s: s.replace(" ", "_"))
@pytest.mark.parametrize("filt", [NONE, TENT])
@pytest.mark.parametrize("ts0", [0, 5])
def test_gpu_equals_emu(ctx, lemu, cornell, which, W, spp, lens, filt, ts0):
    from gpuspectral_amd import scenes

    sc = cornell if which == "cornell" else scenes.cornell_materials(16)
    ref, rst = lemu.scene(sc).render(W, W, spp, lens=LENSES[lens], first_timestamp=ts0, pixel_filter=filt)
    ctx.upload_scene(sc)
    ctx.set_lens(**LENSES[lens])
    ctx.frame_begin(W, W)
    ctx.reset_stats()
    ctx.render(spp=spp, first_timestamp=ts0, pixel_filter=filt)
    img = ctx.download_compact()
    st = ctx.stats()
    bad = np.nonzero(np.any(img.view(np.uint32) != ref.view(np.uint32), axis=1))[0]
    assert len(bad) == 0, "%d of %d pixels differ from the emu (first: %d)" % (len(bad), W * W, bad[0])
    for k in COUNTS:
        assert st[k] == rst[k], k
    assert st["samples"] == W * W * spp and st["memoised_rays"] == 0


def test_lens_image_differs_from_pinhole(ctx, cornell, oracle_mod):
    """(the comparisons above are not vacuous) ... and radius 0 with every other field set is the oracle's image."""
    W = H = 64
    pin = oracle_mod.Oracle(cornell).render(W, H, spp=4)[0]
    ctx.set_lens(**CIRCLE)
    img, _ = frame(ctx, cornell, W, H, [4])
    assert (np.abs(img - pin).max(1) > 0).mean() > 0.5
    ctx.set_lens(radius=0.0, focus_distance=3.0, blades=6, rotation=0.7)
    img, _ = frame(ctx, cornell, W, H, [4], upload=False)
    assert same(img, pin)
    ctx.set_lens(**CIRCLE)
    ctx._check(ctx._L.gsp_set_lens(ctx._h, None), "gsp_set_lens")  # NULL = pinhole
    img, _ = frame(ctx, cornell, W, H, [4], upload=False)
    assert same(img, pin)


# ---- exact composition with the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [dict(radius=0.15, focus_distance=5.0), dict(radius=0.15, focus_distance=4.0, blades=6, rotation=0.4)],
                         ids=["circle", "hexagon"])
def test_emitter_scene_composes_with_the_oracle(ctx, lemu, oracle_mod, lens):
    """Expected image: the emu's lens rays -> Oracle.trace -> the hit primitive's emission (front-facing by construction) -> the
    float32 running mean restated in numpy.  The GPU frame at 16 spp equals it bit for bit."""
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
        o, d, _, _ = lemu.generate(sc, W, H, lens, gids, np.full(W * H, ts, np.uint32))
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
    ctx.set_lens(**lens)
    img, st = frame(ctx, sc, W, H, [SPP])
    bad = np.nonzero(np.any(img.view(np.uint32) != acc.view(np.uint32), axis=1))[0]
    assert len(bad) == 0, "%d pixels differ (first: %d: %s vs %s)" % (len(bad), bad[0], img[bad[0]], acc[bad[0]])
    assert len(np.unique(img[:, 0])) > 100  # (a defocused frame of edges: many partial coverages)


# ---- the primary-hit memo -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [CIRCLE, HEXAGON_ROT], ids=["circle", "hexagon"])
def test_lens_call_does_not_use_the_memo(wctx, oracle_mod, cornell, lens):
    ctx = wctx
    W = H = 64
    ctx.upload_scene(cornell)
    ctx.frame_begin(W, H)
    ctx.render(spp=2)  # pinhole: builds the memo
    ctx.sync()
    s0 = ctx.stats()
    assert s0["memo_build_rays"] > 0 and s0["memoised_rays"] > 0
    ctx.set_lens(**lens)
    ctx.render(spp=4, first_timestamp=2)
    ctx.sync()
    s1 = ctx.stats()
    assert s1["memoised_rays"] == s0["memoised_rays"] and s1["memo_build_rays"] == s0["memo_build_rays"]
    assert s1["extension_rays"] - s0["extension_rays"] >= W * H * 4  # every camera ray was traced
    # a following pinhole call on the same frame REUSES the memo (no rebuild) ...
    ctx.set_lens()
    ctx.render(spp=2, first_timestamp=6)
    ctx.sync()
    s2 = ctx.stats()
    assert s2["memoised_rays"] > s1["memoised_rays"] and s2["memo_build_rays"] == s0["memo_build_rays"]
    # ... and a pinhole frame after lens frames still equals the oracle
    ctx.set_lens(**lens)
    frame(ctx, cornell, W, H, [3], upload=False)
    ctx.set_lens()
    img, st = frame(ctx, cornell, W, H, [5], upload=False)
    assert same(img, oracle_mod.Oracle(cornell).render(W, H, spp=5)[0]) and st["memoised_rays"] > 0
    # a fresh frame through the lens from its first call: no memo at all
    ctx.set_lens(**lens)
    ctx.upload_scene(cornell)
    ctx.frame_begin(W, H)
    ctx.reset_stats()
    ctx.render(spp=4)
    ctx.sync()
    s3 = ctx.stats()
    assert s3["memoised_rays"] == 0 and s3["memo_build_rays"] == 0


# ---- invariances ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens,filt", [(CIRCLE, NONE), (PENTAGON, BOX)], ids=["circle", "pentagon_box"])
def test_progressive_and_pipeline_options(ctx, lemu, cornell, lens, filt):
    import gpuspectral_amd as g

    W = H = 64
    ctx.set_lens(**lens)
    one, _ = frame(ctx, cornell, W, H, [8], pixel_filter=filt)
    assert same(one, lemu.scene(cornell).render(W, H, 8, lens=lens, pixel_filter=filt)[0])
    two, _ = frame(ctx, cornell, W, H, [4, 4], upload=False, pixel_filter=filt)
    assert same(one, two)  # 2 calls x 4 spp == 1 call x 8 spp
    tif, _ = frame(ctx, cornell, W, H, [8], upload=False, timestamps_in_flight=1, pixel_filter=filt)
    assert same(one, tif)
    for opts in (dict(lanes=1), dict(lanes=2), dict(finish_paths=0xFFFFFFFF), dict(lanes=2, finish_paths=0xFFFFFFFF)):
        with g.Context(0, **opts) as c:
            c.set_lens(**lens)
            img, _ = frame(c, cornell, W, H, [3, 5], pixel_filter=filt)
            assert same(one, img), opts


def test_adaptive_with_lens(ctx, lemu, cornell):
    """A pixel that stopped after N samples equals the uniform LENS frame at N spp for that pixel (k_generate_active_lens)."""
    W = H = 64
    es = lemu.scene(cornell)
    ctx.upload_scene(cornell)
    ctx.set_lens(**HEXAGON_ROT)
    for thr in (0.02, 0.03, 0.05, 0.07, 0.1, 0.15, 0.2, 0.3, 0.5):
        ctx.frame_begin(W, H)
        ctx.render(spp=48, adaptive_threshold=thr, adaptive_min_spp=8, adaptive_step=8)
        img = ctx.download_compact()
        _, spp = ctx.pixel_stats()
        if len(np.unique(spp)) >= 3:
            break
    assert len(np.unique(spp)) >= 3, "no threshold stops pixels at three different counts"
    ids = np.arange(W * H, dtype=np.uint32)
    for n in np.unique(spp):
        sel = np.nonzero(spp == n)[0]
        ref, _ = es.render(W, H, int(n), lens=HEXAGON_ROT, pixel_ids=ids[sel])
        assert same(img[sel], ref), "N_p = %d" % n


def test_pixel_ids_share_equals_the_frame(ctx, cornell):
    W, H = 96, 80
    ctx.set_lens(**PENTAGON)
    whole, _ = frame(ctx, cornell, W, H, [2, 3])
    ids = np.arange(W * H, dtype=np.uint32)[1::3]
    part, _ = frame(ctx, cornell, W, H, [5], upload=False, pixel_ids=ids)
    assert same(part, whole[ids])


@pytest.mark.parametrize("world", [2, 3])
def test_multi_render_equals_single_context(ctx, cornell, world):
    from gpuspectral_amd import pt

    W, H = 96, 80
    ctx.set_lens(**HEXAGON_ROT)
    single, _ = frame(ctx, cornell, W, H, [2, 3], pixel_filter=TENT)
    with pt.MultiContext([0] * world) as m:  # a repeated device: the copy route, as in the existing multi tests
        m.upload_scene(cornell)
        m.set_lens(**HEXAGON_ROT)
        m.frame_begin(W, H)
        m.render(spp=2, pixel_filter=TENT)
        m.render(spp=3, first_timestamp=2, pixel_filter=TENT)
        m.gather()
        img = m.download()
        m.set_lens()  # ... and back to the pinhole on every share
        m.frame_begin(W, H)
        m.render(spp=2)
        m.gather()
        pin = m.download()
    assert same(img.reshape(-1, 4), single)
    ctx.set_lens()
    assert same(pin.reshape(-1, 4), frame(ctx, cornell, W, H, [2], upload=False)[0])


# ---- context state --------------------------------------------------------------------------------------------------------
def test_lens_change_between_calls_of_one_frame(ctx, lemu, cornell):
    """No sync between the calls: the lens that holds when gsp_render is called is the lens of that call's samples."""
    W = H = 64
    es = lemu.scene(cornell)
    ref, _ = es.render(W, H, 3, lens=CIRCLE)
    ref, _ = es.render(W, H, 2, lens=None, first_timestamp=3, accum=ref)
    ref, _ = es.render(W, H, 3, lens=HEXAGON_ROT, first_timestamp=5, accum=ref)
    ctx.upload_scene(cornell)
    ctx.frame_begin(W, H)
    ctx.set_lens(**CIRCLE)
    ctx.render(spp=3)
    ctx.set_lens()
    ctx.render(spp=2, first_timestamp=3)
    ctx.set_lens(**HEXAGON_ROT)
    ctx.render(spp=3, first_timestamp=5)
    assert same(ctx.download_compact(), ref)


def test_lens_survives_camera_frame_and_scene(ctx, lemu, cornell, materials_scene):
    import copy

    W, H = 64, 48
    ctx.set_lens(**PENTAGON)  # before any scene: context state
    ctx.upload_scene(cornell)
    ctx.frame_begin(W, H)
    ctx.render(spp=2)
    sc = copy.copy(cornell)
    tw = np.asarray(sc.to_world, np.float32).copy()
    tw[12] += 0.2
    sc.to_world = tw
    ctx.update_camera(sc.to_world, sc.fov)  # keeps the lens
    ctx.frame_begin(W, H)
    ctx.render(spp=4)
    assert same(ctx.download_compact(), lemu.scene(sc).render(W, H, 4, lens=PENTAGON)[0])
    img, _ = frame(ctx, materials_scene, W, H, [3])  # ... and so does another scene
    assert same(img, lemu.scene(materials_scene).render(W, H, 3, lens=PENTAGON)[0])


def test_invalid_lens_is_refused_and_leaves_the_state(ctx, lemu, cornell):
    import gpuspectral_amd as g

    W = H = 32
    ctx.upload_scene(cornell)
    ctx.set_lens(**CIRCLE)
    for bad, word in ((dict(radius=-1.0, focus_distance=1.0), "radius"), (dict(radius=float("nan")), "radius"),
                      (dict(radius=0.1, focus_distance=0.0), "focus_distance"), (dict(radius=0.1, focus_distance=float("inf")), "focus_distance"),
                      (dict(radius=0.1, focus_distance=1.0, blades=2), "blades"), (dict(radius=0.1, focus_distance=1.0, blades=17), "blades"),
                      (dict(radius=0.1, focus_distance=1.0, rotation=float("nan")), "rotation")):
        with pytest.raises(g.GspError, match=word) as e:
            ctx.set_lens(**bad)
        assert "(1)" in str(e.value)  # GSP_ERR_INVALID
    img, _ = frame(ctx, cornell, W, H, [2], upload=False)  # the lens set before the refused calls still holds
    assert same(img, lemu.scene(cornell).render(W, H, 2, lens=CIRCLE)[0])


# ---- autofocus ------------------------------------------------------------------------------------------------------------
def test_focus_distance(ctx, lemu, oracle_mod, cornell):
    """gsp_focus_distance == Oracle.trace's t times the emu's float32 cosine for hit pixels, 0 for misses; no frame needed; an
    active lens and filter change nothing."""
    W, H = 96, 64
    sc = emitter_scene()  # (has background: some pixels miss)
    rng = np.random.RandomState(3)
    frag = np.concatenate([np.stack([rng.randint(0, W, 40), rng.randint(0, H, 40)], 1).astype(np.float32),
                           rng.uniform(0, [W, H], (40, 2)).astype(np.float32)])
    for scene in (sc, cornell):
        d, cosz = lemu.pinhole(scene, W, H, frag)
        rays = np.zeros((len(frag), 8), np.float32)
        rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = np.asarray(scene.to_world, np.float32)[12:15], 0.0, d, 1e10
        hits = oracle_mod.Oracle(scene).trace(rays)
        expect = np.where(hits["prim"] >= 0, hits["t"].astype(np.float32) * cosz, np.float32(0.0)).astype(np.float32)
        ctx.upload_scene(scene)
        ctx.set_lens()
        got = np.array([ctx.focus_distance(W, H, float(x), float(y)) for x, y in frag], np.float32)
        assert same(got, expect)
        if scene is sc:
            assert (expect == 0).any() and (expect > 0).any()
        ctx.set_lens(**HEXAGON_ROT)
        ctx.frame_begin(32, 32)  # another frame size, a lens and a filtered render in between
        ctx.render(spp=1, pixel_filter=TENT)
        got2 = np.array([ctx.focus_distance(W, H, float(x), float(y)) for x, y in frag], np.float32)
        assert same(got2, expect)
    import gpuspectral_amd as g

    with pytest.raises(g.GspError, match="gsp_focus_distance"):
        ctx.focus_distance(0, H, 1.0, 1.0)
    with pytest.raises(g.GspError, match="gsp_focus_distance"):
        ctx.focus_distance(W, H, float("nan"), 1.0)
    with g.Context(0) as c, pytest.raises(g.GspError, match="gsp_upload_scene"):
        c.focus_distance(W, H, 1.0, 1.0)


def test_autofocus_puts_the_pixel_in_focus(ctx, cornell):
    """Focused on what a pixel shows, a frame through a wide aperture keeps that pixel's neighbourhood close to the pinhole
    image while the frame as a whole is visibly defocused (a smoke check of the feature's purpose; bounds are loose by design:
    both frames carry Monte-Carlo noise of 64 samples)."""
    W = H = 64
    fx, fy = 20.0, 40.0
    ctx.upload_scene(cornell)
    D = float(ctx.focus_distance(W, H, fx, fy))
    assert D > 0
    pin, _ = frame(ctx, cornell, W, H, [64], upload=False)
    ctx.set_lens(radius=0.3, focus_distance=D * 0.5)  # focused far in front of everything
    blur, _ = frame(ctx, cornell, W, H, [64], upload=False)
    ctx.set_lens(radius=0.3, focus_distance=D)
    foc, _ = frame(ctx, cornell, W, H, [64], upload=False)

    def edge_energy(img):
        im = img.reshape(H, W, 4)[:, :, :3].astype(np.float64)
        return float((np.diff(im, axis=0) ** 2).sum() + (np.diff(im, axis=1) ** 2).sum())

    print("edge energy: pinhole %.3f, focused %.3f, defocused %.3f" % (edge_energy(pin), edge_energy(foc), edge_energy(blur)))
    assert not same(foc, pin) and not same(blur, foc)


# ---- CLI ------------------------------------------------------------------------------------------------------------------
def _run_cli(args):
    lib = os.path.join(ROOT, "gpuspectral_amd", "lib")
    env = dict(os.environ, LD_LIBRARY_PATH=lib + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([os.path.join(lib, "gsp_render")] + args, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout


def _pfm_equals(path, img, W, H):
    from oracle import mitsuba_loader as ml

    got = np.asarray(ml.read_pfm(path), np.float32).reshape(H, W, -1)[:, :, :3]
    rgb = img.reshape(H, W, 4)[:, :, :3]
    return same(got, rgb) or same(got[::-1], rgb)  # (PFM rows run bottom to top)


def test_cli_lens_flags_equal_python(ctx, cornell, tmp_path):
    W, H, SPP = 64, 48, 4
    out = str(tmp_path / "a.pfm")
    _run_cli(["--aperture", "0.08", "--focus-distance", "5", "--blades", "6:22.5", CORNELL_XML, out, str(W), str(H), str(SPP)])
    ctx.set_lens(radius=0.08, focus_distance=5.0, blades=6, rotation=float(np.float32(22.5) * np.float32(3.14159265358979323846) / np.float32(180.0)))
    img, _ = frame(ctx, cornell, W, H, [SPP])
    assert _pfm_equals(out, img, W, H)
    # --focus-pixel: the autofocus value goes into the lens
    out2 = str(tmp_path / "b.pfm")
    text = _run_cli(["--aperture", "0.08", "--focus-pixel", "20,30", CORNELL_XML, out2, str(W), str(H), str(SPP)])
    D = float(ctx.focus_distance(W, H, 20.0, 30.0))
    assert D > 0 and "focus distance" in text
    ctx.set_lens(radius=0.08, focus_distance=D)
    img, _ = frame(ctx, cornell, W, H, [SPP], upload=False)
    assert _pfm_equals(out2, img, W, H)
    pin_path = str(tmp_path / "p.pfm")
    _run_cli([CORNELL_XML, pin_path, str(W), str(H), str(SPP)])
    ctx.set_lens()
    pin, _ = frame(ctx, cornell, W, H, [SPP], upload=False)
    assert _pfm_equals(pin_path, pin, W, H) and not same(pin, img)


def test_cli_scene_lens(ctx, cornell, tmp_path):
    from test_lens_abi import _scene_xml

    W, H, SPP = 64, 48, 4
    xml = _scene_xml(tmp_path, "thinlens", [("aperture_radius", "0.125"), ("focus_distance", "5.5")])
    out = str(tmp_path / "s.pfm")
    _run_cli(["--scene-lens", xml, out, str(W), str(H), str(SPP)])
    ctx.set_lens(radius=0.125, focus_distance=5.5)
    img, _ = frame(ctx, cornell, W, H, [SPP])
    assert _pfm_equals(out, img, W, H)
    out2 = str(tmp_path / "t.pfm")  # without the flag the sensor is a pinhole, as in the reference
    _run_cli([xml, out2, str(W), str(H), str(SPP)])
    ctx.set_lens()
    pin, _ = frame(ctx, cornell, W, H, [SPP], upload=False)
    assert _pfm_equals(out2, pin, W, H)
