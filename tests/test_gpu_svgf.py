"""The variance-guided filter on the GPU (include/gpuspectral_pt.h, "Variance-guided filter"): k_temporal_reproject_moments,
k_svgf_variance and k_svgf_atrous against the same text run on the host (csrc/pt_svgf.h through tests/emu/svgf_emu.cpp, itself
checked against a float64 restatement in tests/test_svgf_cpu.py).  The history, its moments and the filtered frame equal the
emulation applied to gsp_download + gsp_download_features + the previous emulated history BIT FOR BIT, frame after frame."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import temporal_util as tu
from conftest import ROOT
from display_util import DisplayEmu
from svgf_util import INF, SvgfEmu, same
from temporal_util import FLT_MIN, refusals

pytestmark = pytest.mark.gpu

TENT = 2
LENS = dict(radius=0.08, focus_distance=5.0, blades=0, rotation=0.0)
# four frames on an orbit of 2 degrees per frame, a jump of 40 degrees that disoccludes most of the frame, two more frames
ORBIT = [0.0, 2.0, 4.0, 6.0, 46.0, 48.0, 50.0]


@pytest.fixture(scope="module")
def emu():
    return SvgfEmu()


@pytest.fixture(scope="module")
def scenes_(cornell, materials_scene):
    return {"cornell": cornell, "materials": materials_scene}


@pytest.fixture(scope="module")
def rigs(scenes_):
    """Per scene: one context with the scene uploaded and the moments tracked, shared by the cases below."""
    import gpuspectral_amd as g

    made = {}

    def get(name):
        if name not in made:
            made[name] = g.Context(0)
            made[name].upload_scene(scenes_[name])
        ctx = made[name]
        ctx.set_lens()
        ctx.update_camera(scenes_[name].to_world, scenes_[name].fov)
        ctx.temporal_track_moments(True)
        ctx.temporal_reset()
        return ctx

    yield get
    for ctx in made.values():
        ctx.close()


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def frame(ctx, emu, hist, cam, fov, size, ts, temporal=None, spp=1, filt=0, accum=None, what=""):
    """One frame of the viewer loop under camera `cam`, accumulated on the GPU and by the emulation from `hist`: the new emulated
    MHistory after the bit-for-bit comparison of H and M, and the frame's albedo and geom planes."""
    ctx.update_camera(cam, fov)
    ctx.frame_begin(*size)
    ctx.frame_sample_base(ts * spp)
    ctx.render(spp, ts * spp, pixel_filter=filt)
    ctx.render_features(spp, ts * spp, pixel_filter=filt)
    if accum is not None:
        ctx.upload_accum(accum(ctx.download_compact().copy()))
    ctx.temporal_accumulate(temporal)
    c = ctx.download()
    a, g, i = ctx.download_features()
    new = emu.step(temporal, cam, fov, c, a, g, i, hist)
    for name, got, want in (("history", ctx.download_temporal(), new.H), ("moments", ctx.download_temporal_moments(), new.M)):
        bad = int((words(got) != words(want)).sum())
        assert bad == 0, "%s: %d of %d words of the %s differ" % (what, bad, got.size, name)
    return new, a, g


def filtered(ctx, emu, hist, a, g, denoise=None, svgf=None, what=""):
    got = ctx.download_temporal_svgf(denoise, svgf)
    want = emu.run(denoise, svgf, hist.H, hist.M, a, g)
    bad = int((words(got) != words(want)).sum())
    assert bad == 0, "%s: %d of %d words of the filtered history differ" % (what, bad, got.size)
    return got


def orbit(sc, degrees):
    return [tu.rotated_about_y(sc.to_world, d, pivot=(0.0, 1.0, 0.0)) for d in degrees]


def sequence(ctx, emu, sc, size, degrees=ORBIT, temporal=None, what="", check=lambda k: True, **kw):
    """Frames along an orbit; after every frame `check` names, the filter with every default against the emulation."""
    hist = a = g = None
    for k, cam in enumerate(orbit(sc, degrees)):
        hist, a, g = frame(ctx, emu, hist, cam, sc.fov, size, k, temporal, what="%s frame %d" % (what, k), **kw)
        if check(k):
            filtered(ctx, emu, hist, a, g, what="%s frame %d" % (what, k))
    return hist, a, g


def test_cornell_orbit(rigs, emu, scenes_):
    from gpuspectral_amd import abi

    ctx, sc = rigs("cornell"), scenes_["cornell"]
    hist, lens = None, []
    for k, cam in enumerate(orbit(sc, ORBIT)):
        hist, a, g = frame(ctx, emu, hist, cam, sc.fov, (96, 64), k, what="cornell frame %d" % k)
        lens.append(float(hist.H[..., 3].mean()))
        out = filtered(ctx, emu, hist, a, g, what="cornell frame %d" % k)
        assert same(out[..., 3], hist.H[..., 3])  # out.w = the history length
        if k == 4:  # pixels that kept five frames beside pixels in their first: the temporal and the spatial estimate side by side
            assert (hist.H[..., 3] >= 4.0).any() and (hist.M[..., 2] == 1.0).any()
        if k in (3, 4, 6):  # a long history, right after the jump (both estimates of the variance side by side), recovering
            for it in (1, 3, 8):
                filtered(ctx, emu, hist, a, g, abi.denoise(iterations=it), None, "cornell frame %d, %d iterations" % (k, it))
            for s in (abi.svgf(min_history=65536), abi.svgf(min_history=2), abi.svgf(sigma_variance=INF), abi.svgf(sigma_variance=0.5, min_history=3)):
                filtered(ctx, emu, hist, a, g, abi.denoise(iterations=3, sigma_normal=1.0), s, "cornell frame %d, min_history %d sigma %g" % (k, s.min_history, s.sigma_variance))
    print("mean history length per frame:", ["%.2f" % v for v in lens])
    assert lens[0] == 1.0 and lens[3] > 3.0 and lens[4] < lens[3] - 0.5 and lens[6] > lens[4]  # it builds up, the jump disoccludes, it recovers


@pytest.mark.parametrize("size", [(33, 17), (5, 3), (1, 1)])
def test_materials_scene(rigs, emu, scenes_, size):
    from gpuspectral_amd import abi

    ctx, sc = rigs("materials"), scenes_["materials"]
    hist, a, g = sequence(ctx, emu, sc, size, what="materials %dx%d" % size)
    for it in (1, 2, 8):  # steps beyond the frame
        filtered(ctx, emu, hist, a, g, abi.denoise(iterations=it), abi.svgf(min_history=2), "materials %dx%d, %d iterations" % (size + (it,)))


@pytest.mark.parametrize("scene", ["cornell", "materials"])
def test_ragged_tiles(rigs, emu, scenes_, scene):
    """300 x 200: ten tiles of 32 across (the last one 12 wide), 25 of 8 down; every fetch path of the filter (LDS with halo 2 and
    4, global) and the variance pass's halo of 3 at all four borders."""
    from gpuspectral_amd import abi

    sc, ctx = scenes_[scene], rigs(scene)
    hist, a, g = sequence(ctx, emu, sc, (300, 200), degrees=[0.0, 3.0, -4.0, 9.0], what="%s 300x200" % scene, check=lambda k: k == 3)
    filtered(ctx, emu, hist, a, g, abi.denoise(iterations=1), abi.svgf(min_history=2), "%s 300x200, 1 iteration" % scene)
    filtered(ctx, emu, hist, a, g, abi.denoise(iterations=2), abi.svgf(min_history=65536), "%s 300x200, 2 iterations, all spatial" % scene)
    assert hist.H[..., 3].max() > 3.0 and (hist.H[..., 3] == 1.0).any()


@pytest.mark.parametrize("scene,size,kw", [("cornell", (96, 64), dict(filt=TENT, spp=2)), ("materials", (33, 17), dict(filt=TENT, spp=2)),
                                           ("cornell", (96, 64), dict(lens=LENS, spp=2))], ids=["cornell-tent", "materials-tent", "cornell-lens"])
def test_filtered_and_defocused_inputs(rigs, emu, scenes_, scene, size, kw):
    ctx = rigs(scene)
    lens = kw.pop("lens", None)
    try:
        if lens:
            ctx.set_lens(**lens)
        sequence(ctx, emu, scenes_[scene], size, degrees=[0.0, 2.0, 4.0, 6.0, 30.0], what="%s %s" % (scene, sorted(kw)), check=lambda k: k >= 3, **kw)
    finally:
        ctx.set_lens()


def test_nan_and_inf_in_the_frames(rigs, emu, scenes_):
    W, H = 64, 32
    ctx, sc = rigs("cornell"), scenes_["cornell"]
    rng = np.random.default_rng(5)

    def spoil(a):
        for value in (np.nan, np.inf, -np.inf):
            a[rng.integers(0, W * H, 30), rng.integers(0, 3, 30)] = value
        return a

    hist = None
    for k, cam in enumerate(orbit(sc, [0.0, 2.0, 2.0, 4.0, 30.0])):
        hist, a, g = frame(ctx, emu, hist, cam, sc.fov, (W, H), k, accum=spoil if k != 2 else None, what="NaN / Inf frame %d" % k)
        out = filtered(ctx, emu, hist, a, g, what="NaN / Inf frame %d" % k)
        bad = ~np.isfinite(hist.H[..., :3]).all(-1)
        assert same(out[bad], hist.H[bad]) and np.isfinite(out[~bad]).all()
    assert bad.any() and np.isfinite(hist.M).all()


def test_history_is_the_untracked_history_and_toggling_drops_it(scenes_, emu):
    """The same frames on one context with the moments tracked and on one without: H is the same, bit for bit.  The moments cost
    32 bytes per pixel, the filter's variance planes 8; a change of the switch forgets the history, a repeated value does not."""
    import gpuspectral_amd as g

    sc = scenes_["cornell"]
    w, h = 96, 64
    with g.Context(0) as on, g.Context(0) as off:
        got = {}
        for name, ctx in (("on", on), ("off", off)):
            ctx.upload_scene(sc)
            if name == "on":
                ctx.temporal_track_moments(True)
            for k, cam in enumerate(orbit(sc, [0.0, 2.0, 4.0, 40.0])):
                ctx.update_camera(cam, sc.fov)
                ctx.frame_begin(w, h)
                ctx.frame_sample_base(k)
                ctx.render(1, k)
                ctx.render_features(1, k)
                if k == 0:
                    bytes0 = ctx.stats()["device_bytes"]
                ctx.temporal_accumulate(None)
                if k == 0:
                    assert ctx.stats()["device_bytes"] == bytes0 + (104 if name == "on" else 72) * w * h
                got[name, k] = ctx.download_temporal()
        assert all(same(got["on", k], got["off", k]) for k in range(4))
        ctx = on
        before = ctx.stats()["device_bytes"]
        ctx.download_temporal_denoised(None)
        dn = ctx.stats()["device_bytes"] - before  # (the denoiser's four planes: made by whichever filter runs first)
        assert dn == 64 * w * h
        state = lambda: (ctx.download(), ctx.download_features(), ctx.download_temporal(), ctx.download_temporal_moments())
        s0 = state()
        ctx.download_temporal_svgf(None, None)
        assert ctx.stats()["device_bytes"] == before + dn + 8 * w * h
        s1 = state()
        assert same(s0[0], s1[0]) and all(np.array_equal(words(p), words(q)) for p, q in zip(s0[1], s1[1])) and same(s0[2], s1[2]) and same(s0[3], s1[3])
        ctx.temporal_track_moments(True)  # the current value: nothing happens
        assert np.all(ctx.download_temporal()[..., 3] >= 1.0)
        ctx.temporal_track_moments(False)
        for call in (ctx.download_temporal, ctx.download_temporal_moments, ctx.download_temporal_svgf):
            with pytest.raises(g.GspError, match="gsp_temporal_accumulate"):
                call()
        with pytest.raises(g.GspError, match="already"):
            ctx.temporal_accumulate(None)  # (still the frame that was accumulated)

        def one(ts):
            ctx.frame_begin(w, h)
            ctx.frame_sample_base(ts)
            ctx.render(1, ts)
            ctx.render_features(1, ts)
            ctx.temporal_accumulate(None)
            return ctx.download_temporal()[..., 3]

        assert np.all(one(10) == 1.0) and np.all(one(11) == 2.0)
        with pytest.raises(g.GspError, match="gsp_temporal_track_moments"):
            ctx.download_temporal_moments()
        with pytest.raises(g.GspError, match="gsp_temporal_track_moments"):
            ctx.download_temporal_svgf()
        ctx.temporal_track_moments(True)
        with pytest.raises(g.GspError, match="gsp_temporal_accumulate"):
            ctx.download_temporal()
        assert np.all(one(12) == 1.0)
        m = ctx.download_temporal_moments()
        assert np.all(m[..., 2] == 1.0) and not m[..., 3].any()
        assert np.all(one(13) == 2.0) and np.all(ctx.download_temporal_moments()[..., 2] == 0.5)


_TORCH_CHILD = """
import sys
import torch  # first: the tracer's library then binds to the HIP runtime torch has loaded (see bench.py)
import numpy as np
sys.path.insert(0, sys.argv[1])
import gpuspectral_amd as g
from gpuspectral_amd import abi, scenes
W, H = 96, 64
with g.Context(0) as ctx:
    ctx.upload_scene(scenes.cornell_materials(8))
    ctx.temporal_track_moments(True)
    for ts in range(3):
        ctx.frame_begin(W, H)
        ctx.frame_sample_base(ts)
        ctx.render(1, ts)
        ctx.render_features(1, ts)
        ctx.temporal_accumulate(None)
    sv = abi.svgf(min_history=2)
    want = ctx.download_temporal_svgf(None, sv).reshape(-1)
    assert (want[3::4] == 3.0).all() and not np.array_equal(want, ctx.download_temporal().reshape(-1))
    for off in (0, 1):  # floats: the second destination is not 16-byte aligned
        t = torch.zeros(W * H * 4 + 8, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        ctx.temporal_svgf_to_device(t.data_ptr() + 4 * off, W * H * 16, None, sv)
        back = t.cpu().numpy()
        assert np.array_equal(back[off:off + W * H * 4].view(np.uint32), want.view(np.uint32)) and not back[:off].any() and not back[off + W * H * 4:].any()
    t = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda:0")
    try:
        ctx.temporal_svgf_to_device(t.data_ptr(), W * H * 16 - 4)
        raise SystemExit("a destination of the wrong size was accepted")
    except g.GspError as e:
        assert "destination too small" in str(e), e
    assert not t.cpu().numpy().any()
print("torch tensor ok")
"""


def test_svgf_to_device_torch_tensor():
    """Into a torch tensor, in a process of its own: torch has to be imported before the library is loaded (bench.py does the same)."""
    r = subprocess.run([sys.executable, "-c", _TORCH_CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "torch tensor ok" in r.stdout, r.stdout + r.stderr


def test_download_temporal_svgf_display(rigs, emu, scenes_):
    """The LDR film of the filtered history, statistics included: byte for byte the display emulation of the emulated filter."""
    from gpuspectral_amd import abi

    ctx, sc = rigs("cornell"), scenes_["cornell"]
    hist, a, g = sequence(ctx, emu, sc, (96, 64), degrees=[0.0, 2.0, 4.0], what="display", check=lambda k: False)
    dn, sv = abi.denoise(iterations=3), abi.svgf(min_history=2)
    want = emu.run(dn, sv, hist.H, hist.M, a, g)
    for name, d in (("clamp", abi.display()), ("aces", abi.display(tonemap=abi.TONEMAP_ACES)), ("reinhard measured", abi.display(tonemap=abi.TONEMAP_REINHARD)),
                    ("NULL", None)):
        got = ctx.download_temporal_svgf_display(dn, sv, d)
        assert np.array_equal(got.reshape(-1), DisplayEmu().map(d, want.reshape(-1, 4))), name


def test_validation(scenes_):
    import gpuspectral_amd as g
    from gpuspectral_amd import abi

    with g.Context(0) as ctx:
        calls = (ctx.download_temporal_moments, ctx.download_temporal_svgf, ctx.download_temporal_svgf_display)
        for call in calls:
            with pytest.raises(g.GspError, match="gsp_temporal_accumulate"):
                call()  # before any accumulate
        assert ctx._L.gsp_temporal_svgf_to_device(ctx._h, None, None, 16, 1 << 30) == 1 and "gsp_temporal_accumulate" in ctx._L.gsp_last_error(ctx._h).decode()
        ctx.upload_scene(scenes_["cornell"])
        # the order of the refusals, two broken conditions per call (temporal_util.refusals): first without a frame and a history ...
        buf = np.zeros((16, 16, 4), np.float32).ctypes.data
        bad_dn, tone, bads = C.byref(abi.denoise(iterations=9)), C.byref(abi.display(tonemap=7)), C.byref(abi.svgf(min_history=1))
        names = ("gsp_download_temporal_moments", "gsp_download_temporal_svgf", "gsp_temporal_svgf_to_device", "gsp_download_temporal_svgf_display")
        null, hist, track, full = (dict((n, n + t) for n in names) for t in (
            ": null output pointer", " needs a gsp_temporal_accumulate call since the history was last invalidated",
            " needs gsp_temporal_track_moments(ctx, 1) before the history was accumulated",
            " needs a full frame (no pixel_ids) and a gsp_render_features call since gsp_frame_begin"))
        n0, n1, n2, n3 = names
        refusals(ctx, [(n0, (None,), null[n0]), (n0, (buf,), hist[n0]), (n1, (bad_dn, None, None), null[n1]), (n1, (bad_dn, None, buf), hist[n1]),
                       (n2, (None, None, None, 0), null[n2]), (n2, (None, None, 16, 0), hist[n2]), (n3, (None, None, tone, None), "tonemap"),
                       (n3, (None, None, None, None), null[n3]), (n3, (None, None, None, buf), hist[n3])])
        ctx.frame_begin(16, 16)
        ctx.render(1)
        ctx.render_features(1)
        ctx.temporal_accumulate(None)  # tracking is off
        # ... then with a history without moments, in the next frame before its feature pass ...
        ctx.frame_begin(16, 16)
        refusals(ctx, [(n0, (None,), null[n0]), (n0, (buf,), track[n0]), (n1, (bad_dn, None, buf), track[n1]), (n2, (None, None, 16, 4), "destination too small"),
                       (n2, (None, None, 16, 1 << 20), track[n2]), (n3, (None, None, None, buf), track[n3])])
        ctx.render(1)
        ctx.render_features(1)
        for call in calls:
            with pytest.raises(g.GspError, match="gsp_temporal_track_moments"):
                call()
        ctx.temporal_track_moments(True)
        ctx.frame_begin(16, 16)
        ctx.render(1)
        ctx.render_features(1)
        ctx.temporal_accumulate(None)
        L, h = ctx._L, ctx._h
        err = lambda: L.gsp_last_error(h).decode()
        assert L.gsp_download_temporal_moments(h, None) == 1 and "null output" in err()
        assert L.gsp_download_temporal_svgf(h, None, None, None) == 1 and "null output" in err()
        assert L.gsp_temporal_svgf_to_device(h, None, None, None, 1 << 20) == 1 and "null output" in err()
        assert L.gsp_download_temporal_svgf_display(h, None, None, None, None) == 1 and "null output" in err()
        for bad, word in ((abi.svgf(min_history=1), "min_history"), (abi.svgf(min_history=65537), "min_history"), (abi.svgf(sigma_variance=-1.0), "sigma_variance"),
                          (abi.svgf(sigma_variance=float("nan")), "sigma_variance")):
            with pytest.raises(g.GspError, match=word):
                ctx.download_temporal_svgf(None, bad)
            with pytest.raises(g.GspError, match=word):
                ctx.download_temporal_svgf_display(None, bad, None)
        for bad, word in ((abi.denoise(iterations=9), "iterations"), (abi.denoise(sigma_color=-1.0), "sigma_color"), (abi.denoise(sigma_depth=float("nan")), "sigma_depth")):
            with pytest.raises(g.GspError, match=word):
                ctx.download_temporal_svgf(bad, None)
        with pytest.raises(g.GspError, match="tonemap"):
            ctx.download_temporal_svgf_display(None, None, abi.display(tonemap=7))
        ctx.download_temporal_svgf(None, None)
        refusals(ctx, [(n1, (bad_dn, None, buf), "iterations"), (n1, (None, bads, buf), "min_history"), (n2, (bad_dn, None, 16, 4), "destination too small"),
                       (n3, (bad_dn, None, tone, buf), "tonemap")])
        ctx.frame_begin(16, 16)  # a new frame of the same size: the history stays, the feature planes are stale
        assert np.all(ctx.download_temporal_moments()[..., 2] == 1.0)
        refusals(ctx, [(n1, (bad_dn, None, buf), full[n1]), (n2, (bad_dn, None, 16, 1 << 20), full[n2]), (n3, (bad_dn, None, None, buf), full[n3])])
        with pytest.raises(g.GspError, match="gsp_render_features"):
            ctx.download_temporal_svgf(None, None)
        ctx.frame_begin(16, 16, pixel_ids=g.pt.tile_partition(16, 16, 0, 2))
        ctx.render_features(1)
        with pytest.raises(g.GspError, match="pixel_ids"):
            ctx.download_temporal_svgf(None, None)


def test_host_layer(emu):
    """The C++ host layer: PathTracer::temporalTrackMoments / downloadTemporalMoments / downloadTemporalSvgf."""
    from conftest import CORNELL_XML
    from gpuspectral_amd import abi, host

    W, H = 48, 40
    sc = host.Scene(CORNELL_XML)
    pt = host.PathTracer(W, H)
    try:
        pt.temporal_track_moments(True)
        for k in range(3):
            if k:
                pt.next_frame()
            pt.render(sc, 1)
            pt.render_features(sc, 1)
            pt.temporal_accumulate(abi.temporal(alpha=FLT_MIN))
        a, g = pt.download_features()
        hist, m = pt.download_temporal(), pt.download_temporal_moments()
        assert np.all(hist[..., 3] == 3.0) and np.all(np.abs(m[..., 2] - 1.0 / 3.0) < 1e-6) and not m[..., 3].any()
        for dn, sv in ((None, None), (abi.denoise(iterations=2), abi.svgf(min_history=2, sigma_variance=2.0))):
            assert same(pt.download_temporal_svgf(dn, sv), emu.run(dn, sv, hist, m, a, g))
        pt.temporal_track_moments(False)
        with pytest.raises(Exception, match="gsp_temporal_accumulate"):
            pt.download_temporal()
    finally:
        pt.close()


def test_cli_svgf(tmp_path):
    """--temporal ... --svgf out.pfm: the variance-guided filter of the last frame's history beside the history itself."""
    from oracle import mitsuba_loader as ml
    from conftest import CORNELL_XML

    lib = os.path.join(ROOT, "gpuspectral_amd", "lib")
    env = dict(os.environ, LD_LIBRARY_PATH=lib + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    W, H, S = 64, 48, 1
    t = tmp_path
    pfm = lambda path: np.asarray(ml.read_pfm(str(path)), np.float32).reshape(H, W, -1)[::-1, :, :3]
    r = subprocess.run([os.path.join(lib, "gsp_render"), "--temporal", str(t / "h.pfm"), "--temporal-frames", "6", "--temporal-orbit", "1", "--svgf", str(t / "s.pfm"),
                        "--svgf-sigma", "3", "--svgf-min-history", "3", CORNELL_XML, str(t / "f.pfm"), str(W), str(H), str(S)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "temporal: 6 frames" in r.stdout and "svgf: 5 levels, sigma_variance 3, min history 3" in r.stdout
    assert sorted(os.listdir(str(t))) == ["f.pfm", "f.pfm.ppm", "h.pfm", "s.pfm"]
    hist, out = pfm(t / "h.pfm"), pfm(t / "s.pfm")
    assert np.isfinite(out).all() and out.min() >= 0.0 and not same(out, hist)
    rough = lambda img: float(((img[:, 1:] - img[:, :-1]) ** 2).mean())
    assert rough(np.minimum(out, 1.0)) < rough(np.minimum(hist, 1.0))
