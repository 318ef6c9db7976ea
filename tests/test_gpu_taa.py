"""Temporal anti-aliasing on the GPU (include/gpuspectral_pt.h, "Temporal anti-aliasing"): k_taa_resolve and the encode read-out against
the same text run on the host (csrc/pt_taa.h through tests/emu/taa_emu.cpp, itself held to a float32 restatement bit for bit in
tests/test_taa_cpu.py).  The resolved frame D' and its RGBA8 words equal the emulation applied to the GPU's own source plane, its
motion plane V and the emulation's previous D BIT FOR BIT, frame after frame.  Then the three routes of a source, a context that
resolves beside one that does not, bytes, refusals and taa_valid, the shimmer the feature is for, the host layer and the CLI."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from taa_util import TaaEmu
from temporal_util import refusals, same
from test_gpu_illum import begin, check
from test_gpu_motion import MOVERS, ORBIT, moved_instances, orbit

pytestmark = pytest.mark.gpu

TONEMAPS = {"clamp": dict(tonemap=0), "aces": dict(tonemap=2, exposure=0.5), "reinhard": dict(tonemap=1, key=0.3, burn=0.2)}
GAMMAS = {"srgb": 0.0, "gamma2.2": 2.2}


def make_display(tonemap, gamma):
    from gpuspectral_amd import abi

    return abi.display(gamma=GAMMAS[gamma], **TONEMAPS[tonemap])


@pytest.fixture(scope="module")
def temu():
    return TaaEmu()


@pytest.fixture(scope="module")
def rig(cornell):
    """One context with the Cornell box uploaded and following on, shared by the cases below and put into the case's state."""
    import gpuspectral_amd as g

    ctx = g.Context(0)
    ctx.upload_scene(cornell)

    def get(demod, moments):
        ctx.set_lens()
        ctx.update_camera(cornell.to_world, cornell.fov)
        ctx.update_instances(cornell.instances)
        ctx.temporal_demodulate(demod)
        ctx.temporal_track_moments(moments)
        ctx.temporal_follow_instances(True)
        ctx.temporal_reset()
        return ctx

    yield get
    ctx.close()


def sequence(ctx, temu, sc, size, source, taa, disp, degrees, what):
    """The viewer loop per frame -- the edit, the camera, frame_begin, frame_sample_base, render 1 spp, render_features, the followed
    accumulate, the resolve -- and the emulation on the GPU's own source plane and V and its own previous D.  Returns the last D."""
    from gpuspectral_amd import abi

    prev, used = None, 0
    for k, cam in enumerate(orbit(sc, degrees)):
        begin(ctx, size, k, cam, sc.fov, moved_instances(sc.instances, MOVERS["cornell"], k))
        ctx.temporal_accumulate(None)
        if source == "svgf":
            src = ctx.download_temporal_svgf(None, abi.svgf(min_history=2))
            ctx.temporal_taa(taa, disp, src)
        else:
            src = ctx.download_temporal_image()
            ctx.temporal_taa(taa, disp, None)
        D, words = temu.step(taa, disp, src, ctx.download_temporal_motion(), prev)
        check("%s frame %d" % (what, k), "D'", ctx.download_taa(), D)
        got = ctx.download_taa_display()
        assert np.array_equal(got, words), "%s frame %d: %d of %d words differ" % (what, k, (got != words).sum(), words.size)
        assert k > 0 or not D[..., 3].any()
        used += int(D[..., 3].sum())
        prev = D
    return prev, used


# ---- bit for bit against the emulation -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["null", "svgf"])
@pytest.mark.parametrize("demod", [False, True], ids=["colour", "demod"])
@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("tonemap", TONEMAPS)
def test_cornell_orbit_with_the_tall_box_moving(rig, temu, cornell, tonemap, gamma, demod, source):
    """40 x 24, six one-sample frames of the orbit with the tall box turning and stepping; REINHARD measures the source plane."""
    from gpuspectral_amd import abi

    ctx = rig(demod, source == "svgf")
    D, used = sequence(ctx, temu, cornell, (40, 24), source, abi.taa(0.2, 2.0) if tonemap == "aces" else None, make_display(tonemap, gamma), ORBIT[:6], "cornell")
    assert used > 0.5 * 5 * 40 * 24  # (the history is used)


@pytest.mark.parametrize("size", [(45, 19), (33, 9), (31, 7), (1, 1)])
def test_ragged_and_tiny_frames(rig, temu, cornell, size):
    """A partial tile in both directions, a frame smaller than one tile, a frame whose halo lies outside it altogether."""
    sequence(rig(True, False), temu, cornell, size, "null", None, make_display("aces", "srgb"), ORBIT[:4], "cornell %dx%d" % size)


# ---- one source, three routes ---------------------------------------------------------------------------------------------------------------
_TORCH_CHILD = """
import sys
import torch  # first: the tracer's library then binds to the HIP runtime torch has loaded (see bench.py)
import numpy as np
sys.path.insert(0, sys.argv[1])
import gpuspectral_amd as g
from gpuspectral_amd import abi, scenes
W, H = 45, 19
N = W * H * 4
sc = scenes.cornell_materials(8)
disp = abi.display(tonemap=abi.TONEMAP_ACES, gamma=2.2)
routes = ("host", "device", "device+4", "null")
ctxs = [g.Context(0) for _ in routes]
try:
    for ctx in ctxs:
        ctx.upload_scene(sc)
        ctx.temporal_follow_instances(True)
        ctx.temporal_demodulate(True)
    for ts in range(3):
        got = []
        for route, ctx in zip(routes, ctxs):
            ctx.frame_begin(W, H)
            ctx.frame_sample_base(ts)
            ctx.render(1, ts)
            ctx.render_features(1, ts)
            ctx.temporal_accumulate(None)
            src = ctx.download_temporal_image()
            if route == "host":
                ctx.temporal_taa(None, disp, src)
            elif route == "null":
                ctx.temporal_taa_from_device(None, None, None, disp) if ts & 1 else ctx.temporal_taa(None, disp, None)
            else:
                off = 1 if route == "device+4" else 0  # floats: 4 bytes off a 16-byte boundary
                t = torch.zeros(N + 8, dtype=torch.float32, device="cuda:0")
                t[off:off + N] = torch.from_numpy(src.reshape(-1)).to("cuda:0")
                torch.cuda.synchronize()
                assert (t[off:off + N].data_ptr() & 15) == 4 * off
                ctx.temporal_taa_from_device(t[off:off + N], None, None, disp)
                assert np.array_equal(t.cpu().numpy()[off:off + N].view(np.uint32), src.reshape(-1).view(np.uint32))  # (the source is only read)
            got.append(ctx.download_taa())
        for route, d in zip(routes[1:], got[1:]):
            assert np.array_equal(d.view(np.uint32), got[0].view(np.uint32)), (ts, route)
        assert (got[0][..., 3] == 1.0).mean() > (0.9 if ts else -1.0) and np.isfinite(got[0]).all()
        # the encode into device memory, aligned and not
        ctx = ctxs[0]
        want = ctx.download_taa_display().reshape(-1)
        for off in (0, 1):
            t = torch.zeros(W * H + 8, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            ctx.taa_display_to_device(t[off:off + W * H])
            back = t.cpu().numpy().view(np.uint32)
            assert np.array_equal(back[off:off + W * H], want) and not back[:off].any() and not back[off + W * H:].any()
    ctx = ctxs[1]
    t = torch.zeros(N, dtype=torch.float32, device="cuda:0")
    for call, word in ((lambda: ctx.taa_display_to_device(t.data_ptr(), W * H * 4 - 4), "destination too small"),):
        try:
            call()
            raise SystemExit("a destination of the wrong size was accepted")
        except g.GspError as e:
            assert word in str(e), e
    assert not t.cpu().numpy().any()
    ctx.frame_begin(W, H)
    ctx.frame_sample_base(9)
    ctx.render(1, 9)
    ctx.render_features(1, 9)
    ctx.temporal_accumulate(None)
    try:
        ctx.temporal_taa_from_device(t.data_ptr(), N * 4 - 4, None, disp)
        raise SystemExit("a source of the wrong size was accepted")
    except g.GspError as e:
        assert "source too small" in str(e), e
    ctx.temporal_taa_from_device(t.data_ptr(), N * 4, None, disp)  # (the refused call did not count as the frame's resolve)
finally:
    for ctx in ctxs:
        ctx.close()
print("torch tensor ok")
"""


def test_one_source_three_routes():
    """The host array, a torch tensor through _from_device (also 4 bytes off a 16-byte boundary) and NULL give the same D' bits; in a
    process of its own: torch has to be imported before the library is loaded (bench.py does the same)."""
    r = subprocess.run([sys.executable, "-c", _TORCH_CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "torch tensor ok" in r.stdout, r.stdout + r.stderr


# ---- it touches nothing else --------------------------------------------------------------------------------------------------------------
def test_a_resolving_context_is_one_that_does_not(cornell):
    """Two contexts on the same five frames (moments, following, the anti-lag), a resolving the filter's output every frame under
    REINHARD with measured statistics: H, F, M, V, the filter's output, the features, the frame and gsp_get_stats are equal bit for
    bit (of the statistics the counters; the timings of two contexts differ by themselves and are held to a's own before the resolve),
    device_bytes apart -- which grows by the two D planes at the first resolve (the filter's output plane, through which the host
    source passes, exists by then) and by the 24-byte statistics record of the LDR film."""
    import gpuspectral_amd as g
    from gpuspectral_amd import abi

    W, H = 40, 24
    disp = make_display("reinhard", "srgb")
    sv = abi.svgf(min_history=2)
    with g.Context(0) as a, g.Context(0) as b:
        for ctx in (a, b):
            ctx.upload_scene(cornell)
            ctx.temporal_track_moments(True)
            ctx.temporal_follow_instances(True)
        for k, cam in enumerate(orbit(cornell, ORBIT[:5])):
            inst = moved_instances(cornell.instances, MOVERS["cornell"], k)
            outs = []
            for ctx in (a, b):
                begin(ctx, (W, H), k, cam, cornell.fov, inst)
                ctx.temporal_accumulate(None)
                ctx.temporal_antilag(None)
                outs.append(ctx.download_temporal_svgf(None, sv))
            before = a.stats()
            a.temporal_taa(None, disp, outs[0])
            after = a.stats()
            grown = after.pop("device_bytes") - before.pop("device_bytes")
            assert grown == (2 * W * H * 16 + 24 if k == 0 else 0), (k, grown)
            assert after == before, k  # (every other field of gsp_stats, the timings included, keeps its value)
            assert same(outs[0], outs[1])
            for name in ("download", "download_temporal", "download_temporal_fast", "download_temporal_moments", "download_temporal_motion",
                         "download_temporal_image"):
                assert same(getattr(a, name)(), getattr(b, name)()), (k, name)
            assert same(a.download_temporal_svgf(None, sv), b.download_temporal_svgf(None, sv)), k
            for pa, pb in zip(a.download_features(), b.download_features()):
                assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)), k
            sa, sb = a.stats(), b.stats()
            assert sa["device_bytes"] == sb["device_bytes"] + 2 * W * H * 16 + 24
            timed = ("device_bytes", "render_seconds", "extend_kernel_ms", "shade_kernel_ms", "connect_kernel_ms", "bvh_build_ms")
            assert {n: v for n, v in sa.items() if n not in timed} == {n: v for n, v in sb.items() if n not in timed}
        with pytest.raises(g.GspError, match="gsp_temporal_taa call"):
            b.download_taa()


def test_bytes_of_the_planes_and_the_staging_plane(cornell):
    """A context with nothing but the history: the first resolve of the NULL source reads H where it lies and makes exactly the two D
    planes; the first source in host memory makes the filters' output plane it passes through, once; a read-out of the words makes
    the RGBA8 buffer of the LDR film."""
    import gpuspectral_amd as g

    W, H = 33, 9
    with g.Context(0) as ctx:
        ctx.upload_scene(cornell)
        ctx.temporal_follow_instances(True)
        grown = []
        for k in range(3):
            begin(ctx, (W, H), k)
            ctx.temporal_accumulate(None)
            b0 = ctx.stats()["device_bytes"]
            ctx.temporal_taa(None, None, ctx.download_temporal_image() if k else None)
            grown.append(ctx.stats()["device_bytes"] - b0)
        assert grown == [2 * W * H * 16, W * H * 16, 0]
        b0 = ctx.stats()["device_bytes"]
        ctx.download_taa()
        assert ctx.stats()["device_bytes"] == b0
        ctx.download_taa_display()
        assert ctx.stats()["device_bytes"] == b0 + (W * H + 3) // 4 * 16


# ---- refusals and taa_valid ------------------------------------------------------------------------------------------------------------------
def test_refusals(cornell):
    import gpuspectral_amd as g
    from gpuspectral_amd import abi

    w, h = 40, 24
    size = (w, h)
    src = np.zeros((h, w, 4), np.float32)
    buf = src.ctypes.data
    n0, n1, n2, n3, n4 = "gsp_temporal_taa", "gsp_temporal_taa_from_device", "gsp_download_taa", "gsp_download_taa_display", "gsp_taa_display_to_device"
    hist, done, call = (dict((n, n + t) for n in (n0, n1, n2, n3, n4)) for t in (
        " needs a gsp_temporal_accumulate call since the history was last invalidated", " needs a gsp_temporal_accumulate call since gsp_frame_begin",
        " needs a gsp_temporal_taa call since the history was last invalidated"))
    bad_taa = [(C.byref(abi.taa(alpha=-0.5)), "gsp_taa.alpha"), (C.byref(abi.taa(alpha=1.5)), "gsp_taa.alpha"), (C.byref(abi.taa(alpha=float("nan"))), "gsp_taa.alpha"),
               (C.byref(abi.taa(sigma_clip=-1.0)), "gsp_taa.sigma_clip"), (C.byref(abi.taa(sigma_clip=float("nan"))), "gsp_taa.sigma_clip"),
               (C.byref(abi.taa(sigma_clip=float("inf"))), "gsp_taa.sigma_clip")]
    bad_disp = [(C.byref(abi.display(tonemap=7)), "gsp_display.tonemap"), (C.byref(abi.display(exposure=100.0)), "gsp_display.exposure"),
                (C.byref(abi.display(gamma=-1.0)), "gsp_display.gamma")]
    with g.Context(0) as ctx:
        ctx.upload_scene(cornell)
        # no frame; a frame begun with pixel_ids
        refusals(ctx, [(n0, (bad_taa[0][0], None, None), n0 + " needs gsp_frame_begin first"), (n1, (None, None, 16, 0), n1 + " needs gsp_frame_begin first"),
                       (n2, (None,), n2 + ": null output pointer"), (n2, (buf,), hist[n2]), (n3, (None,), n3 + ": null output pointer"), (n3, (buf,), hist[n3]),
                       (n4, (None, 0), n4 + ": null output pointer"), (n4, (16, 0), hist[n4])])
        ctx.frame_begin(w, h, pixel_ids=np.arange(7, dtype=np.uint32))
        refusals(ctx, [(n0, (bad_taa[0][0], None, None), n0 + ": the frame was begun with pixel_ids")])
        # following off: no accumulate yet, then an accumulate without the motion plane
        begin(ctx, size, 0)
        refusals(ctx, [(n0, (bad_taa[0][0], None, None), hist[n0])])
        ctx.temporal_accumulate(None)
        refusals(ctx, [(n0, (bad_taa[0][0], None, None), n0 + " needs gsp_temporal_follow_instances(ctx, 1)"), (n1, (None, None, 16, 0), n1 + " needs gsp_temporal_follow_instances(ctx, 1)")])
        ctx.temporal_follow_instances(True)
        refusals(ctx, [(n0, (None, None, None), hist[n0])])  # (the toggle dropped the history)
        begin(ctx, size, 1)
        refusals(ctx, [(n0, (bad_taa[0][0], None, None), hist[n0])])  # (a frame, no accumulate yet)
        ctx.temporal_accumulate(None)
        b0 = ctx.stats()["device_bytes"]
        # the fields, each; a short device source; the read-outs before any resolve
        refusals(ctx, [(n0, (p, bad_disp[0][0], None), t) for p, t in bad_taa] + [(n0, (None, p, None), t) for p, t in bad_disp]
                 + [(n1, (None, bad_disp[0][0], 16, 0), "gsp_display.tonemap"), (n1, (None, None, 16, 16 * w * h - 1), n1 + ": source too small"),
                    (n2, (buf,), call[n2]), (n3, (buf,), call[n3]), (n4, (16, 4 * w * h), call[n4])])
        assert ctx.stats()["device_bytes"] == b0  # (no refused call made a plane)
        ctx.temporal_taa(None, None, None)
        d0 = ctx.download_taa()
        # a second resolve for the same accumulate, by either export; short and NULL destinations
        refusals(ctx, [(n0, (bad_taa[0][0], None, None), n0 + ": the frame has been resolved already (one call per gsp_temporal_accumulate)"),
                       (n1, (None, None, None, 0), n1 + ": the frame has been resolved already"), (n4, (16, 4 * w * h - 1), "destination too small"),
                       (n4, (None, 4 * w * h), "null output pointer"), (n2, (None,), "null output pointer"), (n3, (None,), "null output pointer")])
        assert same(ctx.download_taa(), d0)
        # the next frame before its accumulate: no resolve, the read-out of the last one stays
        begin(ctx, size, 2)
        refusals(ctx, [(n0, (None, None, None), done[n0]), (n1, (None, None, None, 0), done[n1])])
        assert same(ctx.download_taa(), d0)


def test_taa_valid(cornell):
    """Whatever clears history_valid clears taa_valid -- gsp_temporal_reset, gsp_upload_scene, a frame of another size, a follow toggle --
    and so does a frame whose accumulate was not resolved: the next resolve has .w = 0 everywhere, the one after it uses its history."""
    import gpuspectral_amd as g

    size = (40, 24)
    with g.Context(0) as ctx:
        ctx.upload_scene(cornell)
        ctx.temporal_follow_instances(True)
        ts = [0]

        def frame(sz=size, resolve=True):
            begin(ctx, sz, ts[0])
            ts[0] += 1
            ctx.temporal_accumulate(None)
            if resolve:
                ctx.temporal_taa(None, None, None)
                return ctx.download_taa()[..., 3]

        def toggle():
            ctx.temporal_follow_instances(False)
            ctx.temporal_follow_instances(True)

        used = lambda w: (w == 1.0).mean() > 0.98  # (a pixel whose sample was not finite is nobody's history, in H and so in V)
        assert not frame().any() and used(frame())
        for name, clear, sz in (("reset", ctx.temporal_reset, size), ("upload", lambda: ctx.upload_scene(cornell), size), ("size", lambda: None, (24, 40)),
                                ("toggle", toggle, (24, 40)), ("unresolved", lambda: frame((24, 40), resolve=False), (24, 40))):
            clear()
            if name in ("reset", "upload", "toggle"):
                with pytest.raises(g.GspError, match="since the history was last invalidated"):
                    ctx.download_taa()
            first, second = frame(sz), frame(sz)
            assert first.shape == sz[::-1] and not first.any(), name
            assert used(second), name
        # the read-out asks for a resolve since the history began: an accumulate that found none behind it starts over
        ctx.temporal_reset()
        frame(resolve=False)
        with pytest.raises(g.GspError, match="needs a gsp_temporal_taa call since the history was last invalidated"):
            ctx.download_taa_display()


# ---- what it is for --------------------------------------------------------------------------------------------------------------------------
def test_less_shimmer_on_real_frames(cornell):
    """Cornell box 64 x 64, unmoved camera, the tent pixel filter, 24 one-sample frames with a fresh frame_sample_base each, the
    filter's output resolved under every default.  Over the pixels whose mean coverage lies strictly between 0.05 and 0.95 -- the
    silhouette of the box against the background -- the temporal standard deviation of the resolved luma over frames 8..23 is smaller
    with the default alpha than with alpha = 1 (the frame itself) on the same sources.  The ratio is printed, not asserted."""
    import gpuspectral_amd as g
    from gpuspectral_amd import abi

    W = H = 64
    sv = abi.svgf(min_history=2)
    luma = lambda d: 0.2126 * d[..., 0].astype(np.float64) + 0.7152 * d[..., 1] + 0.0722 * d[..., 2]
    out, cover, srcs = {}, [], {}
    with g.Context(0) as ctx:
        ctx.upload_scene(cornell)
        ctx.temporal_track_moments(True)
        ctx.temporal_follow_instances(True)
        for alpha in (0.0, 1.0):
            ctx.temporal_reset()
            ys, ss = [], []
            for k in range(24):
                ctx.frame_begin(W, H)
                ctx.frame_sample_base(7000 + k)
                ctx.render(1, 7000 + k, pixel_filter=abi.FILTER_TENT)
                ctx.render_features(1, 7000 + k, pixel_filter=abi.FILTER_TENT)
                ctx.temporal_accumulate(None)
                src = ctx.download_temporal_svgf(None, sv)
                ctx.temporal_taa(abi.taa(alpha=alpha) if alpha else None, None, src)
                ys.append(luma(ctx.download_taa()))
                ss.append(src)
                if alpha == 0.0:
                    cover.append(ctx.download_features()[0][..., 3].astype(np.float64))
            out[alpha], srcs[alpha] = np.asarray(ys), ss
    assert all(same(p, q) for p, q in zip(srcs[0.0], srcs[1.0]))  # (the same sources: the resolve feeds nothing back)
    edge = np.mean(cover, 0)
    edge = (edge > 0.05) & (edge < 0.95)
    assert edge.sum() >= 16, edge.sum()
    sd = {a: float(out[a][8:].std(0)[edge].mean()) for a in out}
    print("shimmer over %d silhouette pixels, frames 8..23: temporal sd of the luma %.5f resolved (default alpha), %.5f at alpha = 1; ratio %.3f"
          % (edge.sum(), sd[0.0], sd[1.0], sd[0.0] / sd[1.0]))
    assert sd[0.0] < sd[1.0]


# ---- host layer, CLI ------------------------------------------------------------------------------------------------------------------------
def test_host_layer(temu):
    """The C++ host layer: PathTracer::temporalTaa / downloadTaa / downloadTaaDisplay against the emulation, three frames."""
    from conftest import CORNELL_XML
    from gpuspectral_amd import abi, host

    W, H = 45, 19
    sc = host.Scene(CORNELL_XML)
    pt = host.PathTracer(W, H)
    disp = make_display("aces", "gamma2.2")
    try:
        pt.temporal_follow_instances(True)
        prev = None
        for k in range(3):
            if k:
                pt.next_frame()
            pt.render(sc, 1)
            pt.render_features(sc, 1)
            with pytest.raises(Exception, match="gsp_temporal_taa"):
                pt.temporal_taa(None, disp, None)  # (no accumulate in this frame yet)
            pt.temporal_accumulate(None)
            src = pt.download_temporal_image()
            pt.temporal_taa(abi.taa(alpha=0.25), disp, src if k & 1 else None)
            D, words = temu.step(abi.taa(alpha=0.25), disp, src, pt.download_temporal_motion(), prev)
            check("host frame %d" % k, "D'", pt.download_taa(), D)
            assert np.array_equal(pt.download_taa_display(), words)
            assert (D[..., 3] == 1.0).mean() > (0.9 if k else -1.0)
            with pytest.raises(Exception, match="resolved already"):
                pt.temporal_taa(None, disp, None)
            prev = D
        with pytest.raises(Exception, match="source buffer too small"):
            pt.temporal_taa(None, disp, np.zeros(8, np.float32))
    finally:
        pt.close()


def test_cli(tmp_path, temu):
    """--taa on the Cornell XML at 64 x 48.  One frame: the resolve has no history, so the PNG decodes to the emulation's words of the
    filter's output as the CLI wrote it.  Then the eight-frame command line of the documents: the history is used and the PNG changes."""
    from oracle import mitsuba_loader as ml
    from conftest import CORNELL_XML
    from gpuspectral_amd import abi, host

    lib = os.path.join(ROOT, "gpuspectral_amd", "lib")
    env = dict(os.environ, LD_LIBRARY_PATH=lib + ":" + os.environ.get("LD_LIBRARY_PATH", ""))

    def run(args, code=0):
        r = subprocess.run([os.path.join(lib, "gsp_render")] + args, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == code, r.stdout + r.stderr
        return r.stdout + r.stderr

    W, H = 64, 48
    t = tmp_path
    png = lambda path: host.decode_png(open(str(path), "rb").read())[::-1]  # (decodePng hands the rows back bottom-up)

    def pfm(path):
        out = np.ones((H, W, 4), np.float32)
        out[..., :3] = np.asarray(ml.read_pfm(str(path)), np.float32).reshape(H, W, -1)[::-1, :, :3]
        return out

    tail = [CORNELL_XML, str(t / "frame.pfm"), str(W), str(H), "1"]
    for name, extra, srcfile in (("svgf", ["--svgf", str(t / "s1.pfm")], "s1.pfm"), ("image", [], "t1.pfm")):
        out = run(["--temporal", str(t / "t1.pfm"), "--temporal-frames", "1", "--temporal-follow", "--taa", str(t / (name + ".png")), "--tonemap", "aces", "--gamma", "2.2",
                   "--taa-alpha", "0.3", "--taa-sigma", "1.5"] + extra + tail)
        assert "taa: " in out and "alpha 0.3, sigma 1.5" in out and "0.0 % of the last frame's pixels blended" in out, out
        _, words = temu.step(None, abi.display(tonemap=abi.TONEMAP_ACES, gamma=2.2), pfm(t / srcfile), np.zeros((H, W, 4), np.float32), None)
        got = png(t / (name + ".png"))
        assert got.shape == (H, W) and np.array_equal(got, words), (name, (got != words).sum())
    out = run(["--temporal", str(t / "t.pfm"), "--temporal-frames", "8", "--temporal-follow", "--svgf", str(t / "s.pfm"), "--taa", str(t / "out.png")] + tail)
    assert "temporal: 8 frames" in out and "resolved over its history on each of 8 frames" in out and "the filter's output" in out, out
    blended = float(out.split("% of the last frame's pixels blended")[0].split(",")[-1])
    got = png(t / "out.png")
    assert got.shape == (H, W) and blended > 90.0 and (got >> 24 == 0xFF).all() and len(np.unique(got)) > 100
    run(["--temporal", str(t / "t.pfm"), "--temporal-frames", "2", "--taa", str(t / "x.png")] + tail, code=2)
