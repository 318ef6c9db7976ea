"""The temporal anti-lag on the GPU (include/gpuspectral_pt.h, "Temporal anti-lag"): k_antilag_fast and k_antilag_clamp against the same
text run on the host (csrc/pt_antilag.h through tests/emu/antilag_emu.cpp, itself checked against a float64 restatement in
tests/test_antilag_cpu.py).  The fast history F' and the clamped history equal the emulation applied to gsp_download +
gsp_download_features + the previous emulated planes BIT FOR BIT, frame after frame, and M and V keep their bits.  (G, I and the older
set have no read-out: the next frame's accumulate and anti-lag read them, so a changed bit there shows one frame later.)  Then the
composition with the feedback, a context that stops calling it, state, bytes and refusals, the two quality orderings the feature is
for, the device-memory read-out, the host layer and the CLI."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from antilag_util import AntilagEmu
from conftest import GOLDEN, ROOT
from illum_util import IllumEmu
from temporal_util import refusals, same
from test_gpu_illum import begin, check
from test_gpu_motion import MOVERS, ORBIT, moved_instances, orbit

pytestmark = pytest.mark.gpu

STATES = [(d, f) for d in (False, True) for f in (False, True)]
STATE_IDS = ["%s-%s" % ("demod" if d else "colour", "follow" if f else "static") for d, f in STATES]


@pytest.fixture(scope="module")
def emus():
    return AntilagEmu(), IllumEmu()


@pytest.fixture(scope="module")
def rig(cornell):
    """One context with the Cornell box uploaded, shared by the cases below and put into the case's state."""
    import gpuspectral_amd as g

    ctx = g.Context(0)
    ctx.upload_scene(cornell)

    def get(demod, follow, moments):
        ctx.set_lens()
        ctx.update_camera(cornell.to_world, cornell.fov)
        ctx.update_instances(cornell.instances)
        ctx.temporal_demodulate(demod)
        ctx.temporal_track_moments(moments)
        ctx.temporal_follow_instances(follow)
        ctx.temporal_reset()
        return ctx

    yield get
    ctx.close()


def frame(ctx, emus, hist, fast, cam, fov, size, ts, inst, demod, follow, moments, al, what, feedback=False):
    """One frame of the viewer loop -- the edit, the camera, the frame, its feature pass, the accumulate, the anti-lag and (feedback) one
    level of the filter fed back -- on the GPU and by the emulations from (hist, fast).  Returns the emulated (history, F') the next
    frame starts from."""
    from gpuspectral_amd import abi

    aemu, iemu = emus
    begin(ctx, size, ts, cam, fov, inst)
    ctx.temporal_accumulate(None)
    c = ctx.download()
    a, g, i = ctx.download_features()
    xforms = inst["transform"] if follow else None
    new = iemu.step(None, cam, fov, c, a, g, i, xforms=xforms, hist=hist, moments=moments, demod=demod)
    check(what, "H before the call", ctx.download_temporal(), new.H)
    ctx.temporal_antilag(al)
    F, Hc = aemu.step(al, None, cam, fov, c, a, g, i, new, old=hist, fast=fast, xforms=xforms, demod=demod)
    check(what, "F'", ctx.download_temporal_fast(), F)
    check(what, "H", ctx.download_temporal(), Hc)
    if moments:
        check(what, "M", ctx.download_temporal_moments(), new.M)
    if follow:
        check(what, "V", ctx.download_temporal_motion(), new.V)
    check(what, "the image", ctx.download_temporal_image(), iemu.image(Hc, a, demod))
    new.H = Hc
    if feedback:
        sv = abi.svgf(min_history=2)
        out, fb = iemu.svgf(None, sv, Hc, new.M, a, g, demod=demod, levels=1)
        check(what, "the feedback's output", ctx.temporal_svgf_feedback(None, sv, 1), out)
        check(what, "H after the feedback", ctx.download_temporal(), fb)
        check(what, "F' after the feedback", ctx.download_temporal_fast(), F)
        new.H = fb
    return new, F


def sequence(ctx, emus, sc, size, demod, follow, moments, al, degrees, what, feedback=False):
    hist = fast = None
    for k, cam in enumerate(orbit(sc, degrees)):
        inst = moved_instances(sc.instances, MOVERS["cornell"], k)
        hist, fast = frame(ctx, emus, hist, fast, cam, sc.fov, size, k, inst, demod, follow, moments, al, "%s frame %d" % (what, k), feedback)
    return hist, fast


# ---- bit for bit against the emulation -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moments", [False, True], ids=["plain", "moments"])
@pytest.mark.parametrize("radius", [1, 3])
@pytest.mark.parametrize("demod,follow", STATES, ids=STATE_IDS)
def test_cornell_orbit_with_the_tall_box_moving(rig, emus, cornell, demod, follow, radius, moments):
    """64 x 64, eight one-sample frames (the last two of the orbit a jump of 40 degrees and a step on from it)."""
    from gpuspectral_amd import abi

    hist, fast = sequence(rig(demod, follow, moments), emus, cornell, (64, 64), demod, follow, moments, abi.antilag(radius=radius), ORBIT[:8], "cornell")
    assert fast[..., 3].max() == 4.0 and hist.H[..., 3].max() >= 3.0


@pytest.mark.parametrize("demod,follow", [(False, False), (True, True)], ids=["colour-static", "demod-follow"])
@pytest.mark.parametrize("size", [(45, 19), (33, 9), (31, 7), (1, 1)])
def test_ragged_and_tiny_frames(rig, emus, cornell, size, demod, follow):
    """Radius 3 on frames whose tile edges and aprons lie outside the frame, wholly (1 x 1, 31 x 7) or in part."""
    from gpuspectral_amd import abi

    sequence(rig(demod, follow, True), emus, cornell, size, demod, follow, True, abi.antilag(radius=3), ORBIT[:4], "cornell %dx%d" % size)


@pytest.mark.parametrize("demod", [False, True], ids=["colour", "demod"])
def test_composition_with_the_feedback(rig, emus, cornell, demod):
    """accumulate -> anti-lag -> gsp_temporal_svgf_feedback(levels = 1) equals the chain of the emulations, six frames at 64 x 64."""
    hist, fast = sequence(rig(demod, False, True), emus, cornell, (64, 64), demod, False, True, None, ORBIT[:6], "composition", feedback=True)
    assert fast[..., 3].max() == 4.0


# ---- not calling it changes nothing -------------------------------------------------------------------------------------------------------
def test_a_context_that_stops_calling_it_is_one_that_never_did(cornell):
    """Context a allocates F (two frames with the call), b never calls it.  At 64 x 64 the histories then differ, both are reset, and two
    accumulates later a returns b's bits.  At 3 x 2 under radius 3 no window counts the 7 records the rule asks for, so the call may
    change no bit of H at all: a equals b on every frame, called or not, without a reset."""
    import gpuspectral_amd as g
    from gpuspectral_amd import abi

    with g.Context(0) as a, g.Context(0) as b:
        for ctx in (a, b):
            ctx.upload_scene(cornell)
            ctx.temporal_track_moments(True)
        bytes_b = None
        for size, al, reset in (((64, 64), None, True), ((3, 2), abi.antilag(radius=3), False)):
            for ctx in (a, b):
                ctx.temporal_reset()
            for k in range(4):
                if k == 2 and reset:
                    assert not same(a.download_temporal(), b.download_temporal())  # (the clamp had acted)
                    a.temporal_reset()
                    b.temporal_reset()
                for ctx in (a, b):
                    begin(ctx, size, 100 + k)
                    ctx.temporal_accumulate(None)
                if k < 2:
                    a.temporal_antilag(al)
                if k >= 2 or not reset:
                    assert same(a.download_temporal(), b.download_temporal()), (size, k)
                    assert same(a.download_temporal_moments(), b.download_temporal_moments()), (size, k)
                    assert same(a.download_temporal_svgf(), b.download_temporal_svgf()), (size, k)
            if bytes_b is None:
                bytes_b = b.stats()["device_bytes"]
                assert a.stats()["device_bytes"] == bytes_b + 32 * 64 * 64  # b holds no plane of the section
        with pytest.raises(g.GspError, match="gsp_temporal_antilag"):
            b.download_temporal_fast()


# ---- state, bytes and refusals ------------------------------------------------------------------------------------------------------------
def test_state_bytes_and_refusals(cornell):
    import gpuspectral_amd as g
    from gpuspectral_amd import abi

    w, h = 64, 48
    size = (w, h)
    need = 16 * w * h
    buf = np.zeros((h, w, 4), np.float32).ctypes.data
    n0, n1, n2 = "gsp_temporal_antilag", "gsp_download_temporal_fast", "gsp_temporal_fast_to_device"
    hist, done, call = (dict((n, n + t) for n in (n0, n1, n2)) for t in (
        " needs a gsp_temporal_accumulate call since the history was last invalidated", " needs a gsp_temporal_accumulate call since gsp_frame_begin",
        " needs a gsp_temporal_antilag call since the newest gsp_temporal_accumulate"))
    bad = [C.byref(abi.antilag(fast_history=65)), C.byref(abi.antilag(radius=4)), C.byref(abi.antilag(sigma_scale=-1.0)), C.byref(abi.antilag(sigma_scale=float("nan")))]
    words_ = ["gsp_antilag.fast_history", "gsp_antilag.radius", "gsp_antilag.sigma_scale", "gsp_antilag.sigma_scale"]
    with g.Context(0) as ctx:
        ctx.upload_scene(cornell)
        ctx.temporal_track_moments(True)
        # the order of the refusals, two broken conditions per call (temporal_util.refusals): without a history ...
        refusals(ctx, [(n0, (bad[0],), hist[n0]), (n1, (None,), n1 + ": null output pointer"), (n1, (buf,), hist[n1]), (n2, (None, 0), n2 + ": null output pointer"),
                       (n2, (16, 0), hist[n2])])
        begin(ctx, size, 0)
        refusals(ctx, [(n0, (None,), hist[n0])])  # (a frame, no accumulate yet)
        ctx.temporal_accumulate(None)
        b0 = ctx.stats()["device_bytes"]
        h0 = ctx.download_temporal()
        # ... with the frame's accumulate: the fields, each; the read-outs before the call
        refusals(ctx, [(n0, (p,), t) for p, t in zip(bad, words_)] + [(n1, (buf,), call[n1]), (n2, (16, 4), call[n2])])
        assert ctx.stats()["device_bytes"] == b0 and same(ctx.download_temporal(), h0)  # (no refused call made a plane or touched H)
        ctx.temporal_antilag(None)
        assert ctx.stats()["device_bytes"] == b0 + 32 * w * h
        f0, h1 = ctx.download_temporal_fast(), ctx.download_temporal()
        assert np.all(f0[..., 3] == 1.0) and same(f0[..., :3], h0[..., :3])  # the first call: F' is the frame, of length 1
        # ... a second call, a too-small destination
        refusals(ctx, [(n0, (bad[1],), "gsp_antilag.radius"), (n0, (None,), n0 + ": the history has been clamped already (one call per gsp_temporal_accumulate)"),
                       (n2, (16, need - 4), "destination too small"), (n2, (None, need - 4), "null output pointer")])
        assert same(ctx.download_temporal_fast(), f0) and same(ctx.download_temporal(), h1)
        # ... in the next frame before its accumulate, and after its feedback
        begin(ctx, size, 1)
        refusals(ctx, [(n0, (bad[2],), "gsp_antilag.sigma_scale"), (n0, (None,), done[n0])])
        assert same(ctx.download_temporal_fast(), f0)  # (the read-out of the newest accumulate's F' stays)
        ctx.temporal_accumulate(None)
        refusals(ctx, [(n1, (buf,), call[n1])])
        ctx.temporal_svgf_feedback(None, abi.svgf(min_history=2), 1, out=False)
        h2 = ctx.download_temporal()
        refusals(ctx, [(n0, (None,), n0 + ": the history has been fed back already (the call belongs before gsp_temporal_svgf_feedback)")])
        assert same(ctx.download_temporal(), h2) and ctx.stats()["device_bytes"] >= b0 + 32 * w * h
        # a frame with no call: fast_valid is false in the next one, whatever the long history holds
        begin(ctx, size, 2)
        ctx.temporal_accumulate(None)
        b1 = ctx.stats()["device_bytes"]
        ctx.temporal_antilag(abi.antilag(sigma_scale=1e30))
        assert ctx.stats()["device_bytes"] == b1  # (the planes are made once)
        assert np.all(ctx.download_temporal_fast()[..., 3] == 1.0) and ctx.download_temporal()[..., 3].max() == 3.0
        begin(ctx, size, 3)
        ctx.temporal_accumulate(None)
        ctx.temporal_antilag(None)
        assert ctx.download_temporal_fast()[..., 3].max() == 2.0
        # everything that clears history_valid clears fast_valid: a reset, a switch of the context state
        for clear in (ctx.temporal_reset, lambda: ctx.temporal_demodulate(True), lambda: ctx.temporal_follow_instances(True)):
            clear()
            refusals(ctx, [(n0, (None,), hist[n0]), (n1, (buf,), hist[n1])])
            begin(ctx, size, 4)
            ctx.temporal_accumulate(None)
            ctx.temporal_antilag(None)
            assert np.all(ctx.download_temporal_fast()[..., 3] <= 1.0)
            begin(ctx, size, 5)
            ctx.temporal_accumulate(None)
            ctx.temporal_antilag(None)
            assert ctx.download_temporal_fast()[..., 3].max() == 2.0
        # a frame of another size
        begin(ctx, (w // 2, h), 6)
        ctx.temporal_accumulate(None)
        ctx.temporal_antilag(None)
        assert ctx.download_temporal_fast().shape == (h, w // 2, 4) and np.all(ctx.download_temporal_fast()[..., 3] <= 1.0)
        # fast_history 1 and max_history below fast_history: the cap is the smaller of the two
        for k, (tp, al, cap) in enumerate(((None, abi.antilag(fast_history=1), 1.0), (abi.temporal(max_history=2), abi.antilag(fast_history=9), 2.0),
                                           (abi.temporal(max_history=2), abi.antilag(fast_history=9), 2.0))):
            begin(ctx, (w // 2, h), 7 + k)
            ctx.temporal_accumulate(tp)
            ctx.temporal_antilag(al)
            assert ctx.download_temporal_fast()[..., 3].max() == cap


# ---- quality ------------------------------------------------------------------------------------------------------------------------------
QUALITY_TESTS = ("test_a_dimmed_light_is_forgotten_sooner", "test_the_clamped_history_is_less_noisy_than_the_fast_one")


def write_quality(name, text):
    """profiles/antilag_quality.txt holds one section per quality test, each headed by the test's id: a test replaces its own section
    and keeps the other's, so either may run alone."""
    path = os.path.join(ROOT, "profiles", "antilag_quality.txt")
    head = "tests/test_gpu_antilag.py::"
    sections = {}
    if os.path.exists(path):
        with open(path) as fh:
            for part in fh.read().split(head)[1:]:
                sections[part.split(" ", 1)[0]] = part.rstrip("\n") + "\n"
    sections[name] = text.rstrip("\n") + "\n"
    with open(path, "w") as fh:
        fh.write("\n".join(head + sections[k] for k in QUALITY_TESTS if k in sections))


def run_frames(ctx, size, first, count, antilag):
    for k in range(count):
        begin(ctx, size, first + k)
        ctx.temporal_accumulate(None)
        if antilag:
            ctx.temporal_antilag(None)


def test_a_dimmed_light_is_forgotten_sooner(cornell):
    """The reason for the feature.  Cornell box 64 x 64, unmoved camera, every default, sixteen 1-spp frames; gsp_update_tables with every
    light's radiance x 0.25; four more frames.  The MSE of gsp_download_temporal_image against the same context's own 4096-spp frame of
    the edited scene is lower with the anti-lag on every frame than without: without it the four frames still carry 0.8^4 = 41 % of the
    old lighting."""
    import copy

    import gpuspectral_amd as g

    W = H = 64
    dim = copy.copy(cornell)
    lights = cornell.lights.copy()
    lights["radiance"][:, :3] *= np.float32(0.25)
    dim.lights = lights
    res = {}
    with g.Context(0) as ctx:
        ctx.upload_scene(cornell)
        for al in (False, True):
            ctx.update_tables(cornell)
            ctx.temporal_reset()
            run_frames(ctx, (W, H), 5000, 16, al)
            ctx.update_tables(dim)
            run_frames(ctx, (W, H), 5016, 4, al)
            res[al] = ctx.download_temporal_image().astype(np.float64)[..., :3]
        ctx.frame_begin(W, H)
        ctx.render(4096, 0)
        ref = ctx.download().astype(np.float64)[..., :3]
    mse = {al: float(((res[al] - ref) ** 2).mean()) for al in res}
    write_quality(QUALITY_TESTS[0],
                  QUALITY_TESTS[0] + " -- Cornell box 64 x 64, unmoved camera, every default, sixteen 1-spp frames, every light's radiance x 0.25\n"
                  "(gsp_update_tables), four more frames; MSE of gsp_download_temporal_image against the context's own 4096-spp frame of the edited scene.\n\n"
                  "no anti-lag   %.6f\nanti-lag      %.6f\nordering (anti-lag < none): %s\n" % (mse[False], mse[True], mse[True] < mse[False]))
    print("MSE four frames after the edit: no anti-lag %.6f, anti-lag %.6f" % (mse[False], mse[True]))
    assert mse[True] < mse[False]


def test_the_clamped_history_is_less_noisy_than_the_fast_one(cornell):
    """The price.  The same scene without an edit, sixteen 1-spp frames, against the committed 4096-spp image: the long history under the
    anti-lag has a lower MSE than the fast history alone -- the clamp does not make it as noisy as the short one.  The ratio to the MSE
    without the anti-lag (how often one-sample noise clamps a converged pixel) is written beside it and not asserted."""
    import gpuspectral_amd as g

    W = H = 64
    ref = np.load(os.path.join(GOLDEN, "cornell_64_4096spp.npy")).astype(np.float64).reshape(H, W, 3)
    mse = lambda x: float(((np.asarray(x, np.float64)[..., :3] - ref) ** 2).mean())
    with g.Context(0) as ctx:
        ctx.upload_scene(cornell)
        run_frames(ctx, (W, H), 5000, 16, False)
        plain = mse(ctx.download_temporal_image())
        ctx.temporal_reset()
        run_frames(ctx, (W, H), 5000, 16, True)
        clamped, fast = mse(ctx.download_temporal_image()), mse(ctx.download_temporal_fast())
        lengths = ctx.download_temporal()[..., 3]
    write_quality(QUALITY_TESTS[1],
                  QUALITY_TESTS[1] + " -- Cornell box 64 x 64, unmoved camera, every default, sixteen 1-spp frames, no edit; MSE against\n"
                  "tests/golden/cornell_64_4096spp.npy.\n\n"
                  "history, no anti-lag        %.6f\nhistory under the anti-lag  %.6f   (x %.3f of the line above; mean history length %.2f of 16)\n"
                  "fast history alone          %.6f\nordering (clamped history < fast history): %s\n" % (plain, clamped, clamped / plain, lengths.mean(), fast, clamped < fast))
    print("MSE: history %.6f, clamped history %.6f (x %.3f), fast history %.6f" % (plain, clamped, clamped / plain, fast))
    assert clamped < fast


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
    for ts in range(3):
        ctx.frame_begin(W, H)
        ctx.frame_sample_base(ts)
        ctx.render(1, ts)
        ctx.render_features(1, ts)
        ctx.temporal_accumulate(None)
        ctx.temporal_antilag(None)
        off = ts  # floats: only the first destination is 16-byte aligned
        want = ctx.download_temporal_fast().reshape(-1)
        assert want.reshape(-1, 4)[:, 3].max() == ts + 1.0
        t = torch.zeros(N + 8, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        ctx.temporal_fast_to_device(t[off:off + N])
        back = t.cpu().numpy()
        assert np.array_equal(back[off:off + N].view(np.uint32), want.view(np.uint32)) and not back[:off].any() and not back[off + N:].any()
    t = torch.zeros(N, dtype=torch.float32, device="cuda:0")
    try:
        ctx.temporal_fast_to_device(t.data_ptr(), N * 4 - 4)
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
    """The C++ host layer: PathTracer::temporalAntilag / downloadTemporalFast."""
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
            pt.temporal_accumulate(None)
            with pytest.raises(Exception, match="gsp_temporal_antilag call"):
                pt.download_temporal_fast()
            pt.temporal_antilag(abi.antilag(fast_history=2) if k else None)
            fast, hist = pt.download_temporal_fast(), pt.download_temporal()
            assert fast[..., 3].max() == min(k + 1.0, 2.0) and np.isfinite(fast).all() and hist[..., 3].max() == k + 1.0
            with pytest.raises(Exception, match="clamped already"):
                pt.temporal_antilag(None)
            pt.temporal_svgf_feedback(None, abi.svgf(min_history=2), 1, out=False)
        with pytest.raises(Exception, match="gsp_antilag.radius"):
            pt.temporal_antilag(abi.antilag(radius=7))
        pt.next_frame()  # a frame whose feedback comes first
        pt.render(sc, 1)
        pt.render_features(sc, 1)
        pt.temporal_accumulate(None)
        pt.temporal_svgf_feedback(None, abi.svgf(min_history=2), 1, out=False)
        with pytest.raises(Exception, match="fed back already"):
            pt.temporal_antilag(None)
    finally:
        pt.close()


def test_cli(tmp_path):
    """--temporal-antilag with its three options on the Cornell XML at 64 x 48 for four frames, before a feedback: finite files and the
    log lines."""
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
    out = run(["--temporal", str(t / "t.pfm"), "--temporal-frames", "4", "--temporal-antilag", "--antilag-fast", "3", "--antilag-radius", "1", "--antilag-sigma", "1.5",
               "--svgf", str(t / "s.pfm"), "--svgf-feedback", "1"] + tail)
    assert "temporal: 4 frames" in out and "temporal antilag: the history clamped" in out and "mean fast history length 3.00" in out and "svgf feedback:" in out
    hist, filt = pfm(t / "t.pfm"), pfm(t / "s.pfm")
    assert hist.shape == filt.shape == (H, W, 3) and np.isfinite(hist).all() and np.isfinite(filt).all() and hist.max() > 0.1
    plain = run(["--temporal", str(t / "p.pfm"), "--temporal-frames", "4"] + tail)
    assert "temporal antilag" not in plain and not np.array_equal(pfm(t / "p.pfm"), hist)
