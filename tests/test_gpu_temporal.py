"""Temporal accumulation on the GPU (include/gpuspectral_pt.h, "Temporal accumulation"): k_temporal_reproject against the same text
run on the host (csrc/pt_temporal.h through tests/emu/temporal_emu.cpp, itself checked against a float64 restatement in
tests/test_temporal_cpu.py).  gsp_download_temporal equals the emulation applied to gsp_download + gsp_download_features + the
previous emulated history BIT FOR BIT, frame after frame."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import temporal_util as tu
from conftest import ROOT
from denoise_util import DenoiseEmu
from display_util import DisplayEmu
from temporal_util import FLT_MIN, TemporalEmu, refusals, same

pytestmark = pytest.mark.gpu

TENT = 2
LENS = dict(radius=0.08, focus_distance=5.0, blades=0, rotation=0.0)
# six frames on an orbit of 2 degrees per frame, a jump of 40 degrees that disoccludes most of the frame, two more frames
ORBIT = [0.0, 2.0, 4.0, 6.0, 8.0, 10.0, 50.0, 52.0, 54.0]


@pytest.fixture(scope="module")
def emu():
    return TemporalEmu()


@pytest.fixture(scope="module")
def demu():
    return DenoiseEmu()


@pytest.fixture(scope="module")
def scenes_(cornell, materials_scene):
    return {"cornell": cornell, "materials": materials_scene}


@pytest.fixture(scope="module")
def rigs(scenes_):
    """Per scene: one context with the scene uploaded, shared by the cases below."""
    import gpuspectral_amd as g

    made = {}

    def get(name):
        if name not in made:
            made[name] = g.Context(0)
            made[name].upload_scene(scenes_[name])
        ctx = made[name]
        ctx.set_lens()
        ctx.update_camera(scenes_[name].to_world, scenes_[name].fov)
        ctx.temporal_reset()
        return ctx

    yield get
    for ctx in made.values():
        ctx.close()


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def frame(ctx, emu, hist, cam, fov, size, ts, temporal=None, spp=1, filt=0, accum=None, adaptive=None, what=""):
    """One frame of the viewer loop under camera `cam`, accumulated on the GPU and by the emulation from `hist`: the new emulated
    History after the bit-for-bit comparison."""
    ctx.update_camera(cam, fov)
    ctx.frame_begin(*size)
    if adaptive:  # (an adaptive frame counts its samples from timestamp 0)
        ctx.render(spp=spp, first_timestamp=0, **adaptive)
    else:  # new random numbers in every frame, and the frame's record is the plain mean of its own samples
        ctx.frame_sample_base(ts * spp)
        ctx.render(spp, ts * spp, pixel_filter=filt)
    ctx.render_features(1 if adaptive else spp, 0 if adaptive else ts * spp, pixel_filter=filt)
    if accum is not None:
        ctx.upload_accum(accum(ctx.download_compact().copy()))
    ctx.temporal_accumulate(temporal)
    c = ctx.download()
    a, g, i = ctx.download_features()
    new = emu.step(temporal, cam, fov, c, a, g, i, hist)
    got = ctx.download_temporal()
    bad = int((words(got) != words(new.H)).sum())
    assert bad == 0, "%s: %d of %d words of the history differ" % (what, bad, got.size)
    return new


def orbit(sc, degrees):
    return [tu.rotated_about_y(sc.to_world, d, pivot=(0.0, 1.0, 0.0)) for d in degrees]


def sequence(ctx, emu, sc, size, degrees=ORBIT, temporal=None, what="", **kw):
    hist, lens = None, []
    for k, cam in enumerate(orbit(sc, degrees)):
        hist = frame(ctx, emu, hist, cam, sc.fov, size, k, temporal, what="%s frame %d" % (what, k), **kw)
        lens.append(float(hist.H[..., 3].mean()))
    return hist, lens


def test_cornell_orbit_and_the_denoised_history(rigs, emu, demu, scenes_):
    from gpuspectral_amd import abi

    ctx, sc = rigs("cornell"), scenes_["cornell"]
    hist = None
    lens = []
    for k, cam in enumerate(orbit(sc, ORBIT)):
        hist = frame(ctx, emu, hist, cam, sc.fov, (96, 64), k, what="cornell frame %d" % k)
        lens.append(float(hist.H[..., 3].mean()))
        a, g, _ = ctx.download_features()
        for d in (None, abi.denoise(iterations=3)) if k in (0, 5, 6, 8) else (None,):
            assert same(ctx.download_temporal_denoised(d), demu.run(d, hist.H, a, g)), "denoised history, frame %d" % k
    print("mean history length per frame:", ["%.2f" % v for v in lens])
    assert lens[0] == 1.0 and lens[5] > 4.0 and lens[6] < lens[5] - 1.0 and lens[8] > lens[6]  # it builds up, the jump disoccludes, it recovers


@pytest.mark.parametrize("size", [(33, 17), (5, 3), (1, 1)])
def test_materials_scene(rigs, emu, scenes_, size):
    sequence(rigs("materials"), emu, scenes_["materials"], size, what="materials %dx%d" % size)


@pytest.mark.parametrize("scene", ["cornell", "materials"])
def test_ragged_tiles_and_reprojections_that_leave_the_frame(rigs, emu, scenes_, scene):
    """300 x 200: ten tiles of 32 across (the last one 12 wide), 25 of 8 down; the turns push the reprojection out on the left and on
    the right, the last two cameras also move up and down."""
    sc = scenes_[scene]
    ctx = rigs(scene)
    cams = orbit(sc, [0.0, 3.0, -4.0, 9.0])
    up = cams[-1].copy()
    up[13] += 0.4
    down = up.copy()
    down[13] -= 0.9
    hist = None
    for k, cam in enumerate(cams + [up, down]):
        hist = frame(ctx, emu, hist, cam, sc.fov, (300, 200), k, what="%s 300x200 frame %d" % (scene, k))
    assert hist.H[..., 3].max() > 3.0 and (hist.H[..., 3] == 1.0).any()


@pytest.mark.parametrize("scene,size,kw", [("cornell", (96, 64), dict(filt=TENT, spp=2)), ("materials", (33, 17), dict(filt=TENT, spp=2)),
                                           ("cornell", (96, 64), dict(lens=LENS, spp=2)),
                                           ("cornell", (64, 48), dict(adaptive=dict(adaptive_threshold=0.05), spp=32))],
                         ids=["cornell-tent", "materials-tent", "cornell-lens", "cornell-adaptive"])
def test_filtered_defocused_and_adaptive_inputs(rigs, emu, scenes_, scene, size, kw):
    """Fractional coverage at silhouettes (n and z are divided by it, pixels under one half are background), a lens, an adaptive
    frame: the history is what the emulation makes of the same planes."""
    ctx = rigs(scene)
    lens = kw.pop("lens", None)
    try:
        if lens:
            ctx.set_lens(**lens)
        sequence(ctx, emu, scenes_[scene], size, degrees=[0.0, 2.0, 4.0, 30.0], what="%s %s" % (scene, sorted(kw)), **kw)
        if "adaptive" in kw:
            assert ctx.stats()["adaptive_rounds"] > 0
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
    for k, cam in enumerate(orbit(sc, [0.0, 2.0, 2.0, 4.0])):
        hist = frame(ctx, emu, hist, cam, sc.fov, (W, H), k, accum=spoil if k != 2 else None, what="NaN / Inf frame %d" % k)
    assert (hist.H[..., 3] == 0.0).sum() + (hist.H[..., 3] > 1.0).sum() > 0
    assert np.isfinite(hist.H[..., :3][hist.H[..., 3] > 0]).all()  # a pixel with a history length has a finite history


def test_unmoved_camera_is_the_running_mean(rigs, emu, scenes_):
    """Eight frames at timestamps 0 .. 7 with alpha = FLT_MIN: len == 8 everywhere, and the history is one 8-spp frame of the same
    timestamps to within the bound tests/test_temporal_cpu.py derives for the running mean (here with the frame's own range)."""
    from gpuspectral_amd import abi

    ctx, sc = rigs("cornell"), scenes_["cornell"]
    t = abi.temporal(alpha=FLT_MIN, max_history=64)
    hist, frames = None, []
    for k in range(8):
        hist = frame(ctx, emu, hist, sc.to_world, sc.fov, (96, 64), k, t, what="unmoved frame %d" % k)
        frames.append(ctx.download()[..., :3].astype(np.float64))
        assert np.all(hist.H[..., 3] == np.float32(k + 1))
    ctx.frame_begin(96, 64)  # (no base: timestamps 0 .. 7 folded as samples 0 .. 7)
    ctx.render(8, 0)
    eight = ctx.download()[..., :3].astype(np.float64)
    R = np.max(frames, 0)  # per pixel and channel: the largest sample (all are >= 0)
    bound = sum(3.0 / k + 1.0 for k in range(1, 9)) * tu.U32 * R
    # the 8-spp frame is itself a float32 running mean of the same samples with the same per-step error bound
    ok = R > 0
    print("largest |H - mean| / bound %.3f, |8 spp - mean| / bound %.3f, |H - 8 spp| / bound %.3f"
          % tuple(float((np.abs(p - q)[ok] / bound[ok]).max()) for p, q in ((hist.H[..., :3], np.mean(frames, 0)), (eight, np.mean(frames, 0)), (hist.H[..., :3], eight))))
    assert np.all(np.abs(hist.H[..., :3] - np.mean(frames, 0)) <= bound) and np.all(np.abs(hist.H[..., :3] - eight) <= bound)


def test_frame_sample_base(scenes_):
    """A frame of timestamps 5 .. 7 with sample base 5 is the plain mean of those three samples: with the frame of timestamps
    0 .. 4 it makes up the frame of timestamps 0 .. 7, (5 C + 3 A) / 8 = B, to within the roundings of three running means (each
    within sum_k (3 / k + 1) u of its range, see tests/test_temporal_cpu.py) -- and without the base the same frame is darker by 3 / 8."""
    import gpuspectral_amd as g

    w, h = 64, 48
    with g.Context(0) as ctx:
        ctx.upload_scene(scenes_["cornell"])
        with pytest.raises(g.GspError, match="gsp_frame_begin"):
            ctx.frame_sample_base(3)

        def render(calls, base=None):
            ctx.frame_begin(w, h)
            if base is not None:
                ctx.frame_sample_base(base)
            for spp, ts in calls:
                ctx.render(spp, ts)
            return ctx.download()[..., :3].astype(np.float64)

        A, B, C5 = render([(3, 5)], base=5), render([(8, 0)]), render([(5, 0)])
        split = render([(1, 5), (2, 6)], base=5)
        assert np.array_equal(split, A)  # the split over calls changes nothing
        dark = render([(3, 5)])
        R = np.maximum(np.maximum(A, B), C5) * 8.0  # no sample of a pixel exceeds eight times its mean of at most eight
        bound = 3 * sum(3.0 / k + 1.0 for k in range(1, 9)) * tu.U32 * R
        assert np.all(np.abs((5 * C5 + 3 * A) / 8 - B) <= bound)
        assert np.all(np.abs(dark - A * 3 / 8) <= bound) and dark.sum() < 0.5 * A.sum()
        assert np.array_equal(render([(3, 0)], base=0), render([(3, 0)]))  # base 0 is the plain frame
        ctx.frame_begin(w, h)
        ctx.frame_sample_base(5)
        with pytest.raises(g.GspError, match="sample base"):
            ctx.render(1, 4)
        with pytest.raises(g.GspError, match="sample base"):
            ctx.render(spp=4, first_timestamp=5, adaptive_threshold=0.05)
        ctx.render(2, 5)
        with pytest.raises(g.GspError, match="first gsp_render"):
            ctx.frame_sample_base(7)
        ctx.sync()
        assert ctx.peek()[1] == 2  # samples folded, counted from the base
        ctx.frame_begin(w, h)  # the base is the frame's: a new frame starts from 0 again
        ctx.render(3, 5)
        assert np.array_equal(ctx.download()[..., :3].astype(np.float64), dark)


def test_a_moved_instance_restarts_where_it_uncovered(rigs, emu, scenes_):
    ctx, sc = rigs("cornell"), scenes_["cornell"]
    size = (96, 64)
    try:
        hist = None
        for k in range(3):
            hist = frame(ctx, emu, hist, sc.to_world, sc.fov, size, k, what="before the move, frame %d" % k)
        before = ctx.download_features()[2][..., 2].copy()
        inst = sc.instances.copy()
        t = inst["transform"][6].copy()
        t[12] += 0.3
        t[14] += 0.2
        inst["transform"][6] = t
        ctx.update_instances(inst)
        hist = frame(ctx, emu, hist, sc.to_world, sc.fov, size, 3, what="after the move")
        after = ctx.download_features()[2][..., 2]
        uncovered = (before == 6) & (after != 6)
        covered = (after == 6) & (before != 6)
        assert uncovered.sum() > 10 and covered.sum() > 10
        assert np.all(hist.H[..., 3][uncovered] == 1.0) and np.all(hist.H[..., 3][covered] == 1.0)
        assert np.all(hist.H[..., 3][(before == after) & (after != 6)] == 4.0)
    finally:
        ctx.update_instances(sc.instances)


def test_frame_state_is_untouched_and_the_history_restarts(scenes_, emu):
    import gpuspectral_amd as g

    sc = scenes_["cornell"]
    w, h = 96, 64
    with g.Context(0) as ctx:
        ctx.upload_scene(sc)
        for call in (ctx.download_temporal, ctx.download_temporal_denoised, ctx.download_temporal_denoised_display):
            with pytest.raises(g.GspError, match="gsp_temporal_accumulate"):
                call()  # before any accumulate
        assert ctx._L.gsp_temporal_to_device(ctx._h, 16, 1 << 30) == 1 and "gsp_temporal_accumulate" in ctx._L.gsp_last_error(ctx._h).decode()
        ctx.frame_begin(w, h)
        kw = dict(adaptive_threshold=0.05, adaptive_min_spp=4, adaptive_step=4)
        ctx.render(8, 0, **kw)
        ctx.render_features(2, 0, pixel_filter=TENT)
        bytes0 = ctx.stats()["device_bytes"]
        state = lambda: (ctx.download(), ctx.download_features(), ctx.pixel_stats(), ctx.stats())
        s0 = state()
        ctx.temporal_accumulate(None)
        s1 = state()
        assert same(s0[0], s1[0]) and all(np.array_equal(words(p), words(q)) for p, q in zip(s0[1], s1[1]))
        assert same(s0[2][0], s1[2][0]) and np.array_equal(s0[2][1], s1[2][1])
        skip = ("render_seconds", "extend_kernel_ms", "shade_kernel_ms", "connect_kernel_ms", "bvh_build_ms", "device_bytes")
        assert all(s1[3][k] == v for k, v in s0[3].items() if k not in skip)
        assert s1[3]["device_bytes"] == bytes0 + 72 * w * h  # two sets of H, G (16 bytes) and I (4 bytes)
        with pytest.raises(g.GspError, match="already"):
            ctx.temporal_accumulate(None)  # a second accumulate in the same frame
        first = ctx.download_temporal()
        assert np.all(first[..., 3] == 1.0) and same(first[..., :3], s0[0][..., :3])

        def one(ts, size=(w, h)):
            ctx.frame_begin(*size)
            ctx.frame_sample_base(ts)
            ctx.render(1, ts)
            ctx.render_features(1, ts)
            ctx.temporal_accumulate(None)
            return ctx.download_temporal()[..., 3]

        # (the first frame's planes were tent-filtered: at silhouettes its mean depth and normal are not the pinhole frame's)
        second, third = one(8), one(9)
        assert (second == 2.0).mean() > 0.9 and np.all((second == 1.0) | (second == 2.0)) and np.all(third == second + 1.0)
        ctx.temporal_reset()
        with pytest.raises(g.GspError, match="gsp_temporal_accumulate"):
            ctx.download_temporal()
        assert np.all(one(10) == 1.0) and np.all(one(11) == 2.0)
        ctx.upload_scene(sc)  # a new scene has no history
        assert np.all(one(12) == 1.0) and np.all(one(13) == 2.0)
        assert np.all(one(14, (w, h - 8)) == 1.0) and np.all(one(15, (w, h - 8)) == 2.0)  # another size


_TORCH_CHILD = """
import sys
import torch  # first: the tracer's library then binds to the HIP runtime torch has loaded (see bench.py)
import numpy as np
sys.path.insert(0, sys.argv[1])
import gpuspectral_amd as g
from gpuspectral_amd import scenes
W, H = 96, 64
with g.Context(0) as ctx:
    ctx.upload_scene(scenes.cornell_materials(8))
    for ts in range(2):
        ctx.frame_begin(W, H)
        ctx.frame_sample_base(ts)
        ctx.render(1, ts)
        ctx.render_features(1, ts)
        ctx.temporal_accumulate(None)
    want = ctx.download_temporal().reshape(-1)
    assert (want[3::4] == 2.0).all()
    for off in (0, 1):  # floats: the second destination is not 16-byte aligned
        t = torch.zeros(W * H * 4 + 8, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        ctx.temporal_to_device(t.data_ptr() + 4 * off, W * H * 16)
        back = t.cpu().numpy()
        assert np.array_equal(back[off:off + W * H * 4].view(np.uint32), want.view(np.uint32)) and not back[:off].any() and not back[off + W * H * 4:].any()
    t = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda:0")
    try:
        ctx.temporal_to_device(t.data_ptr(), W * H * 16 - 4)
        raise SystemExit("a destination of the wrong size was accepted")
    except g.GspError as e:
        assert "destination too small" in str(e), e
    assert not t.cpu().numpy().any()
print("torch tensor ok")
"""


def test_temporal_to_device_torch_tensor():
    """Into a torch tensor, in a process of its own: torch has to be imported before the library is loaded (bench.py does the same)."""
    r = subprocess.run([sys.executable, "-c", _TORCH_CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "torch tensor ok" in r.stdout, r.stdout + r.stderr


def test_download_temporal_denoised_display(rigs, emu, demu, scenes_):
    """The LDR film of the filtered history, statistics included: byte for byte the display emulation of the denoised history."""
    from gpuspectral_amd import abi

    ctx, sc = rigs("cornell"), scenes_["cornell"]
    hist, _ = sequence(ctx, emu, sc, (96, 64), degrees=[0.0, 2.0, 4.0], what="display")
    a, g, _ = ctx.download_features()
    dn = abi.denoise(iterations=3)
    den = demu.run(dn, hist.H, a, g)
    for name, d in (("clamp", abi.display()), ("aces", abi.display(tonemap=abi.TONEMAP_ACES)), ("reinhard measured", abi.display(tonemap=abi.TONEMAP_REINHARD)),
                    ("NULL", None)):
        got = ctx.download_temporal_denoised_display(dn, d)
        assert np.array_equal(got.reshape(-1), DisplayEmu().map(d, den.reshape(-1, 4))), name


def test_validation(scenes_):
    import gpuspectral_amd as g
    from gpuspectral_amd import abi

    with g.Context(0) as ctx:
        with pytest.raises(g.GspError, match="gsp_frame_begin"):
            ctx.temporal_accumulate(None)  # no frame
        ctx.upload_scene(scenes_["cornell"])
        # the order of the refusals, two broken conditions per call (temporal_util.refusals): first without a frame and a history ...
        buf = np.zeros((16, 16, 4), np.float32).ctypes.data
        bad_dn, tone, badt = C.byref(abi.denoise(iterations=9)), C.byref(abi.display(tonemap=7)), C.byref(abi.temporal(max_history=65537))
        acc = "gsp_temporal_accumulate"
        names = ("gsp_download_temporal", "gsp_temporal_to_device", "gsp_download_temporal_denoised", "gsp_download_temporal_denoised_display")
        null, hist, full = (dict((n, n + t) for n in names) for t in (
            ": null output pointer", " needs a gsp_temporal_accumulate call since the history was last invalidated",
            " needs a full frame (no pixel_ids) and a gsp_render_features call since gsp_frame_begin"))
        n0, n1, n2, n3 = names
        refusals(ctx, [(acc, (badt,), acc + " needs gsp_frame_begin first"), (n0, (None,), null[n0]), (n1, (None, 0), null[n1]), (n1, (16, 0), hist[n1]),
                       (n2, (bad_dn, None), null[n2]), (n2, (bad_dn, buf), hist[n2]), (n3, (None, tone, None), "tonemap"), (n3, (bad_dn, None, None), null[n3]),
                       (n3, (bad_dn, None, buf), hist[n3])])
        # ... then the accumulate in a share's frame and in a full one, both without a feature pass ...
        ctx.frame_begin(16, 16, pixel_ids=g.pt.tile_partition(16, 16, 0, 2))
        refusals(ctx, [(acc, (badt,), acc + ": the frame was begun with pixel_ids; a share has no neighbours and there is no multi-GPU variant")])
        ctx.frame_begin(16, 16)
        ctx.render(1)
        refusals(ctx, [(acc, (badt,), acc + " needs a gsp_render_features call since gsp_frame_begin")])
        # ... then with a history: in its frame, in the next one before the feature pass, and in a share's frame after one
        ctx.render_features(1)
        ctx.temporal_accumulate(None)
        refusals(ctx, [(acc, (badt,), acc + ": the frame has been accumulated already (one call per gsp_frame_begin)"),
                       (n2, (bad_dn, buf), "iterations"), (n3, (bad_dn, tone, buf), "tonemap"), (n3, (bad_dn, None, buf), "iterations")])
        ctx.frame_begin(16, 16)
        refusals(ctx, [(n2, (bad_dn, buf), full[n2]), (n3, (bad_dn, None, buf), full[n3])])
        ctx.frame_begin(16, 16, pixel_ids=g.pt.tile_partition(16, 16, 0, 2))
        ctx.render_features(1)
        refusals(ctx, [(n2, (bad_dn, buf), full[n2]), (n3, (bad_dn, None, buf), full[n3])])
        ctx.temporal_reset()
        ctx.frame_begin(16, 16)
        ctx.render(1)
        with pytest.raises(g.GspError, match="gsp_render_features"):
            ctx.temporal_accumulate(None)  # no feature pass in this frame
        ctx.download_features()  # (a download allocates the planes; it is not a feature pass)
        with pytest.raises(g.GspError, match="gsp_render_features"):
            ctx.temporal_accumulate(None)
        ctx.render_features(1)
        for bad, word in ((abi.temporal(max_history=65537), "max_history"), (abi.temporal(alpha=1.5), "alpha"), (abi.temporal(alpha=float("nan")), "alpha"),
                          (abi.temporal(depth_tolerance=-0.5), "depth_tolerance"), (abi.temporal(normal_min=2.0), "normal_min")):
            with pytest.raises(g.GspError, match=word):
                ctx.temporal_accumulate(bad)
        ctx.temporal_accumulate(abi.temporal(alpha=FLT_MIN))
        assert ctx._L.gsp_download_temporal(ctx._h, None) == 1 and "null output" in ctx._L.gsp_last_error(ctx._h).decode()
        assert ctx._L.gsp_temporal_to_device(ctx._h, None, 1 << 20) == 1 and "null output" in ctx._L.gsp_last_error(ctx._h).decode()
        with pytest.raises(g.GspError, match="iterations"):
            ctx.download_temporal_denoised(abi.denoise(iterations=9))
        with pytest.raises(g.GspError, match="tonemap"):
            ctx.download_temporal_denoised_display(None, abi.display(tonemap=7))
        ctx.download_temporal_denoised(None)
        ctx.frame_begin(16, 16)  # a new frame of the same size: the history stays, the feature planes are stale
        assert np.all(ctx.download_temporal()[..., 3] == 1.0)
        with pytest.raises(g.GspError, match="gsp_render_features"):
            ctx.download_temporal_denoised(None)
        ctx.frame_begin(16, 16, pixel_ids=g.pt.tile_partition(16, 16, 0, 2))
        ctx.render_features(1)
        with pytest.raises(g.GspError, match="pixel_ids"):
            ctx.temporal_accumulate(None)
        # a singular camera is refused by the accumulate that would reproject into it
        ctx.frame_begin(16, 16)
        ctx.render(1)
        ctx.render_features(1)
        flat = np.asarray(scenes_["cornell"].to_world, np.float32).copy()
        good = flat.copy()
        flat[8:11] = 0.0
        ctx.update_camera(flat, scenes_["cornell"].fov)  # (after the frame's rays: nothing is traced through this camera)
        ctx.temporal_accumulate(None)  # the history now belongs to the singular camera
        ctx.update_camera(good, scenes_["cornell"].fov)
        ctx.frame_begin(16, 16)
        ctx.render(1)
        ctx.render_features(1)
        refusals(ctx, [(acc, (badt,), "max_history")])  # (the parameters before the cameras)
        with pytest.raises(g.GspError, match="singular"):
            ctx.temporal_accumulate(None)
        ctx.temporal_reset()
        ctx.temporal_accumulate(None)


def test_host_layer(emu, demu):
    """The C++ host layer: PathTracer::temporalAccumulate / downloadTemporal / downloadTemporalDenoised."""
    from conftest import CORNELL_XML
    from gpuspectral_amd import abi, host

    W, H = 48, 40
    sc = host.Scene(CORNELL_XML)
    pt = host.PathTracer(W, H)
    try:
        for k in range(3):
            if k:
                pt.next_frame()
            assert pt.timestamp == k
            pt.render(sc, 1)
            pt.render_features(sc, 1)
            pt.temporal_accumulate(None)
            c = pt.download()
            a, g = pt.download_features()
            got = pt.download_temporal()
            assert np.all(got[..., 3] == float(k + 1))
            if k == 0:
                assert same(got[..., :3], c[..., :3])
        den = pt.download_temporal_denoised(abi.denoise(iterations=2))
        assert same(den, demu.run(abi.denoise(iterations=2), got, a, g))
        pt.temporal_reset()
        pt.reset()
        pt.render(sc, 1)
        pt.render_features(sc, 1)
        pt.temporal_accumulate(abi.temporal(alpha=0.5))
        assert np.all(pt.download_temporal()[..., 3] == 1.0)
    finally:
        pt.close()


def test_cli_temporal(tmp_path):
    """--temporal-frames N --temporal-orbit DEG --temporal out.pfm: the last frame's history (and with --denoise its filtered form);
    N = 1 is the plain frame at --spp."""
    from oracle import mitsuba_loader as ml
    from conftest import CORNELL_XML

    lib = os.path.join(ROOT, "gpuspectral_amd", "lib")
    env = dict(os.environ, LD_LIBRARY_PATH=lib + ":" + os.environ.get("LD_LIBRARY_PATH", ""))

    def run(args):
        r = subprocess.run([os.path.join(lib, "gsp_render")] + args, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return r.stdout

    W, H, S = 64, 48, 2
    t = tmp_path
    pfm = lambda path: np.asarray(ml.read_pfm(str(path)), np.float32).reshape(H, W, -1)[::-1, :, :3]
    one = run(["--temporal", str(t / "a.t.pfm"), "--temporal-frames", "1", CORNELL_XML, str(t / "a.pfm"), str(W), str(H), str(S)])
    assert "temporal: 1 frame" in one and same(pfm(t / "a.t.pfm"), pfm(t / "a.pfm"))
    five = run(["--temporal", str(t / "b.t.pfm"), "--temporal-frames", "5", "--temporal-orbit", "2", "--denoise", str(t / "b.dn.pfm"), CORNELL_XML,
                str(t / "b.pfm"), str(W), str(H), str(S)])
    assert "temporal: 5 frames" in five and "mean history length" in five
    assert sorted(os.listdir(str(t))) == ["a.pfm", "a.pfm.ppm", "a.t.pfm", "b.dn.pfm", "b.pfm", "b.pfm.ppm", "b.t.dn.pfm", "b.t.pfm"]
    acc, last = pfm(t / "b.t.pfm"), pfm(t / "b.pfm")
    assert np.isfinite(acc).all() and not same(acc, last)
    # the history of five frames is smoother than the last frame alone: mean squared difference of horizontal neighbours
    rough = lambda img: float(((img[:, 1:] - img[:, :-1]) ** 2).mean())
    assert rough(np.minimum(acc, 1.0)) < rough(np.minimum(last, 1.0))
