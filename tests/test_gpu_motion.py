"""Moved instances on the GPU (include/gpuspectral_pt.h, "Temporal accumulation: moved instances"): k_temporal_reproject_follow against
the same text run on the host (csrc/pt_motion.h through tests/emu/motion_emu.cpp, itself checked against a float64 restatement in
tests/test_motion_cpu.py).  gsp_download_temporal, the moments plane and gsp_download_temporal_motion equal the emulation applied to
gsp_download + gsp_download_features + the previous emulated history + the two transform arrays BIT FOR BIT, frame after frame."""
import os
import subprocess
import sys

import numpy as np
import pytest

import motion_util as mu
import temporal_util as tu
from conftest import ROOT
from motion_util import MotionEmu
from svgf_util import SvgfEmu
from temporal_util import refusals, same

pytestmark = pytest.mark.gpu

# six frames on an orbit of 2 degrees per frame, a jump of 40 degrees that disoccludes most of the frame, two more frames
ORBIT = [0.0, 2.0, 4.0, 6.0, 8.0, 10.0, 50.0, 52.0, 54.0]
MOVERS = {"cornell": (6,), "materials": (7, 8)}  # the tall box; a sphere and the plastic box


@pytest.fixture(scope="module")
def emu():
    return MotionEmu()


@pytest.fixture(scope="module")
def scenes_(cornell, materials_scene):
    return {"cornell": cornell, "materials": materials_scene}


@pytest.fixture(scope="module")
def rigs(scenes_):
    """Per scene: one context with the scene uploaded and following on, shared by the cases below."""
    import gpuspectral_amd as g

    made = {}

    def get(name, moments=False):
        if name not in made:
            made[name] = g.Context(0)
            made[name].upload_scene(scenes_[name])
            made[name].temporal_follow_instances(True)
        ctx = made[name]
        ctx.set_lens()
        ctx.update_camera(scenes_[name].to_world, scenes_[name].fov)
        ctx.update_instances(scenes_[name].instances)
        ctx.temporal_track_moments(moments)
        ctx.temporal_reset()
        return ctx

    yield get
    for ctx in made.values():
        ctx.close()


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def orbit(sc, degrees):
    return [tu.rotated_about_y(sc.to_world, d, pivot=(0.0, 1.0, 0.0)) for d in degrees]


def moved_instances(inst, movers, k):
    """The scene's instances at frame k: each mover turned by 7 k degrees about a tilted axis through its own origin and shifted."""
    out = inst.copy()
    for j, m in enumerate(movers):
        t = inst["transform"][m]
        out["transform"][m] = mu.moved(t, mu.rotation((0.2, 1.0, 0.1 * (j + 1)), 7.0 * k), mu.affine(t)[1], (0.03 * k, 0.01 * k * (j + 1), -0.04 * k))
    return out


def frame(ctx, emu, hist, cam, fov, size, ts, inst, moments=False, what=""):
    """One frame of the viewer loop: the instance edit, the camera, the frame, its feature pass, the followed accumulate -- on the
    GPU and by the emulation from `hist`.  Returns the new emulated FHistory after the bit-for-bit comparison."""
    ctx.update_instances(inst)  # (before the frame's feature pass, as following asks)
    ctx.update_camera(cam, fov)
    ctx.frame_begin(*size)
    ctx.frame_sample_base(ts)
    ctx.render(1, ts)
    ctx.render_features(1, ts)
    ctx.temporal_accumulate(None)
    c = ctx.download()
    a, g, i = ctx.download_features()
    new = emu.step(None, cam, fov, c, a, g, i, inst["transform"], hist=hist, moments=moments)
    planes = [("H", ctx.download_temporal(), new.H), ("V", ctx.download_temporal_motion(), new.V)]
    if moments:
        planes.append(("M", ctx.download_temporal_moments(), new.M))
    for name, got, want in planes:
        bad = int((words(got) != words(want)).sum())
        assert bad == 0, "%s: %d of %d words of %s differ" % (what, bad, got.size, name)
    return new


def sequence(ctx, emu, sc, size, movers, degrees=ORBIT, moments=False, what=""):
    """Returns the last emulated history and, per frame, the number of followed pixels (sequence.longest: their longest history)."""
    hist, followed, sequence.longest = None, [], []
    for k, cam in enumerate(orbit(sc, degrees)):
        hist = frame(ctx, emu, hist, cam, sc.fov, size, k, moved_instances(sc.instances, movers, k), moments, "%s frame %d" % (what, k))
        on = hist.V[..., 3] == 2.0
        followed.append(int(on.sum()))
        sequence.longest.append(float(hist.H[..., 3][on].max()) if on.any() else 0.0)
    return hist, followed


# ---- bit for bit against the emulation ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moments", [False, True], ids=["plain", "moments"])
def test_cornell_orbit_with_a_box_translating_and_rotating(rigs, emu, scenes_, moments):
    ctx, sc = rigs("cornell", moments), scenes_["cornell"]
    hist, followed = sequence(ctx, emu, sc, (96, 64), MOVERS["cornell"], moments=moments, what="cornell")
    print("followed pixels per frame:", followed)
    assert followed[0] == 0 and min(followed[1:6]) > 50  # the box is followed on the slow part of the orbit
    assert max(sequence.longest) > 4.0  # ... and its history builds up (after the jump it is out of sight)


@pytest.mark.parametrize("moments", [False, True], ids=["plain", "moments"])
@pytest.mark.parametrize("size", [(33, 17), (5, 3), (1, 1)])
def test_materials_scene(rigs, emu, scenes_, size, moments):
    sequence(rigs("materials", moments), emu, scenes_["materials"], size, MOVERS["materials"], moments=moments, what="materials %dx%d" % size)


@pytest.mark.parametrize("moments", [False, True], ids=["plain", "moments"])
def test_ragged_tiles(rigs, emu, scenes_, moments):
    """300 x 200: ten tiles of 32 across (the last one 12 wide), 25 of 8 down."""
    sc = scenes_["materials"]
    hist, followed = sequence(rigs("materials", moments), emu, sc, (300, 200), MOVERS["materials"], degrees=[0.0, 3.0, -4.0, 9.0], moments=moments,
                              what="materials 300x200")
    assert hist.H[..., 3].max() > 3.0 and (hist.H[..., 3] == 1.0).any() and followed[-1] > 500


# ---- many instances in one wave --------------------------------------------------------------------------------------------------------
NX, NY = 10, 7


def quads_scene():
    """70 small quads in the plane z = 0 facing the camera at (0, 0, 5), a wall behind them and a light behind the camera: at 40 x 24
    a quad is about three pixels wide, so a wave (32 x 2 pixels) sees nine or ten instances and the wall."""
    from gpuspectral_amd import scenes

    b = scenes.SceneBuilder()
    rect = b.add_mesh(*scenes.rect_mesh())
    for j in range(NX * NY):
        x, y = j % NX, j // NX
        b.add_object(rect, scenes.trs(((x - 4.5) * 0.36, (y - 3.0) * 0.3, 0.0), 0.15), b.diffuse((0.3 + 0.07 * x, 0.8 - 0.1 * y, 0.5)))
    b.add_object(rect, scenes.trs((0.0, 0.0, -1.0), 3.0), b.diffuse((0.7, 0.7, 0.7)))
    b.add_object(rect, scenes.trs((0.0, 0.0, 6.0), 2.0, 180.0), b.diffuse((0, 0, 0)), twofaced=True, emission=(6, 6, 6))
    b.camera_lookat((0.0, 0.0, 5.0), (0.0, 0.0, 0.0), fov_deg=40.0)
    return b.build()


def quads_at(sc, k):
    """Frame k: quad j is static when j % 5 == 0; hidden (scaled to nothing) in frame 1 when j % 11 == 3 and in frame 2 when
    j % 11 == 7 -- class 2 in that frame and in the one that shows it again; every other quad turns and shifts its own way."""
    rng = np.random.default_rng(21)
    out = sc.instances.copy()
    for j in range(NX * NY):
        axis, deg, shift = rng.normal(size=3), rng.uniform(-12.0, 12.0), rng.uniform(-0.03, 0.03, 3)
        if j % 5 == 0:
            continue
        t = sc.instances["transform"][j]
        if (j % 11 == 3 and k == 1) or (j % 11 == 7 and k == 2):
            out["transform"][j] = mu.compose(np.zeros((3, 3)), mu.affine(t)[1])
        else:
            out["transform"][j] = mu.moved(t, mu.rotation(axis + (0.0, 0.0, 2.0), deg * k), mu.affine(t)[1], shift * k)
    return out


@pytest.mark.parametrize("moments", [False, True], ids=["plain", "moments"])
def test_many_instances_in_one_wave(emu, moments):
    import gpuspectral_amd as g

    sc = quads_scene()
    size = (40, 24)
    with g.Context(0) as ctx:
        ctx.upload_scene(sc)
        ctx.temporal_follow_instances(True)
        ctx.temporal_track_moments(moments)
        hist = None
        for k in range(4):
            cam = sc.to_world.copy()
            cam[12] += 0.02 * k
            inst = quads_at(sc, k)
            hist = frame(ctx, emu, hist, cam, sc.fov, size, k, inst, moments, "quads frame %d" % k)
            if k:
                cls = mu.split_table(emu.table(quads_at(sc, k - 1)["transform"], inst["transform"]))[0]
                seen = np.unique(hist.I[hist.I < NX * NY])
                print("frame %d: %d quads seen, classes of the seen quads %s" % (k, len(seen), np.bincount(cls[seen], minlength=3)))
                assert (cls[seen] == 0).sum() >= 10 and (cls[seen] == 1).sum() >= 30
                if k >= 2:
                    assert (cls[seen] == 2).sum() >= 3  # the quads shown again
                for c_, v in ((0, 1.0), (1, 2.0)):
                    on = np.isin(hist.I, np.flatnonzero(cls == c_)) & (hist.V[..., 3] != 0)
                    assert on.any() and np.all(hist.V[..., 3][on] == v)
                assert not hist.V[np.isin(hist.I, np.flatnonzero(cls == 2))].any()
        rows = hist.V[..., 3].reshape(size[1] // 2, 2, size[0])[:, :, :32]  # the first wave of every tile row pair
        assert any(len(np.unique(r)) == 3 for r in rows)  # no reprojection, static and followed lanes side by side


# ---- static parity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moments", [False, True], ids=["plain", "moments"])
def test_nothing_moved_equals_following_off(scenes_, moments):
    import gpuspectral_amd as g

    sc = scenes_["cornell"]
    with g.Context(0) as on, g.Context(0) as off:
        for ctx in (on, off):
            ctx.upload_scene(sc)
            ctx.temporal_track_moments(moments)
        on.temporal_follow_instances(True)
        for k, cam in enumerate(orbit(sc, ORBIT)):
            for ctx in (on, off):
                ctx.update_camera(cam, sc.fov)
                ctx.frame_begin(96, 64)
                ctx.frame_sample_base(k)
                ctx.render(1, k)
                ctx.render_features(1, k)
                ctx.temporal_accumulate(None)
            assert same(on.download_temporal(), off.download_temporal()), k
            if moments:
                assert same(on.download_temporal_moments(), off.download_temporal_moments()), k
            v = on.download_temporal_motion()
            assert np.all((v[..., 3] == 1.0) | (v[..., 3] == 0.0)) and (k == 0) == (not v.any())


# ---- a move that crosses the depth tolerance --------------------------------------------------------------------------------------------
def approach_scene():
    """A quad of half size 0.5 facing the camera at (0, 0, 5), a wall behind it and a large light far behind the camera (its solid
    angle changes by under 1 % over the move, so the quad's lighting does not lag).  The quad has no face seen at a grazing angle:
    every tap of a followed pixel that lies on it passes the depth and normal tests."""
    from gpuspectral_amd import scenes

    b = scenes.SceneBuilder()
    rect = b.add_mesh(*scenes.rect_mesh())
    b.add_object(rect, scenes.trs((0.1, -0.05, 0.0), 0.5), b.diffuse((0.6, 0.5, 0.4)))
    b.add_object(rect, scenes.trs((0.0, 0.0, -1.0), 3.0), b.diffuse((0.7, 0.7, 0.7)))
    b.add_object(rect, scenes.trs((0.0, 0.0, 400.0), 120.0, 180.0), b.diffuse((0, 0, 0)), twofaced=True, emission=(6, 6, 6))
    b.camera_lookat((0.0, 0.0, 5.0), (0.0, 0.0, 0.0), fov_deg=40.0)
    return b.build()


def test_depth_crossing_move():
    """The camera stays; a quad moves towards the eye by 4 % of its distance per frame, twice the depth tolerance.  Eight 1-spp
    frames at 64 x 64.  Off: every pixel of the quad restarts on every frame.  On: the pixels the quad covers in all eight frames
    reach length 8 -- to rounding: len = sl / sw is a quotient of two float32 sums of up to four products, at most 8 u relative
    per frame on taps that all hold the same length, so after seven reprojections |len - 8| <= 8 * 64 u (the emulation on the CPU
    gives 8 exactly on 297 of 306 such pixels and 8 - 1 ulp or 8 - 2 ulp on the rest).  The MSE over the quad's pixels against a
    1024-spp frame of the final scene is lower with following on."""
    import gpuspectral_amd as g

    sc = approach_scene()
    BOX, W, H, FRAMES = 0, 64, 64, 8
    eye = np.asarray(sc.to_world, np.float64)[12:15]
    fwd = tu.mat3(sc.to_world) @ np.array([0.0, 0.0, 1.0])
    fwd[1] *= -1.0
    fwd /= np.linalg.norm(fwd)
    insts = [sc.instances.copy()]
    for _ in range(FRAMES - 1):
        nxt = insts[-1].copy()
        t = nxt["transform"][BOX]
        dist = float(np.linalg.norm(mu.affine(t)[1] - eye))
        nxt["transform"][BOX] = mu.moved(t, shift=-0.04 * dist * fwd)  # (fwd: the viewing direction)
        insts.append(nxt)
    result = {}
    with g.Context(0) as ctx:
        ctx.upload_scene(sc)
        for follow in (False, True):
            ctx.temporal_follow_instances(follow)
            ctx.temporal_reset()
            always = np.ones((H, W), bool)
            for k in range(FRAMES):
                ctx.update_instances(insts[k])
                ctx.frame_begin(W, H)
                ctx.frame_sample_base(k)
                ctx.render(1, k)
                ctx.render_features(1, k)
                ctx.temporal_accumulate(None)
                hist = ctx.download_temporal()
                box = ctx.download_features()[2][..., 2] == BOX
                always &= box
                if not follow:
                    assert np.all(hist[..., 3][box] == 1.0), k
            print("following %s: lengths on the %d pixels the box always covers: min %g, mean %.3f; on its %d pixels of the last frame: mean %.3f"
                  % ("on" if follow else "off", always.sum(), hist[..., 3][always].min(), hist[..., 3][always].mean(), box.sum(), hist[..., 3][box].mean()))
            result[follow] = (hist, box, always)
        assert result[True][2].sum() > 100
        assert np.all(np.abs(result[True][0][..., 3][result[True][2]] - float(FRAMES)) <= FRAMES * 64 * tu.U32)
        ctx.temporal_follow_instances(False)
        ctx.frame_begin(W, H)
        ctx.render(1024, 0)
        ref = ctx.download()
    box = result[True][1]
    mse = {f: float(((result[f][0][..., :3][box].astype(np.float64) - ref[..., :3][box]) ** 2).mean()) for f in (False, True)}
    with open(os.path.join(ROOT, "profiles", "motion_quality.txt"), "w") as fh:
        fh.write("tests/test_gpu_motion.py::test_depth_crossing_move -- a quad in front of a wall, 64 x 64, moving towards the eye by 4 %% of its\n"
                 "distance per frame, eight 1-spp frames, every default; MSE of the history over the quad's %d pixels of the last frame against\n"
                 "a 1024-spp frame of the final scene.\n\nfollowing off  %.6f\nfollowing on   %.6f\n" % (box.sum(), mse[False], mse[True]))
    print("MSE over the box: following off %.6f, on %.6f" % (mse[False], mse[True]))
    assert mse[True] < mse[False]


# ---- the rest of the surface ----------------------------------------------------------------------------------------------------------
def one(ctx, ts, size, inst=None, late_edit=None):
    if inst is not None:
        ctx.update_instances(inst)
    ctx.frame_begin(*size)
    ctx.frame_sample_base(ts)
    ctx.render(1, ts)
    ctx.render_features(1, ts)
    if late_edit is not None:
        ctx.update_instances(late_edit)
    ctx.temporal_accumulate(None)
    return ctx.download_temporal()[..., 3]


def test_state_bytes_refusal_and_restarts(scenes_, emu):
    import gpuspectral_amd as g

    sc = scenes_["cornell"]
    w, h = 96, 64
    size = (w, h)
    moved1, moved2 = moved_instances(sc.instances, (6,), 1), moved_instances(sc.instances, (6,), 2)
    with g.Context(0) as ctx:
        ctx.upload_scene(sc)
        for call in (ctx.download_temporal_motion,):
            with pytest.raises(g.GspError, match="gsp_temporal_accumulate"):
                call()  # before any accumulate
        # the order of the refusals, two broken conditions per call (temporal_util.refusals): without a history and following off ...
        buf = np.zeros((h, w, 4), np.float32).ctypes.data
        names = ("gsp_download_temporal_motion", "gsp_temporal_motion_to_device")
        null, hist, follow = (dict((n, n + t) for n in names) for t in (
            ": null output pointer", " needs a gsp_temporal_accumulate call since the history was last invalidated",
            " needs gsp_temporal_follow_instances(ctx, 1) before the history was accumulated"))
        n0, n1 = names
        refusals(ctx, [(n0, (None,), null[n0]), (n0, (buf,), hist[n0]), (n1, (None, 0), null[n1]), (n1, (16, 0), hist[n1])])
        # following off: the motion read-outs are refused also with a history, and nothing of the feature is allocated
        ctx.frame_begin(w, h)
        ctx.render(1, 0)
        ctx.render_features(1, 0)
        bytes0 = ctx.stats()["device_bytes"]
        ctx.temporal_accumulate(None)
        assert ctx.stats()["device_bytes"] == bytes0 + 72 * w * h
        with pytest.raises(g.GspError, match="gsp_temporal_follow_instances"):
            ctx.download_temporal_motion()
        assert ctx._L.gsp_temporal_motion_to_device(ctx._h, 16, 1 << 30) == 1 and "gsp_temporal_follow_instances" in ctx._L.gsp_last_error(ctx._h).decode()
        refusals(ctx, [(n0, (None,), null[n0]), (n0, (buf,), follow[n0]), (n1, (None, 4), null[n1]), (n1, (16, 4), follow[n1])])  # ... with one ...
        # with following off a late edit is nobody's business
        assert np.all(one(ctx, 1, size, late_edit=moved1)[ctx.download_features()[2][..., 2] != 6] == 2.0)
        ctx.update_instances(sc.instances)
        # the toggle drops the history; a call with the current value does not
        ctx.temporal_follow_instances(True)
        with pytest.raises(g.GspError, match="gsp_temporal_accumulate"):
            ctx.download_temporal()
        ctx.frame_begin(w, h)
        ctx.frame_sample_base(2)
        ctx.render(1, 2)
        ctx.render_features(1, 2)
        bytes1 = ctx.stats()["device_bytes"]
        state = lambda: (ctx.download(), ctx.download_features(), ctx.stats())
        s0 = state()
        ctx.temporal_accumulate(None)
        s1 = state()
        assert same(s0[0], s1[0]) and all(np.array_equal(words(p), words(q)) for p, q in zip(s0[1], s1[1]))  # the frame's state around a call
        skip = ("render_seconds", "extend_kernel_ms", "shade_kernel_ms", "connect_kernel_ms", "bvh_build_ms", "device_bytes")
        assert all(s1[2][k] == v for k, v in s0[2].items() if k not in skip)
        # one motion plane of 16 bytes per pixel and the table of 96 bytes per instance
        assert s1[2]["device_bytes"] == bytes1 + 16 * w * h + 96 * len(sc.instances)
        assert np.all(ctx.download_temporal()[..., 3] == 1.0) and not ctx.download_temporal_motion().any()
        ctx.temporal_follow_instances(True)
        assert np.all(one(ctx, 3, size) == 2.0)
        assert ctx._L.gsp_download_temporal_motion(ctx._h, None) == 1 and "null output" in ctx._L.gsp_last_error(ctx._h).decode()
        assert ctx._L.gsp_temporal_motion_to_device(ctx._h, None, 1 << 20) == 1 and "null output" in ctx._L.gsp_last_error(ctx._h).decode()
        refusals(ctx, [(n0, (None,), null[n0]), (n1, (None, 4), null[n1])])  # ... and following on
        # the edit counter: an edit after the frame's feature pass is refused, with the text that says where it belongs ...
        with pytest.raises(g.GspError, match="before the frame's gsp_render_features"):
            one(ctx, 4, size, late_edit=moved1)
        assert np.all(ctx.download_temporal()[..., 3] == 2.0)  # ... and the refused call left the history alone
        # ... in the next frame that edit lies before the feature pass, and an edit that changes nothing does not count
        box = lambda: ctx.download_features()[2][..., 2] == 6
        ln = one(ctx, 5, size, late_edit=moved1)
        near = lambda x, v: np.abs(x - v) < 1e-5  # (a followed length is a quotient of float32 sums: v to a few ulp)
        assert near(ln[box()].max(), 3.0) and np.all(ctx.download_temporal_motion()[..., 3][box() & near(ln, 3.0)] == 2.0)
        # ... and a second feature pass of the frame does not record the counter again
        ctx.frame_begin(w, h)
        ctx.frame_sample_base(6)
        ctx.render(1, 6)
        ctx.render_features(1, 6)
        ctx.update_instances(moved2)
        ctx.render_features(1, 7)
        with pytest.raises(g.GspError, match="before the frame's gsp_render_features"):
            ctx.temporal_accumulate(None)
        ln = one(ctx, 8, size)
        assert near(ln[box()].max(), 4.0)
        # reset, upload and another size restart it
        ctx.temporal_reset()
        with pytest.raises(g.GspError, match="gsp_temporal_accumulate"):
            ctx.download_temporal_motion()
        assert np.all(one(ctx, 9, size) == 1.0) and np.all(one(ctx, 10, size, inst=moved1)[~box()] >= 1.0)
        assert near(ctx.download_temporal()[..., 3][box()].max(), 2.0)
        ctx.upload_scene(sc)  # a new scene has no history and no snapshot
        assert np.all(one(ctx, 11, size) == 1.0) and not ctx.download_temporal_motion().any()
        assert np.all(one(ctx, 12, size) == 2.0)
        assert np.all(one(ctx, 13, (w, h - 8)) == 1.0) and np.all(one(ctx, 14, (w, h - 8)) == 2.0)
        assert ctx.download_temporal_motion().shape == (h - 8, w, 4)


def test_download_temporal_svgf_on_a_followed_history(rigs, emu, scenes_):
    from gpuspectral_amd import abi

    ctx, sc = rigs("cornell", True), scenes_["cornell"]
    hist, _ = sequence(ctx, emu, sc, (96, 64), MOVERS["cornell"], degrees=ORBIT[:5], moments=True, what="svgf")
    a, g, _ = ctx.download_features()
    sv = abi.svgf(min_history=2)
    assert same(ctx.download_temporal_svgf(None, sv), SvgfEmu().run(None, sv, hist.H, hist.M, a, g))


_TORCH_CHILD = """
import sys
import torch  # first: the tracer's library then binds to the HIP runtime torch has loaded (see bench.py)
import numpy as np
sys.path.insert(0, sys.argv[1])
import gpuspectral_amd as g
from gpuspectral_amd import scenes
W, H = 96, 64
sc = scenes.cornell_materials(8)
with g.Context(0) as ctx:
    ctx.upload_scene(sc)
    ctx.temporal_follow_instances(True)
    for ts in range(2):
        inst = sc.instances.copy()
        inst["transform"][8][12] += 0.05 * ts
        ctx.update_instances(inst)
        ctx.frame_begin(W, H)
        ctx.frame_sample_base(ts)
        ctx.render(1, ts)
        ctx.render_features(1, ts)
        ctx.temporal_accumulate(None)
    want = ctx.download_temporal_motion().reshape(-1)
    assert (want[3::4] == 2.0).any() and (want[3::4] == 1.0).any()
    for off in (0, 1):  # floats: the second destination is not 16-byte aligned
        t = torch.zeros(W * H * 4 + 8, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        ctx.temporal_motion_to_device(t[off:off + W * H * 4])
        back = t.cpu().numpy()
        assert np.array_equal(back[off:off + W * H * 4].view(np.uint32), want.view(np.uint32)) and not back[:off].any() and not back[off + W * H * 4:].any()
    t = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda:0")
    try:
        ctx.temporal_motion_to_device(t.data_ptr(), W * H * 16 - 4)
        raise SystemExit("a destination of the wrong size was accepted")
    except g.GspError as e:
        assert "destination too small" in str(e), e
    assert not t.cpu().numpy().any()
print("torch tensor ok")
"""


def test_motion_to_device_torch_tensor():
    """Into a torch tensor, in a process of its own: torch has to be imported before the library is loaded (bench.py does the same)."""
    r = subprocess.run([sys.executable, "-c", _TORCH_CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "torch tensor ok" in r.stdout, r.stdout + r.stderr


def test_host_layer():
    """The C++ host layer: PathTracer::temporalFollowInstances / downloadTemporalMotion; render() uploads an edited transform."""
    from conftest import CORNELL_XML
    from gpuspectral_amd import host

    W, H = 48, 40
    sc = host.Scene(CORNELL_XML)
    pt = host.PathTracer(W, H)
    try:
        pt.temporal_follow_instances(True)
        for k in range(3):
            if k:
                pt.next_frame()
            pt.render(sc, 1)
            pt.render_features(sc, 1)
            pt.temporal_accumulate(None)
            assert np.all(pt.download_temporal()[..., 3] == float(k + 1))
            v = pt.download_temporal_motion()
            assert v.shape == (H, W, 4) and (np.all(v == np.float32([0, 0, 1, 1])) if k else not v.any())
        pt.temporal_follow_instances(False)
        pt.next_frame()
        pt.render(sc, 1)
        pt.render_features(sc, 1)
        pt.temporal_accumulate(None)
        assert np.all(pt.download_temporal()[..., 3] == 1.0)  # the switch dropped the history
        with pytest.raises(Exception, match="gsp_temporal_follow_instances"):
            pt.download_temporal_motion()
    finally:
        pt.close()


def test_cli_follow(tmp_path):
    """--temporal-follow --temporal-move INST,DX,DY,DZ --motion out.pfm: the moved object's pixels are followed and keep their history."""
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
    base = ["--temporal-frames", "4", "--temporal-move", "6,0.02,0,0.25", CORNELL_XML]
    out = run(["--temporal", str(t / "on.t.pfm"), "--temporal-follow", "--motion", str(t / "v.pfm")] + base + [str(t / "on.pfm"), str(W), str(H), "1"])
    assert "temporal: 4 frames" in out and "motion:" in out and "followed pixels" in out
    v = pfm(t / "v.pfm")
    n = int(out.split("motion: ")[1].split()[0])  # (the file holds {dx, dy, class})
    assert n > 50 and v.shape == (H, W, 3) and np.isfinite(v).all() and int((v[..., 2] == 2.0).sum()) == n
    assert np.abs(v[..., :2][v[..., 2] == 2.0]).max() > 0.25 and not v[v[..., 2] == 0.0].any()
    assert "no object 99" in run(["--temporal", str(t / "x.t.pfm"), "--temporal-follow", "--temporal-frames", "2", "--temporal-move", "99,0,0,0", CORNELL_XML,
                                  str(t / "x.pfm"), str(W), str(H), "1"], code=1)
