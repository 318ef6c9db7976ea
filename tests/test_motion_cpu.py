"""Moved instances on the CPU (include/gpuspectral_pt.h, "Temporal accumulation: moved instances"): the library's per-pixel text and
its host-side table (csrc/pt_motion.h through tests/emu/motion_emu.cpp) against closed forms, against the emulations of the static
path (temporal_util.TemporalEmu, svgf_util.SvgfEmu) and against the float64 restatement of tests/motion_util.py.  No GPU."""
import copy
import os
import subprocess

import numpy as np
import pytest

import motion_util as mu
import temporal_util as tu
from conftest import GOLDEN, ROOT
from motion_util import MOVED, NO_HISTORY, STATIC, MotionEmu
from svgf_util import SvgfEmu
from temporal_util import U32, TemporalEmu, same

FOV = 0.05  # a narrow camera, as tests/test_temporal_cpu.py: rays are parallel to within 0.025 rad
W, H = 32, 16
DEPTH = 5.0
INST = 3  # tu.plane_frame's instance
IDENT = np.eye(4, dtype=np.float32).reshape(16)


@pytest.fixture(scope="module")
def emu():
    return MotionEmu()


@pytest.fixture(scope="module")
def temu():
    return TemporalEmu()


@pytest.fixture(scope="module")
def semu():
    return SvgfEmu()


def xforms(moving=IDENT, n=INST + 1):
    x = np.tile(IDENT, (n, 1))
    x[INST] = moving
    return x


def f32(x):
    return np.asarray(x, np.float32)


# ---- a translation parallel to the image plane ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3])
def test_image_plane_shift(emu, temu, k):
    """The camera stays; the plane z = 5 (instance 3) moves by dX = k * 5 / zplane along x per frame.  Image column x shows world
    X = -(x - W/2) * 5 / zplane, so the point seen at column x was at column x + k one frame earlier -- exactly k in float64, to
    within a few 1e-5 of a pixel in float32, which step 6 snaps: tap 0 alone with weight 1.  With following on the history is the
    history shifted by k columns: after f moves column x has length min(f, (W - 1 - x) // k) + 1, the k columns on the right whose
    predecessor lies outside the frame are fresh, and H' is prev + (c - prev) * a on the shifted column, in float32, bit for bit.
    With following off the unmoved camera reads its own column."""
    from gpuspectral_amd import abi

    rng = np.random.default_rng(11)
    cam = tu.camera()
    zp = tu.zplane64(W, H, FOV)
    step = k * DEPTH / zp
    on = off = None
    cols = np.arange(W)
    for f in range(4):
        xf = xforms(mu.compose(np.eye(3), (f * step, 0.0, 0.0)))
        c, a, g, i = tu.plane_frame(rng, H, W, cam, FOV, depth=DEPTH)
        prev_on = on
        on = emu.step(abi.temporal(), cam, FOV, c, a, g, i, xf, hist=on)
        off = temu.step(abi.temporal(), cam, FOV, c, a, g, i, hist=off)
        want_len = np.minimum(f, (W - 1 - cols) // k) + 1.0
        assert np.array_equal(on.H[..., 3], np.broadcast_to(f32(want_len), (H, W))), f
        assert np.all(off.H[..., 3] == f + 1.0)
        if f == 0:
            assert not on.V.any()
            continue
        has = cols < W - k
        assert np.all(on.V[:, has] == f32([k, 0.0, 1.0, 2.0])) and not on.V[:, ~has].any()  # V.xy is uniform
        p = prev_on.H[:, k:, :3]
        n_ = on.H[:, :W - k, 3:4]
        a_ = np.maximum(np.float32(0.2), np.float32(1.0) / n_)
        assert same(on.H[:, :W - k, :3], p + (c[:, :W - k, :3] - p) * a_)
        assert same(on.H[:, W - k:, :3], c[:, W - k:, :3])
        assert not same(on.H, off.H)


# ---- a rotation about an axis through the surface ----------------------------------------------------------------------------------------
def rotated_plane_frame(rng, R, pivot):
    """The plane z = 5 turned by R about `pivot` (a point of it), seen by the camera at the origin: P = t d with n . (P - pivot) = 0."""
    cam = tu.camera()
    d = tu.pinhole_dirs64(cam, FOV, W, H)
    n = R @ np.array([0.0, 0.0, -1.0])
    t = (n @ pivot) / (d @ n)
    return tu.plane_frame(rng, H, W, cam, FOV, depth=t * d[..., 2], normal=np.broadcast_to(f32(n), (H, W, 3)))


def test_rotation_about_a_surface_point(emu, temu):
    """30 degrees about the vertical axis through the plane's point on the optical axis, default normal_min 0.9 > cos 30.  The frame
    is 0.25 world units wide at depth 5, so the turned plane stays within 0.25 / 2 * tan 30 / 5 = 1.4 % of its old depth: with
    following off the instance and depth tests pass and the normal test rejects every tap (the pixels restart); with following on
    N takes the normal back (dot = 1 to rounding), P' lies on the old plane, and the pixels whose P' projects into the frame --
    those within cos 30 of the half width, the pivot's column and its neighbours among them -- keep their history."""
    from gpuspectral_amd import abi

    rng = np.random.default_rng(12)
    cam = tu.camera()
    pivot = np.array([0.0, 0.0, DEPTH])
    R = mu.rotation((0, 1, 0), 30.0)
    f0 = tu.plane_frame(rng, H, W, cam, FOV, depth=DEPTH)
    f1 = rotated_plane_frame(rng, R, pivot)
    x0, x1 = xforms(), xforms(mu.moved(IDENT, R, pivot))
    on = emu.step(abi.temporal(), cam, FOV, *f1, x1, hist=emu.step(abi.temporal(), cam, FOV, *f0, x0))
    off = temu.step(abi.temporal(), cam, FOV, *f1, hist=temu.step(abi.temporal(), cam, FOV, *f0))
    assert np.all(off.H[..., 3] == 1.0)
    near = (slice(H // 2 - 2, H // 2 + 3), slice(W // 2 - 4, W // 2 + 5))
    assert np.all(on.H[..., 3][near] == 2.0) and np.all(on.V[..., 3][near] == 2.0)
    assert on.V[H // 2, W // 2, 0] == 0.0 and on.V[H // 2, W // 2, 1] == 0.0  # the pivot did not move
    inside = np.abs(np.arange(W) - W / 2) < 0.8 * (W / 2) * np.cos(np.radians(30.0))
    assert np.all(on.H[..., 3][:, inside] == 2.0)


def test_non_uniform_scale_takes_the_normal_back(emu):
    """A plane through `pivot` with normal n0, then scaled by S = diag(4, 1, 0.25) about the pivot: its normal becomes
    normalize(S^-T n0), and N = transpose(B3^-1) with B3 = S^-1 must take it back to n0.  The table against numpy's
    inverse-transpose in float64 (one rounding to float32: 2^-24 relative, plus the double arithmetic's own 1e-15), and the pixel
    at the pivot, which keeps its history although the dot product of the two normals is 0.80."""
    from gpuspectral_amd import abi

    S = np.diag([4.0, 1.0, 0.25])
    pivot = np.array([0.0, 0.0, DEPTH])
    t_prev = mu.moved(IDENT, mu.rotation((0, 1, 0), 40.0), pivot)
    t_cur = mu.moved(t_prev, S, pivot)
    cls, B, N = mu.split_table(emu.table([t_prev], [t_cur]))
    (Ap, _), (Ac, _) = mu.affine(t_prev), mu.affine(t_cur)
    want = np.linalg.inv(Ap @ np.linalg.inv(Ac)).T
    assert cls[0] == MOVED and np.abs(N[0] - want).max() <= 2 * U32 * np.abs(want).max()
    n0 = mu.rotation((0, 1, 0), 40.0) @ np.array([0.0, 0.0, -1.0])
    n1 = np.linalg.inv(S).T @ n0
    n1 /= np.linalg.norm(n1)
    assert n0 @ n1 < 0.9
    rng = np.random.default_rng(13)
    cam = tu.camera()
    d = tu.pinhole_dirs64(cam, FOV, W, H)

    def frame(n):
        t = (n @ pivot) / (d @ n)
        return tu.plane_frame(rng, H, W, cam, FOV, depth=t * d[..., 2], normal=np.broadcast_to(f32(n), (H, W, 3)))

    h0 = emu.step(abi.temporal(), cam, FOV, *frame(n0), xforms(t_prev))
    h1 = emu.step(abi.temporal(), cam, FOV, *frame(n1), xforms(t_cur), hist=h0)
    assert h1.H[H // 2, W // 2, 3] == 2.0 and np.all(h1.V[H // 2, W // 2] == f32([0, 0, 1, 2]))


# ---- class 2 ---------------------------------------------------------------------------------------------------------------------------
def test_class_2_is_no_history(emu):
    from gpuspectral_amd import abi

    flat = mu.compose(np.diag([1.0, 0.0, 1.0]), (0, 0, 0))
    nan = IDENT.copy()
    nan[5] = np.nan
    inf = IDENT.copy()
    inf[13] = np.inf
    huge = mu.compose(np.eye(3) * 1e30, (0, 0, 0))
    tiny = mu.compose(np.eye(3) * 1e-30, (0, 0, 0))
    shifted = mu.compose(np.eye(3), (0.001, 0, 0))
    pairs = [(flat, IDENT), (IDENT, flat), (nan, IDENT), (IDENT, nan), (IDENT, inf), (huge, tiny), (flat, flat), (IDENT, shifted)]
    cls, B, N = mu.split_table(emu.table([p for p, _ in pairs], [c for _, c in pairs]))
    assert list(cls) == [NO_HISTORY] * 6 + [STATIC, MOVED]  # (huge, tiny): B overflows float32; (flat, flat): equal bits come first
    assert not B[:7].any() and not N[:7].any()
    rng = np.random.default_rng(14)
    cam = tu.camera()
    for prev, cur in pairs[:6]:
        h0 = emu.step(abi.temporal(), cam, FOV, *tu.plane_frame(rng, H, W, cam, FOV), xforms(prev))
        h1 = emu.step(abi.temporal(), cam, FOV, *tu.plane_frame(rng, H, W, cam, FOV), xforms(cur), hist=h0)
        assert np.all(h1.H[..., 3] == 1.0) and not h1.V.any()
    # an instance index the table does not have: the left half of the frame names instance 9 of 4
    inst = np.where(np.arange(W)[None, :] < W // 2, 9, INST) * np.ones((H, W), np.uint32)
    h0 = emu.step(abi.temporal(), cam, FOV, *tu.plane_frame(rng, H, W, cam, FOV, inst=inst), xforms())
    h1 = emu.step(abi.temporal(), cam, FOV, *tu.plane_frame(rng, H, W, cam, FOV, inst=inst), xforms(), hist=h0)
    assert np.all(h1.H[:, :W // 2, 3] == 1.0) and not h1.V[:, :W // 2].any()
    assert np.all(h1.H[:, W // 2:, 3] == 2.0) and np.all(h1.V[:, W // 2:] == f32([0, 0, 1, 1]))


# ---- the static path ---------------------------------------------------------------------------------------------------------------------
def moving_frames(rng, n, nan=False):
    """n frames of a plane with a step in depth and instance, and a strip of background, under a camera that turns and steps, with a
    jump before the last frame (the frames of tests/test_svgf_cpu.py with a background strip)."""
    depth = np.where(np.arange(W)[None, :] < W // 2, 5.0, 7.0) * np.ones((H, W))
    inst = np.where(np.arange(W)[None, :] < W // 2, 3, 2) * np.ones((H, W), np.uint32)
    out = []
    for k in range(n):
        cam = tu.camera(0.0012 * k + (0.02 if k == n - 1 else 0.0), -0.0004 * k, (0.002 * k, 0.0, -1.0))
        c, a, g, i = tu.plane_frame(rng, H, W, cam, FOV, depth=depth, inst=inst)
        bc, ba, bg, bi = tu.background_frame(rng, H, W)
        for p, q in ((c, bc), (a, ba), (g, bg), (i, bi)):
            p[:3] = q[:3]
        if nan:
            for value in (np.nan, np.inf, -np.inf):
                c[rng.integers(0, H, 6), rng.integers(0, W, 6), rng.integers(0, 3, 6)] = value
        out.append((cam, (c, a, g, i)))
    return out


@pytest.mark.parametrize("nan", [False, True], ids=["finite", "nan-inf"])
def test_static_instances_are_bit_for_bit_the_unfollowed_history(emu, temu, semu, nan):
    from gpuspectral_amd import abi

    xf = xforms(mu.moved(IDENT, mu.rotation((1, 2, 3), 40.0), shift=(0.3, 0.1, 0.2)))  # (not the identity, and never changed)
    for t in (None, abi.temporal(alpha=tu.FLT_MIN, max_history=3)):
        rng = np.random.default_rng(7)
        hist = histm = plain = plainm = None
        for k, (cam, f) in enumerate(moving_frames(rng, 6, nan)):
            plain, kept = temu.step(t, cam, FOV, *f, hist=plain, with_kept=True)
            plainm = semu.step(t, cam, FOV, *f, hist=plainm)
            hist = emu.step(t, cam, FOV, *f, xf, hist=hist)
            histm = emu.step(t, cam, FOV, *f, xf, hist=histm, moments=True)
            for got in (hist, histm):
                assert same(got.H, plain.H) and same(got.G, plain.G) and np.array_equal(got.I, plain.I), k
                assert np.array_equal(got.V[..., 3], np.where(kept & 0x80, 1.0, 0.0).astype(np.float32)), k
                assert not got.V[(kept & 0x80) == 0].any()
            assert same(histm.M, plainm.M) and same(histm.V, hist.V)
        assert hist.H[..., 3].max() > 2.0 and (hist.H[..., 3] <= 1.0).any()


def test_nothing_moved(emu):
    from gpuspectral_amd import abi

    rng = np.random.default_rng(15)
    cam = tu.camera(0.1, -0.05, (0.3, 0.2, -1.0))
    hist = None
    for k in range(3):
        hist = emu.step(abi.temporal(), cam, 0.8, *tu.plane_frame(rng, H, W, cam, 0.8), xforms(), hist=hist)
        if k:
            assert np.all(hist.V == f32([0, 0, 1, 1])) and np.all(hist.H[..., 3] == k + 1.0)


# ---- motion_table ---------------------------------------------------------------------------------------------------------------------------
def test_motion_table_against_numpy(emu):
    """Random rigid and affine pairs.  The library forms B and N in double from an adjugate inverse and rounds once: against numpy's
    float64 the entries agree to the one rounding (2^-24 relative to the row's largest entry -- a sum of products of that size) plus
    the double arithmetic, cond(A) * 1e-15, which the draw keeps below 1e-12."""
    rng = np.random.default_rng(16)
    prev, cur = [], []
    for k in range(200):
        if k % 2:  # rigid
            A0, A1 = mu.rotation(rng.normal(size=3), rng.uniform(-180, 180)), mu.rotation(rng.normal(size=3), rng.uniform(-180, 180))
        else:  # affine, well conditioned
            A0, A1 = (np.eye(3) * rng.uniform(0.5, 2.0) + rng.uniform(-0.3, 0.3, (3, 3)) for _ in range(2))
        prev.append(mu.compose(A0, rng.uniform(-5, 5, 3)))
        cur.append(mu.compose(A1, rng.uniform(-5, 5, 3)))
    prev += cur[:10]  # ... and ten pairs of equal bits
    cur += cur[:10]
    cls, B, N = mu.split_table(emu.table(prev, cur))
    c64, B64, N64 = mu.table64(prev, cur)
    assert np.array_equal(cls, c64) and np.all(cls[:200] == MOVED) and np.all(cls[200:] == STATIC)
    tol = lambda x: 2 * U32 * np.abs(x).max(axis=(1, 2), keepdims=True) + 1e-12
    assert np.all(np.abs(B - B64) <= tol(B64)) and np.all(np.abs(N - N64) <= tol(N64))
    # N is the inverse-transpose of B's 3x3
    assert np.abs(np.einsum("nij,nkj->nik", B64[:200, :, :3], N64[:200]) - np.eye(3)).max() < 1e-9


def test_motion_table_under_sanitizers(tmp_path):
    """Host-only code as a program of its own (tests/emu/motion_table_main.cpp) under ASan / UBSan; nothing is loaded into Python."""
    exe = str(tmp_path / "motion_table_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                           "-Wno-unknown-pragmas", "-Wno-unused-function", os.path.join(ROOT, "tests", "emu", "motion_table_main.cpp"), "-o", exe])
    r = subprocess.run([exe, "5", "6000"], capture_output=True, text=True)
    assert r.returncode == 0 and "1000 static" in r.stdout, r.stdout + r.stderr


# ---- agreement with the restatement on the Cornell box ---------------------------------------------------------------------------------
# Bound, as tests/test_temporal_cpu.py derives it, with the record in front: P' = B P is three products and three sums more on numbers
# of the scene's extent and the record itself is float32 on both sides, so the reprojected position carries at most ~96 u * max(W, H)
# of a pixel instead of 64 u: dp = 96 u * 128 = 7.3e-4.  A bilinear weight moves by at most 2 dp, the four by 8 dp in sum, and
# prev = s / sw by at most 8 dp / sw * max |H_q| in the numerator and the same again in the denominator; the blend and the sums add
# a few u of max(|c|, |H_q|).  V.xy carries dp itself, V.z = sw 8 dp.
AGREE_SEEDS = (1, 2, 3, 4)
MOVING = 6  # the tall box of the golden Cornell scene
LEFT_OUT_CAP = 0.01


def cornell_frames(cornell, seed, n=5, size=128):
    import features_util as fu

    rng = np.random.default_rng(seed)
    img = np.load(os.path.join(GOLDEN, "cornell_128_1spp.npy")).reshape(128, 128, 3)
    femu = fu.FeaturesEmu()
    out = []
    to_world = np.asarray(cornell.to_world, np.float32).copy()
    inst = cornell.instances.copy()
    for _ in range(n):
        sc = copy.copy(cornell)
        sc.to_world = to_world.copy()
        sc.instances = inst.copy()
        a, g, i = fu.full(femu.scene(sc).render(size, size, 1), size, size)
        c = np.ones((size, size, 4), np.float32)
        c[..., :3] = img * rng.uniform(0.5, 1.5, (size, size, 1))
        out.append((to_world.copy(), inst["transform"].copy(), (c, a, g, i)))
        to_world = tu.rotated_about_y(to_world, rng.uniform(-2.5, 2.5), pivot=(0.0, 1.0, 0.0))
        to_world[12:15] += rng.uniform(-0.05, 0.05, 3).astype(np.float32)
        # one instance translating and rotating at once: a few degrees about a tilted axis through its own origin, a small step
        t = inst["transform"][MOVING]
        pivot = mu.affine(t)[1]
        inst["transform"][MOVING] = mu.moved(t, mu.rotation((0.2, 1.0, 0.1), rng.uniform(2.0, 6.0)), pivot, rng.uniform(-0.04, 0.04, 3))
    return out


def test_emulation_agrees_with_the_restatement_on_cornell(emu, cornell):
    from gpuspectral_amd import abi

    fov = float(cornell.fov)
    lines, worst_left, worst_ratio = [], 0.0, 0.0
    for seed in AGREE_SEEDS:
        hist = None
        for k, (cam, xf, f) in enumerate(cornell_frames(cornell, seed)):
            new = emu.step(abi.temporal(), cam, fov, *f, xf, hist=hist)
            r = mu.motion64(*f, cam, fov, xf, hist=hist)
            assert same(r["G"], new.G) and np.array_equal(r["I"], new.I)
            # the restatement alone decides what is left out: the pixels one of whose decisions -- the snap, a tap's depth or normal test,
            # sw >= 0.01, steps 4 and 7 -- sits within rounding of its threshold (motion64's `fragile`)
            agree = ~r["fragile"]
            assert np.array_equal(r["V"][..., 3][agree], new.V[..., 3][agree])
            left_out = 1.0 - agree.mean()
            dp = 96 * U32 * 128
            big = float(np.abs(hist.H).max()) if hist is not None else 0.0
            bound = 2 * 8 * dp / np.maximum(r["sw"], 0.01) * big + 16 * U32 * max(big, float(np.abs(f[0][..., :3]).max()))
            dev = np.abs(new.H.astype(np.float64) - r["H"]).max(-1)
            dv = np.abs(new.V.astype(np.float64) - r["V"])
            moved = r["cls"] == MOVED
            lines.append("seed %d frame %d: %.3f %% of the pixels left out, largest |H - H64| %.3e (bound there %.3e), largest |V.xy - V64.xy| %.3e "
                         "(bound %.3e), %d followed pixels of mean length %.2f"
                         % (seed, k, 100 * left_out, dev[agree].max(), bound[agree][np.argmax(dev[agree])], dv[..., :2][agree].max(), dp,
                            int((new.V[..., 3] == 2.0).sum()), new.H[..., 3][moved].mean() if moved.any() else 0.0))
            print(lines[-1])
            worst_left = max(worst_left, left_out)
            worst_ratio = max(worst_ratio, float((dev[agree] / bound[agree]).max()))
            assert left_out <= LEFT_OUT_CAP
            assert np.all(dev[agree] <= bound[agree])
            assert np.all(dv[..., :2][agree] <= dp) and np.all(dv[..., 2][agree] <= 8 * dp)
            if k:
                assert moved.sum() > 200 and new.H[..., 3][moved].mean() > 1.5  # the moved box found its history
            hist = new
    with open(os.path.join(ROOT, "profiles", "motion_cpu_check.txt"), "w") as fh:
        fh.write("tests/test_motion_cpu.py::test_emulation_agrees_with_the_restatement_on_cornell -- csrc/pt_motion.h on the host against the\n"
                 "float64 restatement of tests/motion_util.py; golden Cornell box 128 x 128, seeds %s, five frames, camera moves, instance %d\n"
                 "translating and rotating.  Largest left-out share %.3f %% (cap %.1f %%); largest deviation / bound %.3f.\n\n"
                 % (AGREE_SEEDS, MOVING, 100 * worst_left, 100 * LEFT_OUT_CAP, worst_ratio) + "\n".join(lines) + "\n")
