"""The temporal anti-lag on the CPU (include/gpuspectral_pt.h, "Temporal anti-lag"): the library's per-pixel text (csrc/pt_antilag.h
through tests/emu/antilag_emu.cpp) against the float64 restatement of tests/antilag_util.py, against known answers bit for bit, its
validation, and the emulation as a program of its own under the sanitizers.  No GPU."""
import copy
import os
import subprocess

import numpy as np
import pytest

import antilag_util as au
import illum_util as iu
import motion_util as mu
import temporal_util as tu
from antilag_util import AntilagEmu
from conftest import GOLDEN
from illum_util import IllumEmu
from temporal_util import U32, same

W, H = 40, 24
FRAMES = 6
FRAGILE_CAP = 0.02  # tests/test_illum_cpu.py's
MOVING = 6  # the tall box of the golden Cornell scene
NORMAL = np.float32([0.0, 0.0, -1.0, 5.0])


@pytest.fixture(scope="module")
def emu():
    return AntilagEmu()


@pytest.fixture(scope="module")
def accumulate():
    return IllumEmu()


# ---- the emulation against the restatement -----------------------------------------------------------------------------------------------
_FRAMES = {}


def cornell_frames(cornell):
    """FRAMES frames of the golden Cornell box at W x H under a camera that turns and steps, the tall box translating and rotating
    (tests/test_motion_cpu.py's sequence at this size): (to_world, transforms, (c, albedo, geom, ids)) each; the colour is a crop of the
    committed 1-spp image under per-pixel noise."""
    import features_util as fu

    if "f" in _FRAMES:
        return _FRAMES["f"]
    rng = np.random.default_rng(77)
    img = np.load(os.path.join(GOLDEN, "cornell_128_1spp.npy")).reshape(128, 128, 3)[40:40 + H, 30:30 + W]
    femu = fu.FeaturesEmu()
    out = []
    to_world = np.asarray(cornell.to_world, np.float32).copy()
    inst = cornell.instances.copy()
    for _ in range(FRAMES):
        sc = copy.copy(cornell)
        sc.to_world = to_world.copy()
        sc.instances = inst.copy()
        a, g, i = fu.full(femu.scene(sc).render(W, H, 1), W, H)
        c = np.ones((H, W, 4), np.float32)
        c[..., :3] = (img + 0.05) * rng.uniform(0.2, 1.8, (H, W, 3))
        out.append((to_world.copy(), inst["transform"].copy(), (c, a, g, i)))
        to_world = tu.rotated_about_y(to_world, rng.uniform(-1.5, 1.5), pivot=(0.0, 1.0, 0.0))
        to_world[12:15] += rng.uniform(-0.03, 0.03, 3).astype(np.float32)
        t = inst["transform"][MOVING]
        inst["transform"][MOVING] = mu.moved(t, mu.rotation((0.2, 1.0, 0.1), rng.uniform(2.0, 6.0)), mu.affine(t)[1], rng.uniform(-0.04, 0.04, 3))
    _FRAMES["f"] = out
    return out


# Bounds.  F': tests/test_illum_cpu.py's for a history pulled through the reprojection -- 2 * 8 dp / sw * max |F_q| + 24 u max(|F_q|, |x|),
# dp = 96 u * 128, the restatement alone deciding which pixels are fragile, at most FRAGILE_CAP of the frame.  The clamp, from the
# emulation's own F': 2 delta of antilag_util.clamp64 plus one rounding of the result; len where no comparison sits within delta.
@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("follow", [False, True], ids=["static", "follow"])
@pytest.mark.parametrize("demod", [False, True], ids=["colour", "demod"])
def test_emulation_agrees_with_the_restatement(emu, accumulate, cornell, demod, follow, radius):
    from gpuspectral_amd import abi

    fov = float(cornell.fov)
    al = abi.antilag(radius=radius)
    hist = fast = None
    clamped = kept_len = 0
    worst_f = worst_h = 0.0
    for k, (cam, xf, f) in enumerate(cornell_frames(cornell)):
        xforms = xf if follow else None
        new = accumulate.step(None, cam, fov, *f, xforms=xforms, hist=hist, moments=False, demod=demod)
        F, Hc = emu.step(al, None, cam, fov, *f, new, old=hist, fast=fast, xforms=xforms, demod=demod)
        # Step A
        r = au.fast64(*f, cam, fov, old=hist, fast=fast, xforms=xforms, demod=demod)
        ok = ~r["fragile"]
        assert float(r["fragile"].mean()) <= FRAGILE_CAP
        dp = 96 * U32 * 128
        big = float(np.abs(fast[..., :3]).max()) if fast is not None else 0.0
        xmax = float(np.abs(r["e"][r["u"]]).max()) if demod else float(np.abs(f[0][..., :3]).max())
        bound = 2 * 8 * dp / np.maximum(r["sw"], 0.01) * big + 24 * U32 * max(big, xmax)
        dev = np.abs(F.astype(np.float64) - r["H"]).max(-1)
        print("frame %d: largest |F - F64| / bound %.3f, %.2f %% fragile" % (k, (dev[ok] / bound[ok]).max(), 100 * r["fragile"].mean()))
        assert np.all(dev[ok] <= bound[ok])
        worst_f = max(worst_f, float((dev[ok] / bound[ok]).max()))
        assert F[..., 3].max() <= min(4.0, k + 1.0) and (k == 0 or F[..., 3].max() == min(4.0, k + 1.0))
        # Step B
        q = au.clamp64(F, new.G, new.I, new.H, radius=radius)
        assert float(q["fragile"].mean()) <= FRAGILE_CAP
        okb = ~q["fragile"]
        tol = 2 * q["delta"][..., None] + U32 * np.abs(q["H"][..., :3])
        devh = np.abs(Hc[..., :3].astype(np.float64) - q["H"][..., :3])
        assert np.all(devh[okb] <= tol[okb])
        worst_h = max(worst_h, float((devh[okb] / np.maximum(tol[okb], 1e-300)).max()))
        assert same(Hc[okb & ~q["processed"]], new.H[okb & ~q["processed"]])
        with np.errstate(invalid="ignore"):
            margin = np.minimum(np.abs(new.H[..., :3] - q["lo"]), np.abs(new.H[..., :3] - q["hi"])).min(-1)
        robust = okb & (~q["processed"] | (margin > q["delta"]))
        assert np.array_equal(Hc[..., 3][robust], q["H"][..., 3][robust].astype(np.float32))
        assert same(Hc[robust & ~q["changed"]], new.H[robust & ~q["changed"]])
        clamped += int((robust & q["changed"]).sum())
        kept_len += int((robust & q["changed"] & (Hc[..., 3] < new.H[..., 3])).sum())
        new.H = Hc
        hist, fast = new, F
    assert clamped > 20 and kept_len > 0  # (the clamp acts, and on the later frames it cuts lengths)
    print("largest |F - F64| / bound %.3f, largest |H - H64| / bound %.3f, %d clamped records" % (worst_f, worst_h, clamped))


# ---- known answers, bit for bit ------------------------------------------------------------------------------------------------------------
def plane(h, w, rng=None, const=(0.25, 0.5, 0.75), flen=3.0, hlen=7.0):
    """A frame that is one instance with one normal: F = const with length flen, H random (or const without rng) with length hlen."""
    F = np.zeros((h, w, 4), np.float32)
    F[..., :3], F[..., 3] = const, flen
    G = np.tile(NORMAL, (h, w, 1))
    I = np.full((h, w), 3, np.uint32)
    Hh = F.copy()
    if rng is not None:
        Hh[..., :3] = rng.uniform(0.0, 2.0, (h, w, 3))
    Hh[..., 3] = hlen
    return F, G, I, Hh


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_constant_window_clamps_to_the_constant(emu, radius):
    """sd = 0: lo = hi = the constant, so H becomes exactly that and len = min(len, F.len); a record that already equals it is untouched."""
    from gpuspectral_amd import abi

    rng = np.random.default_rng(radius)
    F, G, I, Hh = plane(17, 35, rng)
    Hh[4, 5, :3] = F[4, 5, :3]
    out = emu.clamp(abi.antilag(radius=radius), F, G, I, Hh)
    want = F.copy()
    want[..., 3] = 3.0
    want[4, 5, 3] = 7.0
    assert same(out, want)
    F[..., 3] = 9.0  # a fast history longer than the long one: the length stays
    assert np.all(emu.clamp(abi.antilag(radius=radius), F, G, I, Hh)[..., 3] == 7.0)


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_inside_the_box_keeps_every_bit(emu, radius):
    from gpuspectral_amd import abi

    rng = np.random.default_rng(10 + radius)
    F, G, I, Hh = plane(17, 35, rng)
    F[..., :3] = rng.uniform(0.0, 2.0, (17, 35, 3))
    # a box of a million standard deviations holds every record ...
    assert same(emu.clamp(abi.antilag(radius=radius, sigma_scale=1e6), F, G, I, Hh), Hh)
    # ... and with the defaults every record the restatement puts inside by more than its bound keeps rgb and len
    out = emu.clamp(abi.antilag(radius=radius), F, G, I, Hh)
    q = au.clamp64(F, G, I, Hh, radius=radius)
    margin = np.minimum(np.abs(Hh[..., :3] - q["lo"]), np.abs(Hh[..., :3] - q["hi"])).min(-1)
    inside = ~q["changed"] & (margin > q["delta"])
    assert inside.sum() > 50 and same(out[inside], Hh[inside])
    assert (q["changed"] & (margin > q["delta"])).sum() > 10 and np.all(out[..., 3][q["changed"] & (margin > q["delta"])] == 3.0)


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_small_instance_is_untouched(emu, radius):
    """An instance with 2 radius pixels in any window -- one fewer than the rule asks -- keeps its bits, the sea around it is clamped."""
    from gpuspectral_amd import abi

    rng = np.random.default_rng(20 + radius)
    F, G, I, Hh = plane(15, 21, rng)
    Hh[..., :3] += 5.0  # (far outside the box)
    I[7, 8:8 + 2 * radius] = 5
    out = emu.clamp(abi.antilag(radius=radius), F, G, I, Hh)
    island = I == 5
    assert island.sum() == 2 * radius and same(out[island], Hh[island])
    assert same(out[~island][:, :3], F[~island][:, :3]) and np.all(out[~island][:, 3] == 3.0)
    I[5:6 + 2 * radius, 8:9 + 2 * radius] = 5  # a block of (2 radius + 1)^2: its corners count (radius + 1)^2 >= 2 radius + 1 records
    out = emu.clamp(abi.antilag(radius=radius), F, G, I, Hh)
    assert same(out[..., :3], F[..., :3])
    # the normal test does the same for a surface pixel, and not for the background
    G[7, 8:8 + 2 * radius, :3] = (1.0, 0.0, 0.0)
    I[...] = 3
    out = emu.clamp(abi.antilag(radius=radius), F, G, I, Hh)
    turned = G[..., 0] == 1.0
    assert same(out[turned], Hh[turned]) and same(out[~turned][:, :3], F[~turned][:, :3])
    I[...] = tu.BACKGROUND
    assert same(emu.clamp(abi.antilag(radius=radius), F, G, I, Hh)[..., :3], F[..., :3])


def test_invalid_records_are_skipped_and_untouched(emu):
    """A NaN or len == 0 record of F' is no part of any window and its own pixel is left alone; so is a pixel whose H is NaN or nobody's."""
    from gpuspectral_amd import abi

    rng = np.random.default_rng(31)
    F, G, I, Hh = plane(12, 20, rng)
    F[3, 4, 1] = np.nan
    F[6, 10, 0] = np.inf
    F[8, 15] = (1e30, 1e30, 1e30, 0.0)
    Hh[2, 2, 2] = np.nan
    Hh[9, 3, 3] = 0.0
    out = emu.clamp(abi.antilag(radius=3), F, G, I, Hh)
    alone = np.zeros((12, 20), bool)
    for y, x in ((3, 4), (6, 10), (8, 15), (2, 2), (9, 3)):
        alone[y, x] = True
    assert same(out[alone], Hh[alone])
    assert same(out[~alone][:, :3], np.tile(np.float32([0.25, 0.5, 0.75]), ((~alone).sum(), 1))) and np.all(out[~alone][:, 3] == 3.0)


def test_frame_corners_and_tiny_frames(emu):
    from gpuspectral_amd import abi

    rng = np.random.default_rng(41)
    for radius in (1, 2, 3):
        F, G, I, Hh = plane(9, 33, rng)
        out = emu.clamp(abi.antilag(radius=radius), F, G, I, Hh)
        for y, x in ((0, 0), (0, 32), (8, 0), (8, 32)):  # (radius + 1)^2 >= 2 radius + 1 records
            assert same(out[y, x], np.float32([0.25, 0.5, 0.75, 3.0]))
    # a frame smaller than the rule's count is left alone at every radius it is smaller for
    for (h, w), untouched in (((1, 1), (1, 2, 3)), ((1, 2), (1, 2, 3)), ((2, 2), (2, 3)), ((2, 3), (3,)), ((3, 3), ())):
        F, G, I, Hh = plane(h, w, rng)
        for radius in (1, 2, 3):
            out = emu.clamp(abi.antilag(radius=radius), F, G, I, Hh)
            assert same(out, Hh) if radius in untouched else same(out[..., :3], F[..., :3]), (h, w, radius)


@pytest.mark.parametrize("demod", [False, True], ids=["colour", "demod"])
def test_without_a_fast_history(emu, accumulate, cornell, demod):
    """fast_valid false -- the first call, or a frame after one without a call -- and history_valid false: F' = {x, 1} for a finite x, and
    the raw record with length 0 otherwise, whatever the long history holds."""
    fov = float(cornell.fov)
    frames = cornell_frames(cornell)
    cam, xf, f = frames[0]
    f = tuple(p.copy() for p in f)
    f[0][3, 4, 1] = np.nan
    first = accumulate.step(None, cam, fov, *f, hist=None, demod=demod)
    x = iu.frame64(f[0], f[1])
    want = np.where(x["u"][..., None], x["e"], f[0][..., :3]) if demod else f[0][..., :3]
    fin = x["u"] if demod else np.isfinite(f[0][..., :3]).all(-1)
    F0, _ = emu.step(None, None, cam, fov, *f, first, demod=demod)
    assert same(F0[..., :3], first.H[..., :3]) and np.array_equal(F0[..., 3], fin.astype(np.float32)) and not fin[3, 4]
    assert np.allclose(F0[..., :3][fin], want[fin], rtol=4 * U32, atol=0)
    cam1, _, f1 = frames[1]
    second = accumulate.step(None, cam1, fov, *f1, hist=first, demod=demod)
    assert second.H[..., 3].max() == 2.0
    # a long history without a fast one (the frame before had no call), and a fast plane without a long history (it was invalidated)
    for old, fast in ((first, None), (None, F0)):
        F1, _ = emu.step(None, None, cam1, fov, *f1, second, old=old, fast=fast, demod=demod)
        assert np.all(F1[..., 3] == 1.0)
    F1, _ = emu.step(None, None, cam1, fov, *f1, second, old=first, fast=F0, demod=demod)
    assert F1[..., 3].max() == 2.0 and (F1[..., 3] == 2.0).mean() > 0.5


# ---- defaults, the struct_size rule, validation ------------------------------------------------------------------------------------------------
def test_defaults_and_struct_size_prefix(emu):
    from gpuspectral_amd import abi

    want = dict(fast_history=4.0, radius=2, sigma_scale=2.0)
    assert emu.resolve(None) == (want, None)
    assert emu.resolve(abi.antilag()) == (want, None)
    assert emu.resolve(abi.Antilag(0, 99, 99, -1.0)) == (want, None)  # struct_size 0: nothing of the struct is read
    assert emu.resolve(abi.Antilag(8, 7, 99, -1.0)) == (dict(want, fast_history=7.0), None)  # ... 8: fast_history alone
    assert emu.resolve(abi.Antilag(12, 7, 3, -1.0)) == (dict(want, fast_history=7.0, radius=3), None)
    assert emu.resolve(abi.Antilag(64, 64, 1, 0.5)) == (dict(fast_history=64.0, radius=1, sigma_scale=0.5), None)  # a larger struct: its prefix
    assert emu.resolve(abi.antilag(1, 3, 1e-30))[0] == dict(fast_history=1.0, radius=3, sigma_scale=float(np.float32(1e-30)))


@pytest.mark.parametrize("kw,word", [
    (dict(fast_history=65), "gsp_antilag.fast_history"), (dict(fast_history=1 << 31), "gsp_antilag.fast_history"), (dict(radius=4), "gsp_antilag.radius"),
    (dict(radius=0xFFFFFFFF), "gsp_antilag.radius"), (dict(sigma_scale=-1.0), "gsp_antilag.sigma_scale"), (dict(sigma_scale=float("nan")), "gsp_antilag.sigma_scale"),
    (dict(sigma_scale=float("inf")), "gsp_antilag.sigma_scale"), (dict(fast_history=65, radius=4, sigma_scale=-1.0), "gsp_antilag.fast_history"),
    (dict(radius=4, sigma_scale=-1.0), "gsp_antilag.radius"),
])
def test_validation(emu, kw, word):
    from gpuspectral_amd import abi

    got, err = emu.resolve(abi.antilag(**kw))
    assert got is None and word in err, err
    F, G, I, Hh = plane(3, 3)
    with pytest.raises(ValueError):
        emu.clamp(abi.antilag(**kw), F, G, I, Hh)


# ---- a program of its own under the sanitizers ---------------------------------------------------------------------------------------------------
def test_emulation_under_sanitizers(tmp_path):
    """tests/emu/antilag_main.cpp: the emulation over a 33 x 9 and a 1 x 1 frame at radius 3 under ASan / UBSan, on planes of exactly the
    frame's size; run directly, nothing is loaded into Python."""
    exe = str(tmp_path / "antilag_main")
    au.build_main(exe)
    r = subprocess.run([exe, "3"], capture_output=True, text=True)
    assert r.returncode == 0 and "33 x 9:" in r.stdout and "1 x 1:" in r.stdout, r.stdout + r.stderr
