"""Adaptive sampling (include/gpuspectral_pt.h, ABI 9) on the GPU.

A pixel that stops after N_p samples must hold exactly the uniform image of that pixel at N_p samples: the oracle renders each
group of pixels that stopped together at its N_p, and every pixel is compared bit for bit.  The stopping rule, m2, the
invariance under call splits / timestamps in flight / lanes, pixel subsets, the edges and the refusals follow."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W = H = 64
MIN, STEP, MAX = 8, 8, 64
THRESHOLDS = (0.02, 0.03, 0.05, 0.07, 0.1, 0.15, 0.2, 0.3, 0.5)


@pytest.fixture(scope="module", params=["default", "wavefront-only"])
def ctx(request):
    """Like tests/test_gpu_parity.py: once with the defaults (frames this small drain in k_finish) and once with
    GSP_FINISH_PATHS=0, which keeps every bounce of every round in the wavefront kernels the bench measures."""
    import os

    import gpuspectral_amd as g

    old = os.environ.get("GSP_FINISH_PATHS")
    if request.param == "wavefront-only":
        os.environ["GSP_FINISH_PATHS"] = "0"
    try:
        c = g.Context(0)
    finally:
        if old is None:
            os.environ.pop("GSP_FINISH_PATHS", None)
        else:
            os.environ["GSP_FINISH_PATHS"] = old
    yield c
    c.close()


def adaptive(ctx, sc, threshold, calls=(MAX,), pixel_ids=None, upload=True, **kw):
    """Frame of adaptive calls with spp = calls[i]; returns (compact colours, m2, spp, stats)."""
    if upload:
        ctx.upload_scene(sc)
    ctx.frame_begin(W, H, pixel_ids=pixel_ids)
    ctx.reset_stats()
    t = 0
    for s in calls:
        ctx.render(spp=s, first_timestamp=t, adaptive_threshold=threshold, adaptive_min_spp=MIN, adaptive_step=STEP, **kw)
        t += s
    img = ctx.download_compact()
    m2, spp = ctx.pixel_stats()
    return img, m2, spp, ctx.stats()


_PICKED = {}


def pick_threshold(ctx, sc):
    """The first threshold of THRESHOLDS whose frame has >= 3 distinct counts and 10-90 % of the pixels stopped early
    (the choice depends on the scene only: the result does not depend on the context's options)."""
    if id(sc) in _PICKED:
        return _PICKED[id(sc)]
    for i, t in enumerate(THRESHOLDS):
        _, _, spp, _ = adaptive(ctx, sc, t, upload=i == 0)
        early = float((spp < MAX).mean())
        if len(np.unique(spp)) >= 3 and 0.1 <= early <= 0.9:
            _PICKED[id(sc)] = t
            return t
    pytest.fail("no threshold of %s splits the frame into >= 3 counts with 10-90 %% stopping early" % (THRESHOLDS,))


def check_against_oracle(oracle_mod, sc, img, spp, st, pixel_ids=None):
    """Every pixel == the oracle's uniform render of its pixel at its own count; samples and extension rays add up."""
    o = oracle_mod.Oracle(sc)
    ids_all = np.arange(W * H, dtype=np.uint32) if pixel_ids is None else np.asarray(pixel_ids, np.uint32)
    ext = 0
    for n in np.unique(spp):
        sel = np.nonzero(spp == n)[0]
        ref, ost = o.render(W, H, spp=int(n), pixel_ids=ids_all[sel])
        ext += ost["extension_rays"]
        bad = np.nonzero(np.any(img[sel] != ref, axis=1))[0]
        assert len(bad) == 0, "N_p = %d: %d of %d pixels differ from the oracle (first: pixel %d)" % (n, len(bad), len(sel), ids_all[sel][bad[0]])
    assert st["samples"] == int(spp.astype(np.int64).sum())
    assert st["extension_rays"] == ext


@pytest.mark.parametrize("which", ["cornell", "materials"])
def test_per_pixel_bit_exact(ctx, oracle_mod, cornell, materials_scene, which):
    sc = cornell if which == "cornell" else materials_scene
    t = pick_threshold(ctx, sc)
    img, m2, spp, st = adaptive(ctx, sc, t)
    assert set(np.unique(spp)) <= set(range(MIN, MAX + 1, STEP))
    assert st["adaptive_active_pixels"] <= int((spp == MAX).sum())
    check_against_oracle(oracle_mod, sc, img, spp, st)


def rule_accepts(mean, m2, n, threshold):
    """The stopping rule of include/gpuspectral_pt.h in float64, and each pixel's distance from its boundary."""
    m = np.asarray(mean, np.float64)
    yb = 0.2126 * m[:, 0] + 0.7152 * m[:, 1] + 0.0722 * m[:, 2]
    n = np.float64(n)
    var = np.maximum(np.asarray(m2, np.float64) - yb * yb, 0.0) * n / (n - 1.0)
    err = np.sqrt(var / n)
    bound = np.float64(np.float32(threshold)) * np.maximum(yb, 1e-3)
    return err <= bound, np.abs(err - bound) <= 1e-5 * bound


def test_rule_consistency(ctx, cornell):
    t = pick_threshold(ctx, cornell)
    ctx.upload_scene(cornell)
    ctx.frame_begin(W, H)
    prev = None
    near_total = 0
    for k, n in enumerate(range(MIN, MAX + 1, STEP)):
        ctx.render(spp=STEP, first_timestamp=n - STEP, adaptive_threshold=t, adaptive_min_spp=MIN, adaptive_step=STEP)
        img = ctx.download_compact()
        m2, spp = ctx.pixel_stats()
        assert spp.max() == n
        if prev is not None:
            # the pixels that reached the previous checkpoint and did not go on are exactly those the rule accepted there
            stopped = prev["reached"] & (spp == n - STEP)
            acc, near = prev["accept"], prev["near"]
            assert np.array_equal(stopped[~near], (prev["reached"] & acc)[~near])
        reached = spp == n
        acc, near = rule_accepts(img, m2, n, t)
        near &= reached
        near_total += int(near.sum())
        prev = dict(reached=reached, accept=acc, near=near)
    assert ctx.stats()["adaptive_active_pixels"] >= int((prev["reached"] & ~prev["accept"] & ~prev["near"]).sum())
    assert ctx.stats()["adaptive_active_pixels"] <= int((prev["reached"] & (~prev["accept"] | prev["near"])).sum())
    assert near_total <= max(4, W * H // 500), "%d pixels within 1e-5 of the rule's boundary" % near_total


def test_second_moment(ctx, oracle_mod, materials_scene):
    """m2 == the running mean of Y^2 of the per-sample values, recovered from one-timestamp oracle renders."""
    sc = materials_scene
    T = 16
    ids = np.arange(0, W * H, 7, dtype=np.uint32)
    ctx.upload_scene(sc)
    ctx.frame_begin(W, H)
    ctx.render(spp=T, adaptive_threshold=1e-30, adaptive_min_spp=T, adaptive_step=T)
    m2, spp = ctx.pixel_stats()
    assert np.all(spp == T)
    o = oracle_mod.Oracle(sc)
    run = np.zeros(len(ids), np.float64)
    for t in range(T):
        acc, _ = o.render(W, H, spp=1, first_timestamp=t, pixel_ids=ids)  # = sample / (t + 1) on a zero buffer
        c = acc[:, :3].astype(np.float64) * (t + 1)
        y = 0.2126 * c[:, 0] + 0.7152 * c[:, 1] + 0.0722 * c[:, 2]
        run = y * y if t == 0 else run + (y * y - run) / (t + 1)
    np.testing.assert_allclose(m2[ids], run, rtol=1e-4, atol=1e-7)


def test_invariance(ctx, cornell):
    import gpuspectral_amd as g

    t = pick_threshold(ctx, cornell)
    base = adaptive(ctx, cornell, t)
    variants = {
        "8 x 8": adaptive(ctx, cornell, t, calls=(8,) * 8, upload=False),
        "5 + 11 + 48": adaptive(ctx, cornell, t, calls=(5, 11, 48), upload=False),
        "timestamps_in_flight 1": adaptive(ctx, cornell, t, upload=False, timestamps_in_flight=1),
    }
    opts = g.abi.CtxOptions()
    C.memmove(C.byref(opts), C.byref(ctx.options), C.sizeof(opts))
    with g.Context(0, options=opts, lanes=2) as c2:
        variants["lanes 2"] = adaptive(c2, cornell, t)
    for name, (img, m2, spp, st) in variants.items():
        assert np.array_equal(img, base[0]), name
        assert np.array_equal(spp, base[2]), name
        assert np.array_equal(m2, base[1]), name
        assert st["samples"] == base[3]["samples"], name


def test_pixel_subset(ctx, cornell):
    """A tile share of the frame stops the same pixels at the same counts as the full-frame render."""
    from gpuspectral_amd import multigpu

    t = pick_threshold(ctx, cornell)
    full = adaptive(ctx, cornell, t)
    ids = np.array(multigpu.tile_pixel_ids(W, H, 1, 3, tile=16))
    img, m2, spp, st = adaptive(ctx, cornell, t, pixel_ids=ids, upload=False)
    assert np.array_equal(img, full[0][ids])
    assert np.array_equal(spp, full[2][ids])
    assert np.array_equal(m2, full[1][ids])


def test_huge_threshold_stops_everything_at_min_spp(ctx, oracle_mod, cornell):
    img, m2, spp, st = adaptive(ctx, cornell, 1e30)
    assert np.all(spp == MIN)
    assert st["adaptive_active_pixels"] == 0 and st["samples"] == W * H * MIN
    ref, _ = oracle_mod.Oracle(cornell).render(W, H, spp=MIN)
    assert np.array_equal(img, ref)
    ctx.render(spp=8, first_timestamp=MAX, adaptive_threshold=1e30, adaptive_min_spp=MIN, adaptive_step=STEP)
    assert ctx.stats()["samples"] == W * H * MIN
    assert np.array_equal(ctx.download_compact(), ref)


def test_textured_scene_bit_exact(ctx, oracle_mod):
    """k_shade<true> (dormant-feature extension: textures + environment map) under adaptive sampling."""
    import textured

    sc = textured.decorate(textured.open_scene(12), seed=3)
    t = pick_threshold(ctx, sc)
    img, m2, spp, st = adaptive(ctx, sc, t)
    check_against_oracle(oracle_mod, sc, img, spp, st)


def test_refusals(ctx, cornell):
    import gpuspectral_amd as g

    def invalid(fn):
        with pytest.raises(g.pt.GspError) as e:
            fn()
        assert "failed (1)" in str(e.value), str(e.value)  # GSP_ERR_INVALID

    ctx.upload_scene(cornell)
    ctx.frame_begin(W, H)
    ctx.render(spp=2)
    invalid(lambda: ctx.render(spp=2, first_timestamp=2, adaptive_threshold=0.1))  # uniform frame, adaptive call
    invalid(lambda: ctx.pixel_stats())  # not an adaptive frame
    ctx.frame_begin(W, H)
    ctx.render(spp=4, adaptive_threshold=0.1)
    invalid(lambda: ctx.render(spp=2, first_timestamp=4))  # adaptive frame, uniform call
    invalid(lambda: ctx.render(spp=2, first_timestamp=3, adaptive_threshold=0.1))  # wrong first_timestamp
    invalid(lambda: ctx.upload_accum(np.zeros((W * H, 4), np.float32)))
    ctx.render(spp=2, first_timestamp=4, adaptive_threshold=0.1)  # (the frame is still usable)
    with g.pt.MultiContext([0, 0]) as m:
        m.upload_scene(cornell)
        m.frame_begin(W, H)
        invalid(lambda: m.render(spp=2, adaptive_threshold=0.1))


def test_work_saved(ctx, cornell):
    """At a threshold where >= 60 % of the pixels stop at min_spp, the extension rays are <= 0.6 x the uniform frame's."""
    ctx.upload_scene(cornell)
    ctx.frame_begin(W, H)
    ctx.reset_stats()
    ctx.render(spp=MAX)
    uniform = ctx.stats()["extension_rays"]
    for t in (0.05, 0.1, 0.2, 0.3, 0.5, 1.0):
        _, _, spp, st = adaptive(ctx, cornell, t, upload=False)
        if (spp == MIN).mean() >= 0.6:
            break
    assert (spp == MIN).mean() >= 0.6
    assert st["extension_rays"] <= 0.6 * uniform, (st["extension_rays"], uniform)
