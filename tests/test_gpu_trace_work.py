"""The traversal statistics of gsp_render (collect_traversal_stats, gsp_debug_visit_histograms) and, through them, the WORK per ray
of the wave traversal: what the hit references cannot see.  As in tests/test_gpu_trace_edits.py nothing here looks into the node
array: only the public API and the statistics hooks.  The CPU side -- the product's per-ray traversal against two plain references,
with mutants -- is tests/test_trace_work_cpu.py.

Which rays the counters cover (pt_render_pipeline.inc, lane_enqueue): a call with collect_traversal_stats != 0 uses no primary-hit
memo (so there is no memo build and no memoised ray) and never hands the tail of a drain to k_finish; every path segment and every
shadow ray of the call is traced by the STATS instantiation of k_trace.  So stat_rays == extension_rays and shadow_stat_rays ==
shadow_rays for such a call, on both context fixtures (GSP_FINISH_PATHS only matters without statistics), and a split scene is put
back into one tree first.  The histograms of mode 2 cover the closest-hit (extension) rays only and add up over calls until they are
read.  gsp_trace adds nothing to any counter.

The gates of the per-octant and occlusion tests come from ONE calibration run of a library whose build-time child order was
negated (the `order_key negated` mutant of the CPU tests; it cannot change a result), which is not committed: the figures are in
profiles/trace_work_gpu.txt and DESIGN.md "Work per ray".
"""
import math

import numpy as np
import pytest

import trace_work as W

pytestmark = pytest.mark.gpu

FRAME = 64
STAT_KEYS = ("nodes_visited", "tris_tested", "stat_rays", "shadow_nodes_visited", "shadow_tris_tested", "shadow_stat_rays", "nodes_from_lds",
             "shadow_nodes_from_lds", "shadow_stat_occluded", "shadow_stat_occluded_nodes", "shadow_stat_no_triangle", "algorithmic_bytes")
RAY_KEYS = ("extension_rays", "shadow_rays", "shaded_vertices")
TOP_NODES = 64  # records of the node array that k_trace serves from LDS (pt_trace.h kTopNodes)


@pytest.fixture(scope="module", params=["default", "wavefront-only"])
def ctx(request):
    """As tests/test_gpu_parity.py: the defaults, and GSP_FINISH_PATHS=0 (every bounce in the wavefront kernels)."""
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


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def lattice_scene(nx, ny, nz, eye, target, fov_deg=30.0, shift=(0.0, 0.0, 0.0)):
    """W.lattice as ONE-SIDED inward-wound boxes: seen from outside every hit is a back face of a one-sided surface, where the path
    ends (rayhit.rchit:776-779), so a frame of it traces camera rays only -- extension_rays == pixels * spp, no shadow rays."""
    from gpuspectral_amd import scenes

    b = scenes.SceneBuilder()
    pos = W.lattice(nx, ny, nz).reshape(-1, 3)
    nrm = np.zeros_like(pos)
    nrm[:, 1] = 1.0
    b.add_object(b.add_mesh(pos, nrm), scenes.trs(shift), b.diffuse((0.5, 0.5, 0.5)), twofaced=False)
    b.camera_lookat(eye, target, fov_deg=fov_deg)
    return b.build()


VIEWS = [tuple(-1.0 if k >> a & 1 else 1.0 for a in range(3)) for k in range(8)]  # the camera's side; the rays run the other way
VIEW_DISTANCE = 14.0


def octant_view(side, n=6):
    """The n^3 lattice from the diagonal `side`, looking at its centre with fov 30 degrees: the corner rays of the frame are 20.7
    degrees off the axis and the diagonal 35.3 degrees off every coordinate plane, so every camera ray has the signs of -side."""
    c = 0.5 * (n - 0.5)
    eye = tuple(c + VIEW_DISTANCE / math.sqrt(3.0) * s for s in side)
    return lattice_scene(n, n, n, eye, (c, c, c))


def layered_view(layers, back):
    """6 x 6 boxes with `layers` more layers along z behind the first, seen along (0.1, 0.1, -1) -- or, `back`, from the opposite
    side along (-0.1, -0.1, 1).  The first layer and the camera are the same whatever lies behind."""
    d = np.array([-0.1, -0.1, 1.0] if back else [0.1, 0.1, -1.0])
    d /= np.linalg.norm(d)
    first = np.array([2.75, 2.75, 0.25])
    return lattice_scene(6, 6, 1 + layers, tuple(first - 12.0 * d), tuple(first), shift=(0.0, 0.0, 0.0 if back else -float(layers)))


def small_tree_scene(ntris):
    """The generator of tests/test_gpu_parity.py::test_trees_around_the_size_of_the_lds_node_copy."""
    from gpuspectral_amd import scenes

    rng = np.random.RandomState(1000 + ntris)
    b = scenes.SceneBuilder()
    c = rng.uniform(-1, 1, (ntris, 1, 3))
    tris = (c + rng.normal(size=(ntris, 3, 3)) * 0.15).astype(np.float32).reshape(-1, 3)
    nrm = np.zeros_like(tris)
    nrm[:, 1] = 1.0
    b.add_object(b.add_mesh(tris, nrm), scenes.trs(), b.diffuse((0.6, 0.6, 0.6)))
    b.add_object(b.add_mesh(*scenes.rect_mesh()), scenes.trs((0, 1.8, 0), 0.5, 0.0), b.diffuse((0, 0, 0)), twofaced=True, emission=(9, 9, 9))
    b.camera_lookat((0.2, 0.4, 3.5), (0, 0, 0), fov_deg=45)
    return b.build()


def named_scene(name):
    from gpuspectral_amd import scenes

    if name == "materials":
        return scenes.cornell_materials(8)
    if name == "textured":
        import textured

        return textured.decorate(textured.open_scene(8), seed=3)
    return small_tree_scene(int(name))


def frame(ctx, spp=2, mode=1, size=(FRAME, FRAME), first_timestamp=0, **overrides):
    """One frame of the uploaded scene from zeroed counters: (statistics, image)."""
    ctx.reset_stats()
    ctx.frame_begin(*size)
    ctx.render(spp=spp, first_timestamp=first_timestamp, collect_traversal_stats=mode, **overrides)
    img = ctx.download().copy()
    return ctx.stats(), img


def per_ray(st):
    """(node records, triangle tests) per extension ray, and the same per shadow ray (nan without shadow rays)."""
    e, s = max(st["stat_rays"], 1), st["shadow_stat_rays"]
    return (st["nodes_visited"] / e, st["tris_tested"] / e, st["shadow_nodes_visited"] / s if s else float("nan"), st["shadow_tris_tested"] / s if s else float("nan"))


# ---- 1. statistics change no result ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["materials", "textured"])
def test_statistics_change_no_result(ctx, name):
    """The same frame with collect_traversal_stats = 0, 1, 2: the image is bit-equal and the path-segment, shadow-ray and vertex counts
    are equal, although mode 0 answers camera rays from the memo and may finish in k_finish and the others do neither."""
    ctx.upload_scene(named_scene(name))
    runs = [frame(ctx, spp=2, mode=m) for m in (0, 1, 2)]
    ctx.visit_histograms()  # (drops the histograms of the mode-2 call)
    for st, img in runs[1:]:
        assert np.array_equal(img.view(np.uint32), runs[0][1].view(np.uint32))
        assert [st[k] for k in RAY_KEYS] == [runs[0][0][k] for k in RAY_KEYS]
    assert runs[0][0]["extension_rays"] > FRAME * FRAME * 2 and runs[0][0]["shadow_rays"] > 0
    assert all(runs[0][0][k] == 0 for k in STAT_KEYS), "a call without statistics fills no traversal counter"
    for st, _ in runs[1:]:
        assert st["stat_rays"] == st["extension_rays"] and st["shadow_stat_rays"] == st["shadow_rays"], "a statistics call covers every ray it traces"


# ---- 2. identities ------------------------------------------------------------------------------------------------------------------------
def primary_rays(orc_scene, w, h):
    rays = np.zeros((w * h, 8), np.float32)
    for y in range(h):
        for x in range(w):
            r = orc_scene.primary_ray(w, h, x, y)
            rays[y * w + x, 0:3], rays[y * w + x, 4:7] = r[0:3], r[3:6]
    rays[:, 7] = 1e10
    return rays


def check_identities(st, node_hist, slot_hist):
    """What the counters of ONE statistics call (mode 2) and the histograms read after it owe each other, exactly."""
    assert int(node_hist.sum()) == st["nodes_visited"] and int(slot_hist.sum()) == st["tris_tested"]
    assert int(node_hist[0]) == st["stat_rays"], "every closest-hit ray reads the root record exactly once"
    if st["num_bvh_nodes"] > TOP_NODES:
        assert int(node_hist[:TOP_NODES].sum()) == st["nodes_from_lds"] < st["nodes_visited"]
    else:
        assert st["nodes_from_lds"] == st["nodes_visited"] and st["shadow_nodes_from_lds"] == st["shadow_nodes_visited"]
    assert st["shadow_nodes_from_lds"] <= st["shadow_nodes_visited"]
    assert st["algorithmic_bytes"] == (48 * st["stat_rays"] + 64 * st["nodes_visited"] + 48 * st["tris_tested"] + 32 * st["shadow_stat_rays"]
                                       + 36 * st["shadow_stat_occluded"] + 64 * st["shadow_nodes_visited"] + 48 * st["shadow_tris_tested"])
    assert st["shadow_stat_occluded"] <= st["shadow_stat_rays"] and st["shadow_stat_occluded_nodes"] <= st["shadow_nodes_visited"]
    assert st["shadow_stat_no_triangle"] <= st["shadow_stat_rays"] - st["shadow_stat_occluded"], "an occluded ray has tested a triangle"
    assert st["shadow_stat_rays"] <= st["shadow_nodes_visited"], "every shadow ray reads the root record"


@pytest.mark.parametrize("name", ["3", "40", "130", "260", "700", "materials"])
def test_counter_identities(ctx, oracle_mod, name):
    """Mode 2 on trees of 1 to ~240 records (at most 64: everything comes from the LDS copy; more: exactly the first 64 indices do):
    the histograms add up to the counters, the root is read once per ray, algorithmic_bytes is its formula, the shadow counters
    nest, at least as many slots were tested as the camera rays hit distinct triangles (which slot a triangle lives in is not
    public, so the slots a hit names are counted, not matched), and the all-zero padding slots around the triangles are never
    tested (an unused child position carries an inverted box, which no ray hits: pt_trace.h)."""
    sc = named_scene(name)
    ctx.upload_scene(sc)
    st, _ = frame(ctx, spp=1, mode=2)
    node_hist, slot_hist = ctx.visit_histograms()
    assert st["stat_rays"] == st["extension_rays"] > FRAME * FRAME and st["shadow_stat_rays"] == st["shadow_rays"] > 0
    assert len(node_hist) == st["num_bvh_nodes"] and len(slot_hist) == st["num_triangles"] + 8
    check_identities(st, node_hist, slot_hist)
    print("%s: %d records, %.2f / %.2f records per extension / shadow ray, %.2f / %.2f triangles" % (
        (name, st["num_bvh_nodes"]) + tuple(per_ray(st)[k] for k in (0, 2, 1, 3))))
    # slots: 4 leading and 4 trailing all-zero triangles around the scene's (pt_bvh.hip kFirstSlot, kWide)
    assert int(slot_hist[:4].sum()) == 0 and int(slot_hist[4 + st["num_triangles"]:].sum()) == 0, "a padding slot was tested"
    hit = ctx.trace(primary_rays(oracle_mod.Oracle(sc), FRAME, FRAME))["prim"]
    assert int((slot_hist > 0).sum()) >= len(np.unique(hit[hit >= 0])) > 0, "fewer slots were tested than distinct triangles were hit"


def test_counters_reset_hold_and_add_up(ctx):
    """Zero after gsp_reset_stats; untouched by a call without statistics and by gsp_trace; the same call twice adds the same ray
    counts again, and -- closest-hit work depends on how the lanes of a wave happen to be batched, so not bit for bit -- the same
    work within the measured spread (profiles/trace_work_gpu.txt)."""
    ctx.upload_scene(named_scene("materials"))
    one, _ = frame(ctx, spp=2, mode=1)
    ctx.reset_stats()
    zero = ctx.stats()
    assert all(zero[k] == 0 for k in STAT_KEYS + RAY_KEYS)
    one_again, _ = frame(ctx, spp=2, mode=1)
    ctx.frame_begin(FRAME, FRAME)
    ctx.render(spp=2, collect_traversal_stats=0)
    ctx.trace(np.array([[0, 1, 5, 0, 0, 0, -1, 1e10]], np.float32))
    held = ctx.stats()
    assert [held[k] for k in STAT_KEYS] == [one_again[k] for k in STAT_KEYS] and held["extension_rays"] == 2 * one_again["extension_rays"]
    ctx.frame_begin(FRAME, FRAME)
    ctx.render(spp=2, collect_traversal_stats=1)
    two = ctx.stats()
    for k in ("stat_rays", "shadow_stat_rays", "shadow_stat_occluded"):
        assert two[k] == 2 * one_again[k] == 2 * one[k], k
    for k in ("nodes_visited", "tris_tested", "shadow_nodes_visited", "shadow_tris_tested", "nodes_from_lds"):
        assert abs(two[k] - 2 * one_again[k]) <= REPEAT_SPREAD * 2 * one_again[k] and abs(one[k] - one_again[k]) <= REPEAT_SPREAD * one[k], k


# ---- 3. all eight octants -------------------------------------------------------------------------------------------------------------------
# Calibration (profiles/trace_work_gpu.txt): node records per camera ray of octant_view(side), the product and the order mutant.
# Bound per view = sqrt(product * mutant).  Three fresh processes and three calls in each gave the SAME counters for these
# camera-ray frames (and num_bvh_nodes = 1311 every time); full-path frames repeat their ray counts exactly and their work to
# 8.8e-4 (tris_tested; closest-hit culling depends on how the lanes of a wave are batched).  REPEAT_SPREAD is twice that, rounded up,
# and widens every gate below.
REPEAT_SPREAD = 0.002
OCTANT_NODES = {  # camera side -> node records per camera ray (product, mutant)
    (1.0, 1.0, 1.0): (8.4846, 13.4443), (-1.0, 1.0, 1.0): (8.4697, 13.3894), (1.0, -1.0, 1.0): (8.5266, 13.4304), (-1.0, -1.0, 1.0): (8.4602, 13.3281),
    (1.0, 1.0, -1.0): (8.4099, 13.2815), (-1.0, 1.0, -1.0): (8.3792, 13.1401), (1.0, -1.0, -1.0): (8.4600, 13.4067), (-1.0, -1.0, -1.0): (8.3242, 13.0356)}
OCTANT_SPREAD = 1.0243  # max / min of the product's eight views


def test_all_eight_octants(ctx):
    """The 6^3 lattice from the eight diagonals, camera rays only: node records per ray stay below the geometric mean of the
    product's and the order mutant's calibration figures in every octant, and the eight octants cost the same within the measured
    spread x 1.15 -- a wrong sign, exchanged axis bits or a wrong table row for one octant shows as that octant reading more."""
    got = {}
    for side in VIEWS:
        ctx.upload_scene(octant_view(side))
        st, _ = frame(ctx, spp=1, mode=1, max_depth=0)
        assert st["stat_rays"] == st["extension_rays"] == FRAME * FRAME and st["shadow_rays"] == 0, "camera rays only"
        got[side] = per_ray(st)[0]
        print("side %s: %.3f records, %.3f triangles per ray" % (side, got[side], per_ray(st)[1]))
    for side in VIEWS:
        product, mutant = OCTANT_NODES[side]
        assert mutant / product >= 1.2
        assert got[side] <= math.sqrt(product * mutant) * (1.0 + REPEAT_SPREAD), (side, got[side], product, mutant)
    assert max(got.values()) / min(got.values()) <= OCTANT_SPREAD * 1.15 * (1.0 + REPEAT_SPREAD)


# ---- 4. work does not grow with what is hidden ----------------------------------------------------------------------------------------------
LAYER_TRIS = {  # (layers behind the first, back) -> triangle tests per camera ray that hits (product, mutant); calibration run
    (1, False): (2.9460, 5.7884), (2, False): (3.1929, 6.7527), (6, False): (3.6036, 9.5817),
    (1, True): (3.1254, 5.7659), (2, True): (3.5562, 6.6462), (6, True): (3.5960, 9.5024)}


def test_work_does_not_grow_with_what_is_hidden(ctx):
    """One layer of boxes behind the first, or six: the triangles tested per camera ray that hits stay at the one-layer figure plus a
    margin, from both sides -- the running t culls what lies behind the hit.  The margin puts the bound at the geometric mean of
    the product's and the order mutant's six-layer figures of the calibration run."""
    for back in (False, True):
        got = {}
        for layers in (1, 2, 6):
            ctx.upload_scene(layered_view(layers, back))
            st, _ = frame(ctx, spp=1, mode=1, max_depth=0)
            assert st["stat_rays"] == FRAME * FRAME and st["shaded_vertices"] > FRAME * FRAME // 8
            got[layers] = st["tris_tested"] / st["shaded_vertices"]
        print("%s: triangles per hit ray with 1 / 2 / 6 layers behind: %.3f %.3f %.3f" % ("back" if back else "front", got[1], got[2], got[6]))
        product, mutant = LAYER_TRIS[(6, back)]
        assert mutant / product >= 1.2
        margin = math.sqrt(product * mutant) - LAYER_TRIS[(1, back)][0]
        assert margin > 0 and got[6] <= got[1] + margin * (1.0 + REPEAT_SPREAD), (back, got, margin)


# ---- 5. reinsertion still pays ------------------------------------------------------------------------------------------------------------------
def test_reinsertion_still_pays():
    """interior(20000) at 96 x 64 x 2 spp, the default build against GSP_BVH_REINSERT=0 (reinsert_rounds = 1: none): the same image and
    ray counts, and NOT MORE node records per extension ray and per shadow ray.  The ordering only; the measured reduction is in
    DESIGN.md "Work per ray"."""
    import gpuspectral_amd as g
    from gpuspectral_amd import scenes

    sc = scenes.interior(20000, seed=7)
    out = {}
    for rounds in (1, 0):  # (gsp_ctx_options.reinsert_rounds: 1 = no round, 0 = the default 6)
        with g.Context(0, reinsert_rounds=rounds) as c:
            c.upload_scene(sc)
            out[rounds] = frame(c, spp=2, mode=1, size=(96, 64))
    (without, img0), (default, img1) = out[1], out[0]
    assert np.array_equal(img0, img1) and [without[k] for k in RAY_KEYS] == [default[k] for k in RAY_KEYS]
    a, b = per_ray(without), per_ray(default)
    print("records per extension / shadow ray: without reinsertion %.3f / %.3f, default %.3f / %.3f (%+.1f %% / %+.1f %%)" % (
        a[0], a[2], b[0], b[2], 100 * (b[0] / a[0] - 1), 100 * (b[2] / a[2] - 1)))
    assert b[0] <= a[0] and b[2] <= a[2]


# ---- 6. a refit is paid for in work, a rebuild is not -----------------------------------------------------------------------------------------
def test_a_refit_is_paid_for_in_work_and_a_rebuild_is_not():
    """The far move of tests/test_gpu_scene_updates.py::test_update_instances_refits_then_rebuilds: the largest object of
    interior(40000) leaves the room.  With the default options the tree is rebuilt and a ray costs what it costs after a fresh upload
    of the moved scene (within the repeat spread); with refit_growth = 1e30 the old topology is kept and a ray does not cost less."""
    import gpuspectral_amd as g
    from gpuspectral_amd import scenes

    sc = scenes.interior(40_000)
    base = sc.instances.copy()
    k = int(np.argmax(base["vertex_count"]))
    moved = base.copy()
    t = moved["transform"][k].copy()
    t[12:15] += np.float32(60.0) * np.array([1.0, 0.3, -0.5], np.float32)
    moved["transform"][k] = t
    got = {}
    for road, growth in (("default", 0.0), ("forced refit", 1e30)):
        with g.Context(0, refit_growth=growth) as c:
            c.upload_scene(sc)
            c.update_instances(moved)
            st, img = frame(c, spp=2, mode=1)
            assert st["scene_refits"] == (1 if growth else 0), (road, st["scene_refits"])
            got[road] = (per_ray(st), img, [st[q] for q in RAY_KEYS])
    sc.instances = moved
    try:
        with g.Context(0) as c:
            c.upload_scene(sc)
            st, img = frame(c, spp=2, mode=1)
            got["fresh"] = (per_ray(st), img, [st[q] for q in RAY_KEYS])
    finally:
        sc.instances = base
    for road in ("default", "forced refit"):
        assert np.array_equal(got[road][1], got["fresh"][1]) and got[road][2] == got["fresh"][2]
    f, d, r = got["fresh"][0], got["default"][0], got["forced refit"][0]
    print("records per extension / shadow ray: fresh %.3f / %.3f, default road %.3f / %.3f, forced refit %.3f / %.3f" % (f[0], f[2], d[0], d[2], r[0], r[2]))
    for i in (0, 2):
        assert abs(d[i] - f[i]) <= REPEAT_SPREAD * f[i]
        assert r[i] >= f[i] * (1.0 - REPEAT_SPREAD)
