"""gsp_trace on trees that were NOT built for the geometry they hold, against the BVH-free reference of tests/trace_reference.py:
the geometry is brought to its final place by gsp_update_instances through each of its roads -- in-place refit, the ring of whole
refitted trees, the split scene with its 64-slot ring, rebuild, drain -- and then asked the questions of
tests/test_gpu_trace_reference.py: closed meshes must not leak at vertices, edges and slab planes, lattice rays hit the exact
crossing, a sliver's hit does not depend on tmax.  Every trace is also bit-equal (prim, t, u, v) to the oracle built on the FINAL
scene, and every test asserts from gsp_get_stats which road it took.  The same cases as fresh scenes on the CPU tracers are the
control: tests/test_trace_reference_cpu.py."""
import hashlib

import numpy as np
import pytest

import trace_reference as R
from trace_scenes import build_scene

pytestmark = pytest.mark.gpu

FRAME = 16
# road -> (gsp_ctx_options fields, samples in flight before every edit: one 16x16 sample rendered and not waited for)
ROADS = {
    "in-place": (dict(refit_growth=1e30), False),  # the topology of the start placement is kept whatever happens to the boxes
    "ring": (dict(), True),
    "split": (dict(), True),
    "rebuild": (dict(refit_growth=1.0), True),
    "drain": (dict(geometry_versions=1), True),
}


@pytest.fixture(scope="module")
def contexts():
    """One context per set of options, made on first use."""
    import gpuspectral_amd as g
    from gpuspectral_amd import abi

    made = {}

    def get(road):
        if road not in made:
            made[road] = g.Context(0, options=abi.CtxOptions(**ROADS[road][0]))
        return made[road]

    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def shared():
    """{key: (final scene, its oracle)} and {(key, any_hit, digest of the rays): the oracle's hits}: one oracle and one answer per
    final scene, whatever road leads there."""
    return {}, {}


def same_records(a, b):
    return a.tobytes() == b.tobytes()


class Edited:
    """The meshes of a scene uploaded under start transforms and edited from there.  edit_to(transforms) is one
    gsp_update_instances (behind one sample in flight where the road has them); tracer(key, final) asserts the road from the
    statistics and returns trace(rays, any_hit), which asserts bit equality with the oracle of the final scene on every call."""

    def __init__(self, contexts, oracle_mod, shared, road, meshes, start, camera=None):
        self.ctx, self.oracle_mod, self.shared, self.road, self.meshes = contexts(road), oracle_mod, shared, road, meshes
        self.live = ROADS[road][1]
        sc = build_scene(list(zip(meshes, start)))
        if camera is not None:
            sc.to_world, sc.fov = camera
        self.inst = sc.instances.copy()
        self.ctx.upload_scene(sc)
        self.nodes = self.ctx.stats()["num_bvh_nodes"]
        self.edits = 0
        if self.live:
            self.ctx.frame_begin(FRAME, FRAME)

    def edit_to(self, transforms):
        if self.live:
            self.ctx.render(spp=1, first_timestamp=self.edits)  # no sync: these samples are in flight when the edit arrives
        from gpuspectral_amd import scenes

        inst = self.inst.copy()
        for i, t in enumerate(transforms):  # (None: the identity as build_scene writes it)
            inst["transform"][i] = scenes.trs() if t is None else np.asarray(t, np.float32).reshape(16)
        assert inst.tobytes() != self.inst.tobytes(), "an edit that changes nothing takes no road"
        self.ctx.update_instances(inst)
        self.inst = inst
        self.edits += 1

    def assert_road(self):
        st = self.ctx.stats()
        got = {k: st[k] for k in ("scene_updates", "scene_refits", "scene_splits", "scene_drains")}
        e = self.edits
        assert e > 0 and got["scene_updates"] == e, got
        if self.road == "in-place":  # an idle context: the tree built for the start placement, re-baked and re-encoded in place
            assert got == dict(scene_updates=e, scene_refits=e, scene_splits=0, scene_drains=0) and st["num_bvh_nodes"] == self.nodes, got
        elif self.road == "ring":  # a scene edited whole does not split; the first edit makes the ring behind a wait, later ones take its next slot
            assert e >= 2 and got == dict(scene_updates=e, scene_refits=e, scene_splits=0, scene_drains=1) and st["num_bvh_nodes"] == self.nodes, got
        elif self.road == "split":  # the first edit splits (without a wait), every later one refits the small tree into the next of 64 slots
            assert got == dict(scene_updates=e, scene_refits=e - 1, scene_splits=1, scene_drains=0), got
        elif self.road == "rebuild":
            assert got["scene_refits"] == 0 and got["scene_splits"] == 0, got
        elif self.road == "drain":  # no ring: every edit first completes the samples in flight, then refits in place
            assert got["scene_drains"] > 0 and got["scene_splits"] == 0 and got["scene_refits"] == e and st["num_bvh_nodes"] == self.nodes, got
        return got

    def tracer(self, key, final, probe=None):
        """final: the final scene's transforms (what the last edit_to was given).  probe: rays traced once BEFORE the statistics
        are read (gsp_get_stats completes the samples in flight): the answer must be the one given afterwards."""
        scenes, oracle_hits = self.shared
        sc = build_scene(list(zip(self.meshes, final)))
        assert sc.instances.tobytes() == self.inst.tobytes(), "the edits did not end at the final scene"
        if key not in scenes:
            scenes[key] = (sc, self.oracle_mod.Oracle(sc))
        assert scenes[key][0].instances.tobytes() == sc.instances.tobytes() and np.array_equal(scenes[key][0].positions, sc.positions)
        orc = scenes[key][1]
        early = self.ctx.trace(probe) if probe is not None else None
        self.assert_road()

        def trace(rays, any_hit):
            got = self.ctx.trace(rays, any_hit=any_hit)
            k = (key, any_hit, hashlib.sha1(np.ascontiguousarray(rays).tobytes()).hexdigest())
            if k not in oracle_hits:
                oracle_hits[k] = orc.trace(rays, any_hit=any_hit)
            want = oracle_hits[k]
            assert np.array_equal(got["prim"], want["prim"]), "%s via %s: GPU and oracle name different triangles on %d rays" % (
                key, self.road, (got["prim"] != want["prim"]).sum())
            hit = want["prim"] >= 0
            for f in ("t", "u", "v"):
                assert np.array_equal(np.ascontiguousarray(got[f][hit]).view(np.uint32), np.ascontiguousarray(want[f][hit]).view(np.uint32)), (key, self.road, f)
            return got

        if early is not None:
            assert same_records(early, trace(probe, False)), "%s via %s: the hits changed when the samples in flight completed" % (key, self.road)
        return trace


@pytest.fixture
def edited(contexts, oracle_mod, shared):
    """edited(road, key, meshes, path, probe=None, camera=None) -> trace: upload under path[0], one edit to each further entry
    of path; the last entry is the final scene."""

    def make(road, key, meshes, path, probe=None, camera=None):
        e = Edited(contexts, oracle_mod, shared, road, meshes, path[0], camera)
        for transforms in path[1:]:
            e.edit_to(transforms)
        return e.tracer(key, path[-1], probe)

    return make


def records(case, trace):
    """Every hit record the leak checks look at, as bytes."""
    out = [trace(case.inside_rays, False), trace(case.inside_rays, True), trace(case.grazing_rays, False)]
    if case.outside_rays is not None:
        out.append(trace(case.outside_rays, False))
    return [h.tobytes() for h in out]


# ---- (a) forced in-place refit on an idle context ---------------------------------------------------------------------------------
KEPT = [c for c in R.EDIT_CASES if c not in R.EDIT_DROPPED]


@pytest.mark.parametrize("name,target", KEPT)
def test_refit_in_place_to_every_target(edited, name, target):
    """The tree built for the mesh's unit placement (identity transform), refitted to the target: rotated, mirrored and stretched,
    shrunk a thousandfold to (100, 100, 100), enlarged ten-thousandfold, flattened to 1e-4.  No ray from inside leaks, at any vertex,
    edge or slab plane; rays from outside stop at the near side; every hit is the mesh's and bit-equal to the oracle's on the
    target scene.  Going there through an unrelated placement first gives the same records, bit for bit."""
    case = R.edit_case(name, target)
    meshes, final = [case.obj_tris], [R.EDIT_TARGETS[target]]
    trace = edited("in-place", case.key, meshes, [[None], final])
    n = R.check_no_leaks(case, trace, "in-place refit", prim_range=(0, len(case.obj_tris)))
    print("in-place refit, %s to %s: %d rays" % (name, target, n))
    one = records(case, trace)
    mid = R.EDIT_TARGETS["rotated" if target == "mirrored-stretched" else "mirrored-stretched"]
    two = records(case, edited("in-place", case.key, meshes, [[None], [mid], final]))
    assert one == two, "the hit records depend on the placement the tree came through"


@pytest.mark.parametrize("target", ["shrunk-far", "huge"])
@pytest.mark.parametrize("name", R.MESHES)
def test_refit_in_place_back_to_the_unit_placement(edited, name, target):
    """The other direction: the tree built for the mesh a thousand times smaller at (100, 100, 100) -- the slivers crumpled by
    rounding, vertices collapsed onto each other -- or ten thousand times larger, refitted to identity."""
    case = R.leak_case(name, "unit", False)
    meshes, start = [case.obj_tris], [R.EDIT_TARGETS[target]]
    key = ("unit", name)
    trace = edited("in-place", key, meshes, [start, [None]])
    n = R.check_no_leaks(case, trace, "in-place refit", prim_range=(0, len(case.obj_tris)))
    print("in-place refit, %s from %s to identity: %d rays" % (name, target, n))
    one = records(case, trace)
    two = records(case, edited("in-place", key, meshes, [start, [R.EDIT_TARGETS["flattened"]], [None]]))
    assert one == two, "the hit records depend on the placement the tree came through"


# ---- (b) the lattice after a refit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start,end", [("1", "2^-10@64"), ("2^12", "2^-3"), ("2^-3", "2^12")])
def test_lattice_after_a_refit(edited, start, end):
    """The lattice in lattice units under one placement's transform, refitted to another's: the world triangles are the exact
    ones (test_lattice_through_a_transform_is_the_lattice), so every ray must hit a triangle that contains the exact crossing
    point of the integer march at its exact parameter, shadow rays end on either side of it, and tmin past it finds the next."""
    ref = R.lattice_reference(8, 1)
    obj, _ = R.lattice_tris_through_transform(ref.solid, end)
    scale, offset = R.LATTICE_PLACEMENTS[end]
    trace = edited("in-place", ("lattice", 8, 1, end), [obj], [[R.lattice_transform(start)], [R.lattice_transform(end)]])
    worst = R.check_lattice(ref, scale, offset, trace, "in-place refit")
    print("in-place refit, lattice 8 from %s to %s: 4 x %d rays, worst relative t error %.3g (bound %.3g)" % (start, end, len(ref.first), worst, R.LATTICE_TOL))


# ---- (c) slivers after a refit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length,width", [(3.0, 2e-3), (3.0, 2e-5), (3.0, 3e-6)])  # aspect 3e3: below the pad's threshold of 32768; 3e5: above; 2e6
def test_sliver_hits_do_not_depend_on_tmax_after_a_refit(edited, length, width):
    """Uploaded under a rotation (no sliver axis-aligned: leaf boxes and pads of another shape), refitted to identity, which is
    exact: the world triangles are the case's own, and the pad is recomputed from them.  A reported hit is reported again, bit for
    bit, and occludes, when tmax shrinks to eight spacings beyond it."""
    assert (length, width) in R.SLIVER_SHAPES
    tris, rays = R.sliver_case(length, width)
    trace = edited("in-place", ("sliver", length, width), [tris], [[R.affine(R.random_rotation(12))], [None]])
    n = R.check_range_consistency(rays, trace, "in-place refit", min_hits=15000)
    print("in-place refit, slivers %g x %g: %d rays, %d hits checked twice more" % (length, width, len(rays), n))


# ---- (d) the ring of whole trees, (f) its controls -----------------------------------------------------------------------------------
def whole_scene_path(target):
    """Start 1.5 times as large and rotated otherwise, one placement in between (1.25 times, another rotation), the target: every
    tree is smaller than the built one, so the growth stays under the default bound."""
    m = R.EDIT_TARGETS[target].astype(np.float64).reshape(4, 4).T
    return [[R.affine(R.random_rotation(13) @ (1.5 * m[:3, :3]), m[:3, 3])], [R.affine(R.random_rotation(14) @ (1.25 * m[:3, :3]), m[:3, 3])],
            [R.EDIT_TARGETS[target]]]


@pytest.mark.parametrize("road", ["ring", "rebuild", "drain"])
@pytest.mark.parametrize("target", ["rotated", "mirrored-stretched"])
def test_whole_scene_edited_with_samples_in_flight(edited, target, road):
    """One instance, so nothing to split off: with the default options the first edit that arrives with samples in flight makes
    the ring of whole trees and the second is refitted into its next slot while those samples finish in theirs (`ring`).  The
    controls take the same edits through a context that always rebuilds and through one without a ring, where every edit first
    completes the samples in flight.  The first trace runs before anything has waited for them."""
    case = R.edit_case("icosphere", target)
    trace = edited(road, case.key, [case.obj_tris], whole_scene_path(target), probe=case.inside_rays)
    n = R.check_no_leaks(case, trace, road, prim_range=(0, len(case.obj_tris)))
    print("%s, icosphere to %s: %d rays" % (road, target, n))


# ---- (e) the split scene, (f) its controls ---------------------------------------------------------------------------------------------
def split_scene(contexts, oracle_mod, shared, road, name):
    from gpuspectral_amd import scenes

    ref = R.lattice_reference(*R.SPLIT_LATTICE)
    lat = ref.solid.world_tris(1.0, 0.0)
    b = scenes.SceneBuilder()
    b.camera_lookat((-1.6, 8.0, 4.0), (6.0, 8.0, 4.0), fov_deg=60.0)  # towards the lattice, the mover in view
    mesh = R.ClosedMesh(name, "unit")
    e = Edited(contexts, oracle_mod, shared, road, [lat, mesh.tris], [None, R.split_mover_transform(name, 0)], camera=(b.to_world, b.fov))
    return ref, lat, e


def check_split(ref, lat, e, name, step):
    case = R.split_mover_case(name, step)
    trace = e.tracer(("split", name, step), [None, R.split_mover_transform(name, step)], probe=case.inside_rays)
    n = R.check_no_leaks(case, trace, e.road, prim_range=(len(lat), len(case.obj_tris)))
    worst = R.check_lattice(ref, 1.0, 0.0, trace, e.road)
    print("%s, lattice 12 + %s after %d edits: %d mover rays, 4 x %d lattice rays (worst relative t error %.3g)" % (e.road, name, step, n, len(ref.first), worst))


def test_split_scene_after_4_and_70_edits(contexts, oracle_mod, shared):
    """The lattice (5728 triangles) stays, the icosphere beside it (1280 triangles) is rotated, rescaled between 0.8 and 1.0 and
    moved before every one-sample frame, no sync: the first edit splits the scene, every later one refits the small tree into the
    next slot of its ring.  After 4 edits, and after 70 (the 64 slots have wrapped), both trees are walked for every ray: the
    sphere must not leak -- a leak towards the lattice would name a lattice triangle -- and the lattice rays hit their exact crossings."""
    ref, lat, e = split_scene(contexts, oracle_mod, shared, "split", "icosphere")
    assert len(lat) == 5728 and len(ref.first) == 30634
    for step in range(1, 71):
        e.edit_to([None, R.split_mover_transform("icosphere", step)])
        if step in (4, 70):
            check_split(ref, lat, e, "icosphere", step)


@pytest.mark.parametrize("road", ["split", "rebuild", "drain"])
def test_split_scene_after_4_edits(contexts, oracle_mod, shared, road):
    """The torus as the mover (`split`), and the controls of the icosphere's four edits: always rebuild, and no ring."""
    name = "torus" if road == "split" else "icosphere"
    ref, lat, e = split_scene(contexts, oracle_mod, shared, road, name)
    for step in range(1, 5):
        e.edit_to([None, R.split_mover_transform(name, step)])
    check_split(ref, lat, e, name, 4)
