"""Ray hits against a BVH-free geometric reference (tests/trace_reference.py), on the CPU: first the reference's own inputs are
checked from the reference alone, then the oracle and the host emulation of the product's traversal (tests/emu: node_test /
intersect_tri) are held to it.  The GPU run of the same properties is tests/test_gpu_trace_reference.py; the cases that arrive
through a transform are the controls of tests/test_gpu_trace_edits.py, which reaches them by edits of a resident scene."""
import math

import numpy as np
import pytest

import trace_reference as R
from trace_scenes import build_scene

WHO = ["oracle", "emu"]


@pytest.fixture(scope="module")
def tracer(oracle_mod, emu):
    cache = {}

    def make(who, key, instances):
        if (who, key) not in cache:
            sc = build_scene(instances)
            cache[(who, key)] = oracle_mod.Oracle(sc) if who == "oracle" else emu.scene(sc)
        return cache[(who, key)].trace

    return make


# ---- the reference's own inputs, from the reference alone ---------------------------------------------------------------------
@pytest.mark.parametrize("name,placement,instanced", R.LEAK_CASES)
def test_origins_are_interior(name, placement, instanced):
    """Every origin of the inside rays has an odd crossing number in three directions of the float64 brute force over the very
    float32 triangles the tracers get; every edge is shared by two triangles whose vertices are one float32 triple."""
    case = R.leak_case(name, placement, instanced)
    crumpled = (name, placement) in R.CRUMPLED
    assert (4 <= len(case.origins) <= 8 if crumpled else len(case.origins) == 8) and R.crossing_parity(case.world_tris, case.origins).all()
    full = len(case.origins) * (len(case.mesh.verts) + 4 * len(case.mesh.edges))
    print("%d inside rays, %d slab-grazing rays" % (len(case.inside_rays), len(case.grazing_rays)))
    assert np.isfinite(case.inside_rays).all() and (0.9 * full < len(case.inside_rays) <= full if crumpled else len(case.inside_rays) == full)
    assert crumpled or R.thickness_in_ulps(case.world_tris.reshape(-1, 3)) > 16
    assert len(case.grazing_rays) > 200 or name.startswith("sliver")  # (few points of a sliver stay inside when moved)
    assert (case.outside_rays is not None) == (name in R.CONVEX and not crumpled)
    if name == "icosphere":
        assert len(case.obj_tris) == 1280 and 66000 < len(case.inside_rays) < 68000
    if case.outside_rays is not None:  # the outside origins are outside: an even crossing number
        assert not R.crossing_parity(case.world_tris, case.outside_rays[::97, 0:3], ndirs=1).any()


@pytest.mark.parametrize("name,placement", R.CRUMPLED)
def test_crumpled_slivers_are_closed_but_not_convex(name, placement):
    """The two slivers at scale 1e-3 around (100, 100, 100) are under four spacings of float32 thick.  They stay closed meshes
    with interior float32 points (test_origins_are_interior finds 8 of odd crossing parity), so the inside properties are kept;
    they are no longer convex -- some vertex lies more than a spacing beyond a face plane that has the mesh on its other side --
    so a ray from outside through the centre line need not meet a near side, and the outside rays are dropped for them alone."""
    for instanced in (False, True):
        case = R.leak_case(name, placement, instanced)
        ulps, dent = R.thickness_in_ulps(case.world_tris.reshape(-1, 3)), R.concavity_in_spacings(case.world_tris)
        print("%s at %s%s: %.2f float32 spacings thick, concave by %.2f spacings" % (name, placement, " (instanced)" if instanced else "", ulps, dent))
        assert ulps < 4 and dent > 1 and case.outside_rays is None
    assert R.concavity_in_spacings(R.leak_case(name, "unit", False).world_tris) < 1  # (the same mesh, resolved: convex)


@pytest.mark.parametrize("name,target", R.EDIT_CASES)
def test_edit_case_origins_are_interior(name, target):
    """The cases of tests/test_gpu_trace_edits.py: the unit mesh under each target transform.  Whether a case keeps its fixed
    origins and its outside rays follows from the two figures printed here and from nothing else; a case with fewer than 4
    interior origins is one the GPU tests leave out, and R.EDIT_DROPPED must say so."""
    case = R.edit_case(name, target)
    world = R.transform_points_f32(R.EDIT_TARGETS[target], case.mesh.verts)[case.mesh.faces]
    assert np.array_equal(case.world_tris.view(np.uint32), world.view(np.uint32)) and case.mesh.placement == "unit"
    ulps, dent = R.thickness_in_ulps(world.reshape(-1, 3)), R.concavity_in_spacings(world)
    resolved = ulps > 16 and (name not in R.CONVEX or dent < 1)
    print("%s under %s: %.2f float32 spacings thick, concave by %.2f spacings -> %s; %d origins, %d inside rays, %d slab-grazing rays, %s"
          % (name, target, ulps, dent, "resolved" if resolved else "crumpled", len(case.origins), len(case.inside_rays), len(case.grazing_rays),
             "no outside rays" if case.outside_rays is None else "%d outside rays" % len(case.outside_rays)))
    assert (ulps, dent, resolved) == (case.thickness, case.concavity, case.resolved)
    dropped = len(case.origins) < 4
    if dropped:
        print("%s under %s is left out of the GPU tests: %d interior origins" % (name, target, len(case.origins)))
    assert dropped == ((name, target) in R.EDIT_DROPPED)
    assert len(case.origins) <= 8 and (len(case.origins) == 8 or not resolved) and R.crossing_parity(case.world_tris, case.origins).all()
    full = len(case.origins) * (len(case.mesh.verts) + 4 * len(case.mesh.edges))
    assert np.isfinite(case.inside_rays).all() and (len(case.inside_rays) == full if resolved else 0.9 * full < len(case.inside_rays) <= full)
    assert np.isfinite(case.grazing_rays).all() and len(case.grazing_rays) <= (len(case.mesh.verts) + 4 * len(case.mesh.edges) + 3) // 4
    if len(case.grazing_rays):
        assert R.crossing_parity(case.world_tris, case.grazing_rays[:, 0:3], ndirs=2).all()
    assert (case.outside_rays is not None) == (name in R.CONVEX and resolved)
    if case.outside_rays is not None:
        assert len(case.outside_rays) == len(case.mesh.verts) + 4 * len(case.mesh.edges)
        assert not R.crossing_parity(case.world_tris, case.outside_rays[::97, 0:3], ndirs=1).any()


@pytest.mark.parametrize("placement", list(R.LATTICE_PLACEMENTS))
@pytest.mark.parametrize("n,seed", [(8, 1), (12, 2)])
def test_lattice_through_a_transform_is_the_lattice(n, seed, placement):
    """The integer lattice triangles under the placement's transform, in float32 with the renderer's association, are
    world_tris(scale, offset) bit for bit: the integer march stays the reference for a lattice that was moved there by an edit."""
    obj, world = R.lattice_tris_through_transform(R.voxel_solid(n, seed), placement)
    assert obj.dtype == np.float32 and world.shape == obj.shape


@pytest.mark.parametrize("n,seed", [(8, 1), (12, 2)])
def test_march_equals_brute_force_on_the_lattice(n, seed):
    """The integer march and the float64 brute force are independent statements of the same geometry: the first meeting of
    every checked ray with the mesh (lattice scale 1, where float64 is exact to ~1e-16) has the same parameter in both, and the
    triangles the march names are those whose float64 barycentrics put the point inside."""
    ref = R.lattice_reference(n, seed)
    solid = ref.solid
    assert len(solid.lattice_tris) <= 6000
    tris, rays = solid.world_tris(1.0, 0.0), solid.world_rays(1.0, 0.0)
    step = 1 if n == 8 else 7
    idx = np.arange(0, len(rays), step)
    for a in range(0, len(idx), 512):
        ii = idx[a:a + 512]
        t, u, v = R.brute_force(tris, rays[ii])
        with np.errstate(invalid="ignore"):
            cand = (u >= -1e-12) & (v >= -1e-12) & (u + v <= 1 + 1e-12) & (t > 0)
        tt = np.where(cand, t, np.inf)
        first = tt.min(1)
        assert np.allclose(first, ref.first_any[ii], rtol=1e-12, atol=0)
        for k, i in enumerate(ii):
            at_first = set(np.nonzero(cand[k] & (np.abs(t[k] - first[k]) <= 1e-12 * first[k]))[0].tolist())
            march = {tid for tid, par in ref.admissible[i].items() if par == ref.first_any[i]}
            assert at_first == march, (i, at_first, march)
    share = ref.zero_bary / len(rays)
    print("lattice %d: %d triangles, %d rays, %.1f %% of the first crossings lie on an edge, a diagonal or a vertex" % (
        n, len(tris), len(rays), 100 * share))
    assert share > 0.5  # (the rays this lattice is for)
    touched = sum(len(set(a.values())) > 1 for a in ref.admissible)
    print("lattice %d: %d rays (%.1f %%) touch an edge or a vertex of the mesh before they cross it" % (n, touched, 100.0 * touched / len(rays)))
    assert touched <= 0.3 * len(rays)  # (a quarter: exact lattice rays do run along edges; for the others only the crossing counts)
    rel_gap = [(b - a) / b for i in range(len(rays)) for a, b in [(ref.first[i], ref.nxt[i])] if not math.isnan(b)]
    assert min(rel_gap) > 2 * R.LATTICE_TOL  # the windows around two successive crossings cannot overlap


def test_soup_left_out_share_is_capped():
    """Part 3's classification, from the reference alone and before any tracer is looked at: at most 2 % of the rays are left out."""
    ref = R.soup_reference()
    n = len(ref.rays)
    out_edge, out_apart = (~ref.edge_clear).sum(), (ref.edge_clear & ~ref.apart).sum()
    print("soup: %d triangles, %d rays, %d hits; left out: %d near an edge or a range end (%.2f %%), %d with a runner-up within the "
          "tolerance (%.2f %%)" % (len(ref.tris), n, ref.hit.sum(), out_edge, 100.0 * out_edge / n, out_apart, 100.0 * out_apart / n))
    assert (~ref.clear).sum() <= 0.02 * n
    assert ref.hit[ref.clear].sum() > 2000 and (~ref.hit[ref.clear]).sum() > 1000
    rng = np.random.RandomState(33)
    decided, occ = ref.anyhit_expectation(rng.uniform(0.05, 4.0, n).astype(np.float32))
    print("soup any-hit: %d of %d left out (%.2f %%)" % ((~decided).sum(), n, 100.0 * (~decided).sum() / n))
    assert (~decided).sum() <= 0.02 * n and 0.1 * n < occ[decided].sum() < 0.9 * n


def test_float32_reference_deviation_defines_the_tolerance():
    """The tolerances of part 3 are twice what the reference's own formula loses in float32 (trace_reference.MT_F32_*)."""
    dt, db = R.soup_reference().float32_deviation()
    print("float32 Moeller-Trumbore against float64: t up to %.2f units of 2^-24 * S, barycentrics up to %.2f units of 2^-24; "
          "tolerances %d and %d units" % (dt, db, R.TOL_T_UNITS, R.TOL_BARY_UNITS))
    assert math.ceil(dt) == R.MT_F32_T_UNITS and math.ceil(db) == R.MT_F32_BARY_UNITS


# ---- part 2: tolerance-free properties -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,placement,instanced", R.LEAK_CASES)
@pytest.mark.parametrize("who", WHO)
def test_closed_meshes_do_not_leak(tracer, who, name, placement, instanced):
    case = R.leak_case(name, placement, instanced)
    R.check_no_leaks(case, tracer(who, case.key, case.instances), who)


@pytest.mark.parametrize("name,target", R.EDIT_CASES)
@pytest.mark.parametrize("who", WHO)
def test_edit_cases_do_not_leak_in_a_fresh_scene(tracer, who, name, target):
    """The control of tests/test_gpu_trace_edits.py: every edit case as a scene built for it, the target as the instance
    transform.  Where this passes and the GPU test of the same case fails, the edit road is at fault and not the case."""
    case = R.edit_case(name, target)
    n = R.check_no_leaks(case, tracer(who, case.key, case.instances), who, prim_range=(0, len(case.obj_tris)))
    print("%s, %s under %s: %d rays" % (who, name, target, n))


@pytest.mark.parametrize("who", WHO)
def test_split_scene_cases_in_a_fresh_scene(tracer, who):
    """The control of the split-scene GPU test: lattice and mover as two objects of a scene built for the mover's last placement.
    The mover's rays name its triangles only (a leak would name the lattice's), and no lattice ray meets the mover: every ray of
    check_lattice that has left the lattice goes on to miss, as it does with the lattice alone."""
    ref = R.lattice_reference(*R.SPLIT_LATTICE)
    lat = ref.solid.world_tris(1.0, 0.0)
    for name, step in (("icosphere", 4), ("icosphere", 70), ("torus", 4)):
        case = R.split_mover_case(name, step)
        trace = tracer(who, ("split", name, step), [(lat, None)] + case.instances)
        n = R.check_no_leaks(case, trace, who, prim_range=(len(lat), len(case.obj_tris)))
        R.check_lattice(ref, 1.0, 0.0, trace, who)
        print("%s, split scene, %s after %d edits: %d mover rays, 4 x %d lattice rays" % (who, name, step, n, len(ref.first)))


def test_split_mover_stays_clear_of_the_lattice_and_its_rays():
    """From the reference alone: at every edit step the mover's bounding ball lies beside the lattice with the origins of its
    outside rays (3 radii out) clear of the lattice box, and no lattice ray passes through the ball."""
    solid = R.voxel_solid(*R.SPLIT_LATTICE)
    rays = solid.world_rays(1.0, 0.0).astype(np.float64)
    o, d = rays[:, 0:3], rays[:, 4:7] / np.linalg.norm(rays[:, 4:7], axis=1, keepdims=True)
    worst = np.inf
    for name in ("icosphere", "torus"):
        mesh = R.ClosedMesh(name, "unit")
        for step in range(0, 71 if name == "icosphere" else 5):
            v = R.transform_points_f32(R.split_mover_transform(name, step), mesh.verts).astype(np.float64)
            c = R.split_mover_transform(name, step).astype(np.float64)[12:15]
            radius = np.linalg.norm(v - c, axis=1).max()
            # (radius: up to rounding of the vertices, a spacing of 1e-6 at coordinate 8; the lattice is [0, 12]^3)
            assert radius <= R.SPLIT_MOVER_RADIUS + 1e-5 and c[0] + 3 * radius < 0.0
            w = c - o
            along = np.maximum((w * d).sum(1), 0.0)
            gap = np.linalg.norm(w - along[:, None] * d, axis=1).min() - radius
            worst = min(worst, gap)
            assert gap > 0, (name, step, gap)
    print("closest approach of a lattice ray to the mover's bounding ball: %.3f" % worst)


@pytest.mark.parametrize("placement", list(R.LATTICE_PLACEMENTS))
@pytest.mark.parametrize("n,seed", [(8, 1), (12, 2)])
@pytest.mark.parametrize("who", WHO)
def test_lattice_rays_hit_the_exact_crossing(tracer, who, n, seed, placement):
    ref = R.lattice_reference(n, seed)
    scale, offset = R.LATTICE_PLACEMENTS[placement]
    trace = tracer(who, ("lattice", n, seed, placement), [(ref.solid.world_tris(scale, offset), None)])
    worst = R.check_lattice(ref, scale, offset, trace, who)
    print("%s lattice %d at %s: worst relative t error %.3g (bound %.3g)" % (who, n, placement, worst, R.LATTICE_TOL))


@pytest.mark.parametrize("who", WHO)
def test_the_first_instance_wins_among_exact_duplicates(tracer, who):
    """Equal t -> the smaller global triangle id: with the mesh a second time as a second instance, every hit is the one the
    mesh alone gives."""
    case = R.leak_case("icosphere", "unit", False)
    ref = R.lattice_reference(8, 1)
    lat = ref.solid.world_tris(1.0, 0.0)
    for key, tris, rays in (("icosphere", case.obj_tris, case.inside_rays[::3]), ("lattice", lat, ref.solid.world_rays(1.0, 0.0))):
        one = tracer(who, ("single", key), [(tris, None)])(rays, False)
        two = tracer(who, ("double", key), [(tris, None), (tris, None)])(rays, False)
        assert (one["prim"] >= 0).all() and (two["prim"] < len(tris)).all()
        assert np.array_equal(one, two)


# ---- part 3: values against the float64 brute force --------------------------------------------------------------------------------
@pytest.mark.parametrize("who", WHO)
def test_soup_hits_equal_the_float64_brute_force(tracer, who):
    ref = R.soup_reference()
    trace = tracer(who, "soup", [(ref.tris, None)])
    R.check_against_soup(ref, trace(ref.rays, False), who)
    sh = ref.rays.copy()
    sh[:, 7] = np.random.RandomState(33).uniform(0.05, 4.0, len(sh)).astype(np.float32)
    decided, occ = ref.anyhit_expectation(sh[:, 7])
    got = trace(sh, True)["prim"] == 0
    assert np.array_equal(got[decided], occ[decided]), "%s: %d any-hit verdicts differ" % (who, (got[decided] != occ[decided]).sum())


@pytest.mark.parametrize("length,width", R.SLIVER_SHAPES)
@pytest.mark.parametrize("who", WHO)
def test_sliver_hits_do_not_depend_on_tmax(tracer, who, length, width):
    tris, rays = R.sliver_case(length, width)
    R.check_range_consistency(rays, tracer(who, ("sliver", length, width), [(tris, None)]), who, min_hits=15000)


@pytest.mark.parametrize("who", WHO)
def test_soup_and_lattice_hits_do_not_depend_on_tmax(tracer, who):
    ref = R.soup_reference()
    R.check_range_consistency(ref.rays, tracer(who, "soup", [(ref.tris, None)]), who, min_hits=3000)
    lat = R.lattice_reference(8, 1)
    R.check_range_consistency(lat.solid.world_rays(1.0, 0.0), tracer(who, ("lattice", 8, 1, "1"), [(lat.solid.world_tris(1.0, 0.0), None)]), who, min_hits=8000)
