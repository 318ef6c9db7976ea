"""Ray hits against a BVH-free geometric reference (tests/trace_reference.py), on the CPU: first the reference's own inputs are
checked from the reference alone, then the oracle and the host emulation of the product's traversal (tests/emu: node_test /
intersect_tri) are held to it.  The GPU run of the same properties is tests/test_gpu_trace_reference.py."""
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
