"""gsp_trace (closest-hit and any-hit kernels, both context modes) against the BVH-free geometric reference of
tests/trace_reference.py: the properties of tests/test_trace_reference_cpu.py on the device, and on the same rays bit equality
with the oracle -- so unnormalised directions, exact edge and vertex hits and the three scales are parity evidence too."""
import os

import numpy as np
import pytest

import trace_reference as R
from trace_scenes import build_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["default", "wavefront-only"])
def ctx(request):
    """As tests/test_gpu_parity.py: the defaults, and GSP_FINISH_PATHS=0 (every bounce in the wavefront kernels)."""
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


@pytest.fixture(scope="module")
def shared():
    """Scenes with their oracle, and the oracle's answers, computed once for both context modes: {key: (scene, oracle)} and
    {(key, any_hit, call number within the test): (rays, hits)}."""
    return {}, {}


@pytest.fixture
def tracer(ctx, oracle_mod, shared):
    """tracer(key, instances) -> trace(rays, any_hit): uploads the scene, traces on the GPU, and asserts on every ray that
    the oracle reports the same bits (prim, t, u, v)."""
    scenes, oracle_hits = shared

    def make(key, instances):
        if key not in scenes:
            sc = build_scene(instances)
            scenes[key] = (sc, oracle_mod.Oracle(sc))
        sc, orc = scenes[key]
        ctx.upload_scene(sc)
        calls = [0]

        def trace(rays, any_hit):
            got = ctx.trace(rays, any_hit=any_hit)
            k = (key, any_hit, calls[0])
            calls[0] += 1
            if k not in oracle_hits or not np.array_equal(oracle_hits[k][0], rays):
                oracle_hits[k] = (rays.copy(), orc.trace(rays, any_hit=any_hit))
            want = oracle_hits[k][1]
            assert np.array_equal(got["prim"], want["prim"]), "%s: GPU and oracle name different triangles on %d rays" % (
                key, (got["prim"] != want["prim"]).sum())
            hit = want["prim"] >= 0
            for f in ("t", "u", "v"):
                assert np.array_equal(np.ascontiguousarray(got[f][hit]).view(np.uint32), np.ascontiguousarray(want[f][hit]).view(np.uint32)), (key, f)
            return got

        return trace

    return make


@pytest.mark.parametrize("name,placement,instanced", R.LEAK_CASES)
def test_closed_meshes_do_not_leak(tracer, name, placement, instanced):
    """Rays from inside at every vertex and 4 points of every edge must hit (closest hit) and be occluded (any hit); rays from
    outside a convex mesh must stop at its near side."""
    case = R.leak_case(name, placement, instanced)
    R.check_no_leaks(case, tracer(case.key, case.instances), "gsp_trace")


@pytest.mark.parametrize("placement", list(R.LATTICE_PLACEMENTS))
@pytest.mark.parametrize("n,seed", [(8, 1), (12, 2)])
def test_lattice_rays_hit_the_exact_crossing(tracer, n, seed, placement):
    """Unnormalised integer directions from cell centres, exactly through face diagonals, lattice edges and lattice vertices:
    every ray hits a triangle that contains the exact crossing point at the exact parameter (2^-10 relative), any-hit rays ending
    2^-10 short of it are free and 2^-10 past it occluded, and closest hits with tmin 2^-10 past it find the next crossing."""
    ref = R.lattice_reference(n, seed)
    scale, offset = R.LATTICE_PLACEMENTS[placement]
    trace = tracer(("lattice", n, seed, placement), [(ref.solid.world_tris(scale, offset), None)])
    worst = R.check_lattice(ref, scale, offset, trace, "gsp_trace")
    print("gsp_trace lattice %d at %s: worst relative t error %.3g (bound %.3g)" % (n, placement, worst, R.LATTICE_TOL))


def test_the_first_instance_wins_among_exact_duplicates(tracer):
    case = R.leak_case("icosphere", "unit", False)
    ref = R.lattice_reference(8, 1)
    lat = ref.solid.world_tris(1.0, 0.0)
    for key, tris, rays in (("icosphere", case.obj_tris, case.inside_rays[::3]), ("lattice", lat, ref.solid.world_rays(1.0, 0.0))):
        one = tracer(("single", key), [(tris, None)])(rays, False)
        two = tracer(("double", key), [(tris, None), (tris, None)])(rays, False)
        assert (one["prim"] >= 0).all() and (two["prim"] < len(tris)).all()
        assert np.array_equal(one, two)


def test_soup_hits_equal_the_float64_brute_force(tracer):
    """Hit or miss, the triangle, and t, u, v within twice the float32 error of the reference's own formula, on the rays the
    float64 brute force finds clear of edges; any-hit verdicts for random tmax."""
    ref = R.soup_reference()
    trace = tracer("soup", [(ref.tris, None)])
    R.check_against_soup(ref, trace(ref.rays, False), "gsp_trace")
    sh = ref.rays.copy()
    sh[:, 7] = np.random.RandomState(33).uniform(0.05, 4.0, len(sh)).astype(np.float32)
    decided, occ = ref.anyhit_expectation(sh[:, 7])
    got = trace(sh, True)["prim"] == 0
    assert np.array_equal(got[decided], occ[decided]), "%d any-hit verdicts differ" % (got[decided] != occ[decided]).sum()


@pytest.mark.parametrize("length,width", R.SLIVER_SHAPES)
def test_sliver_hits_do_not_depend_on_tmax(tracer, length, width):
    """Axis-aligned slivers of aspect 3e3 to 2e7 under rays that graze them along their length: a reported hit is reported again,
    bit for bit, and occludes, when tmax shrinks to eight spacings beyond it -- the property the leaf-box pad exists for."""
    tris, rays = R.sliver_case(length, width)
    R.check_range_consistency(rays, tracer(("sliver", length, width), [(tris, None)]), "gsp_trace", min_hits=15000)


def test_soup_and_lattice_hits_do_not_depend_on_tmax(tracer):
    ref = R.soup_reference()
    R.check_range_consistency(ref.rays, tracer("soup", [(ref.tris, None)]), "gsp_trace", min_hits=3000)
    lat = R.lattice_reference(8, 1)
    R.check_range_consistency(lat.solid.world_rays(1.0, 0.0), tracer(("lattice", 8, 1, "1"), [(lat.solid.world_tris(1.0, 0.0), None)]), "gsp_trace", min_hits=8000)
