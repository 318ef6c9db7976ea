"""Feature buffers on the CPU (include/gpuspectral_pt.h, "Feature buffers"): the host emulation -- the product's pt_features.h,
generate_path and the emulation's traversal -- against an INDEPENDENT composition: rays from the filter / lens emulation, hits
from oracle.trace, the features restated in numpy from the scene arrays (tests/features_util.py).

Bounds.  coverage, depth, ids and the untextured albedo: bit for bit.  The normal is compared with a float64 restatement; the
largest deviation measured over the cases below is 1.09 ulp of 1.0 (profiles/features_cpu_check.txt), the bound is the next power
of two, 2 ulp.  A mean of k samples adds the rounding of k folds, three float32 operations of at most half an ulp each on values
of magnitude <= 1: 1.5 k ulp on top."""
import numpy as np
import pytest

import features_util as fu

W, H = 48, 32
NORMAL_ULP_BOUND = 2.0
TENT = 2
LENS = dict(radius=0.08, focus_distance=5.0, blades=0, rotation=0.0)


@pytest.fixture(scope="module")
def femu():
    return fu.FeaturesEmu()


@pytest.fixture(scope="module")
def cornell_emu(femu, cornell):
    return femu.scene(cornell)


def reference(femu, sc, orc, w, h):
    """One feature sample per pixel of the pinhole, unfiltered w x h frame: rays, oracle hits, restated features."""
    gids = np.arange(w * h, dtype=np.uint32)
    o, d, _, _ = femu.generate(sc, w, h, None, gids, np.zeros(w * h, np.uint32))
    rays = np.zeros((w * h, 8), np.float32)
    rays[:, 0:3], rays[:, 4:7], rays[:, 7] = o, d, 1e10
    hits = orc.trace(rays)
    return dict(o=o, d=d, hits=hits, f=fu.restate(sc, o, d, hits))


@pytest.fixture(scope="module")
def cornell_ref(femu, cornell, oracle_mod):
    return reference(femu, cornell, oracle_mod.Oracle(cornell), W, H)


def normal_ulps(got, ref):
    f = ref["f"] if "f" in ref else ref
    dev = np.abs(got.astype(np.float64) - f["normal"]) / fu.ULP1
    flipped = np.abs(got.astype(np.float64) + f["normal"]) / fu.ULP1  # a two-faced test too close to zero to call: either side
    dev = np.where(f["ambiguous"][:, None], np.minimum(dev, flipped), dev)
    return float(dev.max())


def test_one_sample_against_the_composition(cornell_emu, cornell_ref):
    a, g, i = cornell_emu.render(W, H, 1)
    f = cornell_ref["f"]
    assert fu.same(a, f["albedo"]), "albedo / coverage"
    assert fu.same(g[:, 3], f["depth"]), "depth"
    assert np.array_equal(i[:, :3], f["ids"]), "triangle / bsdf / instance"
    assert (i[:, 3] == 1).all()
    ulps = normal_ulps(g[:, :3], cornell_ref)
    print("normal: largest deviation from the float64 restatement %.3f ulp of 1.0" % ulps)
    assert ulps <= NORMAL_ULP_BOUND
    hit = f["ids"][:, 0] != fu.MISS
    assert np.allclose(np.linalg.norm(g[hit, :3].astype(np.float64), axis=1), 1.0, atol=4 * fu.ULP1)


def test_every_bsdf_type_against_the_composition(femu, materials_scene, oracle_mod):
    sc = materials_scene
    W, H = 48, 40  # (tall enough to show the floor, which carries the rough-floor record)
    f = reference(femu, sc, oracle_mod.Oracle(sc), W, H)["f"]
    a, g, i = femu.scene(sc).render(W, H, 1)
    assert fu.same(a, f["albedo"]) and fu.same(g[:, 3], f["depth"]) and np.array_equal(i[:, :3], f["ids"])
    seen = set(int(h) >> 16 for h in f["ids"][f["ids"][:, 0] != fu.MISS, 1])
    assert seen == set(range(8)), "the frame shows every BSDF type: %s" % sorted(seen)
    ulps = normal_ulps(g[:, :3], f)
    print("materials scene normal: %.3f ulp" % ulps)
    assert ulps <= NORMAL_ULP_BOUND


@pytest.mark.parametrize("filt,lens", [(TENT, None), (0, LENS), (TENT, LENS)])
def test_three_filtered_samples_against_the_composition(femu, cornell, cornell_emu, oracle_mod, filt, lens):
    spp, t0 = 3, 5
    gids = np.arange(W * H, dtype=np.uint32)
    orc = oracle_mod.Oracle(cornell)
    alb = np.zeros((W * H, 4), np.float32)
    dep = np.zeros(W * H, np.float32)
    nrm = np.zeros((W * H, 3), np.float64)
    first = None
    for s in range(spp):
        o, d, _, _ = femu.generate(cornell, W, H, lens, gids, np.full(W * H, t0 + s, np.uint32), filt=filt)
        rays = np.zeros((W * H, 8), np.float32)
        rays[:, 0:3], rays[:, 4:7], rays[:, 7] = o, d, 1e10
        f = fu.restate(cornell, o, d, orc.trace(rays))
        assert not f["ambiguous"].any()
        alb, dep = fu.fold(alb, f["albedo"], s), fu.fold(dep, f["depth"], s)
        nrm = nrm + (f["normal"] - nrm) / (s + 1)
        first = f["ids"] if first is None else first
    a, g, i = cornell_emu.render(W, H, spp, lens=lens, first_timestamp=t0, pixel_filter=filt)
    assert fu.same(a, alb) and fu.same(g[:, 3], dep)
    assert np.array_equal(i[:, :3], first) and (i[:, 3] == spp).all()
    ulps = float((np.abs(g[:, :3].astype(np.float64) - nrm) / fu.ULP1).max())
    print("mean normal of %d samples: %.3f ulp" % (spp, ulps))
    assert ulps <= NORMAL_ULP_BOUND + 1.5 * spp


def test_unfiltered_pinhole_one_sample_equals_seven(cornell_emu):
    one, seven = cornell_emu.render(W, H, 1), cornell_emu.render(W, H, 7)
    assert fu.same(one[0], seven[0]) and fu.same(one[1], seven[1])
    assert np.array_equal(one[2][:, :3], seven[2][:, :3]) and (seven[2][:, 3] == 7).all()


def test_five_samples_in_one_call_equal_two_plus_three(cornell_emu):
    whole = cornell_emu.render(W, H, 5, lens=LENS, pixel_filter=TENT)
    parts = cornell_emu.render(W, H, 2, lens=LENS, pixel_filter=TENT)
    parts = cornell_emu.render(W, H, 3, lens=LENS, pixel_filter=TENT, first_timestamp=2, planes=parts)
    assert all(fu.same(x, y) for x, y in zip(whole, parts))


def test_flip_emitter_and_miss_pixels(femu, cornell_emu, cornell, oracle_mod):
    """One pixel of each kind, chosen where oracle.trace shows the case (a square frame: it shows the light and the room's rim)."""
    w = h = 40
    ref = reference(femu, cornell, oracle_mod.Oracle(cornell), w, h)
    a, g, i = cornell_emu.render(w, h, 1)
    f, hits = ref["f"], ref["hits"]
    flip = np.flatnonzero(f["flipped"] & ~f["ambiguous"])
    emit = np.flatnonzero(f["emitter"])
    miss = np.flatnonzero(hits["prim"] < 0)
    assert len(flip) and len(emit) and len(miss), (len(flip), len(emit), len(miss))
    k = flip[0]  # the shading normal faces the viewer although the geometry's does not
    assert float(g[k, :3].astype(np.float64) @ -ref["d"][k].astype(np.float64)) > 0
    k = emit[0]
    em = cornell.instances[int(i[k, 2])]["emission"]
    assert (em != 0).any() and np.array_equal(a[k, :3], np.minimum(em, np.float32(1))) and a[k, 3] == 1
    k = miss[0]
    assert not a[k].any() and not g[k].any() and (i[k, :3] == fu.MISS).all() and i[k, 3] == 1


def test_instance_index_against_the_vertex_ranges(cornell_emu, cornell):
    _, _, i = cornell_emu.render(W, H, 1)
    first = fu.tri_first(cornell)
    hit = i[:, 0] != fu.MISS
    tri, inst = i[hit, 0].astype(np.int64), i[hit, 2].astype(np.int64)
    assert (inst < len(cornell.instances)).all()
    assert ((first[inst] <= tri) & (tri < first[inst + 1])).all()
    assert np.array_equal(i[hit, 1], cornell.instances["bsdf"][inst])
