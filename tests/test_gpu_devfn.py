"""The device functions of the render kernels, one by one, on the GPU (tests/devfn/pt_devfn.hip: the product's headers compiled for
gfx950 with the product's flags), against
  * the function vectors made from the reference's own shader text (tests/golden/glsl_vectors.npz),
  * the host compile of the same headers (tests/emu, the same call bodies: tests/devfn/devfn_bodies.h), and
  * float64 numpy, for the math family,
at arguments whole frames almost never produce: subnormals, cos(theta) -> 0, alpha -> 0, IOR ratios next to 1 and next to the
critical angle, NaN and inf rows, 1e30 boxes, zero-area triangles, the branch constants of the Cephes kernels.

Comparison rules:
  * bit for bit.  A float component is compared by class (NaN against NaN, any sign and payload) only where the REFERENCE side
    (the fixture or the host compile) holds a NaN: IEEE leaves those bits open.  Words that are not floats (RNG states, flags,
    masks, packed node words) are always compared exactly.  The number of exempted fixture components is asserted, so the
    exemption cannot grow.
  * det_sincosf is compared bit for bit everywhere.  Beyond |x 2/pi| < 2^31 its (int)k used to overflow and the two targets took
    different quadrants (the first GPU run of this test: -inf against -7.4e34 at x = 3.45e12, 337 592 vectors of other class);
    the conversion is stated as the device performs it now (pt_math.h gcvt_i32), so the stricter comparison holds.
  * float64 bounds for the math family: tests/test_oracle_pins.py's own (3e-7 absolute for sin / cos on |x| <= 2 pi, < 4 ulp for
    det_logf on (0, 1] and det_expf on [its underflow limit, 0]); 0.5 ulp for gsqrt and 1 / x (correctly rounded); for
    det_atan2f and normalize the next power of two above the maximum measured on the HOST compile over these vectors
    (profiles/devfn_gpu.txt).
A failing assertion names the family, the function, the vector index, its inputs and both outputs."""
import os
import sys

import numpy as np
import pytest

import devfn_util
import devfn_vectors as V
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

# float64 bounds in ulp (see the module docstring); measured on the host compile: det_atan2f 2.329, normalize 2.766
ATAN2_ULP = 4.0
NORMALIZE_ULP = 4.0
# NaN words of the fixture: only there may a fixture component be compared by class (and only if it is a float component: the
# RNG word and the delta flag that end a row are compared exactly).
FIXTURE_NANS = {"samples": (54, 115200), "evals": (0, 64000), "lights": (495, 24000), "onb": (0, 30000)}  # (NaN words, all words)


@pytest.fixture(scope="module")
def dev():
    d = devfn_util.device()
    print("device harness:", d.path, d.L.devfn_build_info().decode())
    return d


@pytest.fixture(scope="module")
def hst(emu):
    return devfn_util.host(emu)


@pytest.fixture(scope="module")
def vec():
    with np.load(os.path.join(GOLDEN, "glsl_vectors.npz")) as z:
        return {k: np.ascontiguousarray(z[k]) for k in z.files}


@pytest.fixture(scope="module")
def tables(vec):
    sys.path.insert(0, GOLDEN)
    from make_glsl_vectors import tables as mk

    sc = mk()
    for i in range(8):
        assert np.array_equal(sc.bsdfs[i].view(np.uint8), vec["bsdf%d" % i].view(np.uint8))
    assert np.array_equal(sc.lights.view(np.uint8), vec["light_table"].view(np.uint8))
    return sc


def _isnan_words(w):
    return (w & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype != np.uint32 else a


def check(family, what, got, want, inputs, float_cols=None, against="the host compile"):
    """got, want: n x k words (or n).  float_cols: which of the k columns hold floats (default: all); only there a NaN of the
    reference excuses a NaN of other bits.  inputs(i) -> text."""
    got, want = words(got), words(want)
    assert got.shape == want.shape, (family, what, got.shape, want.shape)
    if got.size == 0:
        return
    g2, w2 = got.reshape(len(got), -1), want.reshape(len(want), -1)
    fc = np.ones(g2.shape[1], bool) if float_cols is None else np.asarray(float_cols, bool)
    excused = _isnan_words(w2) & _isnan_words(g2) & fc[None, :]
    bad = np.nonzero(((g2 != w2) & ~excused).any(axis=1))[0]
    if len(bad):
        i = int(bad[0])
        show = lambda r: " ".join("%08x" % x for x in r) + "  " + str(r.view(np.float32))
        raise AssertionError("%s: %s on gfx950 differs from %s at vector %d (%d of %d vectors differ): %s\n got %s\nwant %s"
                             % (family, what, against, i, len(bad), len(g2), inputs(i), show(g2[i]), show(w2[i])))


def ulp_error(got, ref64):
    """|got - ref| in units of the float32 spacing at ref (2^-149 at least)."""
    sp = np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)
    return np.abs(got.astype(np.float64) - ref64) / np.maximum(sp, 2.0 ** -149)


def fixture_nan_count(name, arr):
    """NaN bit patterns among ALL words of a fixture array.  (In `samples` all 54 are RNG states that happen to look like NaNs, in
    `lights` 8 of the 495 are: those words are compared exactly all the same -- check()'s float_cols -- so what is compared by
    class is a subset of what is counted here.)"""
    n = int(_isnan_words(arr).sum())
    assert (n, arr.size) == FIXTURE_NANS[name], (name, n, arr.size)


# ---------------------------------------------------------------------------------------------------------------------------------
def test_math_family(dev, hst):
    x = V.math_x()
    assert x.size > 4_190_000
    g, h = dev.math(x), hst.math(x)
    inp = lambda i: "x = %r (bits %08x)" % (float(x[i]), int(x.view(np.uint32)[i]))
    # det_sincosf: everywhere, the arguments beyond |x 2/pi| < 2^31 included (pt_math.h gcvt_i32)
    assert (np.abs(x[np.isfinite(x)].astype(np.float64)) * 0.63661977236758134308 >= 2.0 ** 31).sum() > 300000
    for k in ("sin", "cos"):
        check("math", "det_sincosf." + k, g[k], h[k], inp)
    for k, name in (("log", "det_logf"), ("exp", "det_expf"), ("sqrt", "gsqrt"), ("rcp", "1 / x")):
        check("math", name, g[k], h[k], inp)
    # float64
    with np.errstate(all="ignore"):
        x64 = x.astype(np.float64)
        m = np.abs(x64) <= 2 * np.pi
        es, ec = np.abs(g["sin"][m] - np.sin(x64[m])).max(), np.abs(g["cos"][m] - np.cos(x64[m])).max()
        m = (x64 > 0) & (x64 <= 1)
        el = ulp_error(g["log"][m], np.log(x64[m])).max()
        m = (x64 <= 0) & (x64 >= -87.33654475055310898657)
        ee = ulp_error(g["exp"][m], np.exp(x64[m])).max()
        m = x64 >= 0
        eq = ulp_error(g["sqrt"][m], np.sqrt(x64[m]))
        m2 = np.isfinite(x64) & (x64 != 0) & (np.abs(1.0 / x64) < 3.4028235677973366e38)
        er = ulp_error(g["rcp"][m2], 1.0 / x64[m2])
    print("math float64: sin %.3g cos %.3g absolute; log %.3f exp %.3f sqrt %.3f rcp %.3f ulp" % (es, ec, el, ee, np.nanmax(eq), er.max()))
    assert es < 3e-7 and ec < 3e-7, ("math: det_sincosf against float64 on |x| <= 2 pi", es, ec)
    assert el < 4, ("math: det_logf against float64 on (0, 1], ulp", el)
    assert ee < 4, ("math: det_expf against float64 on [-87.3365, 0], ulp", ee)
    assert np.nanmax(eq) <= 0.5, ("math: gsqrt is not correctly rounded, ulp", np.nanmax(eq), float(x[x64 >= 0][np.nanargmax(eq)]))
    assert er.max() <= 0.5, ("math: 1 / x is not correctly rounded, ulp", er.max(), float(x[m2][er.argmax()]))

    y, xx = V.atan2_yx()
    ga, ha = dev.atan2(y, xx), hst.atan2(y, xx)
    check("math", "det_atan2f", ga, ha, lambda i: "y = %r x = %r" % (float(y[i]), float(xx[i])))
    m = np.isfinite(y) & np.isfinite(xx) & ((y != 0) | (xx != 0))
    # (det_atan2f picks the sign by `y < 0`: a negative zero y counts as +0, so atan2(-0, x < 0) is +pi where IEEE's is -pi)
    ea = ulp_error(ga[m], np.arctan2(np.where(y[m] == 0, 0.0, y[m].astype(np.float64)), xx[m].astype(np.float64)))
    print("math float64: det_atan2f %.3f ulp" % ea.max())
    assert ea.max() < ATAN2_ULP, ("math: det_atan2f against float64, ulp", ea.max(), float(y[m][ea.argmax()]), float(xx[m][ea.argmax()]))

    v = V.normalize_v()
    gn, hn = dev.normalize(v), hst.normalize(v)
    check("math", "normalize", gn, hn, lambda i: "v = %r" % (v[i],))
    v64 = v.astype(np.float64)
    with np.errstate(all="ignore"):
        ln = np.sqrt((v64 * v64).sum(1))
    m = np.isfinite(ln) & (ln > 1e-18) & (ln < 1e18)
    en = ulp_error(gn[m], v64[m] / ln[m, None])
    print("math float64: normalize %.3f ulp" % en.max())
    assert en.max() < NORMALIZE_ULP, ("math: normalize against float64, ulp", en.max(), v[m][en.max(1).argmax()])


def _np_rng(a, b):
    """The RNG of pt_common.glsl:86-120 restated in numpy uint32 / uint64 (wrapping arithmetic by masking)."""
    M = np.uint64(0xFFFFFFFF)
    a, b = a.astype(np.uint64), b.astype(np.uint64)

    def pcg_out(s):
        w = ((((s >> ((s >> np.uint64(28)) + np.uint64(4))) ^ s) & M) * np.uint64(277803737)) & M
        return ((w >> np.uint64(22)) ^ w) & M

    def step(s):
        return (s * np.uint64(747796405) + np.uint64(2891336453)) & M

    def tea(v0, v1):
        s0 = np.uint64(0)
        for _ in range(4):
            s0 = (s0 + np.uint64(0x9E3779B9)) & M
            v0 = (v0 + ((((v1 << np.uint64(4)) + np.uint64(0xA341316C)) & M) ^ ((v1 + s0) & M) ^ (((v1 >> np.uint64(5)) + np.uint64(0xC8013EA4)) & M))) & M
            v1 = (v1 + ((((v0 << np.uint64(4)) + np.uint64(0xAD90777D)) & M) ^ ((v0 + s0) & M) ^ (((v0 >> np.uint64(5)) + np.uint64(0x7E95761E)) & M))) & M
        return v0

    t = tea(a, b)
    s1, s2, s3 = step(a), step(step(a)), step(step(step(a)))
    # (float)r * 2^-32: uint32 -> float32 rounds to nearest even, the product by a power of two is exact
    u = (pcg_out(s2).astype(np.float32) * np.float32(2.3283064365386962890625e-10)).view(np.uint32).astype(np.uint64)
    return np.stack([t, pcg_out(s1), pcg_out(a), pcg_out(s1), u, s3, pcg_out(step(t))], axis=1).astype(np.uint32)


def test_rng_family(dev, hst, vec):
    a, b = vec["rng_a"].astype(np.uint32), vec["rng_b"].astype(np.uint32)
    assert len(a) >= 1000
    none = np.zeros(7, bool)
    inp = lambda i: "a = %#x b = %#x" % (a[i], b[i])
    check("rng", "tea / pcg_hash / pcg_next / rand_uniform", dev.rng(a, b)[:, :6], vec["rng"], inp, none[:6], "the executed shader text")
    a, b = V.rng_ab()
    assert len(a) == 1_000_000 and {0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF} <= set(a[:25].tolist()) & set(b[:25].tolist())
    g = dev.rng(a, b)
    inp = lambda i: "a = %#x b = %#x" % (a[i], b[i])
    check("rng", "tea / pcg_hash / pcg_next / rand_uniform / frame seed", g, hst.rng(a, b), inp, none)
    check("rng", "tea / pcg_hash / pcg_next / rand_uniform / frame seed", g, _np_rng(a, b), inp, none, "the numpy restatement")


def test_frame_and_helpers_family(dev, hst, vec):
    fixture_nan_count("onb", vec["onb"])
    n, v = vec["onb_n"], vec["onb_v"]
    assert len(n) >= 2000
    check("frame", "make_frame / to_local / to_world", dev.onb(n, v), vec["onb"], lambda i: "n = %r v = %r" % (n[i], v[i]),
          against="the executed shader text")
    f, g, h = vec["helper_f"], vec["helper_g"], vec["helper_handles"]
    assert len(f) >= 505
    flt = [True, True, False]
    check("frame", "power_heuristic / cosine_pdf / bsdf_transmits", dev.helpers(f, g, h), vec["helpers"].astype(np.uint32),
          lambda i: "f = %r g = %r handle = %#x" % (f[i], g[i], h[i]), flt, "the executed shader text")
    n, v = V.frame_nv()
    assert len(n) == 100000
    check("frame", "make_frame / to_local / to_world", dev.onb(n, v), hst.onb(n, v), lambda i: "n = %r v = %r" % (n[i], v[i]))
    f, g, h = V.helper_fgh()
    check("frame", "power_heuristic / cosine_pdf / bsdf_transmits", dev.helpers(f, g, h), hst.helpers(f, g, h),
          lambda i: "f = %r g = %r handle = %#x" % (f[i], g[i], h[i]), flt)
    s, al = V.sampler_seeds_alpha()
    flt = [True, True, True, False] * 2
    check("frame", "sample_cosine_hemisphere / sample_half_beckmann", dev.samplers(s, al), hst.samplers(s, al),
          lambda i: "seed = %#x alpha = %r" % (s[i], al[i]), flt)


BSDF_S_FLOATS = [True] * 7 + [False, False]  # wi, f, pdf | delta flag, RNG state
BSDF_E_FLOATS = [True] * 4 + [False]


def test_bsdf_family(dev, hst, vec, tables):
    fixture_nan_count("samples", vec["samples"])
    fixture_nan_count("evals", vec["evals"])
    hd, wo, wi, sd = vec["handles"].astype(np.uint32), vec["wo"], vec["wi"], vec["seeds"].astype(np.uint32)
    assert len(hd) >= 12800
    gs, ge, gimg = dev.bsdf(tables.bsdfs, hd, wo, sd, wi)
    inp = lambda i: "handle %#x wo %r seed %d wi %r" % (hd[i], wo[i], sd[i], wi[i])
    check("bsdf", "bsdf_sample", gs, vec["samples"], inp, BSDF_S_FLOATS, "the executed shader text")
    check("bsdf", "bsdf_eval", ge, vec["evals"], inp, BSDF_E_FLOATS, "the executed shader text")
    _, _, himg = hst.bsdf(tables.bsdfs, hd, wo, sd, wi)
    assert np.array_equal(gimg, himg), "bsdf: the baked tables of the fixture's records differ from the host's at byte %d" % np.nonzero(gimg != himg)[0][0]

    bsdfs, hd, wo, sd, wi, use_sampled = V.bsdf_cases()
    assert len(hd) == 200000 and all(len(b) == 64 for b in bsdfs)
    hs, _, _ = hst.bsdf(bsdfs, hd, wo, sd, wi)
    wi = wi.copy()
    sampled = hs[:, :3].view(np.float32)
    wi[use_sampled] = sampled[use_sampled]  # evalBSDF at the direction sampleBSDF chose (the MIS use), for half the vectors
    hs, he, himg = hst.bsdf(bsdfs, hd, wo, sd, wi)
    gs, ge, gimg = dev.bsdf(bsdfs, hd, wo, sd, wi)
    bad = np.nonzero(gimg != himg)[0]
    assert len(bad) == 0, "bsdf: bake_bsdf / bake_diffuse: the baked tables differ from the host's at byte %d (layout %r)" % (bad[0], dev.table_layout([64] * 8))
    inp = lambda i: "handle %#x record %r wo %r seed %d wi %r" % (hd[i], bsdfs[hd[i] >> 16][hd[i] & 0xFFFF], wo[i], sd[i], wi[i])
    check("bsdf", "bsdf_sample", gs, hs, inp, BSDF_S_FLOATS)
    check("bsdf", "bsdf_eval", ge, he, inp, BSDF_E_FLOATS)
    f = hs[:, :7].view(np.float32)
    assert np.isnan(f).any() and np.isinf(f).any() and (hs[:, 7].view(np.float32) == 1).any()  # (the family does reach the edges)


def test_light_family(dev, hst, vec, tables):
    fixture_nan_count("lights", vec["lights"])
    flt = [True] * 7 + [False]
    pos, sd = vec["light_pos"], vec["light_seeds"].astype(np.uint32)
    assert len(pos) >= 3000
    g, gb = dev.lights(tables.lights, pos, sd)
    check("light", "sample_light", g, vec["lights"], lambda i: "pos %r seed %d" % (pos[i], sd[i]), flt, "the executed shader text")
    for name, L, pos, sd in V.light_cases():
        g, gb = dev.lights(L, pos, sd)
        h, hb = hst.lights(L, pos, sd)
        check("light", "bake_light (%s)" % name, gb.view(np.uint32).reshape(-1, 16), hb.view(np.uint32).reshape(-1, 16),
              lambda i: "light %r" % (L[i],))
        check("light", "sample_light (%s)" % name, g, h, lambda i: "pos %r seed %#x of %d lights" % (pos[i], sd[i], len(L)), flt)


def test_texture_family(dev, hst):
    textures, texels, ids, uv = V.texture_cases()
    for name, table in (("linear", V.linear_decode_table()), ("sRGB", V.srgb_decode_table())):
        check("texture", "sample_texture (%s decode)" % name, dev.texture(textures, texels, table, ids, uv),
              hst.texture(textures, texels, table, ids, uv), lambda i: "texture %r u, v = %r" % (textures[ids[i]], uv[i]))
    for w, h, tex, m, dirs in V.envmap_cases():
        check("texture", "sample_envmap (%d x %d)" % (w, h), dev.envmap(tex, w, h, m, dirs), hst.envmap(tex, w, h, m, dirs),
              lambda i: "d = %r to_local = %r" % (dirs[i], m))


def test_trace_family(dev, hst):
    rays, tris = V.tri_test_cases()
    g_ref, g_rot = dev.tri_tests(rays, tris)
    h_ref, h_rot = hst.tri_tests(rays, tris)
    inp = lambda i: "ray %r triangle %r" % (rays[i], tris[i])
    # each device form against the OTHER form on the host
    check("trace", "intersect_tri_rot (against the host's intersect_tri)", g_rot, h_ref, inp)
    check("trace", "intersect_tri (against the host's intersect_tri_rot)", g_ref, h_rot, inp)
    d = V.shear_dirs()
    flt = [False] * 3 + [True] * 3 + [False] * 3 + [True] * 3
    check("trace", "make_shear / make_shear_rot", dev.shears(d), hst.shears(d), lambda i: "d = %r" % (d[i],), flt)
    boxes, counts = V.node_encoder_cases()
    g_def, g_fast = dev.encode_nodes(boxes, counts)
    h_def, h_fast = hst.encode_nodes(boxes, counts)
    inp = lambda i: "counts %r boxes %r" % (counts[i], boxes[i])
    none = np.zeros(16, bool)  # packed words: exact
    check("trace", "encode_node_w4 (against the host's encode_node_w4_ref)", g_fast, h_def, inp, none)
    check("trace", "encode_node_w4_ref (against the host's encode_node_w4)", g_def, h_fast, inp, none)
    recs = h_def[::4]  # 100 000 records x 8 rays
    idx, nrays = V.node_test_cases(recs)
    flt = [False] + [True] * 6 + [False] * 3 + [True, False]
    check("trace", "node_test / make_raybox", dev.node_tests(recs, idx, nrays), hst.node_tests(recs, idx, nrays),
          lambda i: "node %r ray %r" % (recs[idx[i]], nrays[i]), flt)
