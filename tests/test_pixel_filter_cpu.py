"""Pixel filter on the CPU: the product's generate_path (tests/emu/filter_emu.cpp compiles gpuspectral_amd/csrc/pt_stages.h for
the host) against the oracle's RNG, the oracle's camera ray, the filters' analytic densities and the oracle's own renders; and
the loader's readFilter option."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import CORNELL_XML, ROOT

NONE, BOX, TENT, GAUSSIAN = 0, 1, 2, 3
NAMES = {NONE: "none", BOX: "box", TENT: "tent", GAUSSIAN: "gaussian"}


class FilterEmu:
    """ctypes handle on tests/emu/libfilter_emu.so (pt_emu.cpp + the filter entries), built here the way conftest.Emu builds
    libpt_emu.so."""

    def __init__(self):
        from gpuspectral_amd import abi

        d = os.path.join(ROOT, "tests", "emu")
        so = os.path.join(d, "libfilter_emu.so")
        srcs = [os.path.join(d, "filter_emu.cpp"), os.path.join(d, "pt_emu.cpp"), os.path.join(ROOT, "include", "gpuspectral_pt.h")]
        csrc = os.path.join(ROOT, "gpuspectral_amd", "csrc")
        srcs += [os.path.join(csrc, h) for h in os.listdir(csrc) if h.endswith(".h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mfma", "-mavx2", "-shared", "-o", so, srcs[0]])
        L = C.CDLL(so)
        vp, u32, u64, f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
        L.emu_create.restype = vp
        L.emu_create.argtypes = [C.POINTER(abi.SceneDesc)]
        L.emu_destroy.argtypes = [vp]
        L.filter_emu_generate.argtypes = [u32, u32, f32, vp, u32, f32, vp, vp, u64, vp, vp]
        L.filter_emu_ray_through.argtypes = [u32, u32, f32, vp, vp, vp, u64, vp]
        L.filter_emu_render.argtypes = [vp, u32, u32, vp, u64, C.POINTER(abi.RenderParams), vp, vp]
        self.L, self.abi = L, abi

    def generate(self, sc, width, height, filt, param, gids, timestamps):
        """(o[n,3], d[n,3], offset[n,2], seed[n]) of the product's generate_path with this filter in the constants."""
        gids = np.ascontiguousarray(gids, np.uint32)
        ts = np.ascontiguousarray(timestamps, np.uint32)
        tw = np.ascontiguousarray(sc.to_world, np.float32)
        out = np.zeros((len(gids), 8), np.float32)
        seeds = np.zeros(len(gids), np.uint32)
        self.L.filter_emu_generate(width, height, float(sc.fov), tw.ctypes.data, filt, param, gids.ctypes.data, ts.ctypes.data, len(gids),
                                   out.ctypes.data, seeds.ctypes.data)
        return out[:, 0:3], out[:, 3:6], out[:, 6:8], seeds

    def ray_through(self, sc, width, height, gids, offsets):
        gids = np.ascontiguousarray(gids, np.uint32)
        off = np.ascontiguousarray(offsets, np.float32)
        tw = np.ascontiguousarray(sc.to_world, np.float32)
        out = np.zeros((len(gids), 3), np.float32)
        self.L.filter_emu_ray_through(width, height, float(sc.fov), tw.ctypes.data, gids.ctypes.data, off.ctypes.data, len(gids), out.ctypes.data)
        return out

    def scene(self, sc):
        return FilterEmuScene(self, sc)


class FilterEmuScene:
    def __init__(self, emu, sc):
        self.emu, self.sc = emu, sc
        self._desc = sc.desc()
        self.h = emu.L.emu_create(C.byref(self._desc))

    def render(self, width, height, spp, first_timestamp=0, pixel_filter=NONE, pixel_filter_param=0.0, pixel_ids=None, accum=None,
               params=None):
        """(accum[n,4], {extension_rays, shadow_rays, shaded_vertices}): emu_render with the filter in the constants."""
        p = params or self.emu.abi.default_render_params()
        p.spp, p.first_timestamp, p.pixel_filter, p.pixel_filter_param = spp, first_timestamp, pixel_filter, pixel_filter_param
        ids = np.ascontiguousarray(pixel_ids, np.uint32) if pixel_ids is not None else None
        n = len(ids) if ids is not None else width * height
        if accum is None:
            accum = np.zeros((n, 4), np.float32)
        counts = np.zeros(3, np.uint64)
        self.emu.L.filter_emu_render(self.h, width, height, ids.ctypes.data if ids is not None else None, n, C.byref(p), accum.ctypes.data,
                                     counts.ctypes.data)
        return accum, dict(extension_rays=int(counts[0]), shadow_rays=int(counts[1]), shaded_vertices=int(counts[2]))

    def render_threads(self, width, height, spp, threads=0, **kw):
        """render() with the frame's rows dealt over threads (the library call releases the GIL; pixels are independent)."""
        from concurrent.futures import ThreadPoolExecutor

        from oracle.oracle import usable_cpus

        threads = threads or usable_cpus()
        ids = np.arange(width * height, dtype=np.uint32)
        parts = [ids[k::threads] for k in range(threads)]
        out = np.zeros((width * height, 4), np.float32)
        with ThreadPoolExecutor(threads) as ex:
            res = list(ex.map(lambda q: self.render(width, height, spp, pixel_ids=q, **kw)[0], parts))
        for q, r in zip(parts, res):
            out[q] = r
        return out

    def __del__(self):
        try:
            self.emu.L.emu_destroy(self.h)
        except Exception:
            pass


@pytest.fixture(scope="module")
def femu():
    return FilterEmu()


# ---- the semantics of include/gpuspectral_pt.h restated in numpy ---------------------------------------------------------
def draws(orc, width, gid, ts):
    """(u1, u2 as float32, state before the draws, state after them) from the oracle's own RNG functions."""
    s0 = orc.pcg_hash(orc.tea(int(width * (gid // width) + gid % width), int(ts)))
    out, s2 = orc.rand_pcg(s0, 2)
    u = (out.astype(np.float32) * np.float32(2.0 ** -32)).astype(np.float32)
    return u[0], u[1], s0, s2


def stream(orc, width, gids, tss):
    u = np.zeros((len(gids), 2), np.float32)
    s0 = np.zeros(len(gids), np.uint32)
    s2 = np.zeros(len(gids), np.uint32)
    for i, (g, t) in enumerate(zip(gids, tss)):
        u[i, 0], u[i, 1], s0[i], s2[i] = draws(orc, width, int(g), int(t))
    return u, s0, s2


def offsets_f64(filt, param, u):
    """The header's formulas in float64 from the float32 variates (for the distribution tests: agreement to rounding)."""
    u = u.astype(np.float64)
    if filt == BOX:
        return u.copy()
    if filt == TENT:
        r = param or 1.0
        t = np.where(u < 0.5, np.sqrt(2 * u) - 1, 1 - np.sqrt(2 - 2 * u))
        return 0.5 + r * t
    s = param or 0.5
    rho = np.minimum(s * np.sqrt(-2 * np.log(np.maximum(1 - u[:, 0], 2.0 ** -32))), 4 * s)
    return 0.5 + rho[:, None] * np.stack([np.cos(2 * np.pi * u[:, 1]), np.sin(2 * np.pi * u[:, 1])], 1)


def cdf_box(x):
    return np.clip(x, 0.0, 1.0)


def cdf_tent(x, r=1.0):
    """CDF of offset = 0.5 + r * t, t tent-distributed on [-1, 1]."""
    t = np.clip((np.asarray(x, np.float64) - 0.5) / r, -1.0, 1.0)
    return np.where(t < 0, 0.5 * (1 + t) ** 2, 1 - 0.5 * (1 - t) ** 2)


def cdf_gauss_radius(rho, s):
    """CDF of rho = min(s * sqrt(-2 log(1 - u)), 4 s): 1 - exp(-rho^2 / 2 s^2) below 4 s, the rest as an atom at 4 s."""
    rho = np.asarray(rho, np.float64)
    return np.where(rho >= 4 * s, 1.0, 1 - np.exp(-rho ** 2 / (2 * s * s)))


def ks(samples, cdf):
    """Kolmogorov-Smirnov distance sup |F_n - F| (both one-sided gaps at every sample)."""
    x = np.sort(np.asarray(samples, np.float64))
    n = len(x)
    f = cdf(x)
    return float(max((np.arange(1, n + 1) / n - f).max(), (f - np.arange(n) / n).max()))


def ray_f64(sc, width, height, frag):
    """rayDir(size, fragCoord, fov) + camera transform + y flip in float64 (raygen.rgen:20-25,41-45)."""
    tw = np.asarray(sc.to_world, np.float64).reshape(4, 4)  # glm memory order: tw[c][r]
    zplane = (max(width, height) / 2.0) / np.tan(np.float64(np.float32(sc.fov)) / 2.0)
    x = frag[:, 0] - width / 2.0
    y = frag[:, 1] - height / 2.0
    dl = np.stack([-x, y, np.full(len(x), zplane)], 1)
    dl /= np.linalg.norm(dl, axis=1, keepdims=True)
    d = dl[:, 0:1] * tw[0, :3] + dl[:, 1:2] * tw[1, :3] + dl[:, 2:3] * tw[2, :3]
    d[:, 1] *= -1.0
    return d


def pairs(width, height, n, seed):
    rng = np.random.RandomState(seed)
    gids = rng.randint(0, width * height, n).astype(np.uint32)
    tss = np.concatenate([rng.randint(0, 64, n // 2), rng.randint(0, 2 ** 31, n - n // 2)]).astype(np.uint32)
    return gids, tss


# ---- draw order and seed hand-off: exact ----------------------------------------------------------------------------------
@pytest.mark.parametrize("filt,param", [(NONE, 0.0), (BOX, 0.0), (TENT, 0.0), (TENT, 1.5), (GAUSSIAN, 0.0), (GAUSSIAN, 0.8)])
def test_draw_order_and_seed(femu, oracle_mod, cornell, filt, param):
    W, H = 96, 64
    gids, tss = pairs(W, H, 1000, 11 + filt)
    o, d, off, seed = femu.generate(cornell, W, H, filt, param, gids, tss)
    u, s0, s2 = stream(oracle_mod, W, gids, tss)
    assert np.array_equal(o, np.tile(np.asarray(cornell.to_world, np.float32)[12:15], (len(gids), 1)))
    if filt == NONE:
        assert np.array_equal(seed, s0)  # no draw: prd.seed = pcgHash(tea(..))
        assert not off.any()
        orc = oracle_mod.Oracle(cornell)
        for i in range(len(gids)):
            ref = orc.primary_ray(W, H, int(gids[i] % W), int(gids[i] // W))
            assert np.array_equal(ref[3:6].view(np.uint32), d[i].view(np.uint32)), i
        return
    assert np.array_equal(seed, s2)  # prd.seed = the state after exactly two draws, whatever the filter
    if filt == BOX:
        assert np.array_equal(off.view(np.uint32), u.view(np.uint32))  # offset = (u1, u2), bit for bit
    else:
        ref = offsets_f64(filt, param, u)
        assert np.abs(off - ref).max() <= 4e-6 * max(1.0, 4 * (param or 1.0))  # float32 formulas against float64: rounding only


def test_filtered_streams_coincide(femu, cornell):
    """Every filter other than NONE draws exactly two variates: the seeds handed to the first bounce are the same."""
    W, H = 64, 64
    gids, tss = pairs(W, H, 500, 5)
    seeds = [femu.generate(cornell, W, H, f, p, gids, tss)[3] for f, p in ((BOX, 0.0), (TENT, 0.0), (TENT, 2.0), (GAUSSIAN, 0.0))]
    for s in seeds[1:]:
        assert np.array_equal(s, seeds[0])
    assert not np.array_equal(seeds[0], femu.generate(cornell, W, H, NONE, 0.0, gids, tss)[3])


# ---- the ray goes through pixel + offset ----------------------------------------------------------------------------------
@pytest.mark.parametrize("filt,param", [(BOX, 0.0), (TENT, 0.0), (TENT, 1.5), (GAUSSIAN, 0.0)])
def test_ray_through_offset_float64(femu, cornell, filt, param):
    """d against rayDir(size, fragCoord, fov) + camera transform + y flip in float64, fragCoord = float32(pixel + offset).
    Bound: 4 float32 ulp per component -- the subtraction is exact, then normalise (dot, sqrt, reciprocal, multiply), the 3x3
    transform and its rounding: a bound from the operation count, not a measurement."""
    W, H = 96, 64
    gids, tss = pairs(W, H, 1000, 23 + filt)
    o, d, off, seed = femu.generate(cornell, W, H, filt, param, gids, tss)
    # fragCoord is a float32 vec2: the sum pixel + offset is rounded once (that rounding is the semantics, not an error)
    frag = (np.stack([gids % W, gids // W], 1).astype(np.float32) + off).astype(np.float64)
    ref = ray_f64(cornell, W, H, frag)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    err = np.abs(d.astype(np.float64) - ref) / ulp
    print("max error in ulp:", err.max(0))
    assert err.max() <= 4.0


def test_ray_through_quarter_offsets_equals_oracle(femu, oracle_mod, cornell):
    """An offset that is a multiple of 1/4: the ray equals the oracle's own primary ray of the 4x frame through pixel
    4 (p + o), bit for bit (scaling x, y and zplane by 4 is exact, so is every later operation's result)."""
    W, H = 48, 40
    rng = np.random.RandomState(3)
    n = 1000
    gids = rng.randint(0, W * H, n).astype(np.uint32)
    q = rng.randint(0, 4, (n, 2))
    d = femu.ray_through(cornell, W, H, gids, q.astype(np.float32) / 4)
    orc = oracle_mod.Oracle(cornell)
    for i in range(n):
        ref = orc.primary_ray(4 * W, 4 * H, int(4 * (gids[i] % W) + q[i, 0]), int(4 * (gids[i] // W) + q[i, 1]))
        assert np.array_equal(ref[3:6].view(np.uint32), d[i].view(np.uint32)), (i, ref[3:6], d[i])


# ---- distribution ---------------------------------------------------------------------------------------------------------
KS_N = 1 << 17
KS_BOUND = 1.95 / np.sqrt(KS_N)  # the 0.1 % critical value of the Kolmogorov-Smirnov statistic


def ks_inputs():
    W = H = 32
    px = (np.arange(512, dtype=np.uint32) * 2) % (W * H)  # 512 pixels
    gids = np.repeat(px, 256)
    tss = np.tile(np.arange(256, dtype=np.uint32), 512)
    return W, H, gids, tss


def ks_stats(filt, param, off):
    """KS distances of the offsets against the filter's analytic CDFs: per axis, or radius + angle for the Gaussian."""
    if filt == BOX:
        return [ks(off[:, 0], cdf_box), ks(off[:, 1], cdf_box)]
    if filt == TENT:
        r = param or 1.0
        return [ks(off[:, 0], lambda x: cdf_tent(x, r)), ks(off[:, 1], lambda x: cdf_tent(x, r))]
    s = param or 0.5
    v = off.astype(np.float64) - 0.5
    rho = np.hypot(v[:, 0], v[:, 1])
    # (the atom at 4 sigma: float32 rounding of 0.5 + rho * cos may leave the recomputed radius a hair off 4 sigma)
    rho = np.where(np.abs(rho - 4 * s) < 1e-5, 4 * s, rho)
    ang = np.mod(np.arctan2(v[:, 1], v[:, 0]), 2 * np.pi) / (2 * np.pi)
    return [ks(rho, lambda x: cdf_gauss_radius(x, s)), ks(ang[rho > 1e-4], cdf_box)]


KS_CASES = [(BOX, 0.0), (TENT, 0.0), (TENT, 1.5), (GAUSSIAN, 0.0)]


def test_oracle_stream_is_inside_the_bound(oracle_mod):
    """Before relying on it: the ORACLE's rand_uniform stream for the chosen (pixel, timestamp) set, passed through the header's
    formulas in numpy, stays inside the KS bound for every filter."""
    W, H, gids, tss = ks_inputs()
    u, _, _ = stream(oracle_mod, W, gids, tss)
    for filt, param in KS_CASES:
        st = ks_stats(filt, param, offsets_f64(filt, param, u))
        print(NAMES[filt], param, "KS", st, "bound", KS_BOUND)
        assert max(st) <= KS_BOUND, (filt, param, st)


@pytest.mark.parametrize("filt,param", KS_CASES)
def test_offset_distribution(femu, cornell, filt, param):
    W, H, gids, tss = ks_inputs()
    off = femu.generate(cornell, W, H, filt, param, gids, tss)[2]
    st = ks_stats(filt, param, off)
    print(NAMES[filt], param, "KS", st, "bound", KS_BOUND)
    assert max(st) <= KS_BOUND


def test_ks_rejects_wrong_density(femu, cornell):
    """The statistic has power: BOX offsets against the tent CDF (and tent offsets against the uniform one) are far outside."""
    W, H, gids, tss = ks_inputs()
    box = femu.generate(cornell, W, H, BOX, 0.0, gids, tss)[2]
    tent = femu.generate(cornell, W, H, TENT, 0.0, gids, tss)[2]
    assert ks(box[:, 0], cdf_tent) > 10 * KS_BOUND and ks(tent[:, 0], cdf_box) > 10 * KS_BOUND
    assert ks(tent[:, 0], lambda x: cdf_tent(x, 1.5)) > 10 * KS_BOUND  # the wrong radius too


# ---- the whole estimator against the oracle, statistically ----------------------------------------------------------------
EST_W = EST_H = 32
EST_CROP = (20, 26, 13, 28)  # coarse rows [20, 26) x columns [13, 28): the short box's top edge and its silhouettes
EST_M, EST_N = 256, 4096     # oracle samples per fine pixel (8x; a quarter of it at 16x), emu samples per coarse pixel


def _cell_weights(cdf, p0, p1, scale):
    """A[P - p0, j]: probability that the offset of coarse pixel P falls into the cell of fine sample j.  The fine frame's pixel
    j is the unjittered ray through coarse coordinate j / scale; it stands for the cell [(j - 1/2) / scale, (j + 1/2) / scale)
    (midpoint rule).  Exact differences of the offset's CDF; the fine window reaches one coarse pixel beyond the crop, which
    covers the tent's support [-0.5, 1.5]."""
    j = np.arange((p0 - 1) * scale, (p1 + 1) * scale)[None, :]
    P = np.arange(p0, p1)[:, None]
    return cdf((j + 0.5) / scale - P) - cdf((j - 0.5) / scale - P)


def _oracle_fine(orc, scale, spp, ts0):
    """The oracle's UNJITTERED render of the crop's window at `scale` x the resolution (same fov), timestamps [ts0, ts0 + spp)."""
    r0, r1, c0, c1 = EST_CROP
    ys = np.arange((r0 - 1) * scale, (r1 + 1) * scale)
    xs = np.arange((c0 - 1) * scale, (c1 + 1) * scale)
    ids = (ys[:, None] * (EST_W * scale) + xs[None, :]).astype(np.uint32).ravel()
    img, _ = orc.render(EST_W * scale, EST_H * scale, spp=spp, first_timestamp=ts0, pixel_ids=ids)
    # the running mean of timestamps [ts0, ts0 + spp) started from a zero buffer is sum / (ts0 + spp): rescaled to the mean
    return img.reshape(len(ys), len(xs), 4)[:, :, :3].astype(np.float64) * ((ts0 + spp) / spp)


def _expectation(fine, cdf, scale):
    r0, r1, c0, c1 = EST_CROP
    return np.einsum("yj,jic,xi->yxc", _cell_weights(cdf, r0, r1, scale), fine, _cell_weights(cdf, c0, c1, scale))


def _rel(a, b):
    return float(np.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()))


def test_estimator_against_oracle_expectation(femu, oracle_mod, cornell):
    """Cornell 32x32, BOX and TENT r = 1: the emu image (the product's generate_path + bounce loop, N spp) against the filter's
    expectation built from the ORACLE's unjittered renders at 8x the resolution, weighted per coarse pixel with the filter's
    exact cell probabilities.  Relative RMSE over the crop EST_CROP.

    floor = the largest relative RMSE between three builds of the expectation: 8x from timestamps [0, M), 8x from [M, 2M),
    16x from [2M, 2M + M/4) (noise + discretisation).  Asserted: the emu image is within 2 x floor; the unfiltered emu image
    and the BOX image against the TENT expectation are outside it, by at least another factor 2.

    Sample counts: the expectation of a BOX pixel holds 64 M oracle samples, the emu image N.  In the noise-only limit
    dist^2 = s^2 (1/N + 1/64M) and floor^2 = 2 s^2 / 64M, so dist <= 2 floor needs N >= 64 M / 7; N = 16 M gives
    dist^2 / floor^2 = 2.5 of the 4 allowed.  Why a crop: on the whole frame the light's edges, which lie exactly on the 8x
    grid, dominate every distance (first-order discretisation, emu / floor = 2.1), and without the light M = 16 leaves noise of
    6 % against a box-tent difference of 4 %.  The crop holds the strongest silhouettes that are not grid-aligned and lets M be 256.

    Measured (M = 256, N = 4096; profiles/pixel_filter_cpu_check.txt):
      BOX   floor 0.0346   emu 0.0409 (1.18 floor)   unfiltered 0.7092   TENT image 0.1268
      TENT  floor 0.0282   emu 0.0377 (1.34 floor)   unfiltered 0.6499   BOX image  0.1348 (2.39 x the threshold)"""
    from concurrent.futures import ThreadPoolExecutor

    orc = oracle_mod.Oracle(cornell)
    M, N = EST_M, EST_N
    f8a = _oracle_fine(orc, 8, M, 0)
    f8b = _oracle_fine(orc, 8, M, M)
    f16 = _oracle_fine(orc, 16, M // 4, 2 * M)
    es = femu.scene(cornell)
    r0, r1, c0, c1 = EST_CROP
    ids = (np.arange(r0, r1)[:, None] * EST_W + np.arange(c0, c1)[None, :]).astype(np.uint32).ravel()

    def emu_image(filt):
        return es.render(EST_W, EST_H, N, pixel_filter=filt, pixel_ids=ids)[0].reshape(r1 - r0, c1 - c0, 4)[:, :, :3].astype(np.float64)

    with ThreadPoolExecutor(3) as ex:  # (the library call releases the GIL)
        img = dict(zip((NONE, BOX, TENT), ex.map(emu_image, (NONE, BOX, TENT))))
    for filt, cdf, other in ((BOX, cdf_box, TENT), (TENT, cdf_tent, BOX)):
        ea, eb, ec = _expectation(f8a, cdf, 8), _expectation(f8b, cdf, 8), _expectation(f16, cdf, 16)
        floor = max(_rel(ea, eb), _rel(ea, ec), _rel(eb, ec))
        d_emu, d_none, d_other = _rel(img[filt], ea), _rel(img[NONE], ea), _rel(img[other], ea)
        print("%-4s floor %.4f (8x/8x %.4f, 8x/16x %.4f %.4f)  emu %.4f  unfiltered %.4f  %s image %.4f"
              % (NAMES[filt], floor, _rel(ea, eb), _rel(ea, ec), _rel(eb, ec), d_emu, d_none, NAMES[other], d_other))
        assert d_emu <= 2 * floor, (NAMES[filt], d_emu, floor)
        assert d_none > 2 * floor, (NAMES[filt], d_none, floor)
        if filt == TENT:
            assert d_other > 2 * floor, (d_other, floor)  # the BOX image against the TENT expectation
            assert d_other >= 4 * floor and d_none >= 4 * floor  # ... and they miss by a factor 2 more, as chosen
        else:
            assert d_none >= 4 * floor


# ---- loader ---------------------------------------------------------------------------------------------------------------
def _scene_bytes(s):
    a = s.arrays()
    parts = [a.instances.tobytes(), a.positions.tobytes(), a.normals.tobytes(), a.lights.tobytes(), np.asarray(a.to_world).tobytes(),
             np.float32(a.fov).tobytes()] + [b.tobytes() for b in a.bsdfs]
    return b"".join(parts)


def test_loader_reads_the_films_filter():
    from gpuspectral_amd import host

    with_f = host.Scene(CORNELL_XML, read_filter=True)
    assert with_f.pixel_filter == (TENT, 0.0)  # <rfilter type="tent" />: param 0 = the default radius 1
    without = host.Scene(CORNELL_XML)
    assert without.pixel_filter == (NONE, 0.0)
    # nothing else changes: the flattened scene is byte-equal, with and without the option
    assert _scene_bytes(with_f) == _scene_bytes(without) and with_f.warnings == without.warnings


def _cornell_with_rfilter(tmp_path, rfilter_xml):
    text = open(CORNELL_XML).read()
    assert '<rfilter type="tent" />' in text
    d = tmp_path / "scene"
    d.mkdir()
    for f in os.listdir(os.path.dirname(CORNELL_XML)):
        if f != "scene.xml":
            os.symlink(os.path.join(os.path.dirname(CORNELL_XML), f), str(d / f))
    (d / "scene.xml").write_text(text.replace('<rfilter type="tent" />', rfilter_xml))
    return str(d / "scene.xml")


@pytest.mark.parametrize("xml,expected", [
    ('<rfilter type="box" />', (BOX, 0.0)),
    ('<rfilter type="tent" ><float name="radius" value="1.5" /></rfilter>', (TENT, 1.5)),
    ('<rfilter type="gaussian" />', (GAUSSIAN, 0.0)),
    ('<rfilter type="gaussian" ><float name="stddev" value="0.75" /></rfilter>', (GAUSSIAN, 0.75)),
])
def test_loader_filter_types(tmp_path, xml, expected):
    from gpuspectral_amd import host

    assert host.Scene(_cornell_with_rfilter(tmp_path, xml), read_filter=True).pixel_filter == expected


@pytest.mark.parametrize("kind", ["mitchell", "catmullrom", "lanczos"])
def test_loader_refuses_negative_lobes(tmp_path, kind):
    from gpuspectral_amd import host

    path = _cornell_with_rfilter(tmp_path, '<rfilter type="%s" />' % kind)
    with pytest.raises(host.GspError) as e:
        host.Scene(path, read_filter=True)
    assert kind in str(e.value)
    assert host.Scene(path).pixel_filter == (NONE, 0.0)  # without the option the film is ignored, as before
