"""Argument vectors of the device functions, generated once and shared by the CPU tests (tests/test_emu_parity.py: the host
compile against itself and the oracle) and the GPU tests (tests/test_gpu_devfn.py: the gfx950 compile against the host compile).
Every generator is deterministic (its own RandomState) and cached: both suites see the same arrays."""
import functools

import numpy as np

F32 = np.float32


def _bits(u):
    return np.ascontiguousarray(u, np.uint32).view(np.float32)


def _neighbours(values, k=64):
    """The k bit-pattern neighbours on each side of every float32 in `values` (and the values themselves)."""
    u = np.ascontiguousarray(values, np.float32).view(np.uint32).astype(np.int64)
    d = np.arange(-k, k + 1, dtype=np.int64)
    return _bits(((u[:, None] + d[None, :]) & 0xFFFFFFFF).reshape(-1).astype(np.uint32))


# ---- math ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def math_x():
    """Every 1024th float32 bit pattern (4 194 304 values: both signs, subnormals, +-inf, NaNs of both signs), then the 64
    neighbours on each side of every branch constant of pt_math.h, both signs:
      0 and the smallest normal 0x00800000 (det_logf's subnormal branch); sqrt(1/2) as a mantissa, at several exponents
      (det_logf's split); det_expf's overflow and underflow limits; (k + 1/2) pi / 2 for k = -8 .. 8 (where rint(x 2/pi) flips
      in det_sincosf, and +-(k + 1/2) / log2(e) where det_expf's does); the largest |x| of det_sincosf's domain (2^31 pi / 2)."""
    grid = _bits(np.arange(0, 2 ** 32, 1024, dtype=np.uint64).astype(np.uint32))
    k = np.arange(-8, 9, dtype=np.float64)
    consts = np.concatenate([
        _bits([0x00000000, 0x00800000, 0x7F800000, 0x3F800000]),
        (np.sqrt(0.5) * 2.0 ** np.array([-148.0, -127.0, -126.0, -1.0, 0.0, 1.0, 24.0, 127.0])).astype(F32),
        np.array([88.72283905206835, -87.33654475055310898657], F32),
        ((k + 0.5) * (np.pi / 2)).astype(F32),
        ((k + 0.5) / 1.44269504088896341).astype(F32),
        np.array([2.0 ** 31 * np.pi / 2], F32),
    ])
    near = _neighbours(consts)
    return np.ascontiguousarray(np.concatenate([grid, near, -near]))


@functools.lru_cache(None)
def atan2_yx():
    """(y, x): the full grid {+-0, +-subnormal, +-1, +-1e30, +-inf, NaN}^2; ratios y / x at the 64 neighbours of tan(pi / 8) and
    tan(3 pi / 8) (det_atanf_pos's two reductions) for x = 1, 3 and 1e-20, every sign; 200 000 random pairs over 80 decades."""
    g = np.array([0.0, -0.0, 1e-40, -1e-40, 1.0, -1.0, 1e30, -1e30, np.inf, -np.inf, np.nan], F32)
    gy, gx = [a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij")]
    t = _neighbours(np.array([0.4142135623730950, 2.414213562373095], F32))
    ys, xs = [gy], [gx]
    for x0 in (1.0, 3.0, 1e-20):
        for sy in (1, -1):
            for sx in (1, -1):
                ys.append((t * F32(x0) * F32(sy)).astype(F32))
                xs.append(np.full(t.size, x0 * sx, F32))
    rng = np.random.RandomState(4242)
    n = 200000
    ys.append((rng.choice([-1, 1], n) * 10.0 ** rng.uniform(-40, 38, n)).astype(F32))
    xs.append((rng.choice([-1, 1], n) * 10.0 ** rng.uniform(-40, 38, n)).astype(F32))
    return np.ascontiguousarray(np.concatenate(ys)), np.ascontiguousarray(np.concatenate(xs))


@functools.lru_cache(None)
def normalize_v():
    """Vectors of every magnitude: random directions scaled over 1e-20 .. 1e18 (squares stay finite and normal), axis-aligned,
    one component subnormal, and the degenerate ones (zero, squares that underflow or overflow, inf, NaN)."""
    rng = np.random.RandomState(99)
    n = 300000
    v = rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-18, 18, (n, 1))
    v = v.astype(F32)
    v[:3000, 1:] = 0
    v[3000:6000, :2] = 0
    v[6000:9000, 1] = F32(1e-41)
    special = np.array([[0, 0, 0], [1e-30, 0, 0], [1e-23, 1e-23, 1e-23], [1e30, 1e30, 0], [np.inf, 1, 0], [np.nan, 1, 0], [0, 0, -0.0],
                        [1e-45, 0, 1]], F32)
    return np.ascontiguousarray(np.concatenate([v, special]))


# ---- rng -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def rng_ab():
    """1 M (a, b) pairs: the edge words {0, 1, 0x7fffffff, 0x80000000, 0xffffffff}^2, then random words."""
    e = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], np.uint32)
    ea, eb = [x.reshape(-1) for x in np.meshgrid(e, e, indexing="ij")]
    rng = np.random.RandomState(31337)
    n = 1_000_000 - ea.size
    a = np.concatenate([ea, rng.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)])
    b = np.concatenate([eb, rng.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)])
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


# ---- frame and helpers ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def frame_nv():
    """100 000 (normal, vector) pairs: random unit normals, then axis-aligned ones, n.z = +-1 exactly, |n.x| == |n.z| (the branch of
    make_frame), one component subnormal, unnormalised and tiny normals."""
    rng = np.random.RandomState(808)
    n = 100000
    nr = rng.normal(size=(n, 3))
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    nr = nr.astype(F32)
    ax = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F32)
    nr[:6000] = ax[np.arange(6000) % 6]
    nr[6000:8000, 0] = nr[6000:8000, 2]  # |n.x| == |n.z|
    nr[8000:9000, 0] = -nr[8000:9000, 2]
    k = np.arange(9000, 12000)
    nr[k, k % 3] = F32(1e-42) * np.where(k % 2, 1, -1).astype(F32)  # one subnormal component
    nr[12000:13000] *= F32(1e-18)  # dot(n, n) ~ 1e-36
    nr[13000:14000] *= F32(1e15)
    nr[14000:14100] = 0  # the zero normal: NaN frame on both sides
    v = (rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3, 3, (n, 1))).astype(F32)
    return np.ascontiguousarray(nr), np.ascontiguousarray(v)


@functools.lru_cache(None)
def helper_fgh():
    """power_heuristic(f, g), cosine_pdf(z = f), bsdf_transmits(h): pdfs over 60 decades, zeros (0 / 0), inf, NaN; every type."""
    rng = np.random.RandomState(5150)
    n = 100000
    f = (10.0 ** rng.uniform(-30, 30, n)).astype(F32)
    g = (10.0 ** rng.uniform(-30, 30, n)).astype(F32)
    f[:2000] = rng.uniform(-1, 1, 2000).astype(F32)  # cosines
    sp = np.array([0.0, -0.0, np.inf, np.nan, 1e-40, 1e-23, 1e20, 3.1415927e-6], F32)
    f[2000:2000 + 64] = np.repeat(sp, 8)
    g[2000:2000 + 64] = np.tile(sp, 8)
    h = ((np.arange(n, dtype=np.uint32) % 10) << 16) | rng.randint(0, 65536, n).astype(np.uint32)
    return np.ascontiguousarray(f), np.ascontiguousarray(g), np.ascontiguousarray(h)


@functools.lru_cache(None)
def sampler_seeds_alpha():
    """100 000 (seed, alpha): alpha in {1e-4 .. 1} log-uniform and the decade values; seeds random plus the edge words and the
    states whose next draws are 0 and 0xffffffff-like (u = 1: log(1 - u) = -inf in sample_half_beckmann)."""
    rng = np.random.RandomState(2718)
    n = 100000
    seeds = rng.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    seeds[:5] = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
    alpha = (10.0 ** rng.uniform(-4, 0, n)).astype(F32)
    alpha[:5000] = np.array([1e-4, 1e-3, 1e-2, 1e-1, 1.0], F32)[np.arange(5000) % 5]
    return np.ascontiguousarray(seeds), np.ascontiguousarray(alpha)


# ---- trace ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def tri_test_cases():
    """400 000 (ray, triangle) pairs -> rays n x {o.xyz, d.xyz, tmin, tmax}, tris n x 9: rays of every dominant axis and sign,
    rays through shared edges and vertices (the double-precision fallback), axis-parallel rays, degenerate and far-away triangles."""
    rng = np.random.RandomState(77)
    n = 400000
    tris = rng.uniform(-2, 2, (n, 9)).astype(np.float32)
    tris[: n // 8] *= np.float32(1e-3)  # tiny
    tris[n // 8: n // 4] += np.float32(1e4)  # far from the origin
    o = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    k = rng.randint(0, 4, n)
    bary = rng.dirichlet((1, 1, 1), n).astype(np.float32)
    bary[k == 1] = np.eye(3, dtype=np.float32)[rng.randint(0, 3, (k == 1).sum())]  # through a vertex
    e = k == 2
    bary[e, 2] = 0
    bary[e, 0] = rng.uniform(0, 1, e.sum()).astype(np.float32)
    bary[e, 1] = np.float32(1) - bary[e, 0]  # through an edge
    tgt = (tris.reshape(n, 3, 3) * bary[:, :, None]).sum(1)
    tgt[k == 3] = rng.uniform(-3, 3, ((k == 3).sum(), 3)).astype(np.float32)  # anywhere: mostly misses
    d = tgt - o
    ax = rng.randint(0, 12, n)
    for a in range(3):  # axis-parallel rays (two zero components), both signs
        m = ax == a
        z = np.zeros((m.sum(), 3), np.float32)
        z[:, a] = np.where(rng.rand(m.sum()) < 0.5, -1, 1)
        d[m] = z
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-30).astype(np.float32)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 3:6] = o, d
    rays[:, 6] = np.where(rng.rand(n) < 0.5, 0.0, 0.01)
    rays[:, 7] = np.where(rng.rand(n) < 0.5, 1e10, rng.uniform(0.1, 8, n))
    tris[-1000:, 6:9] = tris[-1000:, 0:3]  # zero-area triangles
    return np.ascontiguousarray(rays), np.ascontiguousarray(tris)


@functools.lru_cache(None)
def node_encoder_cases():
    """400 000 nodes -> boxes n x 4 x {lo.xyz, hi.xyz}, counts n x {ni, nl}: every child count, boxes of every size from 1e-30 to
    1e30, children that coincide (ties in every octant), flat and point-like nodes, huge offsets from the origin."""
    rng = np.random.RandomState(20250)
    n = 400_000
    centre = rng.uniform(-1, 1, (n, 1, 3)) * 10.0 ** rng.uniform(-3, 6, (n, 1, 1))
    size = 10.0 ** rng.uniform(-30, 30, (n, 1, 1)) * (rng.rand(n, 1, 1) < 0.1) + 10.0 ** rng.uniform(-4, 3, (n, 1, 1)) * 1.0
    size = np.minimum(size, 1e30)
    lo = centre + rng.uniform(-1, 1, (n, 4, 3)) * size
    ext = rng.uniform(0, 1, (n, 4, 3)) * size * (rng.rand(n, 4, 3) > 0.1)  # flat children on some axes
    hi = lo + ext
    boxes = np.concatenate([lo, hi], axis=2).astype(np.float32)
    dup = rng.rand(n) < 0.2  # ties: children 1.. repeat child 0 (or each other)
    boxes[dup, 1] = boxes[dup, 0]
    dup2 = rng.rand(n) < 0.1
    boxes[dup2, 3] = boxes[dup2, 2]
    snap = rng.rand(n) < 0.1  # centres on a coarse grid: equal keys in some octants only
    boxes[snap] = np.round(boxes[snap] * 4) / 4
    boxes[snap, :, 3:] = np.maximum(boxes[snap, :, 3:], boxes[snap, :, :3])
    cnt = rng.randint(0, 5, n)
    ni = (rng.rand(n) * (cnt + 1)).astype(np.int32)
    counts = np.stack([ni, cnt - ni], axis=1).astype(np.int32)
    return np.ascontiguousarray(boxes), np.ascontiguousarray(counts)


@functools.lru_cache(None)
def shear_dirs():
    """Directions for make_shear / make_shear_rot: the rays of tri_test_cases, then ties between the largest components, signed
    zeros, one component subnormal, the zero vector."""
    rays, _ = tri_test_cases()
    d = rays[:100000, 3:6].copy()
    d[:2000, 1] = d[:2000, 0]
    d[2000:4000, 2] = -d[2000:4000, 1]
    d[4000:5000, 0] = F32(-0.0)
    d[5000:6000, 2] = F32(1e-42)
    d[6000:6010] = 0
    d[6010:6020] = F32(-0.0)
    return np.ascontiguousarray(d)


def node_test_cases(records):
    """For encoded node records (n x 16 words): node indices and rays {o.xyz, d.xyz, tmin, tfar}, 8 rays per record -- one per sign
    octant aimed at the node's origin from outside, every second one made axis-parallel (two components exactly 0: 1 / d = inf,
    either sign of zero)."""
    n = len(records)
    rng = np.random.RandomState(606)
    idx = np.repeat(np.arange(n, dtype=np.uint32), 8)
    org = records[:, 0:3].copy().view(np.float32)
    org = np.where(np.isfinite(org), org, 0).astype(np.float32)
    oct_ = np.tile(np.arange(8), n)
    sign = np.stack([np.where(oct_ & 1, -1.0, 1.0), np.where(oct_ & 2, -1.0, 1.0), np.where(oct_ & 4, -1.0, 1.0)], axis=1)
    d = (sign * rng.uniform(0.05, 1.0, (8 * n, 3))).astype(np.float32)
    par = rng.rand(8 * n) < 0.5
    keep = rng.randint(0, 3, 8 * n)
    for a in range(3):
        m = par & (keep != a)
        d[m, a] = np.where(rng.rand(m.sum()) < 0.5, F32(0.0), F32(-0.0))
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    dist = (10.0 ** rng.uniform(-2, 3, (8 * n, 1))).astype(np.float32)
    o = (np.repeat(org, 8, axis=0) - d * dist + rng.normal(size=(8 * n, 3)).astype(np.float32) * dist * F32(0.1)).astype(np.float32)
    rays = np.zeros((8 * n, 8), np.float32)
    rays[:, 0:3], rays[:, 3:6] = o, d
    rays[:, 6] = np.where(rng.rand(8 * n) < 0.5, 0.0, 0.01)
    rays[:, 7] = np.where(rng.rand(8 * n) < 0.5, 1e10, (dist[:, 0] * rng.uniform(0.5, 2.0, 8 * n)))
    return np.ascontiguousarray(idx), np.ascontiguousarray(rays)


# ---- bsdf ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def bsdf_cases(n=200000):
    """64 records per type and n (handle, wo, seed) vectors.
    Records: alpha log-uniform in [1e-4, 1] (ends included); IOR pairs at ratio 1 +- 1e-6, 1 exactly and up to 3, either side
    denser; r0 from 0 to 1 - 1e-6; reflectances and diffuse colours including 0 and > 1; conductor eta / k from 0.05 to 8.
    wo: |wo.z| from 1 down to 1e-7 (log-uniform), exactly (0, 0, +-1), below the surface for half, exactly grazing (z = 0), and for
    the dielectric types just inside and just outside the critical angle of the record."""
    from gpuspectral_amd import abi

    rng = np.random.RandomState(1234)
    R = 64
    alpha = (10.0 ** rng.uniform(-4, 0, R)).astype(F32)
    alpha[:2] = [1e-4, 1.0]
    ratio = np.concatenate([[1.0, 1.0 + 1e-6, 1.0 - 1e-6, 3.0, 1.0 / 3.0, 1.5, 1.0 / 1.5, 1.33], rng.uniform(1.0, 3.0, R - 8) ** rng.choice([-1, 1], R - 8)])
    ior_out = rng.uniform(1.0, 1.6, R).astype(F32)
    ior_out[:8] = 1.0
    ior_in = (ior_out * ratio).astype(F32)
    r0 = rng.uniform(0, 1, R).astype(F32)
    r0[:4] = [0.0, 1.0 - 1e-6, 0.04, 0.5]
    col = rng.uniform(0, 1, (R, 3)).astype(F32)
    col[0] = 0
    col[1] = [1.5, 2.0, 1.0]
    col[2] = [1, 1, 1]
    col[3] = [0, 0.5, 1.25]
    b = [np.zeros(R, dt) for dt in abi.BSDF_DTYPES]
    b[0]["reflectance"] = col
    for t in (1, 2):
        b[t]["ior_in"], b[t]["ior_out"] = ior_in, ior_out
    b[3]["diffuse"], b[3]["ior_in"], b[3]["ior_out"], b[3]["r0"] = col, ior_in, ior_out, r0
    b[4]["eta"] = (10.0 ** rng.uniform(-1.3, 0.9, (R, 3))).astype(F32)
    b[4]["k"] = (10.0 ** rng.uniform(-1.3, 0.9, (R, 3))).astype(F32)
    b[4]["reflectance"], b[4]["alpha"] = col, alpha
    b[5]["diffuse"], b[5]["r0"] = col, r0
    b[6]["diffuse"], b[6]["r0"], b[6]["alpha"] = col, r0, alpha
    b[7]["diffuse"], b[7]["ior_in"], b[7]["ior_out"], b[7]["r0"], b[7]["alpha"] = col, ior_in, ior_out, r0, alpha

    t = (np.arange(n) % 8).astype(np.uint32)
    rec = rng.randint(0, R, n).astype(np.uint32)
    handles = (t << 16) | rec
    z = 10.0 ** rng.uniform(-7, 0, n)
    z[rng.rand(n) < 0.05] = 1.0
    phi = rng.uniform(0, 2 * np.pi, n)
    # critical angle of the record, from the denser side: sin(theta_c) = n_small / n_big
    crit = rng.rand(n) < 0.15
    lo_, hi_ = np.minimum(ior_in, ior_out).astype(np.float64)[rec], np.maximum(ior_in, ior_out).astype(np.float64)[rec]
    sc = np.clip(lo_ / hi_, 0, 1)
    zc = np.sqrt(np.maximum(0.0, 1.0 - (sc * (1.0 + rng.choice([-1, 1], n) * 10.0 ** rng.uniform(-7, -3, n))) ** 2))
    z = np.where(crit, zc, z)
    s = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    sgn = np.where(rng.rand(n) < 0.5, -1.0, 1.0)
    denser_inside = (ior_in > ior_out)[rec]
    sgn = np.where(crit, np.where(denser_inside, -1.0, 1.0), sgn)  # total internal reflection needs wo on the denser side
    wo = np.stack([s * np.cos(phi), s * np.sin(phi), sgn * z], axis=1).astype(F32)
    k = np.arange(n)
    wo[(k % 1000) == 0] = [0, 0, 1]
    wo[(k % 1000) == 1] = [0, 0, -1]
    wo[(k % 1000) == 2] = [1, 0, 0]  # grazing: cos = 0
    wo[(k % 1000) == 3] = [0, -1, -0.0]
    seeds = rng.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    wi_random = rng.normal(size=(n, 3))
    wi_random /= np.linalg.norm(wi_random, axis=1, keepdims=True)
    use_sampled = rng.rand(n) < 0.5  # the caller replaces these rows of wi by the direction the host's bsdf_sample returns
    return tuple(b), np.ascontiguousarray(handles), np.ascontiguousarray(wo), np.ascontiguousarray(seeds), np.ascontiguousarray(wi_random.astype(F32)), use_sampled


# ---- light ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def light_cases():
    """A list of (name, light records, positions, seeds): one light and 720 lights, zero-area lights (two equal vertices, three
    equal vertices), pos on the light's plane, pos at a vertex, pos 1e6 away, lights so small that bake_light's cross products
    and the area are subnormal, no light at all."""
    from gpuspectral_amd import abi

    rng = np.random.RandomState(7071)

    def mk(m):
        L = np.zeros(m, abi.LIGHT_DT)
        L["positions"][:, :, :3] = rng.uniform(-2, 2, (m, 3, 3)).astype(F32)
        L["radiance"][:, :3] = rng.uniform(0, 20, (m, 3)).astype(F32)
        return L

    def pts(n):
        return rng.uniform(-3, 3, (n, 3)).astype(F32), rng.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)

    out = []
    for m in (1, 720):
        p, s = pts(20000)
        out.append(("%d lights" % m, mk(m), p, s))
    L = mk(16)
    L["positions"][:8, 2, :3] = L["positions"][:8, 1, :3]  # zero area: a segment
    L["positions"][8:, 1, :3] = L["positions"][8:, 0, :3]
    L["positions"][8:, 2, :3] = L["positions"][8:, 0, :3]  # ... a point
    p, s = pts(20000)
    out.append(("zero-area lights", L, p, s))
    L = mk(1)
    v = L["positions"][0, :, :3].astype(np.float64)
    w = rng.dirichlet((1, 1, 1), 20000) * 3.0 - 1.0  # affine combinations: on the plane, inside and outside the triangle
    w[:, 2] = 1.0 - w[:, 0] - w[:, 1]
    p = (w @ v).astype(F32)
    p[:3000] = L["positions"][0, np.arange(3000) % 3, :3]  # at a vertex
    out.append(("pos on the plane / at a vertex", L, p, pts(20000)[1]))
    L = mk(4)
    p, s = pts(20000)
    d = rng.normal(size=(20000, 3))
    p = (p + 1e6 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    out.append(("pos 1e6 away", L, p, s))
    L = mk(8)  # edges of 1e-20: the cross products of bake_light (1e-40) and the area are subnormal
    L["positions"][:, 0, :3] = 0
    L["positions"][:, 1:, :3] = rng.uniform(-1, 1, (8, 2, 3)).astype(F32) * F32(1e-20)
    p, s = pts(5000)
    p[:2500] *= F32(1e-19)  # ... and so are the squared distances from positions that close
    out.append(("tiny lights (subnormal cross products and area)", L, p, s))
    p, s = pts(1000)
    out.append(("no light", mk(0), p, s))
    return out


# ---- texture -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def texture_cases():
    """(textures, texels, ids, uv): a 1 x 1, a 3 x 5 and a 64 x 64 RGBA8 texture in one texel array; per texture, u and v from
    {exact texel-grid positions, +-1e-7 off them, +-1e6, negative, beyond 1e9 (texel 0), NaN, inf} and random ones."""
    from gpuspectral_amd import abi

    rng = np.random.RandomState(3535)
    dims = [(1, 1), (3, 5), (64, 64)]
    textures = np.zeros(3, abi.TEXTURE_DT)
    first = 0
    for k, (w, h) in enumerate(dims):
        textures[k] = (w, h, first)
        first += w * h
    texels = rng.randint(0, 2 ** 32, first, dtype=np.uint64).astype(np.uint32)
    ids, uvs = [], []
    for k, (w, h) in enumerate(dims):
        grid = []
        for m in (w, h):
            g = (np.arange(-2 * m - 2, 2 * m + 3) / (2.0 * m)).astype(F32)  # texel centres and texel edges, wrapped both ways
            g = np.concatenate([g, g + F32(1e-7), g - F32(1e-7), np.nextafter(g, F32(np.inf)), np.nextafter(g, F32(-np.inf)),
                                np.array([1e6, -1e6, 1e6 + 0.25, -7.3, 3e9, -3e9, 1e30, np.inf, -np.inf, np.nan, 1e-42, -0.0], F32)])
            grid.append(g.astype(F32))
        n = 4000
        u = np.concatenate([rng.choice(grid[0], n), rng.uniform(-3, 3, n).astype(F32)])
        v = np.concatenate([rng.choice(grid[1], n), rng.uniform(-3, 3, n).astype(F32)])
        ids.append(np.full(2 * n, k, np.uint32))
        uvs.append(np.stack([u, v], axis=1).astype(F32))
    return textures, texels, np.ascontiguousarray(np.concatenate(ids)), np.ascontiguousarray(np.concatenate(uvs))


def srgb_decode_table():
    """The 256-entry sRGB -> linear table a host gives as gsp_scene_desc.texel_decode (float32 of the float64 formula)."""
    c = np.arange(256) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4).astype(F32)


def linear_decode_table():
    """What the upload fills in without a table: (float)b / 255.0f."""
    return (np.arange(256, dtype=F32) / F32(255.0)).astype(F32)


@functools.lru_cache(None)
def envmap_cases():
    """A list of (width, height, texels RGBA32F, to_local, dirs): 1 x 1, 3 x 5 and 64 x 32 maps; directions on the axes, the poles,
    around the -x .. +z seam of atan2(e.x, -e.z), random ones, zero / inf / NaN ones; identity and a rotated frame."""
    rng = np.random.RandomState(4646)
    eye = np.eye(4, dtype=F32).reshape(-1)
    a = 0.7
    rot = np.array([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]], F32).reshape(-1)
    ax = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, 0, 0], [np.inf, 0, 1], [np.nan, 0, 1],
                   [-0.0, 1, -0.0], [0, -1, -0.0], [1e-30, 1, 0], [1e-42, 0, 1], [0, 1e-42, -1]], F32)
    eps = np.concatenate([[0.0], 10.0 ** np.arange(-45.0, 0.0, 1.0)])
    seam = []
    for e in eps:  # atan2(e.x, -e.z) = +-pi at e.x = +-0, e.z > 0
        for y in (0.0, 0.3, -0.9):
            seam += [[e, y, 1.0], [-e, y, 1.0], [e, y, -1.0], [-e, y, -1.0], [1.0, y, e], [1.0, y, -e], [e, 1.0, e], [-e, -1.0, e]]
    seam = np.array(seam, F32)
    out = []
    for (w, h), m in (((1, 1), eye), ((3, 5), rot), ((64, 32), eye), ((64, 32), rot)):
        d = rng.normal(size=(6000, 3)).astype(F32)
        d /= np.linalg.norm(d, axis=1, keepdims=True).astype(F32)
        tex = (rng.uniform(0, 4, (h * w, 4)) * 10.0 ** rng.uniform(-2, 2, (h * w, 1))).astype(F32)
        out.append((w, h, np.ascontiguousarray(tex), m, np.ascontiguousarray(np.concatenate([ax, seam, d]))))
    return out
