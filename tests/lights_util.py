"""Shared by the light-selection tests (not a test module): the ctypes handle on tests/emu/liblights_emu.so -- the product's
pt_lightpick.h and shade_vertex<.., LSEL = true> compiled for the host (tests/emu/lights_emu.cpp; a test harness, never a product
path), built the way MediaEmu (media_util.py) builds its library; the loader of the device harness tests/devfn/liblights_devfn.so;
the scenes of the tests; and the header's "Light selection" rules restated in numpy / float64."""
import ctypes as C
import hashlib
import math
import os
import re
import shutil
import subprocess

import numpy as np

from conftest import ROOT

TWO32 = 4294967296.0
UNIFORM, POWER = 0, 1


class LightsEmu:
    def __init__(self):
        from gpuspectral_amd import abi

        d = os.path.join(ROOT, "tests", "emu")
        so = os.path.join(d, "liblights_emu.so")
        srcs = [os.path.join(d, f) for f in ("lights_emu.cpp", "pt_emu.cpp")] + [os.path.join(ROOT, "include", "gpuspectral_pt.h")]
        csrc = os.path.join(ROOT, "gpuspectral_amd", "csrc")
        srcs += [os.path.join(csrc, h) for h in os.listdir(csrc) if h.endswith(".h")]
        srcs += [os.path.join(ROOT, "tests", "devfn", f) for f in ("devfn_bodies.h", "lights_bodies.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mfma", "-mavx2", "-shared", "-o", so, srcs[0]])
        L = C.CDLL(so)
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        L.emu_create.restype = vp
        L.emu_create.argtypes = [C.POINTER(abi.SceneDesc)]
        L.emu_destroy.argtypes = [vp]
        L.lights_emu_build.argtypes = [vp, u32, vp]
        L.lights_emu_build.restype = None
        L.lights_emu_build_weights.argtypes = [vp, u32, vp]
        L.lights_emu_build_weights.restype = None
        L.lights_emu_weights.argtypes = [vp, u32, vp]
        L.lights_emu_weights.restype = None
        L.lights_emu_pick.argtypes = [vp, u32, vp, u64, vp, vp]
        L.lights_emu_devfn_power.argtypes = [vp, u32, vp, vp, u64, vp, vp]
        L.lights_emu_render.argtypes = [vp, u32, u32, vp, u64, C.POINTER(abi.RenderParams), u32, vp, C.POINTER(abi.Medium), u32, vp, vp, vp, vp]
        self.L, self.abi = L, abi

    def build(self, lights):
        """The product's builder over light records (abi.LIGHT_DT) -> abi.LIGHT_PICK_DT array."""
        lights = np.ascontiguousarray(lights, self.abi.LIGHT_DT)
        out = np.zeros(len(lights), self.abi.LIGHT_PICK_DT)
        self.L.lights_emu_build(lights.ctypes.data, len(lights), out.ctypes.data)
        return out

    def build_weights(self, w):
        w = np.ascontiguousarray(w, np.float64)
        out = np.zeros(len(w), self.abi.LIGHT_PICK_DT)
        self.L.lights_emu_build_weights(w.ctypes.data, len(w), out.ctypes.data)
        return out

    def weights(self, lights):
        lights = np.ascontiguousarray(lights, self.abi.LIGHT_DT)
        out = np.zeros(len(lights), np.float64)
        self.L.lights_emu_weights(lights.ctypes.data, len(lights), out.ctypes.data)
        return out

    def pick(self, table, r):
        """light_pick_index over the draws r -> (counts per light, pmf per draw)."""
        table, r = np.ascontiguousarray(table, self.abi.LIGHT_PICK_DT), np.ascontiguousarray(r, np.uint32)
        counts, pmf = np.zeros(len(table), np.uint64), np.zeros(r.size, np.float32)
        assert self.L.lights_emu_pick(table.ctypes.data, len(table), r.ctypes.data, r.size, counts.ctypes.data, pmf.ctypes.data) == 0
        return counts, pmf

    def devfn_power(self, lights, pos, seeds):
        return _devfn_power(self.L.lights_emu_devfn_power, self.abi, lights, pos, seeds)

    def scene(self, sc):
        return LightsEmuScene(self, sc)


def _devfn_power(fn, abi, lights, pos, seeds):
    lights = np.ascontiguousarray(lights, abi.LIGHT_DT)
    pos, seeds = np.ascontiguousarray(pos, np.float32).reshape(-1, 3), np.ascontiguousarray(seeds, np.uint32)
    assert len(pos) == seeds.size
    out, pick = np.zeros((len(pos), 8), np.float32), np.zeros(len(lights), abi.LIGHT_PICK_DT)
    rc = fn(lights.ctypes.data, len(lights), pos.ctypes.data, seeds.ctypes.data, len(pos), out.ctypes.data, pick.ctypes.data)
    if rc != 0:
        raise RuntimeError("sample_light_power harness returned %d" % rc)
    return out.view(np.uint32), pick


class LightsEmuScene:
    def __init__(self, emu, sc):
        self.emu, self.sc = emu, sc
        self._desc = sc.desc()
        self.h = emu.L.emu_create(C.byref(self._desc))

    def render(self, width, height, spp, mode=UNIFORM, media=None, first_timestamp=0, accum=None, lights=None, pixel_ids=None, moments=False,
               **params):
        """-> (accum[n,4], stats dict with the three ray counts, nee_kept / nee_cut and the NEE / emission sums[, moments[n,6]]).
        lights: the light records the table is built from (default: the scene's; another array = the tables of a later version)."""
        abi = self.emu.abi
        p = abi.default_render_params()
        p.spp, p.first_timestamp = spp, first_timestamp
        for k, v in params.items():
            setattr(p, k, v)
        ids = None if pixel_ids is None else np.ascontiguousarray(pixel_ids, np.uint32)
        n = width * height if ids is None else len(ids)
        accum = np.zeros((n, 4), np.float32) if accum is None else np.ascontiguousarray(accum, np.float32).copy()
        counts, sums = np.zeros(5, np.uint64), np.zeros(6, np.float64)
        mom = np.zeros((n, 6), np.float64) if moments else None
        lt = np.ascontiguousarray(self.sc.lights if lights is None else lights, abi.LIGHT_DT)
        assert len(lt) == len(self.sc.lights)
        arr = abi.media_array(media)
        rc = self.emu.L.lights_emu_render(self.h, width, height, None if ids is None else ids.ctypes.data, n, C.byref(p), mode, lt.ctypes.data, arr,
                                          len(arr) if arr is not None else 0, accum.ctypes.data, counts.ctypes.data, sums.ctypes.data,
                                          None if mom is None else mom.ctypes.data)
        if rc != 0:
            raise ValueError("lights_emu_render returned %d" % rc)
        st = dict(extension_rays=int(counts[0]), shadow_rays=int(counts[1]), shaded_vertices=int(counts[2]), nee_kept=int(counts[3]),
                  nee_cut=int(counts[4]), nee_sum=sums[:3].copy(), emission_sum=sums[3:].copy())
        return (accum, st, mom) if moments else (accum, st)

    def __del__(self):
        try:
            self.emu.L.emu_destroy(self.h)
        except Exception:
            pass


# ---- the device harness of sample_light_power (tests/devfn/lights_devfn.hip) ------------------------------------------------------
DEVFN_DIR = os.path.join(ROOT, "tests", "devfn")
DEVFN_LIB = os.path.join(DEVFN_DIR, "liblights_devfn.so")
_CSRC = os.path.join(ROOT, "gpuspectral_amd", "csrc")
# what tests/devfn/lights.mk hashes, in its order
DEVFN_DIGEST_SOURCES = tuple(os.path.join(DEVFN_DIR, f) for f in ("lights_devfn.hip", "lights_bodies.h", "devfn_bodies.h")) + tuple(
    os.path.join(_CSRC, f) for f in ("pt_lightpick.h", "pt_math.h", "pt_shading.h", "pt_trace.h", "pt_stages.h")) + (
    os.path.join(ROOT, "include", "gpuspectral_pt.h"),)


def devfn_source_digest():
    h = hashlib.sha256()
    for f in DEVFN_DIGEST_SOURCES:
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def devfn_stamped_digest(path=DEVFN_LIB):
    if not os.path.exists(path):
        return None
    with open(path, "rb") as fh:
        m = re.search(rb"arch=(\S+) digest=([0-9a-f]{16}) flags=([^\0]*)\0", fh.read())
    return None if m is None else m.group(2).decode()


def devfn_ensure_built():
    """The path of a device harness that carries the digest of the tree's sources; builds it with hipcc if it has to, raises if it
    cannot (the GPU tests never skip over it)."""
    if devfn_stamped_digest() == devfn_source_digest():
        return DEVFN_LIB
    if shutil.which("hipcc") is None:
        raise RuntimeError("%s is missing or stale and hipcc is not on the path: build it with `make -C tests/devfn -f lights.mk` (build() does)" % DEVFN_LIB)
    subprocess.check_call(["make", "-B", "-C", DEVFN_DIR, "-f", "lights.mk"])
    if devfn_stamped_digest() != devfn_source_digest():
        raise RuntimeError("make -C tests/devfn -f lights.mk left a library without the digest of the tree's sources")
    return DEVFN_LIB


class LightsDevice:
    def __init__(self):
        from gpuspectral_amd import abi

        self.L, self.abi = C.CDLL(devfn_ensure_built()), abi
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        self.L.lights_devfn_power.argtypes = [vp, u32, vp, vp, u64, vp, vp]

    def devfn_power(self, lights, pos, seeds):
        return _devfn_power(self.L.lights_devfn_power, self.abi, lights, pos, seeds)


# ---- the header's rules in numpy / float64 ---------------------------------------------------------------------------------------
def weights64(lights):
    """w_i = max(Y, 0) * 0.5 |cross(v2 - v0, v1 - v0)| in float64; non-finite -> 0."""
    lt = np.asarray(lights)
    p = lt["positions"].astype(np.float64)[:, :, :3]
    rad = lt["radiance"].astype(np.float64)
    with np.errstate(all="ignore"):
        y = 0.2126 * rad[:, 0] + 0.7152 * rad[:, 1] + 0.0722 * rad[:, 2]
        area = 0.5 * np.linalg.norm(np.cross(p[:, 2] - p[:, 0], p[:, 1] - p[:, 0]), axis=1)
        w = np.maximum(y, 0.0) * area
    return np.where(np.isfinite(w), w, 0.0)


def effective_weights(w):
    """Non-finite / negative -> 0; all zero -> all one."""
    w = np.asarray(w, np.float64)
    w = np.where(np.isfinite(w) & (w > 0.0), w, 0.0)
    return np.ones_like(w) if not (w > 0.0).any() else w


def implied_pmf(table):
    """p_i = (T_i + sum_{j != i, alias_j = i} (2^32 - T_j)) / (n 2^32) in float64, T = 2^32 for a saturated entry; and d_i."""
    thr = table["threshold"].astype(np.float64)
    T = np.where(table["threshold"] == 0xFFFFFFFF, TWO32, thr)
    n = len(table)
    mass, d = T.copy(), np.zeros(n, np.int64)
    other = table["alias"] != np.arange(n)
    np.add.at(mass, table["alias"][other], TWO32 - T[other])
    np.add.at(d, table["alias"][other], 1)
    return mass / (n * TWO32), d


def pick64(table, r):
    """The pick rule in numpy integers: r (uint32 array) -> light index per draw."""
    n = len(table)
    m = r.astype(np.uint64) * np.uint64(n)
    j = (m >> np.uint64(32)).astype(np.int64)
    lo = (m & np.uint64(0xFFFFFFFF)).astype(np.uint64)
    thr = table["threshold"].astype(np.uint64)[j]
    self_ = (lo < thr) | (thr == np.uint64(0xFFFFFFFF))
    return np.where(self_, j, table["alias"].astype(np.int64)[j])


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def tri_mesh(tris):
    """tris (n, 3, 3) world-space triangles -> (pos, nrm) with the geometric normal normalize(cross(v1 - v0, v2 - v0)) on every vertex."""
    t = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return t.reshape(-1, 3).astype(np.float32), np.repeat(nrm, 3, axis=0).astype(np.float32)


def down_triangle(cx, cz, y, area, turn=0.0):
    """An equilateral triangle of the given area in the plane y = const, centred on (cx, cz), facing DOWN (normal -y)."""
    r = math.sqrt(area * 4.0 / (3.0 * math.sqrt(3.0)))  # circumradius: area = 3 sqrt(3) / 4 r^2
    a = [turn + k * 2.0 * math.pi / 3.0 for k in range(3)]
    v = [(cx + r * math.cos(t), y, cz + r * math.sin(t)) for t in a]
    return [v[0], v[1], v[2]]  # cross(v1 - v0, v2 - v0) points along -y for increasing angle in the (x, z) plane


def _identity():
    return np.eye(4, dtype=np.float32).reshape(16)


def room_scene(num_lights, seed=3):
    """A Cornell room with a gold and a glass sphere and `num_lights` down-facing triangle lights under the ceiling, their areas
    spread over 1e-4 .. 3e-2 and their radiances over a factor of 30: 3 lights -> the table image fits the 8192 bytes of LDS,
    130 lights (130 x 64 B of records alone) -> it does not."""
    from gpuspectral_amd import scenes

    b = scenes.SceneBuilder()
    scenes._cornell_room(b)
    sph = b.add_mesh(*scenes.sphere_mesh(16, 8))
    b.add_object(sph, scenes.trs((0.45, 0.35, -0.1), 0.35), b.rough_conductor(scenes.GOLD_ETA, scenes.GOLD_K, 0.1))
    b.add_object(sph, scenes.trs((-0.5, 0.35, 0.2), 0.35), b.dielectric(1.3, 1.0), twofaced=False)
    rng = np.random.RandomState(seed)
    black = b.diffuse((0, 0, 0))
    for i in range(num_lights):
        area = 10.0 ** rng.uniform(-4.0, -1.5)
        le = 30.0 ** rng.uniform(0.0, 1.0) * np.array([1.0, 0.8, 0.5])
        tri = down_triangle(rng.uniform(-0.8, 0.8), rng.uniform(-0.8, 0.8), 1.95 - 0.001 * i, area, rng.uniform(0, 6.28))
        b.add_object(b.add_mesh(*tri_mesh([tri])), _identity(), black, twofaced=False, emission=le)
    return b.build()


def one_light_scene():
    """The room under ONE light triangle: power and uniform coincide bit for bit."""
    return room_scene(1)


FLOOR_RHO = (0.7, 0.6, 0.5)


def _floor(b, half=40.0, rho=FLOOR_RHO):
    from gpuspectral_amd import scenes

    tris = [[(-half, 0, -half), (-half, 0, half), (half, 0, half)], [(-half, 0, -half), (half, 0, half), (half, 0, -half)]]  # normal +y
    b.add_object(b.add_mesh(*tri_mesh(tris)), _identity(), b.diffuse(rho), twofaced=False)


def expectation_scene():
    """A diffuse floor (y = 0) under 16 small triangle lights at height 10, facing down: areas 1e-4 .. 1e-1 (log-spaced), luminances
    100 .. 1 (log-spaced the other way, a factor of 100).  Nothing else.  The camera looks down at the floor from (0, 3, 5)."""
    from gpuspectral_amd import scenes

    b = scenes.SceneBuilder()
    _floor(b)
    black = b.diffuse((0, 0, 0))
    for i in range(16):
        area = 1e-4 * 10.0 ** (3.0 * i / 15.0)
        le = 100.0 * 10.0 ** (-2.0 * i / 15.0) * np.array([1.0, 0.9, 0.7])
        tri = down_triangle(-3.0 + 2.0 * (i % 4), -3.0 + 2.0 * (i // 4), 10.0, area, 0.3 * i)
        b.add_object(b.add_mesh(*tri_mesh([tri])), _identity(), black, twofaced=False, emission=le)
    b.camera_lookat((0, 3, 5), (0, 0, 0), fov_deg=30.0)
    return b.build()


def direct_light64(sc, width, height, rho=FLOOR_RHO, levels=4):
    """float64 quadrature of rho / pi * sum_lights Le * integral cos cos' / d^2 dA at the floor point of every pixel's ray (the
    header's pinhole ray, tests/temporal_util.py pinhole_dirs64): every light triangle split into 4^levels sub-triangles, each
    taken at its centroid.  The lights are at most 0.5 across at distance >= 10: the centroid rule's relative error is of the order
    (sub-triangle size / distance)^2 < 1e-5.  -> (h * w, 3)."""
    import temporal_util as tu

    d = tu.pinhole_dirs64(sc.to_world, sc.fov, width, height).reshape(-1, 3)
    o = np.asarray(sc.to_world, np.float64)[12:15]
    t = -o[1] / d[:, 1]
    x = o[None, :] + t[:, None] * d  # floor points, normal +y
    out = np.zeros((len(x), 3))
    for L in sc.lights:
        tri = L["positions"].astype(np.float64)[:, :3][None]
        for _ in range(levels):
            a, b_, c = tri[:, 0], tri[:, 1], tri[:, 2]
            ab, bc, ca = (a + b_) / 2, (b_ + c) / 2, (c + a) / 2
            tri = np.concatenate([np.stack([a, ab, ca], 1), np.stack([ab, b_, bc], 1), np.stack([ca, bc, c], 1), np.stack([ab, bc, ca], 1)])
        cen = tri.mean(1)
        nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        dA = 0.5 * np.linalg.norm(nrm, axis=1)
        nrm /= (2.0 * dA)[:, None]
        v = cen[None, :, :] - x[:, None, :]
        d2 = (v * v).sum(-1)
        dist = np.sqrt(d2)
        cos_f = np.maximum(v[..., 1] / dist, 0.0)
        cos_l = np.maximum(-(v * nrm[None]).sum(-1) / dist, 0.0)
        g = (cos_f * cos_l / d2 * dA[None]).sum(1)
        out += g[:, None] * L["radiance"].astype(np.float64)[None, :3]
    return out * (np.asarray(rho)[None, :] / math.pi)


def fan_and_quad_scene(height=4.0, side=0.2, le=125.0):
    """The floor under a quad light (2 triangles, side x side) and a disk light (a fan of 64 triangles) of the same radiance whose
    area is 1 / 99 of the quad's: the fan holds 1 % of sum(w) in 64 of the 66 triangles, n * sum(p^2) = 66 * (2 * 0.495^2 + 64 *
    (0.01 / 64)^2) = 32.3.  The lights are small and far (0.2 across at height 4), so that next-event estimation carries the direct
    light in both modes: the uniform pick's pdf of the quad, d^2 / (cos A) / 66 >= 16 / 0.04 / 66 = 6, is well above the cosine
    lobe's 1 / pi."""
    from gpuspectral_amd import scenes

    b = scenes.SceneBuilder()
    _floor(b, half=6.0)
    black = b.diffuse((0, 0, 0))
    le = (le, le, le)
    k, y, h = 64, height, side / 2.0
    r = math.sqrt((side * side / 99.0) / (k * 0.5 * math.sin(2.0 * math.pi / k)))
    fan = [[(1.5, y, 0.0), (1.5 + r * math.cos(2 * math.pi * i / k), y, r * math.sin(2 * math.pi * i / k)),
            (1.5 + r * math.cos(2 * math.pi * (i + 1) / k), y, r * math.sin(2 * math.pi * (i + 1) / k))] for i in range(k)]
    b.add_object(b.add_mesh(*tri_mesh(fan)), _identity(), black, twofaced=False, emission=le)
    quad = [[(-h, y, -h), (h, y, -h), (h, y, h)], [(-h, y, -h), (h, y, h), (-h, y, h)]]
    b.add_object(b.add_mesh(*tri_mesh(quad)), _identity(), black, twofaced=False, emission=le)
    b.camera_lookat((0, 2.5, 5), (0, 0, 0), fov_deg=35.0)
    return b.build()


def weak_and_strong_weights():
    """66 lights = 64 weak + 2 strong (the pick-rule test)."""
    return np.concatenate([np.full(64, 0.01 / 64), np.full(2, 0.495)])
