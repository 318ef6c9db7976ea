"""Shared by the delta-light tests (not a test module): the ctypes handle on tests/emu/libdelta_emu.so -- the product's stage headers
with shade_vertex<.., DLT = true>, compiled for the host (tests/emu/delta_emu.cpp; a test harness, never a product path) -- built the
way ScatterEmu (scatter_util.py) builds its library; the device harness of pt_deltalight.h; the scenes of the tests; and the
header's "Delta lights" formulas restated in numpy / float64."""
import ctypes as C
import hashlib
import math
import os
import re
import shutil
import subprocess

import numpy as np

import media_util as mu
from conftest import ROOT

REFERENCE, TEXTBOOK = 0, 1
UNIFORM, POWER = 0, 1
EPS = 2.0 ** -24  # half an ulp of float32, relative: the error of one correctly rounded operation
same = mu.same


class DeltaEmu:
    def __init__(self):
        from gpuspectral_amd import abi

        d = os.path.join(ROOT, "tests", "emu")
        so = os.path.join(d, "libdelta_emu.so")
        srcs = [os.path.join(d, f) for f in ("delta_emu.cpp", "pt_emu.cpp")] + [os.path.join(ROOT, "include", "gpuspectral_pt.h")]
        csrc = os.path.join(ROOT, "gpuspectral_amd", "csrc")
        srcs += [os.path.join(csrc, h) for h in os.listdir(csrc) if h.endswith(".h")]
        srcs += [os.path.join(ROOT, "tests", "devfn", h) for h in ("devfn_bodies.h", "delta_bodies.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mfma", "-mavx2", "-shared", "-o", so, srcs[0]])
        L = C.CDLL(so)
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        DP = C.POINTER(abi.DeltaLight)
        L.emu_create.restype = vp
        L.emu_create.argtypes = [C.POINTER(abi.SceneDesc)]
        L.emu_destroy.argtypes = [vp]
        L.delta_emu_check.argtypes = [DP, u32, DP, C.c_char_p, u32]
        L.delta_emu_spot_falloff.argtypes = [u64, vp, vp, vp, vp]
        L.delta_emu_spot_falloff.restype = None
        L.delta_emu_sample_delta_light.argtypes = [u64, vp, vp, vp, vp]
        L.delta_emu_sample_delta_light.restype = None
        L.delta_emu_light_pick.argtypes = [vp, u32, DP, u32, vp, C.POINTER(C.c_float)]
        L.delta_emu_light_pick.restype = None
        L.delta_emu_render.argtypes = [vp, u32, u32, vp, u64, C.POINTER(abi.RenderParams), u32, u32, vp, DP, u32, C.POINTER(abi.Medium),
                                       C.POINTER(abi.MediumScatter), u32, vp, vp, vp, u32]
        self.L, self.abi = L, abi

    def check(self, lights, count=None):
        """gsp_set_delta_lights' validation: (None, the accepted records) or (the error text, None)."""
        arr = self.abi.delta_light_array(lights)
        n = (len(arr) if arr is not None else 0) if count is None else count
        out = (self.abi.DeltaLight * max(n, 1))()
        err = C.create_string_buffer(256)
        rc = self.L.delta_emu_check(arr, n, out, err, 256)
        return (err.value.decode(), None) if rc else (None, list(out)[:n])

    def spot_falloff(self, c, cos_cutoff, cos_beam):
        return _spot_falloff(self.L.delta_emu_spot_falloff, c, cos_cutoff, cos_beam)

    def sample_delta_light(self, recs, pos, pmf):
        return _sample_delta_light(self.L.delta_emu_sample_delta_light, recs, pos, pmf)

    def light_pick(self, tri_lights, delta):
        """The pick table over the triangle lights (abi.LIGHT_DT) and the ACCEPTED delta records, and the float32 1 / sum(w)."""
        lt = np.ascontiguousarray(tri_lights, self.abi.LIGHT_DT)
        arr = self.abi.delta_light_array(delta)
        nd = len(arr) if arr is not None else 0
        out = np.zeros(len(lt) + nd, self.abi.LIGHT_PICK_DT)
        inv = C.c_float(0.0)
        self.L.delta_emu_light_pick(lt.ctypes.data if len(lt) else None, len(lt), arr, nd, out.ctypes.data, C.byref(inv))
        return out, np.float32(inv.value)

    def scene(self, sc):
        return DeltaEmuScene(self, sc)


class DeltaEmuScene:
    def __init__(self, emu, sc):
        self.emu, self.sc = emu, sc
        self._desc = sc.desc()
        self.h = emu.L.emu_create(C.byref(self._desc))

    def render(self, width, height, spp, delta=None, media=None, scatter=None, first_timestamp=0, accum=None, estimator=REFERENCE, light_mode=UNIFORM,
               narrow=False, samples=False, **params):
        """(accum[n,4], {extension_rays, shadow_rays, shaded_vertices, samples}[, per-sample values float32[n, spp, 4]]); params: fields
        of gsp_render_params."""
        abi = self.emu.abi
        p = abi.default_render_params()
        p.spp, p.first_timestamp = spp, first_timestamp
        for k, v in params.items():
            setattr(p, k, v)
        n = width * height
        accum = np.zeros((n, 4), np.float32) if accum is None else np.ascontiguousarray(accum, np.float32).copy()
        counts = np.zeros(4, np.uint64)
        per = np.zeros((n, spp, 4), np.float32)
        arr, sarr, darr = abi.media_array(media), abi.media_scatter_array(scatter), abi.delta_light_array(delta)
        lt = np.ascontiguousarray(self.sc.lights, abi.LIGHT_DT)
        rc = self.emu.L.delta_emu_render(self.h, width, height, None, n, C.byref(p), estimator, light_mode, lt.ctypes.data if len(lt) else None, darr,
                                         len(darr) if darr is not None else 0, arr, sarr, len(arr) if arr is not None else 0, accum.ctypes.data,
                                         counts.ctypes.data, per.ctypes.data if samples else None, 1 if narrow else 0)
        if rc != 0:
            raise ValueError("delta_emu_render returned %d" % rc)
        st = dict(extension_rays=int(counts[0]), shadow_rays=int(counts[1]), shaded_vertices=int(counts[2]), samples=int(counts[3]))
        return (accum, st, per) if samples else (accum, st)

    def __del__(self):
        try:
            self.emu.L.emu_destroy(self.h)
        except Exception:
            pass


# ---- the device functions: one calling protocol for the host compile (DeltaEmu) and the device harness (DeltaDevice) ----------
def records(lights):
    """[abi.DeltaLight, ...] -> float32[n, 16], the records as words"""
    from gpuspectral_amd import abi

    arr = abi.delta_light_array(lights)
    return np.frombuffer(bytes(arr), np.float32).reshape(len(arr), 16).copy()


def _call(fn, n, arrays, out):
    rc = fn(n, *[a.ctypes.data for a in arrays], out.ctypes.data)
    if rc not in (0, None):
        raise RuntimeError("pt_deltalight.h harness returned %d" % rc)
    return out


def _spot_falloff(fn, c, cos_cutoff, cos_beam):
    a = [np.ascontiguousarray(x, np.float32) for x in (c, cos_cutoff, cos_beam)]
    assert len(a[0]) == len(a[1]) == len(a[2])
    return _call(fn, len(a[0]), a, np.zeros(len(a[0]), np.float32))


def _sample_delta_light(fn, recs, pos, pmf):
    """recs float32[n,16] -> float32[n, 8]: L, Ldist, emission, pdf"""
    a = [np.ascontiguousarray(x, np.float32) for x in (recs, pos, pmf)]
    n = len(a[2])
    assert a[0].shape == (n, 16) and a[1].shape == (n, 3)
    return _call(fn, n, a, np.zeros((n, 8), np.float32))


DEVFN_DIR = os.path.join(ROOT, "tests", "devfn")
DEVFN_LIB = os.path.join(DEVFN_DIR, "libdelta_devfn.so")
_CSRC = os.path.join(ROOT, "gpuspectral_amd", "csrc")
# (the order of tests/devfn/delta.mk)
DEVFN_DIGEST_SOURCES = tuple(os.path.join(DEVFN_DIR, f) for f in ("delta_devfn.hip", "delta_bodies.h", "devfn_bodies.h")) + tuple(
    os.path.join(_CSRC, f) for f in ("pt_deltalight.h", "pt_medium.h", "pt_math.h", "pt_shading.h", "pt_trace.h", "pt_stages.h")) + (
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
        raise RuntimeError("%s is missing or stale and hipcc is not on the path: build it with `make -C tests/devfn -f delta.mk` (build() does)" % DEVFN_LIB)
    subprocess.check_call(["make", "-B", "-C", DEVFN_DIR, "-f", "delta.mk"])
    if devfn_stamped_digest() != devfn_source_digest():
        raise RuntimeError("make -C tests/devfn -f delta.mk left a library without the digest of the tree's sources")
    return DEVFN_LIB


class DeltaDevice:
    """tests/devfn/libdelta_devfn.so: the bodies of delta_bodies.h on the GPU, one thread per vector."""

    def __init__(self):
        self.L = C.CDLL(devfn_ensure_built())
        vp, u64 = C.c_void_p, C.c_uint64
        self.L.delta_devfn_spot_falloff.argtypes = [u64, vp, vp, vp, vp]
        self.L.delta_devfn_sample_delta_light.argtypes = [u64, vp, vp, vp, vp]

    def spot_falloff(self, c, cos_cutoff, cos_beam):
        return _spot_falloff(self.L.delta_devfn_spot_falloff, c, cos_cutoff, cos_beam)

    def sample_delta_light(self, recs, pos, pmf):
        return _sample_delta_light(self.L.delta_devfn_sample_delta_light, recs, pos, pmf)


# ---- the vectors of the device-function tests (CPU and GPU share them) ---------------------------------------------------------------
def falloff_vectors(n=20000, seed=5):
    """(c, cos_cutoff, cos_beam): random cones and cosines, with c exactly at cos_cutoff and at cos_beam, just beside both, and at +-1."""
    rng = np.random.RandomState(seed)
    cc = rng.uniform(-0.9, 0.95, n).astype(np.float32)
    cb = np.minimum(cc + rng.uniform(1e-3, 0.5, n).astype(np.float32), np.float32(1.0))
    cb = np.where(cb > cc, cb, np.nextafter(cc, np.float32(2.0))).astype(np.float32)
    c = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    k = n // 8
    c[:k] = cc[:k]
    c[k:2 * k] = cb[k:2 * k]
    c[2 * k:3 * k] = np.nextafter(cc[2 * k:3 * k], np.float32(2.0))
    c[3 * k:4 * k] = np.nextafter(cb[3 * k:4 * k], np.float32(-2.0))
    c[4 * k:4 * k + 2] = np.float32([1.0, -1.0])
    return c, cc, cb


def sample_vectors(n=20000, seed=9):
    """(records float32[n,16] as accepted, pos, pmf): all three kinds; with pos == position, a grazing L (the shading point almost in the
    spot's cutoff plane and far off-axis), huge and tiny distances, cosines exactly at cos_beam and cos_cutoff (a point on the axis
    with cos_beam = 1)."""
    from gpuspectral_amd import abi

    rng = np.random.RandomState(seed)
    lights = []
    pos = rng.uniform(-3.0, 3.0, (n, 3)).astype(np.float32)
    pmf = rng.uniform(0.01, 1.0, n).astype(np.float32)
    for i in range(n):
        d = rng.normal(size=3)
        d = (d / np.linalg.norm(d)).astype(np.float32)
        p = rng.uniform(-3.0, 3.0, 3).astype(np.float32)
        inten = rng.uniform(0.0, 50.0, 3).astype(np.float32)
        kind = i % 3
        if kind == 0:
            lights.append(abi.point_light(p, inten))
        elif kind == 1:
            cc = np.float32(rng.uniform(-0.5, 0.9))
            cb = np.float32(min(1.0, cc + rng.uniform(0.01, 0.5)))
            lights.append(abi.spot_light(p, d, inten, cc, cb))
        else:
            lights.append(abi.directional_light(d, inten, float(rng.uniform(0.1, 100.0))))
    rec = records(lights)
    k = n // 10
    pos[:k] = rec[:k, 0:3]                                    # pos == position: d2 == 0
    pos[k:2 * k] = rec[k:2 * k, 0:3] + np.float32(1e-22)      # tiny distances: d2 underflows to 0 or a denormal
    pos[2 * k:3 * k] = rec[2 * k:3 * k, 0:3] + np.float32(1e-12)
    pos[3 * k:4 * k] = rec[3 * k:4 * k, 0:3] + np.float32(3e19) * np.sign(rng.normal(size=(k, 3))).astype(np.float32)  # huge: d2 overflows
    pos[4 * k:5 * k] = rec[4 * k:5 * k, 0:3] + np.float32(1e15)
    for i in range(5 * k, 6 * k):  # on the axis of a spot: c == 1 (== cos_beam where that is 1), and exactly on a cone of cosine cos_cutoff = 0
        if int(rec[i, 3:4].view(np.uint32)[0]) == abi.LIGHT_SPOT:
            rec[i, 4:7] = np.float32([0.0, 0.0, -1.0])
            if i % 2:
                rec[i, 11] = 1.0  # cos_beam
                pos[i] = rec[i, 0:3] + np.float32([0.0, 0.0, -2.0])
            else:
                rec[i, 7] = 0.0   # cos_cutoff, c == 0 exactly: the point in the plane of the light
                rec[i, 11] = max(rec[i, 11], np.float32(0.25))
                pos[i] = rec[i, 0:3] + np.float32([3.0, -4.0, 0.0])
    for i in range(6 * k, 7 * k):  # grazing: far off-axis, a hair's breadth below the light's plane
        if int(rec[i, 3:4].view(np.uint32)[0]) == abi.LIGHT_SPOT:
            rec[i, 4:7] = np.float32([0.0, 0.0, -1.0])
            pos[i] = rec[i, 0:3] + np.float32([100.0, 50.0, -1e-4])
    return rec, pos, pmf


# ---- the header's formulas in float64 -------------------------------------------------------------------------------------------
def smoothstep_ref(c, cos_cutoff, cos_beam):
    c, cc, cb = (np.asarray(x, np.float64) for x in (c, cos_cutoff, cos_beam))
    t = np.clip((c - cc) / (cb - cc), 0.0, 1.0)
    return t * t * (3.0 - 2.0 * t), t


def luminance(rgb):
    r = np.asarray(rgb, np.float64)
    return max(0.2126 * r[0] + 0.7152 * r[1] + 0.0722 * r[2], 0.0)


def pick_weight_ref(light):
    """The power-pick weight of an accepted record, float64"""
    from gpuspectral_amd import abi

    y = luminance(list(light.intensity))
    if light.kind == abi.LIGHT_POINT:
        return 4.0 * math.pi * y
    if light.kind == abi.LIGHT_SPOT:
        return 2.0 * math.pi * (1.0 - (float(light.cos_beam) + float(light.cos_cutoff)) / 2.0) * y
    return math.pi * float(light.extent) ** 2 * y


def triangle_weight_ref(lt):
    """Y(radiance) * area of abi.LIGHT_DT records, float64[n]"""
    p = lt["positions"][:, :, :3].astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(p[:, 2] - p[:, 0], p[:, 1] - p[:, 0]), axis=1)
    r = lt["radiance"].astype(np.float64)
    return np.maximum(0.2126 * r[:, 0] + 0.7152 * r[:, 1] + 0.0722 * r[:, 2], 0.0) * area


def pick_pmf(table):
    """The probability of every light under the integer alias table (abi.LIGHT_PICK_DT), float64[n]"""
    n = len(table)
    T = np.where(table["threshold"] == 0xFFFFFFFF, 2.0 ** 32, table["threshold"].astype(np.float64))
    mass = T.copy()
    for j in range(n):
        if table["alias"][j] != j:
            mass[table["alias"][j]] += 2.0 ** 32 - T[j]
    return mass / (n * 2.0 ** 32)


# ---- the closed-form scenes: one diffuse plane seen from above ------------------------------------------------------------------------
PLANE_W, PLANE_H = 48, 36
PLANE_EYE = (0.0, 0.0, 4.0)
PLANE_FOV_DEG = 40.0
PLANE_HALF = 2.5  # half extent of the quad in z = 0: it fills the frame (4 tan(20 deg) = 1.46 at the plane)
ALBEDO = (0.8, 0.5, 0.3)
PLANE_PARAMS = dict(max_depth=50, rr_start_depth=250, clamp=1e30)  # roulette off, no firefly cut-off


def plane_scene(occluder=None, far_occluder=None):
    """A two-sided diffuse quad in z = 0 (normal +z) that fills the frame of a camera looking down -z from PLANE_EYE, nothing else, black
    background.  occluder = (centre, half extent): a black two-sided quad parallel to the plane; far_occluder likewise (a second one)."""
    from gpuspectral_amd import scenes

    b = scenes.SceneBuilder()
    rect = b.add_mesh(*scenes.rect_mesh())
    b.add_object(rect, scenes.trs((0, 0, 0), PLANE_HALF), b.diffuse(ALBEDO))
    for occ in (occluder, far_occluder):
        if occ is not None:
            centre, half = occ
            b.add_object(rect, scenes.trs(centre, half), b.diffuse((0, 0, 0)))
    b.camera_lookat(PLANE_EYE, (0, 0, 0), fov_deg=PLANE_FOV_DEG)
    return b.build()


def plane_points(sc, width=PLANE_W, height=PLANE_H, dx=0.0, dy=0.0):
    """float64[h*w, 3]: where the pinhole ray of fragCoord (px + dx, py + dy) meets z = 0 (the header's ray: dl = normalize(-x, y, zplane),
    d = M dl with d.y negated)"""
    fov = float(sc.fov)
    zplane = (max(width, height) / 2.0) / math.tan(fov / 2.0)
    M = np.asarray(sc.to_world, np.float64).reshape(4, 4).T  # M[r, c]
    y, x = np.meshgrid(np.arange(height, dtype=np.float64) + dy, np.arange(width, dtype=np.float64) + dx, indexing="ij")
    v = np.stack([-(x.ravel() - width / 2.0), y.ravel() - height / 2.0, np.full(width * height, zplane)], 1)
    v /= np.linalg.norm(v, axis=1)[:, None]
    d = v @ M[:3, :3].T
    d[:, 1] *= -1.0
    o = M[:3, 3]
    t = -o[2] / d[:, 2]
    return o[None, :] + d * t[:, None]


def albedo_over_pi():
    """the resident diffuse record: float32(reflectance) / float32(pi), one float32 division (bake_diffuse)"""
    return (np.float32(ALBEDO) / np.float32(math.pi)).astype(np.float64)


def point_radiance(P, position, intensity):
    """(albedo / pi) I cos / d^2 at the plane points P (normal +z), float64[n, 3]"""
    toL = np.asarray(position, np.float64)[None, :] - P
    d2 = (toL * toL).sum(1)
    cos = np.abs(toL[:, 2]) / np.sqrt(d2)
    return albedo_over_pi()[None, :] * np.asarray(intensity, np.float64)[None, :] * (cos / d2)[:, None]


def spot_cosine(P, position, direction):
    """c = dot(direction, -L) at the plane points, float64"""
    toL = np.asarray(position, np.float64)[None, :] - P
    L = toL / np.linalg.norm(toL, axis=1)[:, None]
    d = np.asarray(direction, np.float64)
    return -(L @ (d / np.linalg.norm(d)))


# The bound of the closed form, relative, operation by operation (EPS = one correctly rounded float32 operation):
#   the shading point: the camera direction (normalize: 3 products, 2 sums, sqrt, division = 7; the matrix: 5; one negation), the hit
#   distance t of the traversal (the ray-triangle test on coordinates <= |eye| + half extent: fewer than 16 operations) and
#   position = o + d * t (2) -- fewer than 32 roundings on magnitudes <= 8 (the eye's distance + the quad's extent): |dP| <= 32 * 8 * EPS.
#   The value is (albedo / pi) I h / d^3 for a light at height h and distance d: a displacement dP changes it by at most
#   (3 / d + 1 / h) |dP| relative.
#   the vertex: toL (1), d2 (5), Ldist (1), L (1), NoL = |dot(SN, L)| with the interpolated, normalised SN (12 + 5), the diffuse BSDF's value
#   (the baked record is part of the reference value; its frame change and cosine test do not enter f), (NoL * f) * weight * emission /
#   lightPdf (5), lightPdf = d2 * pmf (1), the running mean of one sample (0): fewer than 40 roundings.
def closed_form_bound(dist_min, height):
    dP = 32 * 8 * EPS
    return (3.0 / dist_min + 1.0 / height) * dP + 40 * EPS


def away_from(mask_a, mask_b, width=PLANE_W, height=PLANE_H, pixels=2):
    """Pixels whose every neighbour within `pixels` in x and y has the same class (mask_a / mask_b / neither) as they have"""
    cls = (mask_a.astype(np.int8) + 2 * mask_b.astype(np.int8)).reshape(height, width)
    pad = np.pad(cls, pixels, mode="edge")  # (beyond the frame's border: the border pixel's class)
    ok = np.ones((height, width), bool)
    for oy in range(2 * pixels + 1):
        for ox in range(2 * pixels + 1):
            ok &= pad[oy:oy + height, ox:ox + width] == cls
    return ok.ravel()
