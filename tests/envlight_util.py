"""Shared by the environment-light tests (not a test module): the ctypes handle on tests/emu/libenvlight_emu.so -- the product's stage
headers with shade_vertex<.., ENV = true> and miss_emitted_env, compiled for the host (tests/emu/envlight_emu.cpp; a test harness,
never a product path) -- built the way DeltaEmu (delta_util.py) builds its library; the device harness of pt_envlight.h; the maps and
scenes of the tests; and the header's "Environment light" formulas restated in numpy / float64."""
import ctypes as C
import hashlib
import math
import os
import re
import shutil
import subprocess

import numpy as np

import delta_util as du
import media_util as mu
import textured
from conftest import ROOT

REFERENCE, TEXTBOOK = 0, 1
UNIFORM, POWER = 0, 1
same = mu.same
MAP_SIZES = ((1, 1), (2, 1), (16, 8), (13, 7), (1030, 3))  # (width, height); the last is wider than the cell cap


def sampling(extent):
    from gpuspectral_amd import abi

    return abi.EnvmapSampling(1, extent, (C.c_uint32 * 2)(0, 0))


class EnvEmu:
    def __init__(self):
        from gpuspectral_amd import abi

        d = os.path.join(ROOT, "tests", "emu")
        so = os.path.join(d, "libenvlight_emu.so")
        srcs = [os.path.join(d, f) for f in ("envlight_emu.cpp", "pt_emu.cpp")] + [os.path.join(ROOT, "include", "gpuspectral_pt.h")]
        csrc = os.path.join(ROOT, "gpuspectral_amd", "csrc")
        srcs += [os.path.join(csrc, h) for h in os.listdir(csrc) if h.endswith(".h")]
        srcs += [os.path.join(ROOT, "tests", "devfn", h) for h in ("devfn_bodies.h", "envlight_bodies.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mfma", "-mavx2", "-shared", "-o", so, srcs[0]])
        L = C.CDLL(so)
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        SP = C.POINTER(abi.EnvmapSampling)
        L.emu_create.restype = vp
        L.emu_create.argtypes = [C.POINTER(abi.SceneDesc)]
        L.emu_destroy.argtypes = [vp]
        L.envlight_emu_check.argtypes = [SP, C.c_char_p, u32]
        L.envlight_emu_is_rotation.argtypes = [vp]
        L.envlight_emu_cells.argtypes = [vp, u32, u32, vp, vp, vp]
        L.envlight_emu_cells.restype = None
        L.envlight_emu_power_weight.argtypes = [vp, u32, u32, C.c_float]
        L.envlight_emu_power_weight.restype = C.c_double
        L.envlight_emu_record.argtypes = [vp, u32, u32, C.c_float, vp]
        L.envlight_emu_record.restype = None
        L.envlight_emu_light_pick.argtypes = [vp, u32, C.POINTER(abi.DeltaLight), u32, C.c_double, vp]
        L.envlight_emu_light_pick.restype = None
        L.envlight_emu_env_eval.argtypes = [u64, vp, u32, u32, vp, vp, vp, vp, vp]
        L.envlight_emu_sample_env_light.argtypes = [u64, vp, u32, u32, vp, vp, vp, vp, vp]
        L.envlight_emu_render.argtypes = [vp, u32, u32, C.POINTER(abi.RenderParams), u32, u32, vp, C.POINTER(abi.DeltaLight), u32, C.POINTER(abi.Medium),
                                          C.POINTER(abi.MediumScatter), u32, SP, vp, vp]
        self.L, self.abi = L, abi

    def check(self, enabled, extent, reserved=(0, 0)):
        """gsp_set_envmap_sampling's own validation: None, or the error text"""
        s = self.abi.EnvmapSampling(enabled, extent, (C.c_uint32 * 2)(*reserved))
        err = C.create_string_buffer(256)
        return err.value.decode() if self.L.envlight_emu_check(C.byref(s), err, 256) else None

    def is_rotation(self, to_local):
        m = np.ascontiguousarray(to_local, np.float32)
        return bool(self.L.envlight_emu_is_rotation(m.ctypes.data))

    def cells(self, env):
        """env float32[h, w, 4] -> (cw, ch, the cell table abi.LIGHT_PICK_DT[cw * ch], the weights float64[cw * ch])"""
        env = np.ascontiguousarray(env, np.float32)
        h, w = env.shape[:2]
        dims = np.zeros(2, np.uint32)
        self.L.envlight_emu_cells(env.ctypes.data, w, h, dims.ctypes.data, None, None)
        n = int(dims[0]) * int(dims[1])
        table, weights = np.zeros(n, self.abi.LIGHT_PICK_DT), np.zeros(n, np.float64)
        self.L.envlight_emu_cells(env.ctypes.data, w, h, dims.ctypes.data, table.ctypes.data, weights.ctypes.data)
        return int(dims[0]), int(dims[1]), table, weights

    def power_weight(self, env, extent):
        env = np.ascontiguousarray(env, np.float32)
        return float(self.L.envlight_emu_power_weight(env.ctypes.data, env.shape[1], env.shape[0], extent))

    def record(self, to_local, cw, ch, p_sel=1.0):
        m = np.ascontiguousarray(to_local, np.float32)
        rec = np.zeros(16, np.float32)
        self.L.envlight_emu_record(m.ctypes.data, cw, ch, p_sel, rec.ctypes.data)
        return rec

    def light_pick(self, tri_lights, delta, env_w):
        lt = np.ascontiguousarray(tri_lights, self.abi.LIGHT_DT)
        arr = self.abi.delta_light_array(delta)
        nd = len(arr) if arr is not None else 0
        out = np.zeros(len(lt) + nd + 1, self.abi.LIGHT_PICK_DT)
        self.L.envlight_emu_light_pick(lt.ctypes.data if len(lt) else None, len(lt), arr, nd, env_w, out.ctypes.data)
        return out

    def env_eval(self, env, to_local, table, rec, dirs):
        return _env_eval(self.L.envlight_emu_env_eval, env, to_local, table, rec, dirs)

    def sample_envmap(self, env, to_local, dirs):
        """The escape's own lookup (sample_envmap, pt_shading.h) on the host: float32[n, 3]"""
        env, m, d = np.ascontiguousarray(env, np.float32), np.ascontiguousarray(to_local, np.float32), np.ascontiguousarray(dirs, np.float32)
        out = np.zeros((len(d), 3), np.float32)
        fn = self.L.emu_devfn_envmap
        fn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        assert fn(env.ctypes.data, env.shape[1], env.shape[0], m.ctypes.data, d.ctypes.data, len(d), out.ctypes.data) == 0
        return out

    def sample_env_light(self, env, to_local, table, rec, draws):
        return _sample_env_light(self.L.envlight_emu_sample_env_light, env, to_local, table, rec, draws)

    def scene(self, sc):
        return EnvEmuScene(self, sc)


class EnvEmuScene:
    def __init__(self, emu, sc):
        self.emu, self.sc = emu, sc
        self._desc = sc.desc()
        self.h = emu.L.emu_create(C.byref(self._desc))

    def render(self, width, height, spp, env=None, delta=None, media=None, scatter=None, first_timestamp=0, accum=None, estimator=TEXTBOOK,
               light_mode=UNIFORM, **params):
        """(accum[n, 4], {extension_rays, shadow_rays, shaded_vertices, samples}); env = the extent of gsp_envmap_sampling, None = the
        switch off; params: fields of gsp_render_params."""
        abi = self.emu.abi
        p = abi.default_render_params()
        p.spp, p.first_timestamp = spp, first_timestamp
        for k, v in params.items():
            setattr(p, k, v)
        n = width * height
        accum = np.zeros((n, 4), np.float32) if accum is None else np.ascontiguousarray(accum, np.float32).copy()
        counts = np.zeros(4, np.uint64)
        arr, sarr, darr = abi.media_array(media), abi.media_scatter_array(scatter), abi.delta_light_array(delta)
        lt = np.ascontiguousarray(self.sc.lights, abi.LIGHT_DT)
        s = sampling(env) if env is not None else None
        rc = self.emu.L.envlight_emu_render(self.h, width, height, C.byref(p), estimator, light_mode, lt.ctypes.data if len(lt) else None, darr,
                                            len(darr) if darr is not None else 0, arr, sarr, len(arr) if arr is not None else 0,
                                            C.byref(s) if s is not None else None, accum.ctypes.data, counts.ctypes.data)
        if rc != 0:
            raise ValueError("envlight_emu_render returned %d" % rc)
        return accum, dict(extension_rays=int(counts[0]), shadow_rays=int(counts[1]), shaded_vertices=int(counts[2]), samples=int(counts[3]))

    def __del__(self):
        try:
            self.emu.L.emu_destroy(self.h)
        except Exception:
            pass


# ---- the device functions: one calling protocol for the host compile (EnvEmu) and the device harness (EnvDevice) -----------------
def _shared(env, to_local, table, rec):
    from gpuspectral_amd import abi

    env = np.ascontiguousarray(env, np.float32)
    return env, np.ascontiguousarray(to_local, np.float32), np.ascontiguousarray(table, abi.LIGHT_PICK_DT), np.ascontiguousarray(rec, np.float32)


def _run(fn, env, to_local, table, rec, inp, out):
    env, m, table, rec = _shared(env, to_local, table, rec)
    assert rec.shape == (16,) and len(table) == int(rec[11:12].view(np.uint32)[0]) * int(rec[12:13].view(np.uint32)[0])
    rc = fn(len(inp), env.ctypes.data, env.shape[1], env.shape[0], m.ctypes.data, table.ctypes.data, rec.ctypes.data, inp.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise RuntimeError("pt_envlight.h harness returned %d" % rc)
    return out


def _env_eval(fn, env, to_local, table, rec, dirs):
    """dirs float32[n, 3] -> (radiance float32[n, 3], density float32[n], cell uint32[n])"""
    d = np.ascontiguousarray(dirs, np.float32)
    out = _run(fn, env, to_local, table, rec, d, np.zeros((len(d), 5), np.float32))
    return out[:, :3].copy(), out[:, 3].copy(), out[:, 4].copy().view(np.uint32)


def _sample_env_light(fn, env, to_local, table, rec, draws):
    """draws = (r2 uint32[n], e1, e2) -> (L float32[n, 3], emission float32[n, 3], pdf float32[n], cell picked uint32[n], cell of L uint32[n])"""
    r2, e1, e2 = draws
    d = np.stack([np.ascontiguousarray(r2, np.uint32).view(np.float32), np.float32(e1), np.float32(e2)], 1).astype(np.float32, copy=False)
    d = np.ascontiguousarray(d)
    out = _run(fn, env, to_local, table, rec, d, np.zeros((len(d), 9), np.float32))
    return out[:, :3].copy(), out[:, 3:6].copy(), out[:, 6].copy(), out[:, 7].copy().view(np.uint32), out[:, 8].copy().view(np.uint32)


DEVFN_DIR = os.path.join(ROOT, "tests", "devfn")
DEVFN_LIB = os.path.join(DEVFN_DIR, "libenvlight_devfn.so")
_CSRC = os.path.join(ROOT, "gpuspectral_amd", "csrc")
# (the order of tests/devfn/envlight.mk)
DEVFN_DIGEST_SOURCES = tuple(os.path.join(DEVFN_DIR, f) for f in ("envlight_devfn.hip", "envlight_bodies.h", "devfn_bodies.h")) + tuple(
    os.path.join(_CSRC, f) for f in ("pt_envlight.h", "pt_deltalight.h", "pt_medium.h", "pt_math.h", "pt_shading.h", "pt_trace.h", "pt_stages.h")) + (
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
        raise RuntimeError("%s is missing or stale and hipcc is not on the path: build it with `make -C tests/devfn -f envlight.mk` (build() does)" % DEVFN_LIB)
    subprocess.check_call(["make", "-B", "-C", DEVFN_DIR, "-f", "envlight.mk"])
    if devfn_stamped_digest() != devfn_source_digest():
        raise RuntimeError("make -C tests/devfn -f envlight.mk left a library without the digest of the tree's sources")
    return DEVFN_LIB


class EnvDevice:
    """tests/devfn/libenvlight_devfn.so: the bodies of envlight_bodies.h on the GPU, one thread per vector."""

    def __init__(self):
        self.L = C.CDLL(devfn_ensure_built())
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        self.L.envlight_devfn_env_eval.argtypes = [u64, vp, u32, u32, vp, vp, vp, vp, vp]
        self.L.envlight_devfn_sample_env_light.argtypes = [u64, vp, u32, u32, vp, vp, vp, vp, vp]

    def env_eval(self, env, to_local, table, rec, dirs):
        return _env_eval(self.L.envlight_devfn_env_eval, env, to_local, table, rec, dirs)

    def sample_env_light(self, env, to_local, table, rec, draws):
        return _sample_env_light(self.L.envlight_devfn_sample_env_light, env, to_local, table, rec, draws)


# ---- maps ------------------------------------------------------------------------------------------------------------------------
TO_LOCAL = textured.rotation(25.0, -35.0)  # a frame that is a rotation and not the identity


def random_map(width, height, seed=3):
    """float32[h, w, 4]: a random sky with one texel far brighter than the rest"""
    rng = np.random.RandomState(seed + 7 * width + height)
    env = rng.uniform(0.0, 1.5, (height, width, 4)).astype(np.float32)
    env[rng.randint(0, height), rng.randint(0, width), :3] = 60.0
    return env


def rot3(to_local):
    """the upper 3x3 A of a to_local in glm memory order: e = A d"""
    return np.asarray(to_local, np.float64).reshape(4, 4).T[:3, :3]


def local_dirs(u, v):
    """the map-frame direction of (u, v), float64: the inverse of the header's mapping"""
    theta, phi = (1.0 - v) * math.pi, (u - 0.5) * 2.0 * math.pi
    return np.stack([np.sin(theta) * np.sin(phi), np.cos(theta), -np.sin(theta) * np.cos(phi)], -1)


def uv_of(e):
    """(u, v) of map-frame directions, float64: the header's mapping"""
    u = np.arctan2(e[..., 0], -e[..., 2]) / (2.0 * math.pi) + 0.5
    v = 1.0 - np.arctan2(np.hypot(e[..., 0], e[..., 2]), e[..., 1]) / math.pi
    return u, v


def lookup(env, u, v):
    """The bilinear lookup of sample_envmap restated in numpy / float64: wrap in u, clamp in v, texel centres at (i + 0.5) / n.  [..., 3]"""
    env = np.asarray(env, np.float64)
    h, w = env.shape[:2]
    x, y = u * w - 0.5, v * h - 0.5
    fx, fy = np.floor(x), np.floor(y)
    x0 = np.mod(fx.astype(np.int64), w)
    x1 = np.mod(x0 + 1, w)
    y0 = np.clip(fy.astype(np.int64), 0, h - 1)
    y1 = np.clip(fy.astype(np.int64) + 1, 0, h - 1)
    tx, ty = (x - fx)[..., None], (y - fy)[..., None]
    a = env[y0, x0, :3] * (1.0 - tx) + env[y0, x1, :3] * tx
    b = env[y1, x0, :3] * (1.0 - tx) + env[y1, x1, :3] * tx
    return a * (1.0 - ty) + b * ty


def density_ref(table, cw, ch, u, v):
    """pmf(cell of (u, v)) * cw * ch / (2 pi^2 sin theta), float64, with sin theta from v"""
    ci = np.clip(np.floor(u * cw), 0, cw - 1).astype(np.int64)
    cj = np.clip(np.floor(v * ch), 0, ch - 1).astype(np.int64)
    pmf = du.pick_pmf(table)[cj * cw + ci]
    return pmf * cw * ch / (2.0 * math.pi ** 2 * np.sin((1.0 - v) * math.pi))


# ---- the scene of the independent value: one diffuse plane under a dim sky with a sun ----------------------------------------------
SKY = (0.05, 0.07, 0.1)
SUN_GAIN = 250.0
SUN_TOWARDS = (0.35, 0.25, 0.9)  # world; the plane's normal is +z


def sun_map(width=16, height=8, to_local=TO_LOCAL, gain=SUN_GAIN):
    """float32[h, w, 4]: SKY everywhere, and the texel whose centre looks closest to SUN_TOWARDS `gain` times brighter"""
    env = np.zeros((height, width, 4), np.float32)
    env[:, :, :3] = np.float32(SKY)
    v, u = np.meshgrid((np.arange(height) + 0.5) / height, (np.arange(width) + 0.5) / width, indexing="ij")
    world = local_dirs(u, v) @ rot3(to_local)  # d = A^T e, row vectors
    t = np.asarray(SUN_TOWARDS, np.float64)
    k = np.argmax(world @ (t / np.linalg.norm(t)))
    env[k // width, k % width, :3] = np.float32(SKY) * np.float32(gain)
    return env


def under_the_sky(sc, env=None, to_local=TO_LOCAL):
    sc.env_texels = sun_map() if env is None else env
    sc.env_to_local = np.asarray(to_local, np.float32)
    return sc


def small_sun_map():
    """The sun of sun_map() with the same power in a sixteenth of the solid angle: a 64 x 32 map, one texel 16 * SUN_GAIN times the sky"""
    return sun_map(64, 32, gain=16.0 * SUN_GAIN)


def sky_plane(box=False):
    """delta_util's plane (z = 0, normal +z, albedo du.ALBEDO, fills the frame) under the sun map; box: a diffuse box standing on it,
    under the small sun"""
    from gpuspectral_amd import scenes

    if not box:
        return under_the_sky(du.plane_scene())
    b = scenes.SceneBuilder()
    rect = b.add_mesh(*scenes.rect_mesh())
    cube = b.add_mesh(*scenes.box_mesh())
    b.add_object(rect, scenes.trs((0, 0, 0), du.PLANE_HALF), b.diffuse(du.ALBEDO))
    b.add_object(cube, scenes.trs((-0.2, 0.1, 0.35), 0.35), b.diffuse((0.6, 0.6, 0.6)))
    b.camera_lookat(du.PLANE_EYE, (0, 0, 0), fov_deg=du.PLANE_FOV_DEG)
    return under_the_sky(b.build(), small_sun_map())


def plane_irradiance_value(env, to_local=TO_LOCAL, nu=4096, nv=2048):
    """(albedo / pi) * integral over the hemisphere about +z of L cos(theta) d(omega), float64[3], by the midpoint rule over (u, v) --
    and the step of that rule.  The integrand is the bilinear map (piecewise bilinear, Lipschitz) times max(d.z, 0) sin(theta)."""
    v, u = np.meshgrid((np.arange(nv) + 0.5) / nv, (np.arange(nu) + 0.5) / nu, indexing="ij")
    world = local_dirs(u, v) @ rot3(to_local)
    cosz = np.maximum(world[..., 2], 0.0)
    d_omega = np.sin((1.0 - v) * math.pi) * (2.0 * math.pi / nu) * (math.pi / nv)
    E = (lookup(env, u, v) * (cosz * d_omega)[..., None]).sum((0, 1))
    return du.albedo_over_pi() * E
