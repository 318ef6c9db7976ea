"""Shared by the light-grid tests (not a test module): the ctypes handle on tests/emu/liblightgrid_emu.so -- the product's stage
headers with shade_vertex<.., GRD = true> and pt_lightgrid.h, compiled for the host (tests/emu/lightgrid_emu.cpp; a test harness,
never a product path) -- built the way EnvEmu (envlight_util.py) builds its library; the device harness of pt_lightgrid.h; the
scenes of the tests; and the header's "Light grid" rules restated in numpy / float64."""
import ctypes as C
import hashlib
import math
import os
import re
import shutil
import subprocess

import numpy as np

import lights_util as lu
from conftest import ROOT

REFERENCE, TEXTBOOK = 0, 1
UNIFORM, POWER = 0, 1
NO_CELL = 0xFFFFFFFF
MAX_ENTRIES = 1 << 20
same = lu.same
HEADER_DT = np.dtype([("lo", "<f4", 3), ("nx", "<u4"), ("inv_cell", "<f4", 3), ("ny", "<u4"), ("cell", "<f4", 3), ("nz", "<u4"), ("hi", "<f4", 3), ("half_diag", "<f4")])
assert HEADER_DT.itemsize == 64


class Grid:
    """A built grid: header, per-cell tables [cells, n] (abi.LIGHT_PICK_DT), tails float32[cells], weights float64[cells, n], the
    fallback table and its tail, and the raw image the device functions read."""

    def __init__(self, abi, header, image, n, fallback, fallback_tail, weights, build_ms):
        self.header, self.image, self.n, self.fallback, self.fallback_tail, self.build_ms = header, image, n, fallback, fallback_tail, build_ms
        self.res = (int(header["nx"]), int(header["ny"]), int(header["nz"]))
        self.cells = self.res[0] * self.res[1] * self.res[2]
        body = image[64:].view(abi.LIGHT_PICK_DT).reshape(self.cells, n + 1)
        self.tables = body[:, :n]
        self.tails = body[:, n].copy().view(np.float32).reshape(self.cells, 4)[:, 0]
        self.weights = weights.reshape(self.cells, n)

    def centre(self, ix, iy, iz):
        h = self.header
        return h["lo"].astype(np.float64) + (np.array([ix, iy, iz]) + 0.5) * h["cell"].astype(np.float64)

    def number(self, ix, iy, iz):
        return (iz * self.res[1] + iy) * self.res[0] + ix


class GridEmu:
    def __init__(self):
        from gpuspectral_amd import abi

        d = os.path.join(ROOT, "tests", "emu")
        so = os.path.join(d, "liblightgrid_emu.so")
        srcs = [os.path.join(d, f) for f in ("lightgrid_emu.cpp", "pt_emu.cpp")] + [os.path.join(ROOT, "include", "gpuspectral_pt.h")]
        csrc = os.path.join(ROOT, "gpuspectral_amd", "csrc")
        srcs += [os.path.join(csrc, h) for h in os.listdir(csrc) if h.endswith(".h")]
        srcs += [os.path.join(ROOT, "tests", "devfn", h) for h in ("devfn_bodies.h", "lightgrid_bodies.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mfma", "-mavx2", "-shared", "-o", so, srcs[0]])
        L = C.CDLL(so)
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        GP = C.POINTER(abi.LightGrid)
        L.emu_create.restype = vp
        L.emu_create.argtypes = [C.POINTER(abi.SceneDesc)]
        L.emu_destroy.argtypes = [vp]
        L.lightgrid_emu_check.argtypes = [GP, C.c_char_p, u32]
        L.lightgrid_emu_bounds.argtypes = [vp, vp]
        L.lightgrid_emu_resolve.argtypes = [GP, vp, u32, vp]
        L.lightgrid_emu_header.argtypes = [vp, vp, vp]
        L.lightgrid_emu_header.restype = None
        L.lightgrid_emu_build.argtypes = [vp, vp, u32, C.POINTER(abi.DeltaLight), u32, vp, vp, vp, vp]
        L.lightgrid_emu_build.restype = C.c_double
        L.lightgrid_emu_cell.argtypes = [u64, vp, vp, vp]
        L.lightgrid_emu_pick.argtypes = [u64, vp, vp, u32, vp, vp, vp]
        L.lightgrid_emu_hit_pmf.argtypes = [u64, vp, vp, u32, vp, vp, vp]
        L.lightgrid_emu_render.argtypes = [vp, u32, u32, C.POINTER(abi.RenderParams), u32, u32, vp, C.POINTER(abi.DeltaLight), u32, C.POINTER(abi.Medium),
                                           C.POINTER(abi.MediumScatter), u32, GP, vp, vp, vp, vp, vp]
        self.L, self.abi = L, abi

    def check(self, enabled, resolution=(0, 0, 0), reserved=(0, 0, 0, 0)):
        """gsp_set_light_grid's own validation: None, or the error text"""
        s = self.abi.LightGrid(enabled, (C.c_uint32 * 3)(*resolution), (C.c_uint32 * 4)(*reserved))
        err = C.create_string_buffer(256)
        return err.value.decode() if self.L.lightgrid_emu_check(C.byref(s), err, 256) else None

    def resolve(self, bounds, num_lights, resolution=None):
        """(nx, ny, nz) a grid over `bounds` (6 floats) is built with, or None when it is beyond the cap"""
        b = np.ascontiguousarray(bounds, np.float32).reshape(6)
        res = np.zeros(3, np.uint32)
        want = self.abi.light_grid(resolution)
        return None if self.L.lightgrid_emu_resolve(C.byref(want), b.ctypes.data, num_lights, res.ctypes.data) else tuple(int(x) for x in res)

    def header(self, bounds, res):
        b, r = np.ascontiguousarray(bounds, np.float32).reshape(6), np.ascontiguousarray(res, np.uint32)
        h = np.zeros(1, HEADER_DT)
        self.L.lightgrid_emu_header(b.ctypes.data, r.ctypes.data, h.ctypes.data)
        return h[0]

    def build(self, bounds, res, lights, delta=None):
        """The product's builder over UNBAKED light records (+ delta records) -> Grid"""
        abi = self.abi
        lt = np.ascontiguousarray(lights, abi.LIGHT_DT)
        darr = abi.delta_light_array(delta)
        nd = len(darr) if darr is not None else 0
        n = len(lt) + nd
        head = np.zeros(1, HEADER_DT)
        head[0] = self.header(bounds, res)
        cells = int(res[0]) * int(res[1]) * int(res[2])
        assert cells * n <= MAX_ENTRIES
        image = np.zeros(64 + cells * (n + 1) * 16, np.uint8)
        fallback, tail, weights = np.zeros(n, abi.LIGHT_PICK_DT), np.zeros(4, np.float32), np.zeros(cells * n, np.float64)
        ms = self.L.lightgrid_emu_build(head.ctypes.data, lt.ctypes.data if len(lt) else None, len(lt), darr, nd, fallback.ctypes.data, tail.ctypes.data,
                                        image.ctypes.data, weights.ctypes.data)
        return Grid(abi, head[0], image, n, fallback, tail, weights, ms)

    # the device functions on the host
    def cell(self, grid, pos):
        return _cell(lambda n, g, gb, p, o: self.L.lightgrid_emu_cell(n, g, p, o), grid, pos)

    def pick(self, grid, pos, r):
        return _pick(lambda n, g, gb, f, nl, p, rr, o: self.L.lightgrid_emu_pick(n, g, f, nl, p, rr, o), grid, pos, r)

    def hit_pmf(self, grid, pos, tris):
        return _hit_pmf(lambda n, g, gb, f, nl, p, t, o: self.L.lightgrid_emu_hit_pmf(n, g, f, nl, p, t, o), grid, pos, tris)

    def scene(self, sc):
        return GridEmuScene(self, sc)


class GridEmuScene:
    def __init__(self, emu, sc):
        self.emu, self.sc = emu, sc
        self._desc = sc.desc()
        self.h = emu.L.emu_create(C.byref(self._desc))

    def bounds(self):
        b = np.zeros(6, np.float32)
        assert self.emu.L.lightgrid_emu_bounds(self.h, b.ctypes.data) == 1
        return b

    def render(self, width, height, spp, grid=False, delta=None, media=None, scatter=None, first_timestamp=0, accum=None, estimator=TEXTBOOK, light_mode=POWER,
               lights=None, bounds=None, moments=False, **params):
        """(accum[n, 4], {extension_rays, shadow_rays, shaded_vertices, samples, resolution}[, moments[n, 6]]).  grid: False = the switch
        off, None / True = auto, or (nx, ny, nz).  lights: the light records the tables are built from (default: the scene's).  bounds:
        the bounds of the scene as uploaded when they are not this scene's own (an instance moved behind the upload).  params: fields of
        gsp_render_params."""
        abi = self.emu.abi
        p = abi.default_render_params()
        p.spp, p.first_timestamp = spp, first_timestamp
        for k, v in params.items():
            setattr(p, k, v)
        n = width * height
        accum = np.zeros((n, 4), np.float32) if accum is None else np.ascontiguousarray(accum, np.float32).copy()
        counts, res = np.zeros(4, np.uint64), np.zeros(3, np.uint32)
        mom = np.zeros((n, 6), np.float64) if moments else None
        arr, sarr, darr = abi.media_array(media), abi.media_scatter_array(scatter), abi.delta_light_array(delta)
        lt = np.ascontiguousarray(self.sc.lights if lights is None else lights, abi.LIGHT_DT)
        g = None if grid is False else abi.light_grid(None if grid in (None, True) else grid)
        b = None if bounds is None else np.ascontiguousarray(bounds, np.float32).reshape(6)
        rc = self.emu.L.lightgrid_emu_render(self.h, width, height, C.byref(p), estimator, light_mode, lt.ctypes.data if len(lt) else None, darr,
                                             len(darr) if darr is not None else 0, arr, sarr, len(arr) if arr is not None else 0,
                                             C.byref(g) if g is not None else None, None if b is None else b.ctypes.data, accum.ctypes.data, counts.ctypes.data,
                                             None if mom is None else mom.ctypes.data, res.ctypes.data)
        if rc != 0:
            raise ValueError("lightgrid_emu_render returned %d" % rc)
        st = dict(extension_rays=int(counts[0]), shadow_rays=int(counts[1]), shaded_vertices=int(counts[2]), samples=int(counts[3]),
                  resolution=tuple(int(x) for x in res))
        return (accum, st, mom) if moments else (accum, st)

    def __del__(self):
        try:
            self.emu.L.emu_destroy(self.h)
        except Exception:
            pass


# ---- the device functions: one calling protocol for the host compile (GridEmu) and the device harness (GridDevice) ----------------
def _check(rc):
    if rc != 0:
        raise RuntimeError("pt_lightgrid.h harness returned %d" % rc)


def _cell(fn, grid, pos):
    """pos float32[n, 3] -> (cell uint32[n], ixyz uint32[n, 3]; 0xffffffff = the fallback)"""
    p = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    out = np.zeros((len(p), 4), np.uint32)
    _check(fn(len(p), grid.image.ctypes.data, grid.image.size, p.ctypes.data, out.ctypes.data))
    return out[:, 0].copy(), out[:, 1:].copy()


def _fallback_with_tail(grid):
    f = np.zeros(grid.n + 1, grid.fallback.dtype)
    f[: grid.n] = grid.fallback
    f[grid.n :].view(np.float32)[:4] = grid.fallback_tail
    return f


def _pick(fn, grid, pos, r):
    """-> (light index uint32[n], pmf float32[n])"""
    p, r = np.ascontiguousarray(pos, np.float32).reshape(-1, 3), np.ascontiguousarray(r, np.uint32)
    assert len(p) == r.size
    f = _fallback_with_tail(grid)
    out = np.zeros((len(p), 2), np.uint32)
    _check(fn(len(p), grid.image.ctypes.data, grid.image.size, f.ctypes.data, grid.n, p.ctypes.data, r.ctypes.data, out.ctypes.data))
    return out[:, 0].copy(), out[:, 1].copy().view(np.float32)


def _hit_pmf(fn, grid, pos, tris):
    """tris float32[n, 12] = {v0, v1, v2, emission} -> p_sel float32[n]"""
    p, t = np.ascontiguousarray(pos, np.float32).reshape(-1, 3), np.ascontiguousarray(tris, np.float32).reshape(-1, 12)
    assert len(p) == len(t)
    f = _fallback_with_tail(grid)
    out = np.zeros(len(p), np.float32)
    _check(fn(len(p), grid.image.ctypes.data, grid.image.size, f.ctypes.data, grid.n, p.ctypes.data, t.ctypes.data, out.ctypes.data))
    return out


DEVFN_DIR = os.path.join(ROOT, "tests", "devfn")
DEVFN_LIB = os.path.join(DEVFN_DIR, "liblightgrid_devfn.so")
_CSRC = os.path.join(ROOT, "gpuspectral_amd", "csrc")
# (the order of tests/devfn/lightgrid.mk)
DEVFN_DIGEST_SOURCES = tuple(os.path.join(DEVFN_DIR, f) for f in ("lightgrid_devfn.hip", "lightgrid_bodies.h", "devfn_bodies.h")) + tuple(
    os.path.join(_CSRC, f) for f in ("pt_lightgrid.h", "pt_lightpick.h", "pt_envlight.h", "pt_deltalight.h", "pt_medium.h", "pt_math.h", "pt_shading.h", "pt_trace.h",
                                     "pt_stages.h")) + (os.path.join(ROOT, "include", "gpuspectral_pt.h"),)


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
        raise RuntimeError("%s is missing or stale and hipcc is not on the path: build it with `make -C tests/devfn -f lightgrid.mk` (build() does)" % DEVFN_LIB)
    subprocess.check_call(["make", "-B", "-C", DEVFN_DIR, "-f", "lightgrid.mk"])
    if devfn_stamped_digest() != devfn_source_digest():
        raise RuntimeError("make -C tests/devfn -f lightgrid.mk left a library without the digest of the tree's sources")
    return DEVFN_LIB


class GridDevice:
    """tests/devfn/liblightgrid_devfn.so: the bodies of lightgrid_bodies.h on the GPU, one thread per vector."""

    def __init__(self):
        self.L = C.CDLL(devfn_ensure_built())
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        self.L.lightgrid_devfn_cell.argtypes = [u64, vp, u64, vp, vp]
        self.L.lightgrid_devfn_pick.argtypes = [u64, vp, u64, vp, u32, vp, vp, vp]
        self.L.lightgrid_devfn_hit_pmf.argtypes = [u64, vp, u64, vp, u32, vp, vp, vp]

    def cell(self, grid, pos):
        return _cell(self.L.lightgrid_devfn_cell, grid, pos)

    def pick(self, grid, pos, r):
        return _pick(self.L.lightgrid_devfn_pick, grid, pos, r)

    def hit_pmf(self, grid, pos, tris):
        return _hit_pmf(self.L.lightgrid_devfn_hit_pmf, grid, pos, tris)


# ---- the header's rules in numpy / float64 ---------------------------------------------------------------------------------------
def luminance(c):
    c = np.asarray(c, np.float64)
    return np.maximum(0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2], 0.0)


def tri_weight64(header, centre, light):
    """The triangle weight of "Light grid" in float64 (the cull included, with the header's margin), for one light record."""
    v = light["positions"].astype(np.float64)[:, :3]
    cell = header["cell"].astype(np.float64)
    rcell = 0.5 * math.sqrt((cell * cell).sum())
    cen = v.mean(0)
    rtri = math.sqrt(((v - cen) ** 2).sum(1).max())
    n = np.cross(v[1] - v[0], v[2] - v[0])
    area = 0.5 * np.linalg.norm(n)
    d = np.asarray(centre, np.float64) - cen
    smax = n @ d + (np.abs(n) * 0.5 * cell).sum()
    S = np.abs(centre).sum() + np.abs(cen).sum() + rcell + rtri
    if smax < -1e-4 * S * np.linalg.norm(n):
        return 0.0
    R = rcell + rtri
    return float(luminance(light["radiance"][:3]) * area / max(d @ d, R * R))


def probe_positions(bounds, res, seed=5, random=2000):
    """Positions for the cell lookup: random points in and around the box, points on every cell face of the x axis, the box's own
    corners, points outside on each side, NaN and infinities."""
    lo, hi = np.asarray(bounds[:3], np.float64), np.asarray(bounds[3:], np.float64)
    rng = np.random.RandomState(seed)
    ext = np.maximum(hi - lo, 1.0)
    pts = [lo - 0.3 * ext + rng.uniform(0.0, 1.6, (random, 3)) * ext]
    mid = 0.5 * (lo + hi)
    faces = np.tile(mid, (res[0] + 1, 1))
    faces[:, 0] = lo[0] + (hi[0] - lo[0]) * np.arange(res[0] + 1) / res[0]
    pts.append(faces)
    pts.append(np.array([lo, hi, mid]))
    for c in range(3):
        for s in (-1.0, 1.0):
            q = mid.copy()
            q[c] = (lo[c] if s < 0 else hi[c]) + s * 0.01 * ext[c]
            pts.append(q[None])
    pts.append(np.array([[np.nan, mid[1], mid[2]], [mid[0], np.inf, mid[2]], [mid[0], mid[1], -np.inf], [np.nan, np.nan, np.nan]]))
    return np.concatenate(pts).astype(np.float32)


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def floor_under_lights(floor_centre=(0.0, 0.0), floor_half=8.0, eye=(0, 14, 10), fov_deg=30.0, height=10.0, equal=False, spacing=2.0, area=None):
    """A diffuse floor (y = 0, lu.FLOOR_RHO) under a 4 x 4 array of small down-facing triangle lights `spacing` apart at `height`:
    lu.expectation_scene's lights (areas 1e-4 .. 1e-1, luminances 100 .. 1) or, equal=True, sixteen equal ones of `area`.  The floor
    is an object of its own (instance 0), so a test can move it behind the upload."""
    from gpuspectral_amd import scenes

    b = scenes.SceneBuilder()
    h = floor_half
    tris = [[(-h, 0, -h), (-h, 0, h), (h, 0, h)], [(-h, 0, -h), (h, 0, h), (h, 0, -h)]]  # normal +y
    b.add_object(b.add_mesh(*lu.tri_mesh(tris)), scenes.trs((floor_centre[0], 0.0, floor_centre[1])), b.diffuse(lu.FLOOR_RHO), twofaced=False)
    black = b.diffuse((0, 0, 0))
    for i in range(16):
        a = area if equal else 1e-4 * 10.0 ** (3.0 * i / 15.0)
        le = (40.0 if equal else 100.0 * 10.0 ** (-2.0 * i / 15.0)) * np.array([1.0, 0.9, 0.7])
        tri = lu.down_triangle(spacing * (i % 4 - 1.5), spacing * (i // 4 - 1.5), height, a, 0.3 * i)
        b.add_object(b.add_mesh(*lu.tri_mesh([tri])), np.eye(4, dtype=np.float32).reshape(16), black, twofaced=False, emission=le)
    b.camera_lookat(eye, (0, 0, 0), up=(0, 1, 0) if eye[0] or eye[2] else (0, 0, -1), fov_deg=fov_deg)
    return b.build()


def moved(sc, instance, dx=0.0, dy=0.0, dz=0.0):
    """A copy of the scene with one instance translated (the scene a context holds after gsp_update_instances)."""
    import copy

    out = copy.copy(sc)
    out.instances = sc.instances.copy()
    out.instances["transform"][instance, 12:15] += np.array([dx, dy, dz], np.float32)
    return out


UNBIASED_SHIFT = 6.0


def unbiased_scene():
    """The floor under lu.expectation_scene's 16 lights, uploaded with the floor 6 to the left of where it is rendered: the box ends
    at the right-most light (x = 3 and a bit), and after moved(sc, 0, dx=6) the floor fills the view, whose right part (x > 3.2) lies
    outside the box: those pixels pick from the fallback table."""
    return floor_under_lights(floor_centre=(-UNBIASED_SHIFT, 0.0), floor_half=10.0, fov_deg=38.0)


HELP_RES = (16, 2, 16)


def help_scene():
    """16 equal small down-facing lights in a 4 x 4 array at spacing 8 and height 1 above the floor (half 16), the camera looking
    straight down from y = 30 (fov 68 degrees along the frame's longer side: a 48 x 32 frame sees x within 20, z within 13.5): the
    feet of the lights are at x, z in {-12, -4, 4, 12}."""
    return floor_under_lights(floor_half=16.0, eye=(0, 30, 0), fov_deg=68.0, height=1.0, equal=True, spacing=8.0, area=2e-3)


def floor_points64(sc, width, height):
    """The floor point (y = 0) of every pixel's pinhole ray, float64 [h * w, 3]"""
    import temporal_util as tu

    d = tu.pinhole_dirs64(sc.to_world, sc.fov, width, height).reshape(-1, 3)
    o = np.asarray(sc.to_world, np.float64)[12:15]
    return o[None, :] + (-o[1] / d[:, 1])[:, None] * d
