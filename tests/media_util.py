"""Shared by the interior-media tests (not a test module): the ctypes handle on tests/emu/libmedia_emu.so -- the product's stage
headers with shade_vertex<.., MED = true>, compiled for the host (tests/emu/media_emu.cpp; a test harness, never a product path) --
built the way LensEmu (lens_util.py) builds its library; the scenes of the tests; and the header's "Interior media" semantics
restated in numpy / float64."""
import copy
import ctypes as C
import math
import os
import subprocess

import numpy as np

from conftest import ROOT

SLAB_SIGMA = (0.5, 2.0, 4.0)
SLAB_EMISSION = (2.0, 3.0, 4.0)
SLAB_HALF = (0.5, 0.5, 0.25)  # half extents of the box: 0.5 thick along z
SLAB_EYE_Z = 5.0
SLAB_FOV_DEG = 30.0


class MediaEmu:
    def __init__(self):
        from gpuspectral_amd import abi

        d = os.path.join(ROOT, "tests", "emu")
        so = os.path.join(d, "libmedia_emu.so")
        srcs = [os.path.join(d, f) for f in ("media_emu.cpp", "pt_emu.cpp")] + [os.path.join(ROOT, "include", "gpuspectral_pt.h")]
        csrc = os.path.join(ROOT, "gpuspectral_amd", "csrc")
        srcs += [os.path.join(csrc, h) for h in os.listdir(csrc) if h.endswith(".h")]
        dev = os.path.join(ROOT, "tests", "devfn", "devfn_bodies.h")
        if os.path.exists(dev):
            srcs.append(dev)
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mfma", "-mavx2", "-shared", "-o", so, srcs[0]])
        L = C.CDLL(so)
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        MP = C.POINTER(abi.Medium)
        L.emu_create.restype = vp
        L.emu_create.argtypes = [C.POINTER(abi.SceneDesc)]
        L.emu_destroy.argtypes = [vp]
        L.media_emu_check.argtypes = [MP, u32, C.c_char_p, u32]
        L.media_emu_max_number.argtypes = [vp]
        L.media_emu_max_number.restype = u32
        L.media_emu_render.argtypes = [vp, u32, u32, vp, u64, C.POINTER(abi.RenderParams), MP, u32, vp, vp, vp]
        self.L, self.abi = L, abi

    def check(self, sigmas, count=None):
        """gsp_set_media's validation of the table: None, or the error text."""
        arr = self.abi.media_array(sigmas)
        err = C.create_string_buffer(256)
        rc = self.L.media_emu_check(arr, (len(arr) if arr is not None else 0) if count is None else count, err, 256)
        return err.value.decode() if rc else None

    def scene(self, sc):
        return MediaEmuScene(self, sc)


class MediaEmuScene:
    def __init__(self, emu, sc):
        self.emu, self.sc = emu, sc
        self._desc = sc.desc()
        self.h = emu.L.emu_create(C.byref(self._desc))

    def render(self, width, height, spp, media=None, first_timestamp=0, log=False, accum=None, **params):
        """(accum[n,4], {extension_rays, shadow_rays, shaded_vertices}[, back-face log: one byte per pixel]); params: fields of
        gsp_render_params (max_depth, rr_start_depth, clamp, ...)."""
        p = self.emu.abi.default_render_params()
        p.spp, p.first_timestamp = spp, first_timestamp
        for k, v in params.items():
            setattr(p, k, v)
        n = width * height
        accum = np.zeros((n, 4), np.float32) if accum is None else np.ascontiguousarray(accum, np.float32).copy()
        counts = np.zeros(3, np.uint64)
        back = np.zeros(n, np.uint8)
        arr = self.emu.abi.media_array(media)
        rc = self.emu.L.media_emu_render(self.h, width, height, None, n, C.byref(p), arr, len(arr) if arr is not None else 0, accum.ctypes.data,
                                         counts.ctypes.data, back.ctypes.data if log else None)
        if rc != 0:
            raise ValueError("media_emu_render: BSDF handle out of range (a medium number above the count)")
        st = dict(extension_rays=int(counts[0]), shadow_rays=int(counts[1]), shaded_vertices=int(counts[2]))
        return (accum, st, back) if log else (accum, st)

    def __del__(self):
        try:
            self.emu.L.emu_destroy(self.h)
        except Exception:
            pass


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def with_medium(sc, instances, number):
    """A copy of the scene whose `instances` (indices) carry medium `number` in bits 19..30 of their handle."""
    out = copy.copy(sc)
    out.instances = sc.instances.copy()
    for i in np.atleast_1d(instances):
        out.instances["bsdf"][i] = (int(out.instances["bsdf"][i]) & 0x8007FFFF) | ((int(number) & 0xFFF) << 19)
    return out


def glass_instances(sc):
    """Indices of the instances with a smooth dielectric."""
    from gpuspectral_amd import abi

    return np.flatnonzero(((sc.instances["bsdf"] >> 16) & 7) == abi.BSDF_SMOOTH_DIELECTRIC)


def slab_scene(medium=0, twofaced=False):
    """The analytic slab: an emitter rectangle at z = -2 (scale 3, not two-sided, facing the camera), an index-matched dielectric
    box of half extents SLAB_HALF at the origin, the camera at (0, 0, 5) looking down -z."""
    from gpuspectral_amd import scenes

    b = scenes.SceneBuilder()
    rect = b.add_mesh(*scenes.rect_mesh())
    box = b.add_mesh(*scenes.box_mesh())
    b.add_object(rect, scenes.trs((0, 0, -2), 3.0), b.diffuse((0, 0, 0)), twofaced=False, emission=SLAB_EMISSION)
    b.add_object(box, scenes.trs((0, 0, 0), SLAB_HALF), b.dielectric(1.0, 1.0), twofaced=twofaced)
    b.camera_lookat((0, 0, SLAB_EYE_Z), (0, 0, 0), fov_deg=SLAB_FOV_DEG)
    sc = b.build()
    return with_medium(sc, [1], medium) if medium else sc


def slab_reference(width, height, sigma=SLAB_SIGMA, thickness=2.0 * SLAB_HALF[2]):
    """float64, from the pixel's ray direction alone (the header's pinhole ray: v = (-(x - W/2), y - H/2, zplane), camera looking
    down -z from (0, 0, SLAB_EYE_Z)).  -> (expected[h*w,3] for a ray that crosses the slab through both z faces, inside[h*w] = the
    ray does so, outside[h*w] = the ray misses the box; the rest are the silhouette-edge pixels).  A ray crosses through both z
    faces when its point on the far face lies inside the box's x / y extent (|x| and |y| grow along the ray, so the near point
    then does too); it misses the box when its point on the near face lies outside that extent in x or in y.  Both with a margin of
    1e-3 in x / y, so that no float32 rounding of the traced ray can change the class of a pixel that is not left out."""
    fov = float(np.float32(np.float64(np.float32(SLAB_FOV_DEG)) * math.pi / 180.0))
    zplane = (max(width, height) / 2.0) / math.tan(fov / 2.0)
    y, x = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    vx, vy = (x - width / 2.0).ravel(), (y - height / 2.0).ravel()  # (signs do not matter: box and camera are symmetric)
    cos = zplane / np.sqrt(vx * vx + vy * vy + zplane * zplane)
    expected = np.asarray(SLAB_EMISSION)[None, :] * np.exp(-np.asarray(sigma)[None, :] * (thickness / cos)[:, None])
    hx, hy, hz = SLAB_HALF
    margin = 1e-3
    def extent(zdist):  # |x|, |y| of the ray at this distance along the view axis
        return np.abs(vx) / zplane * zdist, np.abs(vy) / zplane * zdist
    nx_, ny_ = extent(SLAB_EYE_Z - hz)
    fx_, fy_ = extent(SLAB_EYE_Z + hz)
    inside = (fx_ < hx - margin) & (fy_ < hy - margin)  # (the far point is the wider one)
    outside = (nx_ > hx + margin) | (ny_ > hy + margin)  # (|x| grows along the ray: outside at the near face = outside all along)
    return expected, inside, outside
