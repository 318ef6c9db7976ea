"""Shared by the estimator tests (not a test module): the ctypes handle on tests/emu/libestimator_emu.so -- the product's
shade_vertex<.., EST> and path loop compiled for the host (tests/emu/estimator_emu.cpp; a test harness, never a product path),
built the way LightsEmu (lights_util.py) builds its library; the oracle with its test-only mask oracle_set_quirks_off; the scenes
of the tests; and frame statistics."""
import contextlib
import ctypes as C
import math
import os
import subprocess

import numpy as np

from conftest import GOLDEN, ROOT

REFERENCE, TEXTBOOK = 0, 1
UNIFORM, POWER = 0, 1
# oracle/oracle_bsdf.h kQuirk*: NEE weight | emitter-hit weight | rough plastic's floor (4, the firefly cut-off, is a render parameter)
ORACLE_TEXTBOOK_MASK = 1 | 2 | 8


class EstimatorEmu:
    def __init__(self):
        from gpuspectral_amd import abi

        d = os.path.join(ROOT, "tests", "emu")
        so = os.path.join(d, "libestimator_emu.so")
        srcs = [os.path.join(d, f) for f in ("estimator_emu.cpp", "pt_emu.cpp")] + [os.path.join(ROOT, "include", "gpuspectral_pt.h")]
        csrc = os.path.join(ROOT, "gpuspectral_amd", "csrc")
        srcs += [os.path.join(csrc, h) for h in os.listdir(csrc) if h.endswith(".h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mfma", "-mavx2", "-shared", "-o", so, srcs[0]])
        L = C.CDLL(so)
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        L.emu_create.restype = vp
        L.emu_create.argtypes = [C.POINTER(abi.SceneDesc)]
        L.emu_destroy.argtypes = [vp]
        L.estimator_emu_psel.argtypes = [vp, u32, vp, vp]
        L.estimator_emu_psel.restype = None
        L.estimator_emu_hit_weight.argtypes = [C.c_float, C.c_float, vp, vp, C.c_float, C.c_float]
        L.estimator_emu_hit_weight.restype = C.c_float
        L.estimator_emu_light_image_bytes.argtypes = [u32, u32, u32]
        L.estimator_emu_light_image_bytes.restype = u64
        L.estimator_emu_render.argtypes = [vp, u32, u32, vp, u64, C.POINTER(abi.RenderParams), u32, u32, vp, C.POINTER(abi.Medium), u32, vp, vp, vp]
        self.L, self.abi = L, abi

    def psel(self, lights):
        """The product's p_sel of every light record hit as itself -> (p_sel float32[n], inv_sum_w)."""
        lights = np.ascontiguousarray(lights, self.abi.LIGHT_DT)
        out, inv = np.zeros(len(lights), np.float32), np.zeros(1, np.float32)
        self.L.estimator_emu_psel(lights.ctypes.data, len(lights), out.ctypes.data, inv.ctypes.data)
        return out, float(inv[0])

    def hit_weight(self, last_pdf, t, d, n, area, p_sel):
        d, n = np.ascontiguousarray(d, np.float32), np.ascontiguousarray(n, np.float32)
        return float(self.L.estimator_emu_hit_weight(last_pdf, t, d.ctypes.data, n.ctypes.data, area, p_sel))

    def light_image_bytes(self, n, light_mode, estimator):
        return int(self.L.estimator_emu_light_image_bytes(n, light_mode, estimator))

    def scene(self, sc):
        return EstimatorEmuScene(self, sc)


class EstimatorEmuScene:
    def __init__(self, emu, sc):
        self.emu, self.sc = emu, sc
        self._desc = sc.desc()
        self.h = emu.L.emu_create(C.byref(self._desc))

    def render(self, width, height, spp, estimator=REFERENCE, light_mode=UNIFORM, media=None, first_timestamp=0, accum=None, lights=None,
               pixel_ids=None, moments=False, **params):
        """-> (accum[n,4], stats dict: the three ray counts + the path log's emitter hits[, moments[n,6]]).
        lights: the light records the tables are built from (default: the scene's)."""
        abi = self.emu.abi
        p = abi.default_render_params()
        p.spp, p.first_timestamp = spp, first_timestamp
        for k, v in params.items():
            setattr(p, k, v)
        ids = None if pixel_ids is None else np.ascontiguousarray(pixel_ids, np.uint32)
        n = width * height if ids is None else len(ids)
        accum = np.zeros((n, 4), np.float32) if accum is None else np.ascontiguousarray(accum, np.float32).copy()
        counts = np.zeros(6, np.uint64)
        mom = np.zeros((n, 6), np.float64) if moments else None
        lt = np.ascontiguousarray(self.sc.lights if lights is None else lights, abi.LIGHT_DT)
        assert len(lt) == len(self.sc.lights)
        arr = abi.media_array(media)
        rc = self.emu.L.estimator_emu_render(self.h, width, height, None if ids is None else ids.ctypes.data, n, C.byref(p), estimator, light_mode,
                                             lt.ctypes.data, arr, len(arr) if arr is not None else 0, accum.ctypes.data, counts.ctypes.data,
                                             None if mom is None else mom.ctypes.data)
        if rc != 0:
            raise ValueError("estimator_emu_render returned %d" % rc)
        st = dict(extension_rays=int(counts[0]), shadow_rays=int(counts[1]), shaded_vertices=int(counts[2]), emitter_hits_after_occluded=int(counts[3]),
                  emitter_hits_after_clear=int(counts[4]), emitter_hits_after_delta=int(counts[5]))
        return (accum, st, mom) if moments else (accum, st)

    def __del__(self):
        try:
            self.emu.L.emu_destroy(self.h)
        except Exception:
            pass


# ---- the oracle under its mask ------------------------------------------------------------------------------------------------------
def _oracle_lib():
    from oracle import oracle as orc

    L = orc.lib()
    L.oracle_set_quirks_off.argtypes = [C.c_uint32]
    L.oracle_set_quirks_off.restype = None
    L.oracle_get_quirks_off.restype = C.c_uint32
    return L


@contextlib.contextmanager
def oracle_textbook():
    """The oracle's test-only mask set to the textbook estimator for the block; 0 again afterwards, whatever happens (process state)."""
    L = _oracle_lib()
    assert L.oracle_get_quirks_off() == 0
    L.oracle_set_quirks_off(ORACLE_TEXTBOOK_MASK)
    try:
        yield
    finally:
        L.oracle_set_quirks_off(0)
    assert L.oracle_get_quirks_off() == 0


def oracle_quirks_off():
    return int(_oracle_lib().oracle_get_quirks_off())


def oracle_textbook_render(sc, width, height, spp, first_timestamp=0, **params):
    """oracle_render with oracle_set_quirks_off(1 | 2 | 8) -> (accum[n,4], stats); the mask is 0 again on return."""
    from gpuspectral_amd import abi
    from oracle import oracle as orc

    p = abi.default_render_params(spp, first_timestamp)
    for k, v in params.items():
        setattr(p, k, v)
    o = orc.Oracle(sc)
    try:
        with oracle_textbook():
            return o.render(width, height, spp=spp, first_timestamp=first_timestamp, params=p)
    finally:
        o.close()


_ORACLE_FRAMES = {}


def oracle_frame(name, first_timestamp=0):
    """The textbook oracle's frame of one of FRAMES, computed once per process and shared (left unchanged by its readers)."""
    key = (name, first_timestamp)
    if key not in _ORACLE_FRAMES:
        w, h, spp = FRAMES[name]
        img, st = oracle_textbook_render(frame_scene(name), w, h, spp, first_timestamp=first_timestamp)
        img.setflags(write=False)
        _ORACLE_FRAMES[key] = (img, st)
    return _ORACLE_FRAMES[key]


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
# the two frames held to the oracle: Cornell (diffuse walls and boxes under one quad light: occluded shadow rays behind the boxes)
# and Cornell with all eight BSDF types (rough plastic: the floor of the eval pdf; glass and a mirror: wasDelta)
FRAMES = {"cornell": (64, 64, 8), "materials": (96, 80, 4)}
_SCENES = {}


def frame_scene(name):
    if name not in _SCENES:
        from gpuspectral_amd import scenes
        from oracle import mitsuba_loader as ml

        _SCENES[name] = ml.load_scene(os.path.join(GOLDEN, "cornell-box", "scene.xml")) if name == "cornell" else scenes.cornell_materials(8)
    return _SCENES[name]


def same(a, b):
    a, b = np.ascontiguousarray(a, np.float32).reshape(-1), np.ascontiguousarray(b, np.float32).reshape(-1)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


COUNT_KEYS = ("extension_rays", "shadow_rays", "shaded_vertices")


def counts_of(st):
    return tuple(int(st[k]) for k in COUNT_KEYS)


def luminance(rgb):
    rgb = np.asarray(rgb, np.float64)
    return 0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1] + 0.0722 * rgb[..., 2]


def frame_mean_and_se(moments, n):
    """moments[npix, 6] (per pixel sum and sum of squares of r, g, b over n samples) -> (frame mean of the RED channel, its standard
    error).  Pixels are independent (their seeds differ), so the variance of the frame mean is the sum of the pixels' variances of
    their means over npix^2."""
    m = np.asarray(moments, np.float64)
    mean_p = m[:, 0] / n
    var_p = np.maximum(m[:, 3] / n - mean_p * mean_p, 0.0) * (n / (n - 1.0))
    npix = len(m)
    return float(mean_p.mean()), math.sqrt(float(var_p.sum()) / n) / npix


def occluded_light_scene():
    """The occluded-commit case: a diffuse floor under a small bright light A (0.4 across, 3 up) that a plate (1.2 across, 2.5 up) hides
    from the middle of the floor, and a large dim emitter B (6 across, 4 up) over everything.  Half of the floor's light samples pick
    A and are occluded by the plate; the path that continues upwards past the plate ends on B -- an emitter hit behind an occluded
    shadow ray, the case whose commit must leave lastPdf alone."""
    import lights_util as lu
    from gpuspectral_amd import scenes

    b = scenes.SceneBuilder()
    lu._floor(b, half=6.0)
    black, grey = b.diffuse((0, 0, 0)), b.diffuse((0.5, 0.5, 0.5))

    def down_quad(h, y):
        return [[(-h, y, -h), (h, y, -h), (h, y, h)], [(-h, y, -h), (h, y, h), (-h, y, h)]]  # normal -y

    b.add_object(b.add_mesh(*lu.tri_mesh(down_quad(0.2, 3.0))), lu._identity(), black, twofaced=False, emission=(50.0, 50.0, 50.0))
    b.add_object(b.add_mesh(*lu.tri_mesh(down_quad(0.6, 2.5))), lu._identity(), grey, twofaced=True)
    b.add_object(b.add_mesh(*lu.tri_mesh(down_quad(3.0, 4.0))), lu._identity(), black, twofaced=False, emission=(1.0, 1.0, 1.0))
    b.camera_lookat((0, 2.0, 5), (0, 0, 0), fov_deg=25.0)
    return b.build()
