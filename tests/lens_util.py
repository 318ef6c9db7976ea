"""Shared by the thin-lens tests (not a test module): the ctypes handle on tests/emu/liblens_emu.so -- the product's stage headers
with a lens in the constants, compiled for the host (tests/emu/lens_emu.cpp; a test harness, never a product path) -- built the
way FilterEmu in test_pixel_filter_cpu.py builds its library, and the header's "Thin lens" semantics restated in numpy."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT

CIRCLE = dict(radius=0.08, focus_distance=5.0, blades=0, rotation=0.0)
PENTAGON = dict(radius=0.08, focus_distance=5.0, blades=5, rotation=0.0)
HEXAGON_ROT = dict(radius=0.08, focus_distance=5.0, blades=6, rotation=0.4)
LENSES = {"circle": CIRCLE, "5 blades": PENTAGON, "6 blades rotated": HEXAGON_ROT}


class LensEmu:
    def __init__(self):
        from gpuspectral_amd import abi

        d = os.path.join(ROOT, "tests", "emu")
        so = os.path.join(d, "liblens_emu.so")
        srcs = [os.path.join(d, f) for f in ("lens_emu.cpp", "filter_emu.cpp", "pt_emu.cpp")] + [os.path.join(ROOT, "include", "gpuspectral_pt.h")]
        csrc = os.path.join(ROOT, "gpuspectral_amd", "csrc")
        srcs += [os.path.join(csrc, h) for h in os.listdir(csrc) if h.endswith(".h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mfma", "-mavx2", "-shared", "-o", so, srcs[0]])
        L = C.CDLL(so)
        vp, u32, u64, f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
        LP = C.POINTER(abi.Lens)
        L.emu_create.restype = vp
        L.emu_create.argtypes = [C.POINTER(abi.SceneDesc)]
        L.emu_destroy.argtypes = [vp]
        L.lens_emu_resolve.argtypes = [LP, LP, C.c_char_p, u32]
        L.lens_emu_consts.argtypes = [u32, u32, f32, vp, LP, vp]
        L.lens_emu_generate.argtypes = [u32, u32, f32, vp, u32, f32, LP, vp, vp, u64, vp, vp]
        L.lens_emu_points.argtypes = [f32, u32, f32, vp, u64, vp, vp]
        L.lens_emu_ray_through.argtypes = [u32, u32, f32, vp, LP, vp, vp, u64, vp]
        L.lens_emu_pinhole.argtypes = [u32, u32, f32, vp, vp, u64, vp]
        L.lens_emu_render.argtypes = [vp, u32, u32, vp, u64, C.POINTER(abi.RenderParams), LP, vp, vp]
        self.L, self.abi = L, abi

    def _lens(self, lens):
        if lens is None:
            return None
        return lens if isinstance(lens, self.abi.Lens) else self.abi.lens(**lens)

    def resolve(self, lens):
        """gsp_set_lens's validation: (stored abi.Lens, None) or (None, error text)."""
        out = self.abi.Lens()
        err = C.create_string_buffer(256)
        l = self._lens(lens)
        rc = self.L.lens_emu_resolve(C.byref(l) if l is not None else None, C.byref(out), err, 256)
        return (None, err.value.decode()) if rc else (out, None)

    def consts(self, sc, width, height, lens):
        """{radius, focus, s, blades, rotation, zplane} as render_consts resolves them."""
        tw = np.ascontiguousarray(sc.to_world, np.float32)
        out = np.zeros(6, np.float32)
        l = self._lens(lens)
        self.L.lens_emu_consts(width, height, float(sc.fov), tw.ctypes.data, C.byref(l) if l is not None else None, out.ctypes.data)
        return dict(zip(("radius", "focus", "s", "blades", "rotation", "zplane"), out))

    def generate(self, sc, width, height, lens, gids, timestamps, filt=0, param=0.0):
        """(o[n,3], d[n,3], lens point[n,2], seed[n]) of the product's generate_path with this lens (and filter)."""
        gids = np.ascontiguousarray(gids, np.uint32)
        ts = np.ascontiguousarray(timestamps, np.uint32)
        tw = np.ascontiguousarray(sc.to_world, np.float32)
        out = np.zeros((len(gids), 8), np.float32)
        seeds = np.zeros(len(gids), np.uint32)
        l = self._lens(lens)
        self.L.lens_emu_generate(width, height, float(sc.fov), tw.ctypes.data, filt, param, C.byref(l) if l is not None else None,
                                 gids.ctypes.data, ts.ctypes.data, len(gids), out.ctypes.data, seeds.ctypes.data)
        return out[:, 0:3], out[:, 3:6], out[:, 6:8], seeds

    def points(self, radius, blades, rotation, states):
        """(lens points[n,2], states after) of the product's lens_point from the given RNG states."""
        st = np.ascontiguousarray(states, np.uint32)
        out = np.zeros((len(st), 2), np.float32)
        after = np.zeros(len(st), np.uint32)
        self.L.lens_emu_points(radius, blades, rotation, st.ctypes.data, len(st), out.ctypes.data, after.ctypes.data)
        return out, after

    def ray_through(self, sc, width, height, lens, frag, lpts):
        frag = np.ascontiguousarray(frag, np.float32)
        lpts = np.ascontiguousarray(lpts, np.float32)
        tw = np.ascontiguousarray(sc.to_world, np.float32)
        out = np.zeros((len(frag), 6), np.float32)
        l = self._lens(lens)
        self.L.lens_emu_ray_through(width, height, float(sc.fov), tw.ctypes.data, C.byref(l), frag.ctypes.data, lpts.ctypes.data, len(frag),
                                    out.ctypes.data)
        return out[:, 0:3], out[:, 3:6]

    def pinhole(self, sc, width, height, frag):
        """(d[n,3], cos[n]): the pinhole ray of each fragCoord and the float32 cosine of gsp_focus_distance."""
        frag = np.ascontiguousarray(frag, np.float32)
        tw = np.ascontiguousarray(sc.to_world, np.float32)
        out = np.zeros((len(frag), 4), np.float32)
        self.L.lens_emu_pinhole(width, height, float(sc.fov), tw.ctypes.data, frag.ctypes.data, len(frag), out.ctypes.data)
        return out[:, 0:3], out[:, 3]

    def scene(self, sc):
        return LensEmuScene(self, sc)


class LensEmuScene:
    def __init__(self, emu, sc):
        self.emu, self.sc = emu, sc
        self._desc = sc.desc()
        self.h = emu.L.emu_create(C.byref(self._desc))

    def render(self, width, height, spp, lens=None, first_timestamp=0, pixel_filter=0, pixel_filter_param=0.0, pixel_ids=None, accum=None):
        """(accum[n,4], {extension_rays, shadow_rays, shaded_vertices})."""
        p = self.emu.abi.default_render_params()
        p.spp, p.first_timestamp, p.pixel_filter, p.pixel_filter_param = spp, first_timestamp, pixel_filter, pixel_filter_param
        ids = np.ascontiguousarray(pixel_ids, np.uint32) if pixel_ids is not None else None
        n = len(ids) if ids is not None else width * height
        if accum is None:
            accum = np.zeros((n, 4), np.float32)
        counts = np.zeros(3, np.uint64)
        l = self.emu._lens(lens)
        self.emu.L.lens_emu_render(self.h, width, height, ids.ctypes.data if ids is not None else None, n, C.byref(p),
                                   C.byref(l) if l is not None else None, accum.ctypes.data, counts.ctypes.data)
        return accum, dict(extension_rays=int(counts[0]), shadow_rays=int(counts[1]), shaded_vertices=int(counts[2]))

    def __del__(self):
        try:
            self.emu.L.emu_destroy(self.h)
        except Exception:
            pass


def same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def polygon_vertices(radius, blades, rotation):
    """The header's vertices in float64."""
    j = np.arange(blades)
    a = rotation + 2 * np.pi * j / blades
    return radius * np.stack([np.cos(a), np.sin(a)], 1)


def inside_polygon(pts, verts, slack):
    """Every point on the inner side of every edge (counter-clockwise vertices), up to `slack` in length units."""
    ok = np.ones(len(pts), bool)
    n = len(verts)
    for k in range(n):
        a, b = verts[k], verts[(k + 1) % n]
        e = b - a
        nrm = np.array([-e[1], e[0]]) / np.hypot(*e)  # inward for counter-clockwise order
        ok &= ((pts - a) @ nrm) >= -slack
    return ok
