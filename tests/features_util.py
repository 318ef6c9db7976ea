"""Shared by the feature-buffer tests (not a test module): the ctypes handle on tests/emu/libfeatures_emu.so -- the product's
pt_features.h, generate_path and the emulation's traversal compiled for the host (tests/emu/features_emu.cpp; a test harness,
never a product path), built the way LensEmu builds its library -- and the header's "Feature buffers" semantics restated in
numpy from the scene arrays."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT
from lens_util import LensEmu

MISS = 0xFFFFFFFF
ULP1 = 2.0 ** -23  # ulp of 1.0 in float32


class FeaturesEmu(LensEmu):
    def __init__(self):
        from gpuspectral_amd import abi

        d = os.path.join(ROOT, "tests", "emu")
        so = os.path.join(d, "libfeatures_emu.so")
        srcs = [os.path.join(d, f) for f in ("features_emu.cpp", "lens_emu.cpp", "filter_emu.cpp", "pt_emu.cpp")] + [os.path.join(ROOT, "include", "gpuspectral_pt.h")]
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
        L.lens_emu_generate.argtypes = [u32, u32, f32, vp, u32, f32, LP, vp, vp, u64, vp, vp]
        L.features_emu_render.argtypes = [vp, u32, u32, vp, u64, C.POINTER(abi.RenderParams), LP, vp, vp, vp]
        self.L, self.abi = L, abi

    def scene(self, sc):
        return FeaturesEmuScene(self, sc)


class FeaturesEmuScene:
    def __init__(self, emu, sc):
        self.emu, self.sc = emu, sc
        self._desc = sc.desc()
        self.h = emu.L.emu_create(C.byref(self._desc))

    def render(self, width, height, spp, lens=None, first_timestamp=0, pixel_filter=0, pixel_filter_param=0.0, pixel_ids=None, planes=None):
        """Compact planes (albedo[n,4] f32, geom[n,4] f32, ids[n,4] u32) after spp more feature samples; `planes` continues a frame."""
        p = self.emu.abi.default_render_params()
        p.spp, p.first_timestamp, p.pixel_filter, p.pixel_filter_param = spp, first_timestamp, pixel_filter, pixel_filter_param
        pid = np.ascontiguousarray(pixel_ids, np.uint32) if pixel_ids is not None else None
        n = len(pid) if pid is not None else width * height
        if planes is None:
            planes = (np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32), np.zeros((n, 4), np.uint32))
        a, g, i = planes
        l = self.emu._lens(lens)
        self.emu.L.features_emu_render(self.h, width, height, pid.ctypes.data if pid is not None else None, n, C.byref(p),
                                       C.byref(l) if l is not None else None, a.ctypes.data, g.ctypes.data, i.ctypes.data)
        return a, g, i

    def __del__(self):
        try:
            self.emu.L.emu_destroy(self.h)
        except Exception:
            pass


def full(planes, width, height):
    """Compact whole-frame planes in the layout of Context.download_features."""
    return tuple(p.reshape(height, width, 4) for p in planes)


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def tri_first(sc):
    return np.concatenate([[0], np.cumsum(sc.instances["vertex_count"] // 3)]).astype(np.int64)


def record_albedo(sc, handle):
    """The header's albedo table for an untextured record, in float32 as the library forms it."""
    from gpuspectral_amd import abi

    t, i = handle >> 16, handle & 0xFFFF
    name = abi.BSDF_NAMES[t]
    rec = sc.bsdfs[t][i]
    if name == "diffuse":  # the resident record holds reflectance / pi
        pi = np.float32(3.14159265358979323846)
        return (rec["reflectance"].astype(np.float32) / pi) * pi
    if name in ("smooth_plastic", "rough_plastic", "smooth_floor", "rough_floor"):
        return rec["diffuse"].astype(np.float32)
    if name == "rough_conductor":
        return rec["reflectance"].astype(np.float32)
    return np.ones(3, np.float32)


def restate(sc, o, d, hits):
    """One feature sample per ray from the scene arrays and the oracle's hits.
    Returns dict(albedo[n,4] f32, depth[n] f32, ids[n,3] u32, normal[n,3] f64, ambiguous[n] bool, flipped[n] bool, emitter[n] bool):
    the normal is the float64 restatement of SN; `ambiguous` marks hits whose two-faced test dot(N, -d) is too close to zero to
    call in another precision."""
    n = len(hits)
    first = tri_first(sc)
    out = dict(albedo=np.zeros((n, 4), np.float32), depth=np.zeros(n, np.float32), ids=np.full((n, 3), MISS, np.uint32),
               normal=np.zeros((n, 3), np.float64), ambiguous=np.zeros(n, bool), flipped=np.zeros(n, bool), emitter=np.zeros(n, bool))
    pos = np.asarray(sc.positions, np.float64)
    nrm = np.asarray(sc.normals, np.float64)
    for k in range(n):
        g = int(hits["prim"][k])
        if g < 0:
            continue
        inst = int(np.searchsorted(first, g, "right") - 1)
        I = sc.instances[inst]
        v0 = int(I["first_vertex"]) + 3 * (g - int(first[inst]))
        M = np.asarray(I["transform"], np.float64).reshape(4, 4).T  # glm memory order -> the matrix
        inv_t = np.linalg.inv(M[:3, :3]).T
        u, v = float(hits["u"][k]), float(hits["v"][k])
        sn = (1.0 - u - v) * (inv_t @ nrm[v0]) + u * (inv_t @ nrm[v0 + 1]) + v * (inv_t @ nrm[v0 + 2])
        sn /= np.linalg.norm(sn)
        p = [M[:3, :3] @ pos[v0 + j] + M[:3, 3] for j in range(3)]
        N = np.cross(p[1] - p[0], p[2] - p[0])
        N /= np.linalg.norm(N)
        facing = float(N @ -np.asarray(d[k], np.float64))
        em = np.asarray(I["emission"], np.float32)
        emits = bool((em != 0).any())
        out["ambiguous"][k] = abs(facing) < 1e-5
        if facing < 0 and int(I["twofaced"]) == 1 and not emits:
            sn = -sn
            out["flipped"][k] = True
        out["emitter"][k] = emits
        out["normal"][k] = sn
        out["depth"][k] = hits["t"][k]
        out["ids"][k] = (g, int(I["bsdf"]), inst)
        out["albedo"][k, :3] = np.minimum(em, np.float32(1.0)) if emits else record_albedo(sc, int(I["bsdf"]))
        out["albedo"][k, 3] = 1.0
    return out


def fold(mean, x, n):
    """The header's running mean in float32: mean + (x - mean) * (1 / (n + 1))."""
    a = np.float32(1.0) / np.float32(n + 1)
    mean = np.asarray(mean, np.float32)
    return (mean + (np.asarray(x, np.float32) - mean) * a).astype(np.float32)
