"""Shared by the temporal-accumulation tests (not a test module): the ctypes handle on tests/emu/libtemporal_emu.so -- the
library's csrc/pt_temporal.h compiled for the host (tests/emu/temporal_emu.cpp; a test harness, never a product path), built the
way denoise_util.DenoiseEmu builds its library -- and the header's "Temporal accumulation" semantics restated in float64 numpy,
written from include/gpuspectral_pt.h alone."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT

FLT_MIN = 1.1754943508222875e-38
BACKGROUND = 0xFFFFFFFF
DEFAULTS = dict(max_history=32, alpha=0.2, depth_tolerance=0.02, normal_min=0.9)
U32 = 2.0 ** -24  # unit roundoff of float32


def refusals(ctx, cases):
    """Every (export, its arguments behind the context, text) of `cases`: the call on the library itself returns GSP_ERR_INVALID (1)
    and leaves a gsp_last_error that contains `text`.  A case breaks two of the export's conditions at once and `text` is that of the
    one the export tests first, so two refusals that change places fail here.  (A device destination of such a call is never written:
    16 stands for one.)"""
    for export, args, text in cases:
        rc = getattr(ctx._L, export)(ctx._h, *args)
        err = ctx._L.gsp_last_error(ctx._h).decode()
        assert rc == 1 and text in err, (export, text, rc, err)


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


class History:
    """One history set and the camera it belongs to."""

    def __init__(self, H, G, I, to_world, fov):
        self.H, self.G, self.I, self.to_world, self.fov = H, G, I, np.asarray(to_world, np.float32).reshape(16).copy(), float(np.float32(fov))


class TemporalEmu:
    def __init__(self):
        from gpuspectral_amd import abi

        d = os.path.join(ROOT, "tests", "emu")
        so = os.path.join(d, "libtemporal_emu.so")
        csrc = os.path.join(ROOT, "gpuspectral_amd", "csrc")
        srcs = [os.path.join(d, "temporal_emu.cpp"), os.path.join(ROOT, "include", "gpuspectral_pt.h")] + [
            os.path.join(csrc, n) for n in ("pt_temporal.h", "pt_denoise.h", "pt_display.h", "pt_math.h", "pt_stages.h", "pt_shading.h", "pt_trace.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mfma", "-mavx2", "-shared", "-o", so, srcs[0]])
        L = C.CDLL(so)
        vp, u32 = C.c_void_p, C.c_uint32
        TP, CP = C.POINTER(abi.Temporal), C.POINTER(abi.Camera)
        L.temporal_emu_resolve.argtypes = [TP, vp, C.c_char_p, u32]
        L.temporal_emu_run.argtypes = [TP, CP, CP, C.c_int, u32, u32] + [vp] * 11 + [C.c_char_p, u32]
        self.L, self.abi = L, abi

    @staticmethod
    def _ref(d):
        return C.byref(d) if d is not None else None

    def _camera(self, to_world, fov):
        cam = self.abi.Camera()
        for i, v in enumerate(np.asarray(to_world, np.float32).reshape(16)):
            cam.to_world[i] = float(v)
        cam.fov = float(fov)
        return cam

    def resolve(self, temporal):
        """The library's validation: (dict(max_history, alpha, depth_tolerance, normal_min), None) or (None, error text)."""
        out = np.zeros(4, np.uint32)
        err = C.create_string_buffer(256)
        if self.L.temporal_emu_resolve(self._ref(temporal), out.ctypes.data, err, 256):
            return None, err.value.decode()
        f = out.view(np.float32)
        return dict(max_history=f[0], alpha=f[1], depth_tolerance=f[2], normal_min=f[3]), None

    def step(self, temporal, to_world, fov, accum, albedo, geom, ids, hist=None, with_kept=False):
        """One gsp_temporal_accumulate: the frame (h, w, 4) float32 / uint32 planes under camera (to_world, fov), on `hist` (a History,
        None = no valid history).  Returns the new History (and the kept-tap mask (h, w) uint8 with with_kept)."""
        c = np.ascontiguousarray(accum, np.float32)
        a = np.ascontiguousarray(albedo, np.float32)
        g = np.ascontiguousarray(geom, np.float32)
        i = np.ascontiguousarray(ids, np.uint32)
        h, w = c.shape[:2]
        assert c.shape == a.shape == g.shape == i.shape == (h, w, 4)
        H, G, I = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32), np.zeros((h, w), np.uint32)
        kept = np.zeros((h, w), np.uint8)
        cur = self._camera(to_world, fov)
        prev = self._camera(hist.to_world, hist.fov) if hist is not None else None
        if hist is not None:
            assert hist.H.shape == (h, w, 4) and hist.H.flags.c_contiguous and hist.G.flags.c_contiguous and hist.I.flags.c_contiguous
        err = C.create_string_buffer(256)
        rc = self.L.temporal_emu_run(self._ref(temporal), C.byref(cur), C.byref(prev) if prev is not None else None, 1 if hist is not None else 0, w, h,
                                     c.ctypes.data, a.ctypes.data, g.ctypes.data, i.ctypes.data,
                                     hist.H.ctypes.data if hist is not None else None, hist.G.ctypes.data if hist is not None else None,
                                     hist.I.ctypes.data if hist is not None else None, H.ctypes.data, G.ctypes.data, I.ctypes.data, kept.ctypes.data, err, 256)
        if rc:
            raise ValueError(err.value.decode())
        new = History(H, G, I, to_world, fov)
        return (new, kept) if with_kept else new


# ---- cameras ------------------------------------------------------------------------------------------------------------------
def mat3(to_world):
    """The upper-left 3x3 of a to_world in glm memory order (m[4 * c + r]) as a row-major matrix."""
    return np.asarray(to_world, np.float64).reshape(4, 4).T[:3, :3].copy()


def rotated_about_y(to_world, degrees, pivot=(0.0, 0.0, 0.0)):
    """to_world turned by `degrees` about the world y axis through `pivot`; 16 float32 in glm memory order."""
    m = np.asarray(to_world, np.float64).reshape(4, 4).T
    a = np.radians(degrees)
    r = np.eye(4)
    r[0, 0], r[0, 2], r[2, 0], r[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    t, ti = np.eye(4), np.eye(4)
    t[:3, 3], ti[:3, 3] = pivot, -np.asarray(pivot, np.float64)
    return (t @ r @ ti @ m).T.astype(np.float32).reshape(16)


def zplane64(w, h, fov):
    return (max(w, h) / 2.0) / np.tan(float(np.float32(fov)) / 2.0)


def pinhole_dirs64(to_world, fov, w, h):
    """Step 1 of the header for every pixel: (h, w, 3) float64."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    v = np.stack([-(xs - w / 2.0), ys - h / 2.0, np.full((h, w), zplane64(w, h, fov))], -1)
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    d = v @ mat3(to_world).T
    d[..., 1] *= -1.0
    return d


# ---- the header's "Temporal accumulation" section in float64 numpy ----------------------------------------------------------------
def temporal64(accum, albedo, geom, ids, to_world, fov, hist=None, max_history=0, alpha=0.0, depth_tolerance=0.0, normal_min=0.0):
    """Returns dict(H (h, w, 4) float64, G, I, kept (h, w) uint8 in the emulation's encoding, fragile (h, w) bool: a decision of the
    pixel -- the snap, sw >= 0.01 -- sits so close to its threshold that float32 rounding may take it the other way)."""
    c = np.asarray(accum, np.float32).astype(np.float64)
    alb = np.asarray(albedo, np.float32).astype(np.float64)
    g = np.asarray(geom, np.float32).astype(np.float64)
    inst = np.asarray(ids, np.uint32)[..., 2]
    h, w = c.shape[:2]
    maxh = float(max_history or DEFAULTS["max_history"])
    al = float(np.float32(alpha)) if alpha else float(np.float32(DEFAULTS["alpha"]))
    tol = float(np.float32(depth_tolerance)) if depth_tolerance else float(np.float32(DEFAULTS["depth_tolerance"]))
    nmin = float(np.float32(normal_min)) if normal_min else float(np.float32(DEFAULTS["normal_min"]))
    cov = alb[..., 3]
    surface = (inst != BACKGROUND) & (np.asarray(albedo, np.float32)[..., 3] >= np.float32(0.5))
    safe = np.where(surface, cov, 1.0)
    n = np.where(surface[..., None], g[..., :3] / safe[..., None], 0.0)
    z = np.where(surface, g[..., 3] / safe, 0.0)
    I = np.where(surface, inst, BACKGROUND).astype(np.uint32)
    fin = np.isfinite(np.asarray(accum, np.float32)[..., :3]).all(-1)
    sw = np.zeros((h, w))
    s = np.zeros((h, w, 3))
    sl = np.zeros((h, w))
    kept = np.zeros((h, w), np.uint8)
    fragile = np.zeros((h, w), bool)
    if hist is not None:
        Hp, Gp, Ip = hist.H.astype(np.float64), hist.G.astype(np.float64), hist.I
        Hfin = np.isfinite(hist.H[..., :3]).all(-1) & (hist.H[..., 3] > 0)
        d = pinhole_dirs64(to_world, fov, w, h)
        eye = np.asarray(to_world, np.float32).astype(np.float64)[12:15]
        eye_prev = hist.to_world.astype(np.float64)[12:15]
        P = eye + d * z[..., None]
        v = np.where(surface[..., None], P - eye_prev, d)
        ze = np.linalg.norm(v, axis=-1)
        minv = np.linalg.inv(mat3(hist.to_world)).astype(np.float32).astype(np.float64)
        l = (v * np.array([1.0, -1.0, 1.0])) @ minv.T
        front = l[..., 2] > 0
        with np.errstate(all="ignore"):
            t = zplane64(w, h, hist.fov) / np.where(front, l[..., 2], 1.0)
            fx = w / 2.0 - l[..., 0] * t
            fy = h / 2.0 + l[..., 1] * t
        for f in (fx, fy):
            r = np.rint(f)
            dist = np.abs(f - r)
            fragile |= front & (np.abs(dist - 1e-3) < 2e-4)
            f[...] = np.where(dist < np.float32(1e-3), r, f)
        ok = front & (fx > -1) & (fx < w) & (fy > -1) & (fy < h)
        fx, fy = np.where(ok, fx, 0.0), np.where(ok, fy, 0.0)
        x0, y0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
        wx, wy = fx - x0, fy - y0
        kept[ok] = 0x80
        for i, (ox, oy, wt) in enumerate(((0, 0, (1 - wx) * (1 - wy)), (1, 0, wx * (1 - wy)), (0, 1, (1 - wx) * wy), (1, 1, wx * wy))):
            qx, qy = x0 + ox, y0 + oy
            use = ok & (wt != 0) & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            Hq, Gq, Iq = Hp[qy, qx], Gp[qy, qx], Ip[qy, qx]
            use &= Hfin[qy, qx] & (Iq == I)
            with np.errstate(all="ignore"):
                geo = ~(np.abs(ze - Gq[..., 3]) > tol * ze) & ~((n * Gq[..., :3]).sum(-1) < nmin)
            use &= np.where(surface, geo, True)
            wt = np.where(use, wt, 0.0)
            Hq = np.where(use[..., None], Hq, 0.0)
            sw += wt
            s += wt[..., None] * Hq[..., :3]
            sl += wt * Hq[..., 3]
            kept |= (use.astype(np.uint8) << i).astype(np.uint8)
        fragile |= np.abs(sw - 0.01) < 1e-4
    has = sw >= np.float32(0.01)
    sws = np.where(has, sw, 1.0)
    prev = s / sws[..., None]
    ln = sl / sws
    N = np.minimum(np.where(fin, ln + 1.0, ln), maxh)
    with np.errstate(all="ignore"):
        a = np.maximum(al, 1.0 / np.where(N > 0, N, 1.0))
        blended = prev + (np.where(fin[..., None], c[..., :3], 0.0) - prev) * a[..., None]
    H = np.zeros((h, w, 4))
    H[..., :3] = np.where(has[..., None], np.where(fin[..., None], blended, prev), c[..., :3])
    H[..., 3] = np.where(has, N, np.where(fin, 1.0, 0.0))
    G = np.concatenate([n, z[..., None]], -1)
    return dict(H=H, G=G, I=I, kept=kept, fragile=fragile, sw=sw)


# ---- synthetic frames ----------------------------------------------------------------------------------------------------------
def plane_frame(rng, h, w, to_world, fov, depth=5.0, inst=3, normal=(0.0, 0.0, -1.0)):
    """The world plane z = depth seen by the pinhole camera (to_world, fov): random finite colours in [0, 2), albedo {0.5, 1}, geom
    {normal, the distance along the pixel's pinhole ray: (depth - eye.z) / d.z, in float64 and rounded}, ids {0, 0, inst, 1}.
    depth / inst / normal may be (h, w) / (h, w, 3) arrays."""
    d = pinhole_dirs64(to_world, fov, w, h)
    eye_z = float(np.asarray(to_world, np.float32)[14])
    accum = np.zeros((h, w, 4), np.float32)
    accum[..., :3] = rng.uniform(0.0, 2.0, (h, w, 3))
    accum[..., 3] = 1.0
    albedo = np.ones((h, w, 4), np.float32)
    albedo[..., :3] = 0.5
    geom = np.zeros((h, w, 4), np.float32)
    geom[..., :3] = normal
    geom[..., 3] = (np.asarray(depth, np.float64) - eye_z) / d[..., 2]
    ids = np.zeros((h, w, 4), np.uint32)
    ids[..., 2] = inst
    ids[..., 3] = 1
    return accum, albedo, geom, ids


def camera(yaw=0.0, pitch=0.0, eye=(0.0, 0.0, 0.0)):
    """to_world (16 float32, glm memory order) of a camera at `eye` that looks along +z, turned by yaw about its up axis and then by
    pitch about its right axis (radians)."""
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    m = np.eye(4)
    m[:3, :3] = ry @ rx
    m[:3, 3] = eye
    return m.T.astype(np.float32).reshape(16)


def background_frame(rng, h, w):
    accum = np.zeros((h, w, 4), np.float32)
    accum[..., :3] = rng.uniform(0.0, 2.0, (h, w, 3))
    accum[..., 3] = 1.0
    ids = np.full((h, w, 4), BACKGROUND, np.uint32)
    ids[..., 3] = 1
    return accum, np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32), ids
