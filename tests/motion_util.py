"""Shared by the moved-instances tests (not a test module): the ctypes handle on tests/emu/libmotion_emu.so -- the library's
csrc/pt_motion.h compiled for the host (tests/emu/motion_emu.cpp; a test harness, never a product path), built the way
temporal_util.TemporalEmu builds its library -- and the header's "Temporal accumulation: moved instances" semantics restated in
float64 numpy, written from include/gpuspectral_pt.h alone."""
import ctypes as C
import os
import subprocess

import numpy as np

import temporal_util as tu
from conftest import ROOT
from svgf_util import MHistory

STATIC, MOVED, NO_HISTORY = 0, 1, 2
RECORD_WORDS = 24
CSRC_HEADERS = ("pt_motion.h", "pt_svgf.h", "pt_temporal.h", "pt_denoise.h", "pt_display.h", "pt_math.h", "pt_stages.h", "pt_shading.h", "pt_trace.h")


class FHistory(MHistory):
    """A history set (M = None without moments) with the instance transforms (n, 16) float32 it belongs to and its motion plane V."""

    def __init__(self, H, G, I, M, V, to_world, fov, xforms):
        super().__init__(H, G, I, M, to_world, fov)
        self.V, self.xforms = V, np.ascontiguousarray(xforms, np.float32).reshape(-1, 16).copy()


class MotionEmu:
    def __init__(self):
        from gpuspectral_amd import abi

        d = os.path.join(ROOT, "tests", "emu")
        so = os.path.join(d, "libmotion_emu.so")
        csrc = os.path.join(ROOT, "gpuspectral_amd", "csrc")
        srcs = [os.path.join(d, "motion_emu.cpp"), os.path.join(ROOT, "include", "gpuspectral_pt.h")] + [os.path.join(csrc, n) for n in CSRC_HEADERS]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mfma", "-mavx2", "-shared", "-o", so, srcs[0]])
        L = C.CDLL(so)
        vp, u32 = C.c_void_p, C.c_uint32
        TP, CP = C.POINTER(abi.Temporal), C.POINTER(abi.Camera)
        L.motion_emu_table.argtypes = [vp, vp, u32, vp]
        L.motion_emu_table.restype = None
        L.motion_emu_run.argtypes = [TP, CP, CP, C.c_int, u32, u32, C.c_int] + [vp] * 9 + [u32] + [vp] * 5 + [C.c_char_p, u32]
        self.L, self.abi = L, abi

    def _camera(self, to_world, fov):
        cam = self.abi.Camera()
        for i, v in enumerate(np.asarray(to_world, np.float32).reshape(16)):
            cam.to_world[i] = float(v)
        cam.fov = float(fov)
        return cam

    def table(self, xf_prev, xf_cur):
        """motion_table: (n, 24) uint32 -- per instance the rows of B (3 x 4 floats), the rows of N (3 x {3 floats, a word}); word 15
        is the class."""
        p = np.ascontiguousarray(xf_prev, np.float32).reshape(-1, 16)
        c = np.ascontiguousarray(xf_cur, np.float32).reshape(-1, 16)
        assert p.shape == c.shape
        out = np.zeros((len(p), RECORD_WORDS), np.uint32)
        self.L.motion_emu_table(p.ctypes.data, c.ctypes.data, len(p), out.ctypes.data)
        return out

    def step(self, temporal, to_world, fov, accum, albedo, geom, ids, xforms, hist=None, moments=False, table=None):
        """One followed gsp_temporal_accumulate: the frame under camera (to_world, fov) and instance transforms `xforms` on `hist` (an
        FHistory, None = no valid history).  table overrides the records (tests of the table read).  Returns the new FHistory."""
        c = np.ascontiguousarray(accum, np.float32)
        a = np.ascontiguousarray(albedo, np.float32)
        g = np.ascontiguousarray(geom, np.float32)
        i = np.ascontiguousarray(ids, np.uint32)
        h, w = c.shape[:2]
        assert c.shape == a.shape == g.shape == i.shape == (h, w, 4)
        xf = np.ascontiguousarray(xforms, np.float32).reshape(-1, 16)
        H, G, M, V = (np.zeros((h, w, 4), np.float32) for _ in range(4))
        I = np.zeros((h, w), np.uint32)
        cur = self._camera(to_world, fov)
        prev = self._camera(hist.to_world, hist.fov) if hist is not None else None
        if hist is not None:
            assert hist.H.shape == (h, w, 4) and all(p.flags.c_contiguous for p in (hist.H, hist.G, hist.I))
            assert not moments or hist.M is not None
            if table is None:
                table = self.table(hist.xforms, xf)
        tab = np.ascontiguousarray(table, np.uint32) if table is not None else np.zeros((0, RECORD_WORDS), np.uint32)
        ptr = lambda p: p.ctypes.data if (hist is not None and p is not None) else None
        err = C.create_string_buffer(256)
        rc = self.L.motion_emu_run(C.byref(temporal) if temporal is not None else None, C.byref(cur), C.byref(prev) if prev is not None else None,
                                   1 if hist is not None else 0, w, h, 1 if moments else 0, c.ctypes.data, a.ctypes.data, g.ctypes.data, i.ctypes.data,
                                   *((ptr(hist.H), ptr(hist.G), ptr(hist.I), ptr(hist.M) if moments else None) if hist is not None else (None,) * 4),
                                   tab.ctypes.data if len(tab) else None, len(tab), H.ctypes.data, G.ctypes.data, I.ctypes.data, M.ctypes.data, V.ctypes.data,
                                   err, 256)
        if rc:
            raise ValueError(err.value.decode())
        return FHistory(H, G, I, M if moments else None, V, to_world, fov, xf)


# ---- transforms (glm memory order: t[4 * c + r]) ---------------------------------------------------------------------------------
def affine(t16):
    """(A (3, 3), t (3,)) float64 of a transform."""
    m = np.asarray(t16, np.float32).astype(np.float64).reshape(4, 4).T
    return m[:3, :3].copy(), m[:3, 3].copy()


def compose(A, t):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = A, t
    return m.T.astype(np.float32).reshape(16)


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = np.radians(degrees)
    return np.eye(3) + np.sin(r) * K + (1 - np.cos(r)) * (K @ K)


def moved(t16, R=np.eye(3), pivot=(0.0, 0.0, 0.0), shift=(0.0, 0.0, 0.0)):
    """The transform t16 followed by the world-space map x -> R (x - pivot) + pivot + shift; 16 float32."""
    A, t = affine(t16)
    pivot, shift = np.asarray(pivot, np.float64), np.asarray(shift, np.float64)
    return compose(R @ A, R @ (t - pivot) + pivot + shift)


def table64(xf_prev, xf_cur):
    """The header's record in numpy float64: (cls (n,), B (n, 3, 4), N (n, 3, 3)); B and N are zero unless cls == 1."""
    p = np.asarray(xf_prev, np.float32).reshape(-1, 16)
    c = np.asarray(xf_cur, np.float32).reshape(-1, 16)
    n = len(p)
    cls, B, N = np.zeros(n, np.uint32), np.zeros((n, 3, 4)), np.zeros((n, 3, 3))
    for i in range(n):
        if np.array_equal(p[i].view(np.uint32), c[i].view(np.uint32)):
            continue
        (Ap, tp), (Ac, tc) = affine(p[i]), affine(c[i])
        with np.errstate(all="ignore"):
            dp, dc = np.linalg.det(Ap), np.linalg.det(Ac)
            ok = np.isfinite(dp) and np.isfinite(dc) and dp != 0 and dc != 0
            if ok:
                B3 = Ap @ np.linalg.inv(Ac)
                b = np.concatenate([B3, (tp - B3 @ tc)[:, None]], 1)
                nn = (Ac @ np.linalg.inv(Ap)).T
                ok = np.isfinite(b.astype(np.float32)).all() and np.isfinite(nn.astype(np.float32)).all()
        if not ok:
            cls[i] = NO_HISTORY
            continue
        cls[i], B[i], N[i] = MOVED, b, nn
    return cls, B, N


def split_table(tab):
    """(cls, B (n, 3, 4) float32, N (n, 3, 3) float32) of MotionEmu.table's words."""
    f = tab.view(np.float32).reshape(-1, 6, 4)
    return tab[:, 15].copy(), f[:, :3, :].copy(), f[:, 3:, :3].copy()


# ---- the header's "Temporal accumulation: moved instances" section in float64 numpy --------------------------------------------------
def motion64(accum, albedo, geom, ids, to_world, fov, xforms, hist=None, max_history=0, alpha=0.0, depth_tolerance=0.0, normal_min=0.0):
    """temporal_util.temporal64 with the instances followed (hist: an FHistory or None).  The records are float32 -- the header
    rounds them once -- so they come from table64 rounded.  Returns temporal64's dict with V (h, w, 4) float64, cls (h, w) and
    `fragile` widened by the followed pixels' own threshold: s > 0 never sits near it for a finite record."""
    D = tu.DEFAULTS
    c = np.asarray(accum, np.float32).astype(np.float64)
    alb32 = np.asarray(albedo, np.float32)
    g = np.asarray(geom, np.float32).astype(np.float64)
    inst = np.asarray(ids, np.uint32)[..., 2]
    h, w = c.shape[:2]
    maxh = float(max_history or D["max_history"])
    al = float(np.float32(alpha or D["alpha"]))
    tol = float(np.float32(depth_tolerance or D["depth_tolerance"]))
    nmin = float(np.float32(normal_min or D["normal_min"]))
    cov = alb32[..., 3].astype(np.float64)
    surface = (inst != tu.BACKGROUND) & (alb32[..., 3] >= np.float32(0.5))
    safe = np.where(surface, cov, 1.0)
    n = np.where(surface[..., None], g[..., :3] / safe[..., None], 0.0)
    z = np.where(surface, g[..., 3] / safe, 0.0)
    I = np.where(surface, inst, tu.BACKGROUND).astype(np.uint32)
    fin = np.isfinite(np.asarray(accum, np.float32)[..., :3]).all(-1)
    sw, s, sl = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w))
    kept = np.zeros((h, w), np.uint8)
    fragile = np.zeros((h, w), bool)
    V = np.zeros((h, w, 4))
    pix_cls = np.zeros((h, w), np.uint32)
    if hist is not None:
        cls, B, N = table64(hist.xforms, xforms)
        B, N = B.astype(np.float32).astype(np.float64), N.astype(np.float32).astype(np.float64)
        known = surface & (inst < len(cls))
        idx = np.where(known, inst, 0)
        pix_cls = np.where(surface, np.where(known, cls[idx] if len(cls) else NO_HISTORY, NO_HISTORY), STATIC).astype(np.uint32)
        Hp, Gp, Ip = hist.H.astype(np.float64), hist.G.astype(np.float64), hist.I
        Hfin = np.isfinite(hist.H[..., :3]).all(-1) & (hist.H[..., 3] > 0)
        d = tu.pinhole_dirs64(to_world, fov, w, h)
        eye = np.asarray(to_world, np.float32).astype(np.float64)[12:15]
        eye_prev = hist.to_world.astype(np.float64)[12:15]
        P = eye + d * z[..., None]
        mv = pix_cls == MOVED
        if len(cls):
            Pm = np.einsum("hwrc,hwc->hwr", B[idx][..., :3], P) + B[idx][..., 3]
            m = np.einsum("hwrc,hwc->hwr", N[idx], n)
        else:
            Pm, m = P, n
        P = np.where(mv[..., None], Pm, P)
        ss = (m * m).sum(-1)
        s_ok = ~mv | (ss > 0)
        with np.errstate(all="ignore"):
            nt = np.where(mv[..., None], m / np.sqrt(np.where(ss > 0, ss, 1.0))[..., None], n)  # what the tap test sees
        v = np.where(surface[..., None], P - eye_prev, d)
        ze = np.linalg.norm(v, axis=-1)
        minv = np.linalg.inv(tu.mat3(hist.to_world)).astype(np.float32).astype(np.float64)
        l = (v * np.array([1.0, -1.0, 1.0])) @ minv.T
        front = (l[..., 2] > 0) & (pix_cls != NO_HISTORY) & s_ok
        with np.errstate(all="ignore"):
            t = tu.zplane64(w, h, hist.fov) / np.where(front, l[..., 2], 1.0)
            fx = w / 2.0 - l[..., 0] * t
            fy = h / 2.0 + l[..., 1] * t
        for f in (fx, fy):
            r = np.rint(f)
            dist = np.abs(f - r)
            fragile |= front & (np.abs(dist - 1e-3) < 2e-4)
            f[...] = np.where(dist < np.float32(1e-3), r, f)
        ok = front & (fx > -1) & (fx < w) & (fy > -1) & (fy < h)
        with np.errstate(all="ignore"):
            border = front & ((np.abs(fx + 1) < 1e-3) | (np.abs(fx - w) < 1e-3) | (np.abs(fy + 1) < 1e-3) | (np.abs(fy - h) < 1e-3))
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
                geo = ~(np.abs(ze - Gq[..., 3]) > tol * ze) & ~((nt * Gq[..., :3]).sum(-1) < nmin)
                # a tap whose depth or normal test sits within rounding of its threshold (ze, z_q and the dot product carry a few u
                # of relative error; 1e-5 is a hundred times that) may be kept by one evaluation and dropped by the other
                near = (np.abs(np.abs(ze - Gq[..., 3]) - tol * ze) < 1e-5 * ze) | (np.abs((nt * Gq[..., :3]).sum(-1) - nmin) < 1e-5)
            fragile |= use & surface & near
            use &= np.where(surface, geo, True)
            wt = np.where(use, wt, 0.0)
            Hq = np.where(use[..., None], Hq, 0.0)
            sw += wt
            s += wt[..., None] * Hq[..., :3]
            sl += wt * Hq[..., 3]
            kept |= (use.astype(np.uint8) << i).astype(np.uint8)
        fragile |= np.abs(sw - 0.01) < 1e-4
        with np.errstate(all="ignore"):  # ... and a projection on the frame's border (step 7) or on the previous camera's plane (step 4)
            fragile |= border
            fragile |= (pix_cls != NO_HISTORY) & s_ok & (np.abs(l[..., 2]) < 1e-5 * np.maximum(ze, 1.0))
        ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
        V = np.where(ok[..., None], np.stack([fx - xs, fy - ys, sw, np.where(mv, 2.0, 1.0)], -1), 0.0)
    has = sw >= np.float32(0.01)
    sws = np.where(has, sw, 1.0)
    prev = s / sws[..., None]
    ln = sl / sws
    Nn = np.minimum(np.where(fin, ln + 1.0, ln), maxh)
    with np.errstate(all="ignore"):
        a = np.maximum(al, 1.0 / np.where(Nn > 0, Nn, 1.0))
        blended = prev + (np.where(fin[..., None], c[..., :3], 0.0) - prev) * a[..., None]
    H = np.zeros((h, w, 4))
    H[..., :3] = np.where(has[..., None], np.where(fin[..., None], blended, prev), c[..., :3])
    H[..., 3] = np.where(has, Nn, np.where(fin, 1.0, 0.0))
    G = np.concatenate([n, z[..., None]], -1)
    return dict(H=H, G=G, I=I, kept=kept, fragile=fragile, sw=sw, V=V, cls=pix_cls)
