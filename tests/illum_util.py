"""Shared by the illumination-history tests (not a test module): the ctypes handle on tests/emu/libillum_emu.so -- the library's
csrc/pt_illum.h compiled for the host (tests/emu/illum_emu.cpp; a test harness, never a product path), built the way
motion_util.MotionEmu builds its library -- and the header's "Illumination history" semantics restated in float64 numpy, written
from include/gpuspectral_pt.h alone on top of the restatements of the sections it refers to (temporal_util.temporal64,
motion_util.motion64, svgf_util.svgf64)."""
import ctypes as C
import os
import subprocess

import numpy as np

import motion_util as mu
import svgf_util as su
import temporal_util as tu
from conftest import ROOT
from denoise_util import luma64
from motion_util import FHistory

U32 = tu.U32
FLT_MAX = 3.4028234663852886e38
CSRC_HEADERS = ("pt_illum.h",) + mu.CSRC_HEADERS


class IllumEmu:
    def __init__(self):
        from gpuspectral_amd import abi

        d = os.path.join(ROOT, "tests", "emu")
        so = os.path.join(d, "libillum_emu.so")
        csrc = os.path.join(ROOT, "gpuspectral_amd", "csrc")
        srcs = [os.path.join(d, "illum_emu.cpp"), os.path.join(ROOT, "include", "gpuspectral_pt.h")] + [os.path.join(csrc, n) for n in CSRC_HEADERS]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mfma", "-mavx2", "-shared", "-o", so, srcs[0]])
        L = C.CDLL(so)
        vp, u32 = C.c_void_p, C.c_uint32
        TP, CP, DP, SP = C.POINTER(abi.Temporal), C.POINTER(abi.Camera), C.POINTER(abi.Denoise), C.POINTER(abi.Svgf)
        L.illum_emu_run.argtypes = [TP, CP, CP, C.c_int, u32, u32, C.c_int, C.c_int, C.c_int] + [vp] * 9 + [u32] + [vp] * 5 + [C.c_char_p, u32]
        L.illum_emu_image.argtypes = [vp, vp, C.c_uint64, C.c_int, vp]
        L.illum_emu_image.restype = None
        L.illum_emu_svgf.argtypes = [DP, SP, vp, vp, vp, vp, u32, u32, C.c_int, u32, C.c_int, vp, vp]
        L.illum_emu_denoise.argtypes = [DP, vp, vp, vp, u32, u32, C.c_int, vp]
        self.L, self.abi = L, abi
        self._motion = None

    @staticmethod
    def _ref(d):
        return C.byref(d) if d is not None else None

    def _camera(self, to_world, fov):
        cam = self.abi.Camera()
        for i, v in enumerate(np.asarray(to_world, np.float32).reshape(16)):
            cam.to_world[i] = float(v)
        cam.fov = float(fov)
        return cam

    def step(self, temporal, to_world, fov, accum, albedo, geom, ids, xforms=None, hist=None, moments=False, demod=True):
        """One gsp_temporal_accumulate under the context state (moments, follow = xforms is not None, demod): the frame under camera
        (to_world, fov) on `hist` (an FHistory, None = no valid history).  Returns the new FHistory (M, V = None where not kept)."""
        c = np.ascontiguousarray(accum, np.float32)
        a = np.ascontiguousarray(albedo, np.float32)
        g = np.ascontiguousarray(geom, np.float32)
        i = np.ascontiguousarray(ids, np.uint32)
        h, w = c.shape[:2]
        assert c.shape == a.shape == g.shape == i.shape == (h, w, 4)
        follow = xforms is not None
        xf = np.ascontiguousarray(xforms, np.float32).reshape(-1, 16) if follow else np.zeros((0, 16), np.float32)
        H, G, M, V = (np.zeros((h, w, 4), np.float32) for _ in range(4))
        I = np.zeros((h, w), np.uint32)
        cur = self._camera(to_world, fov)
        prev = self._camera(hist.to_world, hist.fov) if hist is not None else None
        tab = np.zeros((0, mu.RECORD_WORDS), np.uint32)
        if hist is not None:
            assert hist.H.shape == (h, w, 4) and all(p.flags.c_contiguous for p in (hist.H, hist.G, hist.I))
            assert not moments or hist.M is not None
            if follow:
                if self._motion is None:
                    self._motion = mu.MotionEmu()
                tab = np.ascontiguousarray(self._motion.table(hist.xforms, xf), np.uint32)
        prevs = (hist.H.ctypes.data, hist.G.ctypes.data, hist.I.ctypes.data, hist.M.ctypes.data if moments else None) if hist is not None else (None,) * 4
        err = C.create_string_buffer(256)
        rc = self.L.illum_emu_run(self._ref(temporal), C.byref(cur), C.byref(prev) if prev is not None else None, 1 if hist is not None else 0, w, h,
                                  1 if moments else 0, 1 if follow else 0, 1 if demod else 0, c.ctypes.data, a.ctypes.data, g.ctypes.data, i.ctypes.data, *prevs,
                                  tab.ctypes.data if len(tab) else None, len(tab), H.ctypes.data, G.ctypes.data, I.ctypes.data, M.ctypes.data, V.ctypes.data,
                                  err, 256)
        if rc:
            raise ValueError(err.value.decode())
        return FHistory(H, G, I, M if moments else None, V if follow else None, to_world, fov, xf)

    def image(self, H, albedo, demod=True):
        """gsp_download_temporal_image of the history H under this frame's albedo plane."""
        H = np.ascontiguousarray(H, np.float32)
        a = np.ascontiguousarray(albedo, np.float32)
        assert H.shape == a.shape and H.shape[-1] == 4
        out = np.zeros_like(H)
        self.L.illum_emu_image(H.ctypes.data, a.ctypes.data, H.size // 4, 1 if demod else 0, out.ctypes.data)
        return out

    def svgf(self, denoise, svgf, H, M, albedo, geom, demod=True, levels=None):
        """gsp_download_temporal_svgf (levels None: returns out) or gsp_temporal_svgf_feedback (returns (out, H after the feedback))."""
        H, M, a, g = (np.ascontiguousarray(p, np.float32) for p in (H, M, albedo, geom))
        h, w = H.shape[:2]
        assert H.shape == M.shape == a.shape == g.shape == (h, w, 4)
        out, fb = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
        rc = self.L.illum_emu_svgf(self._ref(denoise), self._ref(svgf), H.ctypes.data, M.ctypes.data, a.ctypes.data, g.ctypes.data, w, h, 1 if demod else 0,
                                   levels or 0, 0 if levels is None else 1, out.ctypes.data, fb.ctypes.data)
        if rc:
            raise ValueError("illum_emu_svgf: %d" % rc)
        return out if levels is None else (out, fb)

    def denoise(self, denoise, H, albedo, geom, demod=True):
        """gsp_download_temporal_denoised of the history H."""
        H, a, g = (np.ascontiguousarray(p, np.float32) for p in (H, albedo, geom))
        h, w = H.shape[:2]
        out = np.zeros((h, w, 4), np.float32)
        assert self.L.illum_emu_denoise(self._ref(denoise), H.ctypes.data, a.ctypes.data, g.ctypes.data, w, h, 1 if demod else 0, out.ctypes.data) == 0
        return out


# ---- the header's "Illumination history" section in float64 numpy ------------------------------------------------------------------
def albedo64(albedo):
    """(a' (h, w, 3), A = max(a', 0.01)) of "Denoiser: Prepare" in float64."""
    alb = np.asarray(albedo, np.float32).astype(np.float64)
    ap = alb[..., :3] + (1.0 - alb[..., 3:4])
    return ap, np.where(ap < 0.01, 0.01, ap)


def frame64(accum, albedo):
    """Demodulation: dict(e (h, w, 3) float64, u (h, w) bool, L (h, w), fragile (h, w) bool: the floor of A or the overflow of the
    quotient sits within rounding of its threshold)."""
    c32 = np.asarray(accum, np.float32)
    c = c32.astype(np.float64)
    ap, A = albedo64(albedo)
    fin = np.isfinite(c32[..., :3]).all(-1)
    with np.errstate(all="ignore"):
        e = c[..., :3] / A
        u = fin & (np.abs(e) <= FLT_MAX).all(-1)
        near_max = fin & ((np.abs(e) > FLT_MAX * (1 - 1e-6)) & (np.abs(e) < FLT_MAX * (1 + 1e-6))).any(-1)
    fragile = (np.abs(ap - 0.01) < 1e-7).any(-1) | near_max
    return dict(e=e, u=u, L=luma64(np.where(u[..., None], e, 0.0)), fragile=fragile, A=A)


def illum64(accum, albedo, geom, ids, to_world, fov, xforms=None, hist=None, moments=False, **temporal):
    """A demodulated gsp_temporal_accumulate.  The header says: the sections "Temporal accumulation: Blend", "1. Moments" and "moved
    instances" apply as written with u for "c finite" and e.k for c.k -- so the frame handed to their restatements is e where u and
    NaN where not (e rounded to float32, the format those restatements read: one rounding of the up to three the float32 evaluation
    of e makes, counted in the caller's bound), and what they return is the answer but for the one case the header words
    differently: without history and not u, H' is the raw record {c.rgb, 0}.  Returns their dict with M (moments) and `fragile`
    widened by frame64's; `e`, `u` of the frame beside it."""
    f = frame64(accum, albedo)
    c32 = np.asarray(accum, np.float32)
    h, w = f["u"].shape
    sur = np.full((h, w, 4), np.nan, np.float32)
    with np.errstate(all="ignore"):
        sur[..., :3] = np.where(f["u"][..., None], f["e"], np.nan).astype(np.float32)
    sur[..., 3] = c32[..., 3]
    follow = xforms is not None

    def reproject(frame, hst):
        if follow:
            return mu.motion64(frame, albedo, geom, ids, to_world, fov, xforms, hist=hst, **temporal)
        return tu.temporal64(frame, albedo, geom, ids, to_world, fov, hist=hst, **temporal)

    r = reproject(sur, hist)
    has = r["sw"] >= np.float32(0.01) if hist is not None else np.zeros((h, w), bool)
    raw = ~has & ~f["u"]
    r["H"][..., :3] = np.where(raw[..., None], c32[..., :3].astype(np.float64), r["H"][..., :3])
    assert np.all(r["H"][..., 3][raw] == 0.0) and np.all(r["H"][..., 3][~has & f["u"]] == 1.0)
    r["fragile"] = r["fragile"] | f["fragile"]
    r["e"], r["u"] = f["e"], f["u"]
    if moments:
        # "1. Moments" as svgf_util.moments64 restates it: M pulled through the same reprojection as the colour of a history whose
        # new frame is not finite, the blend weight from the real call's N
        l = np.where(f["u"], f["L"], 0.0)
        M = np.zeros((h, w, 4))
        M[..., 0], M[..., 1], M[..., 2] = l, l * l, 1.0
        M[~f["u"], :2] = 0.0
        if hist is not None:
            fake = FHistory(np.concatenate([hist.M[..., :3], hist.H[..., 3:4]], -1).astype(np.float32), hist.G, hist.I, None, None, hist.to_world, hist.fov,
                            hist.xforms if follow else np.zeros((0, 16), np.float32))
            p = reproject(np.full((h, w, 4), np.nan, np.float32), fake)
            assert np.array_equal(p["sw"] >= np.float32(0.01), has)
            prev = p["H"][..., :3]
            al = float(np.float32(temporal.get("alpha", 0.0) or tu.DEFAULTS["alpha"]))
            with np.errstate(all="ignore"):
                a = np.maximum(al, 1.0 / np.where(r["H"][..., 3] > 0, r["H"][..., 3], 1.0))
            blended = np.stack([prev[..., 0] + (l - prev[..., 0]) * a, prev[..., 1] + (l * l - prev[..., 1]) * a, (1 - a) * (1 - a) * prev[..., 2] + a * a], -1)
            M[..., :3] = np.where(has[..., None], np.where(f["u"][..., None], blended, prev), M[..., :3])
        r["M"] = M
    return r


def image64(H, albedo):
    """The image read-out of a demodulated history: H.k * A_k where H.len > 0, H as stored where H.len == 0; float64."""
    Hd = np.asarray(H, np.float32).astype(np.float64)
    _, A = albedo64(albedo)
    out = Hd.copy()
    with np.errstate(all="ignore"):
        out[..., :3] = np.where((Hd[..., 3] > 0)[..., None], Hd[..., :3] * A, Hd[..., :3])
    return out


def svgf_demod64(H, M, albedo, geom, levels=None, **params):
    """The variance-guided filter of a demodulated history, and (levels) its feedback.  In exact arithmetic Prepare of the demodulated
    H -- e = H.rgb -- is Prepare of the modulated history {H.rgb * A, len} -- e = (H.rgb * A) / A -- and everything after Prepare is
    unchanged, so this is svgf_util.svgf64 of that history.  svgf64 reads float32 planes: the product is rounded once, which moves
    its e by at most u |e| from the e the float32 evaluation holds exactly -- the u |e| svgf64's running bound already starts from
    (there: the rounding of c / A).  Returns svgf64's dict of the full filter (out = e_final * A, err) and, with levels,
    fb = dict(e, err): e_after of level levels - 1 with its bound, per pixel."""
    Hd = np.asarray(H, np.float32)
    _, A = albedo64(albedo)
    mod = Hd.copy()
    with np.errstate(all="ignore"):
        mod[..., :3] = (Hd[..., :3].astype(np.float64) * A).astype(np.float32)
    r = su.svgf64(mod, M, albedo, geom, **params)
    if levels is not None:
        p = dict(params, iterations=levels)
        q = su.svgf64(mod, M, albedo, geom, **p)
        # q.err = dE * max_k A_k + u max_k |out_k| per pixel, dE svgf64's bound on |e32 - e64| of every channel: so dE <= q.err / max_k A_k
        r["fb"] = dict(e=q["e"], err=q["err"] / A.max(-1), out=q["out"], out_err=q["err"])
    r["valid"] = np.isfinite(Hd[..., :3]).all(-1)
    return r
