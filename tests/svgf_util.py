"""Shared by the variance-guided-filter tests (not a test module): the ctypes handle on tests/emu/libsvgf_emu.so -- the library's
csrc/pt_svgf.h compiled for the host (tests/emu/svgf_emu.cpp; a test harness, never a product path), built the way
temporal_util.TemporalEmu builds its library -- and the header's "Variance-guided filter" semantics restated in float64 numpy,
written from include/gpuspectral_pt.h alone.  The restatement of the filter carries a running first-order error bound of the
float32 evaluation beside every value (see svgf64)."""
import ctypes as C
import os
import subprocess

import numpy as np

import temporal_util as tu
from conftest import ROOT
from denoise_util import DEFAULT_ITERATIONS, DEFAULT_SIGMAS, KERNEL, inv_sigma2, luma64

INF = float("inf")
U32 = 2.0 ** -24  # unit roundoff of float32
DEFAULT_MIN_HISTORY = 4
DEFAULT_SIGMA_VARIANCE = 4.0
TENT = np.array([0.25, 0.5, 0.25])
EXP_CUT = 87.33654475  # det_expf returns 0 below -87.34


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


class MHistory(tu.History):
    """A history set with its moments plane M = {m1, m2, r, 0}."""

    def __init__(self, H, G, I, M, to_world, fov):
        super().__init__(H, G, I, to_world, fov)
        self.M = M


class SvgfEmu:
    def __init__(self):
        from gpuspectral_amd import abi

        d = os.path.join(ROOT, "tests", "emu")
        so = os.path.join(d, "libsvgf_emu.so")
        csrc = os.path.join(ROOT, "gpuspectral_amd", "csrc")
        srcs = [os.path.join(d, "svgf_emu.cpp"), os.path.join(ROOT, "include", "gpuspectral_pt.h")] + [
            os.path.join(csrc, n) for n in ("pt_svgf.h", "pt_temporal.h", "pt_denoise.h", "pt_display.h", "pt_math.h", "pt_stages.h", "pt_shading.h", "pt_trace.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mfma", "-mavx2", "-shared", "-o", so, srcs[0]])
        L = C.CDLL(so)
        vp, u32 = C.c_void_p, C.c_uint32
        DP, SP, TP, CP = C.POINTER(abi.Denoise), C.POINTER(abi.Svgf), C.POINTER(abi.Temporal), C.POINTER(abi.Camera)
        L.svgf_emu_resolve.argtypes = [DP, SP, vp, C.c_char_p, u32]
        L.svgf_emu_accumulate.argtypes = [TP, CP, CP, C.c_int, u32, u32] + [vp] * 12 + [C.c_char_p, u32]
        L.svgf_emu_run.argtypes = [DP, SP, vp, vp, vp, vp, u32, u32, vp, vp, vp]
        L.svgf_emu_level.argtypes = [DP, SP, u32, vp, vp, vp, vp, u32, u32, vp, vp]
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

    def resolve(self, denoise, svgf):
        """The library's validation: (dict(iterations, inv_sn2, inv_sz2, inv_sa2, min_history, sigma_v, lum_on), None) or (None, text)."""
        out = np.zeros(7, np.uint32)
        err = C.create_string_buffer(256)
        if self.L.svgf_emu_resolve(self._ref(denoise), self._ref(svgf), out.ctypes.data, err, 256):
            return None, err.value.decode()
        f = out.view(np.float32)
        return dict(iterations=int(out[0]), inv_sn2=f[1], inv_sz2=f[2], inv_sa2=f[3], min_history=f[4], sigma_v=f[5], lum_on=int(out[6])), None

    def step(self, temporal, to_world, fov, accum, albedo, geom, ids, hist=None):
        """One gsp_temporal_accumulate with tracking on: TemporalEmu.step with the moments; `hist` is an MHistory or None."""
        c = np.ascontiguousarray(accum, np.float32)
        a = np.ascontiguousarray(albedo, np.float32)
        g = np.ascontiguousarray(geom, np.float32)
        i = np.ascontiguousarray(ids, np.uint32)
        h, w = c.shape[:2]
        assert c.shape == a.shape == g.shape == i.shape == (h, w, 4)
        H, G, M = (np.zeros((h, w, 4), np.float32) for _ in range(3))
        I = np.zeros((h, w), np.uint32)
        cur = self._camera(to_world, fov)
        prev = self._camera(hist.to_world, hist.fov) if hist is not None else None
        if hist is not None:
            assert hist.H.shape == (h, w, 4) and all(p.flags.c_contiguous for p in (hist.H, hist.G, hist.I, hist.M))
        ptr = lambda p: p.ctypes.data if hist is not None else None
        err = C.create_string_buffer(256)
        rc = self.L.svgf_emu_accumulate(self._ref(temporal), C.byref(cur), C.byref(prev) if prev is not None else None, 1 if hist is not None else 0, w, h,
                                        c.ctypes.data, a.ctypes.data, g.ctypes.data, i.ctypes.data,
                                        *((ptr(hist.H), ptr(hist.G), ptr(hist.I), ptr(hist.M)) if hist is not None else (None,) * 4),
                                        H.ctypes.data, G.ctypes.data, I.ctypes.data, M.ctypes.data, err, 256)
        if rc:
            raise ValueError(err.value.decode())
        return MHistory(H, G, I, M, to_world, fov)

    def run(self, denoise, svgf, hist_h, moments, albedo, geom, with_variance=False):
        """gsp_download_temporal_svgf of a history given as (h, w, 4) float32 planes (and, with_variance, the initial variance and
        the input variance of the last level, (h, w) float32 each)."""
        H = np.ascontiguousarray(hist_h, np.float32)
        M = np.ascontiguousarray(moments, np.float32)
        a = np.ascontiguousarray(albedo, np.float32)
        g = np.ascontiguousarray(geom, np.float32)
        h, w = H.shape[:2]
        assert H.shape == M.shape == a.shape == g.shape == (h, w, 4)
        out = np.zeros((h, w, 4), np.float32)
        v0, v = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
        assert self.L.svgf_emu_run(self._ref(denoise), self._ref(svgf), H.ctypes.data, M.ctypes.data, a.ctypes.data, g.ctypes.data, w, h, out.ctypes.data,
                                   v0.ctypes.data, v.ctypes.data) == 0
        return (out, v0, v) if with_variance else out

    def level(self, denoise, svgf, level, E, A, G, V):
        """One level on planes given as they are: (E', V')."""
        E, A, G = (np.ascontiguousarray(p, np.float32) for p in (E, A, G))
        V = np.ascontiguousarray(V, np.float32)
        h, w = V.shape
        assert E.shape == A.shape == G.shape == (h, w, 4)
        e2, v2 = np.zeros((h, w, 4), np.float32), np.zeros((h, w), np.float32)
        assert self.L.svgf_emu_level(self._ref(denoise), self._ref(svgf), level, E.ctypes.data, A.ctypes.data, G.ctypes.data, V.ctypes.data, w, h,
                                     e2.ctypes.data, v2.ctypes.data) == 0
        return e2, v2


# ---- the header's "Variance-guided filter" section in float64 numpy -------------------------------------------------------------
def frame_luminance64(accum, albedo):
    """l of a frame: L of "Denoiser: Prepare" on (c, albedo)."""
    c = np.asarray(accum, np.float32).astype(np.float64)
    alb = np.asarray(albedo, np.float32).astype(np.float64)
    ap = alb[..., :3] + (1.0 - alb[..., 3:4])
    with np.errstate(all="ignore"):
        return luma64(c[..., :3] / np.where(ap < 0.01, 0.01, ap))


def moments64(accum, albedo, geom, ids, to_world, fov, hist=None, **temporal):
    """Section 1 of the header.  The reprojection is temporal_util.temporal64's: M is pulled through it as the colour of a history
    whose new frame is not finite (H' = prev then), the blend weight a follows from the real call's N.  Returns temporal64's dict
    of the real call with M (h, w, 4) float64 added."""
    r = tu.temporal64(accum, albedo, geom, ids, to_world, fov, hist=hist, **temporal)
    fin = np.isfinite(np.asarray(accum, np.float32)[..., :3]).all(-1)
    l = np.where(fin, frame_luminance64(accum, albedo), 0.0)
    h, w = fin.shape
    M = np.zeros((h, w, 4))
    M[..., 0], M[..., 1], M[..., 2] = l, l * l, 1.0
    M[~fin, :2] = 0.0
    if hist is not None:
        fake = tu.History(np.concatenate([hist.M[..., :3], hist.H[..., 3:4]], -1).astype(np.float32), hist.G, hist.I, hist.to_world, hist.fov)
        nan = np.full((h, w, 4), np.nan, np.float32)
        p = tu.temporal64(nan, albedo, geom, ids, to_world, fov, hist=fake, **temporal)
        has = p["sw"] >= np.float32(0.01)
        assert np.array_equal(has, r["sw"] >= np.float32(0.01))
        prev = p["H"][..., :3]
        al = float(np.float32(temporal.get("alpha", 0.0) or tu.DEFAULTS["alpha"]))
        with np.errstate(all="ignore"):
            a = np.maximum(al, 1.0 / np.where(r["H"][..., 3] > 0, r["H"][..., 3], 1.0))
        blended = np.stack([prev[..., 0] + (l - prev[..., 0]) * a, prev[..., 1] + (l * l - prev[..., 1]) * a,
                            (1 - a) * (1 - a) * prev[..., 2] + a * a], -1)
        M[..., :3] = np.where(has[..., None], np.where(fin[..., None], blended, prev), M[..., :3])
    r["M"] = M
    return r


def _shifted(h, w, oy, ox):
    """Slices (P, Q): centres P whose tap P + (oy, ox) = Q lies inside the frame; None when there are none."""
    y0, y1 = max(0, -oy), min(h, h - oy)
    x0, x1 = max(0, -ox), min(w, w - ox)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def svgf64(hist_h, moments, albedo, geom, iterations=0, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0, min_history=0, sigma_variance=0.0):
    """Section 2 of the header in float64 numpy on the float32 planes H, M, albedo, geom.  Returns dict(out (h, w, 4), V0 (h, w),
    temporal (h, w) bool: the pixel took the temporal estimate, err (h, w): a bound on |float32 evaluation - out| per channel).

    The error bound is a running first-order analysis (u = 2^-24; every float32 operation is within u relative, det_expf within
    4 u): every quantity q carries dq >= |q32 - q64|.
      * prepare: e = c / A is one rounding, L three products and two sums of them.
      * V0, temporal: m2 - m1*m1 cancels, so its absolute error is 2 u (m2 + m1^2); max(., 0) is 1-Lipschitz; the ratio adds 3 u.
      * V0, spatial: a weight g = exp(-xg) carries g (8 u xg + 6 u) (xg: <= 8 roundings of non-negative terms); the three sums
        carry their terms' errors plus 49 roundings; m = s1 / sg and s2 / sg - m^2 propagate by the quotient and product rules
        (sg >= 1: the centre tap).
      * a level: Vg is a convex combination (error: that of its V_q, plus 11 u).  sqrt is monotone, so inv_l lies between its
        values at Vg - dVg (floored at 0) and Vg + dVg.  x carries 8 u of its guide part, the luminance term
        inv_l_max (dL_p + dL_q) + |dL| d(inv_l) + 3 u of itself; w = h exp(-x) then carries w (expm1(dx) + 6 u) and never more than
        h.  The centre tap has x = 0 and w = h exactly.  The sums add 25 roundings of non-negative terms (|e_q| in sum_k).
        The quotients propagate with the denominator sum_w - d(sum_w) >= 9/64."""
    Hh = np.asarray(hist_h, np.float32)
    c = Hh.astype(np.float64)
    M = np.asarray(moments, np.float32).astype(np.float64)
    alb = np.asarray(albedo, np.float32).astype(np.float64)
    g = np.asarray(geom, np.float32).astype(np.float64)
    h, w = c.shape[:2]
    n_it = iterations or DEFAULT_ITERATIONS
    isn = inv_sigma2(sigma_normal, DEFAULT_SIGMAS["sigma_normal"])
    isz = inv_sigma2(sigma_depth, DEFAULT_SIGMAS["sigma_depth"])
    isa = inv_sigma2(sigma_albedo, DEFAULT_SIGMAS["sigma_albedo"])
    minh = float(min_history or DEFAULT_MIN_HISTORY)
    sv = float(np.float32(sigma_variance)) if sigma_variance else DEFAULT_SIGMA_VARIANCE
    lum_on = not np.isinf(sv)
    u = U32
    valid = np.isfinite(Hh[..., :3]).all(-1)
    ap = alb[..., :3] + (1.0 - alb[..., 3:4])
    A = np.where(ap < 0.01, 0.01, ap)
    with np.errstate(all="ignore"):
        e = np.where(valid[..., None], c[..., :3] / A, 0.0)
    dE = u * np.abs(e).max(-1)
    nrm, z = g[..., :3], g[..., 3]

    def lum(e, dE):
        return luma64(e), dE + 3 * u * luma64(np.abs(e))

    def guides(P, Q):
        dn = ((nrm[P] - nrm[Q]) ** 2).sum(-1)
        with np.errstate(all="ignore"):
            rz = np.where(z[P] == z[Q], 0.0, (z[P] - z[Q]) / np.where(z[P] == z[Q], 1.0, z[P] + z[Q]))
        return dn * isn + rz * rz * isz

    def expw(x):
        with np.errstate(all="ignore"):
            return np.where(x > EXP_CUT, 0.0, np.exp(-x))

    L, dL = lum(e, dE)
    # ---- initial variance ----
    m1, m2, r = M[..., 0], M[..., 1], M[..., 2]
    temporal = valid & (c[..., 3] >= minh) & (r < 1.0)
    with np.errstate(all="ignore"):
        ratio = np.where(temporal, r / np.where(temporal, 1.0 - r, 1.0), 0.0)
        d = m2 - m1 * m1
        Vt = np.maximum(d, 0.0) * ratio
        dVt = (2 * u * (np.abs(m2) + m1 * m1) + 3 * u * np.abs(d)) * ratio
    sg, s1, s2 = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w))
    dsg, ds1, ds2, s1a = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w))
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            s = _shifted(h, w, dy, dx)
            if s is None:
                continue
            P, Q = s
            xg = guides(P, Q)
            gq = np.where(valid[Q], expw(xg), 0.0)
            dg = gq * (8 * u * xg + 6 * u)
            Lq, dLq = L[Q], dL[Q]
            sg[P] += gq
            s1[P] += gq * Lq
            s2[P] += gq * Lq * Lq
            s1a[P] += gq * np.abs(Lq)
            dsg[P] += dg
            ds1[P] += dg * np.abs(Lq) + gq * dLq + u * gq * np.abs(Lq)
            ds2[P] += dg * Lq * Lq + gq * (2 * np.abs(Lq) * dLq + 2 * u * Lq * Lq)
    dsg += 49 * u * sg
    ds1 += 49 * u * s1a
    ds2 += 49 * u * s2
    sgs = np.where(valid, sg, 1.0)
    den = np.maximum(sgs - dsg, 0.5)
    m = s1 / sgs
    q2 = s2 / sgs
    dm = (ds1 + np.abs(m) * dsg) / den + u * np.abs(m)
    dq2 = (ds2 + q2 * dsg) / den + u * q2
    Vs = np.maximum(q2 - m * m, 0.0)
    dVs = dq2 + 2 * np.abs(m) * dm + dm * dm + 2 * u * (q2 + m * m)
    V = np.where(valid, np.where(temporal, Vt, Vs), 0.0)
    dV = np.where(valid, np.where(temporal, dVt, dVs), 0.0)
    V0 = V.copy()
    # ---- levels ----
    for level in range(n_it):
        s = 1 << level
        inv_l = np.zeros((h, w))
        inv_hi = np.zeros((h, w))
        d_inv = np.zeros((h, w))
        if lum_on:
            st, sv_, dsv = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w))
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    sh = _shifted(h, w, dy, dx)
                    if sh is None:
                        continue
                    P, Q = sh
                    t = np.where(valid[Q], TENT[dx + 1] * TENT[dy + 1], 0.0)
                    st[P] += t
                    sv_[P] += t * V[Q]
                    dsv[P] += t * dV[Q]
            sts = np.where(valid, st, 1.0)
            Vg = sv_ / sts
            dVg = dsv / sts + 11 * u * Vg
            with np.errstate(all="ignore"):
                inv_l = 1.0 / (sv * np.sqrt(Vg) + 1e-4)
                inv_hi = 1.0 / (sv * np.sqrt(np.maximum(Vg - dVg, 0.0)) * (1 - 4 * u) + 1e-4) * (1 + 4 * u)
                inv_lo = 1.0 / (sv * np.sqrt(Vg + dVg) * (1 + 4 * u) + 1e-4) * (1 - 4 * u)
            d_inv = np.maximum(inv_hi - inv_l, inv_l - inv_lo)
        sw, sk, sq, ska = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w))
        taps = []
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                sh = _shifted(h, w, s * dy, s * dx)
                if sh is None:
                    continue
                P, Q = sh
                hk = KERNEL[dx + 2] * KERNEL[dy + 2]
                xg = guides(P, Q) + ((ap[P] - ap[Q]) ** 2).sum(-1) * isa
                dl = np.abs(L[P] - L[Q])
                with np.errstate(all="ignore"):
                    xl = np.where(dl > 0, dl * inv_l[P], 0.0)
                    dx_ = 10 * u * xg + inv_hi[P] * (dL[P] + dL[Q]) + dl * d_inv[P] + 3 * u * xl
                    wq = np.where(valid[Q], hk * expw(xg + xl), 0.0)
                    dw = np.where(valid[Q], np.minimum(wq * (np.expm1(np.minimum(dx_, 50.0)) + 6 * u) + 1e-37, hk), 0.0)
                if dy == 0 and dx == 0:
                    dw = np.zeros_like(dw)
                sw[P] += wq
                sk[P] += wq[..., None] * e[Q]
                sq[P] += wq * wq * V[Q]
                ska[P] += wq * np.abs(e[Q]).max(-1)
                taps.append((P, Q, wq, dw))
        sws = np.where(valid, sw, 1.0)
        with np.errstate(all="ignore"):
            e2 = sk / sws[..., None]
            V2 = sq / (sws * sws)
        # second pass: a perturbed weight moves a quotient by its distance from the quotient -- exactly,
        #   sum (w + dw) e_q / sum (w + dw) - e' = sum dw (e_q - e') / sum (w + dw)
        dsw, dek, dvk, din_e, din_v = (np.zeros((h, w)) for _ in range(5))
        for P, Q, wq, dw in taps:
            dsw[P] += dw
            dek[P] += dw * np.abs(e[Q] - e2[P]).max(-1)
            dvk[P] += dw * (np.abs(2 * wq * V[Q] - 2 * sws[P] * V2[P]) + dw * V[Q])
            din_e[P] += wq * dE[Q]
            din_v[P] += wq * wq * dV[Q]
        den = np.maximum(sws - dsw, 9.0 / 64.0)
        e2a = np.abs(e2).max(-1)
        with np.errstate(all="ignore"):
            # + the inputs' own errors (a convex combination) + 25 products and 24 additions per sum, the division, on |e| <= ska / sw
            dE2 = dek / den + din_e / sws + 28 * u * (ska / sws + e2a)
            # V' = N / S^2:  (N + dN) / (S + dS)^2 - N / S^2 = (sum dw ((2 w + dw) V_q - 2 S V') - V' dS^2) / (S + dS)^2
            dV2 = (dvk + V2 * dsw * dsw + din_v) / (den * den) + 60 * u * V2
        e = np.where(valid[..., None], e2, e)
        dE = np.where(valid, dE2, dE)
        V = np.where(valid, V2, V)
        dV = np.where(valid, dV2, dV)
        L, dL = lum(e, dE)
    out = c.copy()
    out[..., :3] = np.where(valid[..., None], e * A, c[..., :3])
    err = np.where(valid, dE * A.max(-1) + u * np.abs(out[..., :3]).max(-1), 0.0)
    return dict(out=out, V0=V0, V=V, temporal=temporal, err=err, e=e)
