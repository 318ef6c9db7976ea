"""Shared by the denoiser tests (not a test module): the ctypes handle on tests/emu/libdenoise_emu.so -- the library's
csrc/pt_denoise.h compiled for the host (tests/emu/denoise_emu.cpp; a test harness, never a product path), built the way
display_util.DisplayEmu builds its library -- and the header's "Denoiser" semantics restated in float64 numpy, written from
include/gpuspectral_pt.h alone."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT

INF = float("inf")
DEFAULT_SIGMAS = dict(sigma_color=0.5, sigma_normal=0.3, sigma_depth=0.05, sigma_albedo=0.1)
DEFAULT_ITERATIONS = 5
KERNEL = np.array([0.0625, 0.25, 0.375, 0.25, 0.0625])
EPS32 = 2.0 ** -24  # unit roundoff of float32


class DenoiseEmu:
    def __init__(self):
        from gpuspectral_amd import abi

        d = os.path.join(ROOT, "tests", "emu")
        so = os.path.join(d, "libdenoise_emu.so")
        csrc = os.path.join(ROOT, "gpuspectral_amd", "csrc")
        srcs = [os.path.join(d, "denoise_emu.cpp"), os.path.join(ROOT, "include", "gpuspectral_pt.h"), os.path.join(csrc, "pt_denoise.h"),
                os.path.join(csrc, "pt_display.h"), os.path.join(csrc, "pt_math.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mfma", "-mavx2", "-shared", "-o", so, srcs[0]])
        L = C.CDLL(so)
        vp, u32 = C.c_void_p, C.c_uint32
        DP = C.POINTER(abi.Denoise)
        L.denoise_emu_resolve.argtypes = [DP, vp, C.c_char_p, u32]
        L.denoise_emu_run.argtypes = [DP, vp, vp, vp, u32, u32, vp]
        self.L, self.abi = L, abi

    @staticmethod
    def _ref(d):
        return C.byref(d) if d is not None else None

    def resolve(self, denoise):
        """The library's validation: (dict(iterations, inv_sc2, inv_sn2, inv_sz2, inv_sa2), None) or (None, error text)."""
        out = np.zeros(5, np.uint32)
        err = C.create_string_buffer(256)
        if self.L.denoise_emu_resolve(self._ref(denoise), out.ctypes.data, err, 256):
            return None, err.value.decode()
        f = out.view(np.float32)
        return dict(iterations=int(out[0]), inv_sc2=f[1], inv_sn2=f[2], inv_sz2=f[3], inv_sa2=f[4]), None

    def run(self, denoise, accum, albedo, geom):
        """gsp_download_denoised of a frame given as (h, w, 4) float32 planes."""
        c = np.ascontiguousarray(accum, np.float32)
        a = np.ascontiguousarray(albedo, np.float32)
        g = np.ascontiguousarray(geom, np.float32)
        h, w = c.shape[:2]
        assert c.shape == a.shape == g.shape == (h, w, 4)
        out = np.zeros((h, w, 4), np.float32)
        assert self.L.denoise_emu_run(self._ref(denoise), c.ctypes.data, a.ctypes.data, g.ctypes.data, w, h, out.ctypes.data) == 0
        return out


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def luma64(e):
    return (0.2126 * e[..., 0] + 0.7152 * e[..., 1]) + 0.0722 * e[..., 2]


def inv_sigma2(sigma, default):
    """1 / sigma^2 as the header forms it: in double, rounded to float32; 0 = the default, +Inf = the term is off."""
    s = default if sigma == 0 else sigma
    return 0.0 if np.isinf(s) else float(np.float32(min(1.0 / (float(s) * float(s)), 3.402823466e38)))


def denoise64(accum, albedo, geom, iterations=0, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0):
    """The header's "Denoiser" section in float64 numpy: (h, w, 4) float64.  Inputs are the float32 planes."""
    c = np.asarray(accum, np.float32).astype(np.float64)
    alb = np.asarray(albedo, np.float32).astype(np.float64)
    g = np.asarray(geom, np.float32).astype(np.float64)
    h, w = c.shape[:2]
    n_it = iterations or DEFAULT_ITERATIONS
    isc = inv_sigma2(sigma_color, DEFAULT_SIGMAS["sigma_color"])
    isn = inv_sigma2(sigma_normal, DEFAULT_SIGMAS["sigma_normal"])
    isz = inv_sigma2(sigma_depth, DEFAULT_SIGMAS["sigma_depth"])
    isa = inv_sigma2(sigma_albedo, DEFAULT_SIGMAS["sigma_albedo"])
    valid = np.isfinite(np.asarray(accum, np.float32)[..., :3]).all(-1)
    ap = alb[..., :3] + (1.0 - alb[..., 3:4])
    A = np.where(ap < 0.01, 0.01, ap)
    with np.errstate(all="ignore"):
        e = np.where(valid[..., None], c[..., :3] / A, 0.0)
    nrm, z = g[..., :3], g[..., 3]
    for level in range(n_it):
        s = 1 << level
        L = luma64(e)
        sw = np.zeros((h, w))
        sk = np.zeros((h, w, 3))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = s * dy, s * dx
                # centres [y0:y1, x0:x1] whose tap (y + oy, x + ox) lies inside the frame
                y0, y1 = max(0, -oy), min(h, h - oy)
                x0, x1 = max(0, -ox), min(w, w - ox)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                dn = ((nrm[P] - nrm[Q]) ** 2).sum(-1)
                with np.errstate(all="ignore"):
                    rz = np.where(z[P] == z[Q], 0.0, (z[P] - z[Q]) / np.where(z[P] == z[Q], 1.0, z[P] + z[Q]))
                da = ((ap[P] - ap[Q]) ** 2).sum(-1)
                rl = (L[P] - L[Q]) / ((L[P] + L[Q]) + 1e-3)
                x = dn * isn + rz * rz * isz + da * isa + rl * rl * (isc * 4.0 ** level)
                with np.errstate(all="ignore"):
                    wgt = KERNEL[dx + 2] * KERNEL[dy + 2] * np.where(x > 87.33654475, 0.0, np.exp(-x))
                wgt = np.where(valid[Q], wgt, 0.0)
                sw[P] += wgt
                sk[P] += wgt[..., None] * e[Q]
        with np.errstate(all="ignore"):
            e = np.where(valid[..., None], sk / np.where(valid, sw, 1.0)[..., None], e)
    out = c.copy()
    out[..., :3] = np.where(valid[..., None], e * A, c[..., :3])
    return out


def random_guides(rng, h, w, regions=4):
    """Piecewise-constant guides with noise: albedo {rgb, cov}, geom {unit normal, depth}; a band of misses at the top."""
    ys, xs = np.mgrid[0:h, 0:w]
    lab = ((xs * regions) // max(w, 1) + 2 * ((ys * 2) // max(h, 1))) % (regions + 1)
    pal_a = rng.uniform(0.05, 0.95, (regions + 1, 3))
    pal_n = rng.normal(size=(regions + 1, 3))
    pal_n /= np.linalg.norm(pal_n, axis=1, keepdims=True)
    pal_z = rng.uniform(1.0, 9.0, regions + 1)
    albedo = np.zeros((h, w, 4), np.float32)
    geom = np.zeros((h, w, 4), np.float32)
    albedo[..., :3] = pal_a[lab] + rng.normal(0, 0.01, (h, w, 3))
    albedo[..., 3] = 1.0
    n = pal_n[lab] + rng.normal(0, 0.02, (h, w, 3))
    geom[..., :3] = n / np.linalg.norm(n, axis=-1, keepdims=True)
    geom[..., 3] = pal_z[lab] * (1.0 + rng.normal(0, 0.002, (h, w)))
    miss = ys < max(1, h // 8)
    albedo[miss] = 0.0
    geom[miss] = 0.0
    return albedo, geom
