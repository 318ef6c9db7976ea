"""Shared by the LDR-film tests (not a test module): the ctypes handle on tests/emu/libdisplay_emu.so -- the library's
csrc/pt_display.h compiled for the host (tests/emu/display_emu.cpp; a test harness, never a product path), built the way
lens_util.LensEmu builds its library -- and the header's "LDR film" semantics restated in float64 numpy."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np

from conftest import ROOT

TONEMAPS = {"clamp": 0, "reinhard": 1, "aces": 2}
GAMMAS = {"gamma2.2": 2.2, "srgb": 0.0}
EXPOSURES = (-2.0, 0.0, 1.5)
# every tonemap x {gamma 2.2, sRGB} x exposure {-2, 0, +1.5}
COMBOS = list(itertools.product(TONEMAPS, GAMMAS, EXPOSURES))


def combo_display(abi, tonemap, gamma, exposure, **kw):
    return abi.display(tonemap=TONEMAPS[tonemap], gamma=GAMMAS[gamma], exposure=exposure, **kw)


class DisplayEmu:
    def __init__(self):
        from gpuspectral_amd import abi

        d = os.path.join(ROOT, "tests", "emu")
        so = os.path.join(d, "libdisplay_emu.so")
        csrc = os.path.join(ROOT, "gpuspectral_amd", "csrc")
        srcs = [os.path.join(d, "display_emu.cpp"), os.path.join(ROOT, "include", "gpuspectral_pt.h"), os.path.join(csrc, "pt_display.h"),
                os.path.join(csrc, "pt_math.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mfma", "-mavx2", "-shared", "-o", so, srcs[0]])
        L = C.CDLL(so)
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        DP = C.POINTER(abi.Display)
        L.display_emu_resolve.argtypes = [DP, DP, C.c_char_p, u32]
        L.display_emu_stats.argtypes = [vp, u64, C.POINTER(abi.Luminance)]
        L.display_emu_stats.restype = None
        L.display_emu_combine.argtypes = [C.c_int64, u64, C.c_float, C.POINTER(abi.Luminance)]
        L.display_emu_combine.restype = None
        L.display_emu_consts.argtypes = [DP, vp, u64, vp]
        L.display_emu_map.argtypes = [DP, vp, u64, vp]
        L.display_emu_reinhard_luma.argtypes = [DP, vp, u64, C.c_float]
        L.display_emu_reinhard_luma.restype = C.c_float
        self.L, self.abi = L, abi

    @staticmethod
    def _ref(display):
        return C.byref(display) if display is not None else None

    def resolve(self, display):
        """The library's validation: (stored abi.Display, None) or (None, error text)."""
        out = self.abi.Display()
        err = C.create_string_buffer(256)
        rc = self.L.display_emu_resolve(self._ref(display), C.byref(out), err, 256)
        return (None, err.value.decode()) if rc else (out, None)

    def stats(self, rgba):
        rgba = np.ascontiguousarray(rgba, np.float32).reshape(-1, 4)
        out = self.abi.Luminance()
        self.L.display_emu_stats(rgba.ctypes.data, len(rgba), C.byref(out))
        return out.as_dict()

    def combine(self, log_sum, pixels, mx):
        out = self.abi.Luminance()
        self.L.display_emu_combine(int(log_sum), int(pixels), float(mx), C.byref(out))
        return out.as_dict()

    def consts(self, display, rgba):
        rgba = np.ascontiguousarray(rgba, np.float32).reshape(-1, 4)
        out = np.zeros(6, np.uint32)
        assert self.L.display_emu_consts(self._ref(display), rgba.ctypes.data, len(rgba), out.ctypes.data) == 0
        f = out.view(np.float32)
        return dict(tonemap=int(out[0]), srgb=int(out[1]), exposure_scale=f[2], inv_gamma=f[3], scale=f[4], inv_wp2=f[5])

    def map(self, display, rgba):
        """gsp_download_display of a buffer of RGBA32F records: uint32 RGBA8 words of the same leading shape."""
        a = np.ascontiguousarray(rgba, np.float32)
        flat = a.reshape(-1, 4)
        out = np.zeros(len(flat), np.uint32)
        assert self.L.display_emu_map(self._ref(display), flat.ctypes.data, len(flat), out.ctypes.data) == 0
        return out.reshape(a.shape[:-1])

    def reinhard_luma(self, display, rgba, Y):
        rgba = np.ascontiguousarray(rgba, np.float32).reshape(-1, 4)
        return float(self.L.display_emu_reinhard_luma(self._ref(display), rgba.ctypes.data, len(rgba), float(Y)))


def luma64(rgb):
    return 0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1] + 0.0722 * rgb[..., 2]


def stats64(rgba):
    """(Lavg, Lmax, n) of the header's frame statistics in float64, WITHOUT the 2^-20 quantisation."""
    a = np.asarray(rgba, np.float32).reshape(-1, 4)[:, :3]
    ok = np.isfinite(a).all(1)
    c = np.maximum(a[ok].astype(np.float64), 0.0)
    Y = luma64(c)
    ok2 = np.isfinite(Y)
    Y = Y[ok2]
    if len(Y) == 0:
        return 0.0, 0.0, 0
    return float(np.exp(np.mean(np.log(Y + 1e-3)))), float(Y.max()), len(Y)


def bytes64(rgba, tonemap, gamma, exposure, key=0.0, burn=0.0, lavg=None, lmax=None):
    """The header's per-pixel steps 1-6 in float64 (finite input): (..., 3) uint8.  lavg / lmax: the statistics to use (Reinhard)."""
    a = np.asarray(rgba, np.float32)[..., :3].astype(np.float64)
    c = np.where(np.isnan(a) | (a < 0), 0.0, a) * 2.0 ** exposure
    if tonemap == 2:
        c = (c * (2.51 * c + 0.03)) / (c * (2.43 * c + 0.59) + 0.14)
    elif tonemap == 1:
        Y = luma64(c)
        scale, inv_wp2 = 1.0, 0.0
        if lavg is not None and lavg > 0 and lmax > 0:
            scale = (key if key else 0.18) / lavg
            b = min(max(1.0 - burn, 1e-8), 1.0)
            inv_wp2 = 1.0 / ((lmax * scale) ** 2 * b ** 4)
        Lp = Y * scale
        Yp = Lp * (1.0 + Lp * inv_wp2) / (1.0 + Lp)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(Y > 0, Yp / np.where(Y > 0, Y, 1.0), 0.0)
        c = c * ratio[..., None]
    v = np.clip(c, 0.0, 1.0)
    if gamma > 0:
        e = v ** (1.0 / gamma)
    else:
        e = np.where(v <= 0.0031308, 12.92 * v, 1.055 * v ** (1.0 / 2.4) - 0.055)
    return np.floor(e * 255.0 + 0.5).astype(np.uint8)


def unpack(words):
    """uint32 RGBA8 words -> (..., 4) uint8."""
    w = np.asarray(words, np.uint32)
    return np.stack([(w >> s) & 0xFF for s in (0, 8, 16, 24)], -1).astype(np.uint8)
