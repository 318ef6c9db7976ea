"""Shared by the temporal anti-aliasing tests (not a test module): the ctypes handle on tests/emu/libtaa_emu.so -- the library's
csrc/pt_taa.h compiled for the host (tests/emu/taa_emu.cpp; a test harness, never a product path), built the way
antilag_util.AntilagEmu builds its library -- and the header's "Temporal anti-aliasing" semantics restated in float32 numpy,
written from include/gpuspectral_pt.h alone.  numpy's float32 + - * / sqrt floor are the IEEE operations the definition names, so
restatement and emulation agree bit for bit.  The restatement takes the constants of the LDR film (2^exposure, scale, invWp2: formed
on the host in double, "LDR film") and the RGBA8 encode of D' (the deterministic log and exp) from the LDR film's own emulation,
display_util.DisplayEmu, which tests/test_display_cpu.py pins."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT
from display_util import DisplayEmu

F32 = np.float32
DEFAULTS = dict(alpha=0.1, sigma_clip=1.0)
CSRC_HEADERS = ("pt_taa.h", "pt_display.h", "pt_denoise.h", "pt_math.h")
SANITIZE = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
            "-Wno-unknown-pragmas", "-Wno-unused-function"]


class TaaEmu:
    def __init__(self):
        from gpuspectral_amd import abi

        d = os.path.join(ROOT, "tests", "emu")
        so = os.path.join(d, "libtaa_emu.so")
        csrc = os.path.join(ROOT, "gpuspectral_amd", "csrc")
        srcs = [os.path.join(d, "taa_emu.cpp"), os.path.join(ROOT, "include", "gpuspectral_pt.h")] + [os.path.join(csrc, n) for n in CSRC_HEADERS]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mfma", "-mavx2", "-shared", "-o", so, srcs[0]])
        L = C.CDLL(so)
        vp, u32 = C.c_void_p, C.c_uint32
        TP, DP = C.POINTER(abi.Taa), C.POINTER(abi.Display)
        L.taa_emu_resolve.argtypes = [TP, vp, C.c_char_p, u32]
        L.taa_emu_run.argtypes = [TP, DP, C.c_int, u32, u32, vp, vp, vp, vp, vp, C.c_char_p, u32]
        self.L, self.abi = L, abi

    @staticmethod
    def _ref(d):
        return C.byref(d) if d is not None else None

    def resolve(self, taa):
        """The library's validation: (dict(alpha, sigma_clip), None) or (None, error text)."""
        out = np.zeros(2, np.float32)
        err = C.create_string_buffer(256)
        if self.L.taa_emu_resolve(self._ref(taa), out.ctypes.data, err, 256):
            return None, err.value.decode()
        return dict(alpha=float(out[0]), sigma_clip=float(out[1])), None

    def step(self, taa, display, src, V, prev=None):
        """One gsp_temporal_taa: the source plane src and the motion plane V, (h, w, 4) float32 each, on the older plane prev (None =
        taa_valid is false).  Returns (D' (h, w, 4) float32, words (h, w) uint32)."""
        src, V = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(V, np.float32)
        h, w = src.shape[:2]
        assert src.shape == V.shape == (h, w, 4)
        if prev is not None:
            prev = np.ascontiguousarray(prev, np.float32)
            assert prev.shape == (h, w, 4)
        D = np.zeros((h, w, 4), np.float32)
        words = np.zeros((h, w), np.uint32)
        err = C.create_string_buffer(256)
        rc = self.L.taa_emu_run(self._ref(taa), self._ref(display), 1 if prev is not None else 0, w, h, src.ctypes.data, V.ctypes.data,
                                prev.ctypes.data if prev is not None else None, D.ctypes.data, words.ctypes.data, err, 256)
        if rc:
            raise ValueError(err.value.decode())
        return D, words


def build_main(exe):
    """tests/emu/taa_main.cpp as a program of its own under AddressSanitizer / UndefinedBehaviorSanitizer."""
    subprocess.check_call(SANITIZE + [os.path.join(ROOT, "tests", "emu", "taa_main.cpp"), "-o", exe])


# ---- the header's "Temporal anti-aliasing" section in float32 numpy ------------------------------------------------------------------
def ycocg(r, g, b):
    """Step 2, float32 arrays."""
    q, hf = F32(0.25), F32(0.5)
    return (q * r + hf * g) + q * b, hf * r - hf * b, (-q * r + hf * g) - q * b


def rgb(y, co, cg):
    t = y - cg
    return t + co, y + cg, t - co


def clamp01(v):
    """Step 4 of "LDR film": v < 1 ? (v > 0 ? v : 0) : 1 -- a NaN becomes 1."""
    with np.errstate(invalid="ignore"):
        return np.where(v < F32(1), np.where(v > F32(0), v, F32(0)), F32(1)).astype(np.float32)


def tone(src, k):
    """Step 1: steps 1-4 of "LDR film" on (..., >= 3) float32 under the constants k (DisplayEmu.consts).  Returns r, g, b float32."""
    src = np.asarray(src, np.float32)
    es = F32(k["exposure_scale"])
    with np.errstate(all="ignore"):
        c = [np.where(src[..., i] > F32(0), src[..., i], F32(0)).astype(np.float32) * es for i in range(3)]
        if k["tonemap"] == 2:  # ACES
            c = [(x * (F32(2.51) * x + F32(0.03))) / (x * (F32(2.43) * x + F32(0.59)) + F32(0.14)) for x in c]
        elif k["tonemap"] == 1:  # REINHARD
            Y = (F32(0.2126) * c[0] + F32(0.7152) * c[1]) + F32(0.0722) * c[2]
            Lp = Y * F32(k["scale"])
            Yp = (Lp * (F32(1) + Lp * F32(k["inv_wp2"]))) / (F32(1) + Lp)
            ratio = Yp / Y
            c = [np.where(Y == F32(0), F32(0), x * ratio).astype(np.float32) for x in c]
    return [clamp01(x) for x in c]


def taa_ref(src, V, prev=None, alpha=0.0, sigma_clip=0.0, display=None, demu=None):
    """One resolve, written from the header: src, V (h, w, 4) float32, prev = the older D plane (None: !taa_valid), display = an
    abi.Display (None = clamp + sRGB), demu = a DisplayEmu.  Returns dict(D (h, w, 4) float32, words (h, w) uint32, history (h, w)
    bool, X, lo, hi, Hc, o (h, w, 3) float32 -- Hc zero where there is no history, o before the final clamp)."""
    from gpuspectral_amd import abi

    demu = demu or DisplayEmu()
    src, V = np.asarray(src, np.float32), np.asarray(V, np.float32)
    h, w = src.shape[:2]
    a = F32(alpha) if alpha else F32(DEFAULTS["alpha"])
    sig = F32(sigma_clip) if sigma_clip else F32(DEFAULTS["sigma_clip"])
    k = demu.consts(display, src)
    X = np.stack(ycocg(*tone(src, k)), -1)  # (h, w, 3)
    # step 3: the box, dy outer and dx inner, pixels inside the frame only
    n = np.zeros((h, w), np.float32)
    s1, s2 = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 3), np.float32)
    ys, xs = np.mgrid[0:h, 0:w]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            qy, qx = ys + dy, xs + dx
            ok = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            Xq = X[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)]
            n = np.where(ok, n + F32(1), n)
            s1 = np.where(ok[..., None], s1 + Xq, s1)
            s2 = np.where(ok[..., None], s2 + Xq * Xq, s2)
    m = s1 / n[..., None]
    sd = np.sqrt(np.maximum(s2 / n[..., None] - m * m, F32(0)))
    lo, hi = m - sig * sd, m + sig * sd
    # step 4: the history through V
    history = np.zeros((h, w), bool)
    Hc = np.zeros((h, w, 3), np.float32)
    if prev is not None:
        prev = np.asarray(prev, np.float32)
        with np.errstate(invalid="ignore"):
            cand = (V[..., 3] != 0) & ~(V[..., 2] < F32(0.01))
            fx, fy = xs.astype(np.float32) + V[..., 0], ys.astype(np.float32) + V[..., 1]
            # (no tap lies inside the frame unless fx is within (-1, W) and fy within (-1, H): also keeps the integer casts defined)
            cand &= (fx > F32(-1)) & (fx < F32(w)) & (fy > F32(-1)) & (fy < F32(h))
        fx, fy = np.where(cand, fx, F32(0)), np.where(cand, fy, F32(0))
        x0, y0 = np.floor(fx), np.floor(fy)
        wx, wy = fx - x0, fy - y0
        one = F32(1)
        weights = [(one - wx) * (one - wy), wx * (one - wy), (one - wx) * wy, wx * wy]
        sw = np.zeros((h, w), np.float32)
        s = np.zeros((h, w, 3), np.float32)
        for i, wt in enumerate(weights):
            qx, qy = x0.astype(np.int64) + (i & 1), y0.astype(np.int64) + (i >> 1)
            keep = cand & (wt != 0) & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            Dq = prev[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1), :3]
            sw = np.where(keep, sw + wt, sw)
            s = np.where(keep[..., None], s + wt[..., None] * Dq, s)
        history = cand & ~(sw < F32(0.01))
        with np.errstate(all="ignore"):
            hh = s / sw[..., None]
        hh = np.where(history[..., None], hh, F32(0)).astype(np.float32)
        Hc = np.stack(ycocg(hh[..., 0], hh[..., 1], hh[..., 2]), -1)
    # steps 5 and 6
    c = np.where(Hc < lo, lo, np.where(Hc > hi, hi, Hc))
    o = X if a == F32(1) else c + (X - c) * a  # (alpha == 1: the frame itself, to the bit)
    pick = np.where(history[..., None], o, X).astype(np.float32)
    D = np.zeros((h, w, 4), np.float32)
    for i, ch in enumerate(rgb(pick[..., 0], pick[..., 1], pick[..., 2])):
        D[..., i] = clamp01(ch)
    D[..., 3] = history
    # step 7: steps 5-6 of "LDR film" on D' -- the LDR film's emulation under CLAMP at exposure 0, whose steps 1-4 leave [0, 1] as it is
    gamma = display.gamma if display is not None else 0.0
    words = demu.map(abi.display(tonemap=0, gamma=gamma, exposure=0.0), D)
    return dict(D=D, words=words, history=history, X=X, lo=lo, hi=hi, Hc=Hc, o=o)
