"""Shared by the temporal anti-lag tests (not a test module): the ctypes handle on tests/emu/libantilag_emu.so -- the library's
csrc/pt_antilag.h compiled for the host (tests/emu/antilag_emu.cpp; a test harness, never a product path), built the way
illum_util.IllumEmu builds its library -- and the header's "Temporal anti-lag" semantics restated in float64 numpy, written from
include/gpuspectral_pt.h alone on top of the restatements of the sections it refers to (temporal_util.temporal64,
motion_util.motion64, illum_util.illum64)."""
import ctypes as C
import os
import subprocess

import numpy as np

import illum_util as iu
import motion_util as mu
import temporal_util as tu
from conftest import ROOT
from motion_util import FHistory

U32 = tu.U32
BACKGROUND = tu.BACKGROUND
DEFAULTS = dict(fast_history=4, radius=2, sigma_scale=2.0)
CSRC_HEADERS = ("pt_antilag.h",) + iu.CSRC_HEADERS
SANITIZE = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
            "-Wno-unknown-pragmas", "-Wno-unused-function"]


class AntilagEmu:
    def __init__(self):
        from gpuspectral_amd import abi

        d = os.path.join(ROOT, "tests", "emu")
        so = os.path.join(d, "libantilag_emu.so")
        csrc = os.path.join(ROOT, "gpuspectral_amd", "csrc")
        srcs = [os.path.join(d, "antilag_emu.cpp"), os.path.join(ROOT, "include", "gpuspectral_pt.h")] + [os.path.join(csrc, n) for n in CSRC_HEADERS]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mfma", "-mavx2", "-shared", "-o", so, srcs[0]])
        L = C.CDLL(so)
        vp, u32 = C.c_void_p, C.c_uint32
        AP, TP, CP = C.POINTER(abi.Antilag), C.POINTER(abi.Temporal), C.POINTER(abi.Camera)
        L.antilag_emu_resolve.argtypes = [AP, vp, C.c_char_p, u32]
        L.antilag_emu_clamp.argtypes = [AP, C.c_float, u32, u32, vp, vp, vp, vp]
        L.antilag_emu_run.argtypes = [AP, TP, CP, CP, C.c_int, C.c_int, u32, u32, C.c_int, C.c_int] + [vp] * 8 + [u32] + [vp] * 4 + [C.c_char_p, u32]
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

    def resolve(self, antilag):
        """The library's validation: (dict(fast_history, radius, sigma_scale), None) or (None, error text)."""
        out = np.zeros(3, np.float32)
        err = C.create_string_buffer(256)
        if self.L.antilag_emu_resolve(self._ref(antilag), out.ctypes.data, err, 256):
            return None, err.value.decode()
        return dict(fast_history=float(out[0]), radius=int(out[1]), sigma_scale=float(out[2])), None

    def clamp(self, antilag, F, G, I, H, normal_min=0.9):
        """Step B alone: H of the newest set (a copy is returned) clamped into the box of F' = F with the set's G and I."""
        F, G, H = (np.ascontiguousarray(p, np.float32) for p in (F, G, H))
        I = np.ascontiguousarray(I, np.uint32)
        h, w = H.shape[:2]
        assert F.shape == G.shape == H.shape == (h, w, 4) and I.shape == (h, w)
        out = H.copy()
        rc = self.L.antilag_emu_clamp(self._ref(antilag), float(np.float32(normal_min)), w, h, F.ctypes.data, G.ctypes.data, I.ctypes.data, out.ctypes.data)
        if rc:
            raise ValueError("antilag_emu_clamp: %d" % rc)
        return out

    def step(self, antilag, temporal, to_world, fov, accum, albedo, geom, ids, new, old=None, fast=None, xforms=None, demod=False):
        """One gsp_temporal_antilag after the gsp_temporal_accumulate that made `new` (an FHistory) from the frame under camera
        (to_world, fov) on `old` (the older set, None = the accumulate had no valid history), under the context state (follow =
        xforms is not None, demod).  fast: F of the older fast plane, None = fast_valid is false.  Returns (F', H clamped)."""
        c = np.ascontiguousarray(accum, np.float32)
        a = np.ascontiguousarray(albedo, np.float32)
        g = np.ascontiguousarray(geom, np.float32)
        i = np.ascontiguousarray(ids, np.uint32)
        h, w = c.shape[:2]
        assert c.shape == a.shape == g.shape == i.shape == (h, w, 4)
        follow = xforms is not None
        cur = self._camera(to_world, fov)
        prev = self._camera(old.to_world, old.fov) if old is not None else None
        tab = np.zeros((0, mu.RECORD_WORDS), np.uint32)
        if old is not None and follow:
            if self._motion is None:
                self._motion = mu.MotionEmu()
            tab = np.ascontiguousarray(self._motion.table(old.xforms, np.ascontiguousarray(xforms, np.float32).reshape(-1, 16)), np.uint32)
        fast_valid = fast is not None and old is not None
        if fast_valid:
            fast = np.ascontiguousarray(fast, np.float32)
            assert fast.shape == (h, w, 4) and old.G.flags.c_contiguous and old.I.flags.c_contiguous
        H = np.ascontiguousarray(new.H, np.float32).copy()
        G, I = np.ascontiguousarray(new.G, np.float32), np.ascontiguousarray(new.I, np.uint32)
        F = np.zeros((h, w, 4), np.float32)
        err = C.create_string_buffer(256)
        rc = self.L.antilag_emu_run(self._ref(antilag), self._ref(temporal), C.byref(cur), C.byref(prev) if prev is not None else None, 1 if old is not None else 0,
                                    1 if fast_valid else 0, w, h, 1 if follow else 0, 1 if demod else 0, c.ctypes.data, a.ctypes.data, g.ctypes.data, i.ctypes.data,
                                    fast.ctypes.data if fast_valid else None, old.G.ctypes.data if fast_valid else None, old.I.ctypes.data if fast_valid else None,
                                    tab.ctypes.data if len(tab) else None, len(tab), H.ctypes.data, G.ctypes.data, I.ctypes.data, F.ctypes.data, err, 256)
        if rc:
            raise ValueError(err.value.decode())
        return F, H


def build_main(exe):
    """tests/emu/antilag_main.cpp as a program of its own under AddressSanitizer / UndefinedBehaviorSanitizer."""
    subprocess.check_call(SANITIZE + [os.path.join(ROOT, "tests", "emu", "antilag_main.cpp"), "-o", exe])


# ---- the header's "Temporal anti-lag" section in float64 numpy -----------------------------------------------------------------------
def fast64(accum, albedo, geom, ids, to_world, fov, old=None, fast=None, xforms=None, demod=False, fast_history=0, **temporal):
    """Step A.  The header says: F' is what the accumulate computed for H' with F of the older fast plane for H, G and I of the older
    set, min(fast_history, max_history) for max_history and history_valid && fast_valid for history_valid -- so this is the
    restatement of the accumulate of the context state, handed a history whose H is F.  Returns its dict (H = F')."""
    cap = min(int(fast_history or DEFAULTS["fast_history"]), int(temporal.get("max_history", 0) or tu.DEFAULTS["max_history"]))
    kw = dict(temporal, max_history=cap)
    follow = xforms is not None
    hist = None
    if old is not None and fast is not None:
        hist = FHistory(np.ascontiguousarray(fast, np.float32), old.G, old.I, None, None, old.to_world, old.fov,
                        old.xforms if follow else np.zeros((0, 16), np.float32))
    if demod:
        return iu.illum64(accum, albedo, geom, ids, to_world, fov, xforms=xforms, hist=hist, **kw)
    if follow:
        return mu.motion64(accum, albedo, geom, ids, to_world, fov, xforms, hist=hist, **kw)
    return tu.temporal64(accum, albedo, geom, ids, to_world, fov, hist=hist, **kw)


def clamp64(F, G, I, H, radius=0, sigma_scale=0.0, normal_min=0.0):
    """Step B on float32 planes in float64.  Returns dict(H (h, w, 4): the clamped history, processed / changed (h, w) bool, n, lo, hi,
    delta (h, w): the bound on |lo32 - lo64| and |hi32 - hi64| derived below, fragile (h, w) bool: a window record's normal test sits
    within 1e-6 of normal_min, so float32 may count another n).

    delta.  With n <= (2 r + 1)^2 records of magnitude <= Fmax (the largest |F'.k| of the window) the float32 sums carry at most
    (n - 1) u of their absolute sum, so m = s1 / n moves by at most n u Fmax, s2 / n by (n + 1) u Fmax^2 and m * m by
    2 Fmax * n u Fmax + u Fmax^2: v by dv = (3 n + 3) u Fmax^2.  |sqrt(a) - sqrt(b)| <= min(sqrt(|a - b|), |a - b| / sqrt(b)), so sd
    moves by at most dsd = min(sqrt(dv), dv / sd) + u sd (sd the smallest of the three channels' in the second form), and
    lo, hi = m -+ sigma sd by delta = (n + 2) u Fmax + sigma (dsd + 3 u sd).  Where float32 and float64
    decide a comparison H < lo differently, H lies within delta of the bound one of them returns: the clamped values differ by at
    most 2 delta either way."""
    F, G, H = (np.asarray(p, np.float32) for p in (F, G, H))
    I = np.asarray(I, np.uint32)
    h, w = H.shape[:2]
    r = int(radius or DEFAULTS["radius"])
    sig = float(np.float32(sigma_scale)) if sigma_scale else DEFAULTS["sigma_scale"]
    nmin = float(np.float32(normal_min)) if normal_min else float(np.float32(tu.DEFAULTS["normal_min"]))
    Fd, Gd, Hd = F.astype(np.float64), G.astype(np.float64), H.astype(np.float64)
    Fok = (F[..., 3] > 0) & np.isfinite(F[..., :3]).all(-1)
    Hok = (H[..., 3] > 0) & np.isfinite(H[..., :3]).all(-1)
    surface = I != BACKGROUND
    pad = lambda p, fill: np.pad(p, [(r, r), (r, r)] + [(0, 0)] * (p.ndim - 2), constant_values=fill)
    Fp, Gp, Ip, okp = pad(np.where(Fok[..., None], Fd[..., :3], 0.0), 0.0), pad(Gd[..., :3], 0.0), pad(I, 0), pad(Fok, False)
    inside = pad(np.ones((h, w), bool), False)
    n = np.zeros((h, w))
    s1, s2, fmax = np.zeros((h, w, 3)), np.zeros((h, w, 3)), np.zeros((h, w))
    fragile = np.zeros((h, w), bool)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            sl = (slice(r + dy, r + dy + h), slice(r + dx, r + dx + w))
            dot = (Gd[..., 0] * Gp[sl][..., 0] + Gd[..., 1] * Gp[sl][..., 1]) + Gd[..., 2] * Gp[sl][..., 2]
            cand = inside[sl] & okp[sl] & (Ip[sl] == I)
            fragile |= cand & surface & (np.abs(dot - nmin) < 1e-6)
            cnt = cand & np.where(surface, dot >= nmin, True)
            n += cnt
            s1 += np.where(cnt[..., None], Fp[sl], 0.0)
            s2 += np.where(cnt[..., None], Fp[sl] * Fp[sl], 0.0)
            fmax = np.maximum(fmax, np.where(cnt, np.abs(Fp[sl]).max(-1), 0.0))
    processed = Hok & Fok & (n >= 2 * r + 1)
    ns = np.where(n > 0, n, 1.0)[..., None]
    m = s1 / ns
    sd = np.sqrt(np.maximum(s2 / ns - m * m, 0.0))
    lo, hi = m - sig * sd, m + sig * sd
    with np.errstate(invalid="ignore"):
        below, above = Hd[..., :3] < lo, Hd[..., :3] > hi
    changed = processed & (below | above).any(-1)
    out = Hd.copy()
    out[..., :3] = np.where(changed[..., None], np.where(below, lo, np.where(above, hi, Hd[..., :3])), Hd[..., :3])
    out[..., 3] = np.where(changed, np.minimum(Hd[..., 3], Fd[..., 3]), Hd[..., 3])
    dv = (3 * n + 3) * U32 * fmax * fmax
    with np.errstate(all="ignore"):
        dsd = np.minimum(np.sqrt(dv), np.where(sd.min(-1) > 0, dv / sd.min(-1), np.inf))
    delta = (n + 2) * U32 * fmax + sig * (dsd + 3 * U32 * sd.max(-1))
    return dict(H=out, processed=processed, changed=changed, n=n, lo=lo, hi=hi, delta=delta, fragile=fragile)
