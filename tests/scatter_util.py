"""Shared by the scattering-media tests (not a test module): the ctypes handle on tests/emu/libscatter_emu.so -- the product's stage
headers with shade_vertex<.., MED, .., SCT = true>, compiled for the host (tests/emu/scatter_emu.cpp; a test harness, never a product
path) -- built the way MediaEmu (media_util.py) builds its library; the scenes of the tests; the furnace; and the header's
"Scattering media" formulas restated in numpy / float64."""
import copy
import ctypes as C
import hashlib
import math
import os
import re
import shutil
import subprocess

import numpy as np

import media_util as mu
from conftest import ROOT

REFERENCE, TEXTBOOK = 0, 1
UNIFORM, POWER = 0, 1
EPS = 2.0 ** -24  # half an ulp of float32, relative: the error of one correctly rounded operation

# the scene of the GPU == emulation tests: the tinted materials scene with a scattering medium on the glass sphere
SIGMA_A = (1.0, 3.0, 5.0)
SIGMA_S = (2.0, 4.0, 8.0)
G = 0.6

FURNACE_L = 1.0
FURNACE_HALF = 8.0  # half extent of the emitter box: it holds the slab and the camera of slab_scene


class ScatterEmu:
    def __init__(self):
        from gpuspectral_amd import abi

        d = os.path.join(ROOT, "tests", "emu")
        so = os.path.join(d, "libscatter_emu.so")
        srcs = [os.path.join(d, f) for f in ("scatter_emu.cpp", "pt_emu.cpp")] + [os.path.join(ROOT, "include", "gpuspectral_pt.h")]
        csrc = os.path.join(ROOT, "gpuspectral_amd", "csrc")
        srcs += [os.path.join(csrc, h) for h in os.listdir(csrc) if h.endswith(".h")]
        srcs += [os.path.join(ROOT, "tests", "devfn", h) for h in ("devfn_bodies.h", "medium_bodies.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mfma", "-mavx2", "-shared", "-o", so, srcs[0]])
        L = C.CDLL(so)
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        SP = C.POINTER(abi.MediumScatter)
        L.emu_create.restype = vp
        L.emu_create.argtypes = [C.POINTER(abi.SceneDesc)]
        L.emu_destroy.argtypes = [vp]
        L.scatter_emu_check.argtypes = [SP, u32, u32, C.c_char_p, u32]
        L.scatter_emu_sample_hg.argtypes = [u64, vp, vp, vp, vp, vp]
        L.scatter_emu_sample_hg.restype = None
        L.scatter_emu_hg_pdf.argtypes = [u64, vp, vp, vp]
        L.scatter_emu_hg_pdf.restype = None
        L.scatter_emu_medium_event.argtypes = [u64, vp, vp, vp, vp, vp, vp, vp]
        L.scatter_emu_medium_event.restype = None
        L.scatter_emu_render.argtypes = [vp, u32, u32, vp, u64, C.POINTER(abi.RenderParams), u32, u32, vp, C.POINTER(abi.Medium), SP, u32, vp, vp, vp, vp]
        self.L, self.abi = L, abi

    def check(self, scatter, have, count=None):
        """gsp_set_media_scattering's validation against a context of `have` media: None, or the error text."""
        arr = self.abi.media_scatter_array(scatter)
        err = C.create_string_buffer(256)
        rc = self.L.scatter_emu_check(arr, (len(arr) if arr is not None else 0) if count is None else count, have, err, 256)
        return err.value.decode() if rc else None

    # ---- pt_medium.h, one function at a time (float32 arrays in; words out, as the device harness returns them) ----
    def sample_hg(self, d, g, u1, u2):
        return _sample_hg(self.L.scatter_emu_sample_hg, d, g, u1, u2)

    def hg_pdf(self, g, cos_theta):
        return _hg_pdf(self.L.scatter_emu_hg_pdf, g, cos_theta)

    def medium_event(self, sigma_a, sigma_s, t, u_c, u_d, weight):
        return _medium_event(self.L.scatter_emu_medium_event, sigma_a, sigma_s, t, u_c, u_d, weight)

    def scene(self, sc):
        return ScatterEmuScene(self, sc)


class ScatterEmuScene:
    def __init__(self, emu, sc):
        self.emu, self.sc = emu, sc
        self._desc = sc.desc()
        self.h = emu.L.emu_create(C.byref(self._desc))

    def render(self, width, height, spp, media=None, scatter=None, first_timestamp=0, log=False, accum=None, estimator=REFERENCE, light_mode=UNIFORM,
               pixel_ids=None, **params):
        """(accum[n,4], {extension_rays, shadow_rays, shaded_vertices, medium_events, samples}[, back-face log: one byte per pixel, bit 0 =
        a medium's back face, bit 1 = a scatterer's; events: uint32[n, spp] medium events per sample]); params: fields of gsp_render_params."""
        abi = self.emu.abi
        p = abi.default_render_params()
        p.spp, p.first_timestamp = spp, first_timestamp
        for k, v in params.items():
            setattr(p, k, v)
        ids = None if pixel_ids is None else np.ascontiguousarray(pixel_ids, np.uint32)
        n = width * height if ids is None else len(ids)
        accum = np.zeros((n, 4), np.float32) if accum is None else np.ascontiguousarray(accum, np.float32).copy()
        counts = np.zeros(5, np.uint64)
        back = np.zeros(n, np.uint8)
        events = np.zeros((n, spp), np.uint32)
        arr, sarr = abi.media_array(media), abi.media_scatter_array(scatter)
        assert sarr is None or (arr is not None and len(sarr) == len(arr))
        lt = np.ascontiguousarray(self.sc.lights, abi.LIGHT_DT)
        rc = self.emu.L.scatter_emu_render(self.h, width, height, None if ids is None else ids.ctypes.data, n, C.byref(p), estimator, light_mode, lt.ctypes.data, arr, sarr,
                                           len(arr) if arr is not None else 0, accum.ctypes.data, counts.ctypes.data, back.ctypes.data if log else None,
                                           events.ctypes.data if log else None)
        if rc != 0:
            raise ValueError("scatter_emu_render returned %d" % rc)
        st = dict(extension_rays=int(counts[0]), shadow_rays=int(counts[1]), shaded_vertices=int(counts[2]), medium_events=int(counts[3]),
                  samples=int(counts[4]))
        return (accum, st, back, events) if log else (accum, st)

    def __del__(self):
        try:
            self.emu.L.emu_destroy(self.h)
        except Exception:
            pass


same = mu.same


# ---- the device functions: one calling protocol for the host compile (ScatterEmu) and the device harness (MediumDevice) ----------
def _f32(*arrays):
    return [np.ascontiguousarray(a, np.float32) for a in arrays]


def _call(fn, n, arrays, out):
    rc = fn(n, *[a.ctypes.data for a in arrays], out.ctypes.data)
    if rc not in (0, None):
        raise RuntimeError("pt_medium.h harness returned %d" % rc)
    return out


def _sample_hg(fn, d, g, u1, u2):
    """-> (direction float32[n,3], pdf float32[n])"""
    d, g, u1, u2 = _f32(d, g, u1, u2)
    assert d.shape == (len(g), 3) and len(u1) == len(u2) == len(g)
    out = _call(fn, len(g), (d, g, u1, u2), np.zeros((len(g), 4), np.float32))
    return out[:, :3].copy(), out[:, 3].copy()


def _hg_pdf(fn, g, cos_theta):
    g, c = _f32(g, cos_theta)
    assert len(g) == len(c)
    return _call(fn, len(g), (g, c), np.zeros(len(g), np.float32))


def _medium_event(fn, sigma_a, sigma_s, t, u_c, u_d, weight):
    """-> float32[n, 6]: scatter (0 / 1), valid (0 / 1), s, w.r, w.g, w.b"""
    a = _f32(sigma_a, sigma_s, t, u_c, u_d, weight)
    n = len(a[2])
    assert a[0].shape == a[1].shape == a[5].shape == (n, 3) and len(a[3]) == len(a[4]) == n
    return _call(fn, n, a, np.zeros((n, 6), np.float32))


DEVFN_DIR = os.path.join(ROOT, "tests", "devfn")
DEVFN_LIB = os.path.join(DEVFN_DIR, "libmedium_devfn.so")
_CSRC = os.path.join(ROOT, "gpuspectral_amd", "csrc")
# (the order of tests/devfn/medium.mk)
DEVFN_DIGEST_SOURCES = tuple(os.path.join(DEVFN_DIR, f) for f in ("medium_devfn.hip", "medium_bodies.h", "devfn_bodies.h")) + tuple(
    os.path.join(_CSRC, f) for f in ("pt_medium.h", "pt_math.h", "pt_shading.h", "pt_trace.h", "pt_stages.h")) + (os.path.join(ROOT, "include", "gpuspectral_pt.h"),)


def devfn_source_digest():
    h = hashlib.sha256()
    for f in DEVFN_DIGEST_SOURCES:
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def devfn_stamped_digest(path=DEVFN_LIB):
    if not os.path.exists(path):
        return None
    with open(path, "rb") as fh:
        m = re.search(rb"arch=(\S+) digest=([0-9a-f]{16}) flags=([^\0]*)\0", fh.read())
    return None if m is None else m.group(2).decode()


def devfn_ensure_built():
    """The path of a device harness that carries the digest of the tree's sources; builds it with hipcc if it has to, raises if it
    cannot (the GPU tests never skip over it)."""
    if devfn_stamped_digest() == devfn_source_digest():
        return DEVFN_LIB
    if shutil.which("hipcc") is None:
        raise RuntimeError("%s is missing or stale and hipcc is not on the path: build it with `make -C tests/devfn -f medium.mk` (build() does)" % DEVFN_LIB)
    subprocess.check_call(["make", "-B", "-C", DEVFN_DIR, "-f", "medium.mk"])
    if devfn_stamped_digest() != devfn_source_digest():
        raise RuntimeError("make -C tests/devfn -f medium.mk left a library without the digest of the tree's sources")
    return DEVFN_LIB


class MediumDevice:
    """tests/devfn/libmedium_devfn.so: the bodies of medium_bodies.h on the GPU, one thread per vector."""

    def __init__(self):
        self.L = C.CDLL(devfn_ensure_built())
        vp, u64 = C.c_void_p, C.c_uint64
        self.L.medium_devfn_sample_hg.argtypes = [u64, vp, vp, vp, vp, vp]
        self.L.medium_devfn_hg_pdf.argtypes = [u64, vp, vp, vp]
        self.L.medium_devfn_medium_event.argtypes = [u64, vp, vp, vp, vp, vp, vp, vp]

    def sample_hg(self, d, g, u1, u2):
        return _sample_hg(self.L.medium_devfn_sample_hg, d, g, u1, u2)

    def hg_pdf(self, g, cos_theta):
        return _hg_pdf(self.L.medium_devfn_hg_pdf, g, cos_theta)

    def medium_event(self, sigma_a, sigma_s, t, u_c, u_d, weight):
        return _medium_event(self.L.medium_devfn_medium_event, sigma_a, sigma_s, t, u_c, u_d, weight)


# ---- the vectors of the device-function tests (CPU and GPU share them) ---------------------------------------------------------------
HG_GS = (-0.9, -0.3, 0.0, 1e-4, 0.3, 0.9)
HG_GRID = (400, 250)  # strata in u1 x u2: 1e5 samples per g


def hg_vectors(g, seed=3):
    """1e5 stratified (u1, u2) for one g, jittered inside their strata, about a fixed oblique unit direction."""
    rng = np.random.RandomState(seed)
    n1, n2 = HG_GRID
    i, j = np.meshgrid(np.arange(n1), np.arange(n2), indexing="ij")
    u1 = np.minimum(((i + rng.uniform(size=i.shape)) / n1).ravel().astype(np.float32), np.float32(1.0 - 2.0 ** -24))
    u2 = np.minimum(((j + rng.uniform(size=j.shape)) / n2).ravel().astype(np.float32), np.float32(1.0 - 2.0 ** -24))
    d = np.float64([0.3, -0.5, 0.81])
    d = (d / np.linalg.norm(d)).astype(np.float32)
    return np.tile(d, (len(u1), 1)), np.full(len(u1), g, np.float32), u1, u2


def event_vectors(n=20000, seed=11):
    """Random (sigma_a, sigma_s, t, u_c, u_d, weight) with the edge cases in front: sigma_t = 0 in one or all channels, t = 0, and
    sigma_t * t so large that exp underflows."""
    rng = np.random.RandomState(seed)
    sa = (rng.uniform(0.0, 4.0, (n, 3)) * (rng.uniform(size=(n, 3)) < 0.8)).astype(np.float32)
    ss = (rng.uniform(0.0, 8.0, (n, 3)) * (rng.uniform(size=(n, 3)) < 0.8)).astype(np.float32)
    t = (10.0 ** rng.uniform(-3.0, 1.0, n)).astype(np.float32)
    u_c = rng.uniform(size=n).astype(np.float32)
    u_d = np.minimum(rng.uniform(size=n).astype(np.float32), np.float32(1.0 - 2.0 ** -24))
    w = rng.uniform(0.0, 2.0, (n, 3)).astype(np.float32)
    k = n // 10
    sa[:k], ss[:k] = 0.0, 0.0  # sigma_t = 0 in every channel: always the surface, w = weight
    ss[k:2 * k, 0], sa[k:2 * k, 0] = 0.0, 0.0  # ... in one channel
    ss[k:2 * k, 1] = np.maximum(ss[k:2 * k, 1], 0.5)
    t[2 * k:3 * k] = 0.0  # t = 0: always the surface
    t[3 * k:4 * k] = 1e4  # huge sigma_t * t: the transmittances underflow
    ss[3 * k:4 * k] = np.maximum(ss[3 * k:4 * k], 1.0)
    u_d[3 * k:3 * k + k // 2] = np.float32(1.0 - 2.0 ** -24)  # ... with the longest free path float32 can draw
    sa[5 * k:6 * k], ss[5 * k:6 * k] = np.float32([1e-3, 300.0, 50.0]), np.float32([1e-3, 700.0, 50.0])  # surface events through channel 0
    t[5 * k:6 * k] = 1.0                                                                                  # ... whose other two channels underflow
    u_c[5 * k:6 * k] = np.minimum(u_c[5 * k:6 * k], np.float32(0.33))
    u_c[4 * k:4 * k + 8] = np.float32([0.0, 1.0 / 3.0, 0.33333334, 2.0 / 3.0, 0.6666667, 0.99999994, 0.5, 0.3333333])
    u_d[4 * k + 8:4 * k + 12] = np.float32([0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24])
    return sa, ss, t, u_c, u_d, w


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def two_glass_scene(materials_scene):
    """cornell_materials with a second glass sphere (the rough-plastic sphere takes the dielectric's handle): medium 1 on the first,
    medium 2 on the second."""
    glass = int(mu.glass_instances(materials_scene)[0])
    sc = copy.copy(materials_scene)
    sc.instances = materials_scene.instances.copy()
    second = glass + 1  # (cornell_materials adds the rough-plastic sphere straight behind the glass one)
    sc.instances["bsdf"][second] = sc.instances["bsdf"][glass]
    sc.instances["twofaced"][second] = sc.instances["twofaced"][glass]
    return mu.with_medium(mu.with_medium(sc, [glass], 1), [second], 2), glass, second


def inward_box_mesh():
    """box_mesh turned inside out: winding reversed and normals negated, so every face looks at the centre."""
    from gpuspectral_amd import scenes

    pos, nrm = scenes.box_mesh()
    pos = np.asarray(pos, np.float32).reshape(-1, 3, 3)[:, [0, 2, 1], :].reshape(-1, 3)
    nrm = -np.asarray(nrm, np.float32).reshape(-1, 3, 3)[:, [0, 2, 1], :].reshape(-1, 3)
    return pos, nrm


def furnace_scene(medium=1, L=FURNACE_L):
    """The furnace: a closed box of one-sided emitters of radiance L that face inward (reflectance 0), the camera of slab_scene
    inside it, the index-matched dielectric box of slab_scene in the middle, carrying medium `medium`."""
    from gpuspectral_amd import scenes

    b = scenes.SceneBuilder()
    walls = b.add_mesh(*inward_box_mesh())
    box = b.add_mesh(*scenes.box_mesh())
    b.add_object(walls, scenes.trs((0, 0, 0), FURNACE_HALF), b.diffuse((0, 0, 0)), twofaced=False, emission=(L, L, L))
    b.add_object(box, scenes.trs((0, 0, 0), mu.SLAB_HALF), b.dielectric(1.0, 1.0), twofaced=False)
    b.camera_lookat((0, 0, mu.SLAB_EYE_Z), (0, 0, 0), fov_deg=mu.SLAB_FOV_DEG)
    sc = b.build()
    return mu.with_medium(sc, [1], medium) if medium else sc


FURNACE_PARAMS = dict(max_depth=250, rr_start_depth=250, clamp=1e30)


def slab_cos(width, height):
    """cos of the angle between the pixel's ray and the view axis (the recipe of slab_reference), float64[h*w]"""
    fov = float(np.float32(np.float64(np.float32(mu.SLAB_FOV_DEG)) * math.pi / 180.0))
    zplane = (max(width, height) / 2.0) / math.tan(fov / 2.0)
    y, x = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    vx, vy = (x - width / 2.0).ravel(), (y - height / 2.0).ravel()
    return zplane / np.sqrt(vx * vx + vy * vy + zplane * zplane)


# ---- the header's formulas in float64 -------------------------------------------------------------------------------------------
def hg_pdf_ref(g, c):
    g, c = np.asarray(g, np.float64), np.asarray(c, np.float64)
    d = 1.0 + g * g - 2.0 * g * c
    return np.where(np.abs(g) < 1e-3, 1.0 / (4.0 * math.pi), (1.0 - g * g) / (4.0 * math.pi * d ** 1.5))


def hg_cos_ref(g, u1):
    g, u1 = np.asarray(g, np.float64), np.asarray(u1, np.float64)
    gs = np.where(np.abs(g) < 1e-3, 1.0, g)
    sq = (1.0 - gs * gs) / (1.0 - gs + 2.0 * gs * u1)
    return np.where(np.abs(g) < 1e-3, 1.0 - 2.0 * u1, np.clip((1.0 + gs * gs - sq * sq) / (2.0 * gs), -1.0, 1.0))


def hg_cos_bound(g, u1):
    """Absolute rounding bound of hg_cos in float32 against hg_cos_ref, operation by operation (half-ulp EPS each, first order):
    den = (1 - g) + (2 g) u1 cancels for u1 near 1 (g < 0) or 0 (g > 0), and B = (1 + g^2) - sq^2 cancels near cos = 0; the bound
    follows both.  Isotropic form: 1 - 2 u1, two roundings of values <= 2."""
    g, u1 = np.asarray(g, np.float64), np.asarray(u1, np.float64)
    gs = np.where(np.abs(g) < 1e-3, 0.5, g)
    den = (1.0 - gs) + 2.0 * gs * u1
    e_den = EPS * (np.abs(1.0 - gs) + 2.0 * np.abs(2.0 * gs * u1) + np.abs(den))
    num = 1.0 - gs * gs
    r_sq = e_den / np.abs(den) + EPS * (gs * gs + np.abs(num)) / np.abs(num) + EPS
    sq2 = (num / den) ** 2
    A = 1.0 + gs * gs
    e_B = EPS * (gs * gs + A) + sq2 * (2.0 * r_sq + EPS) + EPS * np.abs(A - sq2)
    e_cos = e_B / np.abs(2.0 * gs) + EPS * np.abs((A - sq2) / (2.0 * gs))
    return np.where(np.abs(g) < 1e-3, 4.0 * EPS, e_cos)


def hg_pdf_bound(g, c):
    """Relative rounding bound of hg_pdf in float32 against hg_pdf_ref at the same float32 (g, c): d = (1 + g^2) - (2 g) c cancels
    towards the peak (d -> (1 - |g|)^2); d sqrt(d) carries 1.5 of d's relative error."""
    g, c = np.asarray(g, np.float64), np.asarray(c, np.float64)
    d = 1.0 + g * g - 2.0 * g * c
    r_d = EPS * (g * g + (1.0 + g * g) + 2.0 * np.abs(2.0 * g * c) + np.abs(d)) / np.abs(d)
    num = 1.0 - g * g
    r = 1.5 * r_d + 2.0 * EPS + 2.0 * EPS + EPS * (g * g + np.abs(num)) / np.abs(num) + EPS  # d sqrt(d); 4 pi and its product; 1 - g^2; the division
    return np.where(np.abs(g) < 1e-3, 2.0 * EPS, r)


def medium_event_ref(sigma_a, sigma_s, t, u_c, u_d, weight):
    """float64 restatement of the free-path decision on float32 inputs -> (scatter, valid, s, w[n,3], x[n,3] = sigma_t * distance, the
    exponents; terms[n,3] = the summands of p).  sigma_t = sigma_a + sigma_s and 1 - u_d are single float32 operations on the inputs
    and are taken as such (their rounding is part of the rule, not an error of it); everything behind them is float64."""
    sa, ss, w = (np.asarray(x, np.float32).astype(np.float64) for x in (sigma_a, sigma_s, weight))
    t = np.asarray(t, np.float32).astype(np.float64)
    one_minus = (np.float32(1.0) - np.asarray(u_d, np.float32)).astype(np.float64)
    st = (np.asarray(sigma_a, np.float32) + np.asarray(sigma_s, np.float32)).astype(np.float64)
    c = np.minimum((np.asarray(u_c, np.float32) * np.float32(3.0)).astype(np.uint32), 2)
    stc = st[np.arange(len(t)), c]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        s = np.where(stc == 0.0, np.inf, -np.log(one_minus) / np.where(stc == 0.0, 1.0, stc))
        scatter = s < t
        dist = np.where(scatter, s, t)
        x = st * dist[:, None]
        Tr = np.exp(-x)
        terms = np.where(scatter[:, None], st * Tr, Tr)
        p = terms.sum(1) / 3.0
        wout = np.where(scatter[:, None], w * ss * Tr, w * Tr) / p[:, None]
    return scatter, np.isfinite(p) & (p != 0.0), s, wout, x, terms


# ---- the furnace's checks, on a frame wherever it was rendered (the emulation or the GPU) ------------------------------------------------
FURNACE_MAX_EVENTS = 50


def furnace_bound(events, spp=1, rr=False):
    """Relative rounding bound of a furnace sample whose path had `events` medium events, in units of 1: per medium event 7 half-ulps
    (numerator (weight * sigma_s) * Tr: 2, p: three products, two sums and / 3 folded as 4 on a sum of positive terms, the division: 1),
    per surface event 5 (weight * Tr: 1, p: 3, the division: 1), per boundary crossing 8 (the index-matched dielectric's f * NoW /
    pdf and the entry piece's exp and product), 2 per vertex under Russian roulette (the division by q twice rounded), 3 per sample
    of the running mean.  A path crosses the box once (two crossings, one surface event); it is convex and the walls are black."""
    return ((7 + (2 if rr else 0)) * events + 5 + 16 + (6 if rr else 0) + 3 * spp) * EPS


def check_furnace_white(img, spp, rr=False):
    """(a) grey, albedo 1: every pixel is L.  The issue's figure, 250 * 2^-23 relative, is the bound asserted; by furnace_bound it
    covers paths of up to FURNACE_MAX_EVENTS medium events (9 * 50 + 33 = 483 half-ulps < 500 = 250 * 2^-23 / 2^-24 with roulette on), and the
    CPU test asserts from the emulation's log that no path here has more."""
    assert furnace_bound(FURNACE_MAX_EVENTS, spp, rr) <= 250 * 2.0 ** -23
    rel = np.abs(img[:, :3].astype(np.float64) / FURNACE_L - 1.0)
    print("white furnace: largest relative deviation from L %.3g = %.1f half-ulps (bound %.3g)" % (rel.max(), rel.max() / EPS, 250 * 2.0 ** -23))
    assert rel.max() <= 250 * 2.0 ** -23


def check_furnace_half(frames, n, sigma_a, sigma_t, albedo, timestamps):
    """(b) grey, albedo a, 1 spp per frame, frame i rendered with first_timestamp = timestamps[i] on an empty frame.  Every sample of a pixel that slab_reference classes inside or outside is
    L * a^k * E, k an integer, E = exp(-sigma_a * 1e-4 / cos_i) the entry piece of "Interior media" (rule 5 keeps its absorption
    over the 1e-4 offset: it is part of the rule, 1e-4 relative here, and known per pixel; E = 1 outside), to furnace_bound(k).
    The share of k = 0 among the inside samples is the free-path law: the mean of exp(-sigma_t * (d - 1e-4) / cos_i) -- the traced
    segment is the slab less the offset -- within 5 binomial standard deviations.  -> k per frame."""
    _, inside, outside = mu.slab_reference(n, n)
    left_out = (~(inside | outside)).mean()
    assert left_out <= 0.08  # (what tests/test_gpu_media.py accepts of slab_reference on the same frame size today)
    cos = slab_cos(n, n)
    E = np.where(inside, np.exp(-sigma_a * 1e-4 / cos), 1.0)
    d = 2.0 * mu.SLAB_HALF[2]
    ks, hits, total = [], 0, 0
    for img, ts in zip(frames, timestamps):
        assert same(img[:, 0], img[:, 1]) and same(img[:, 0], img[:, 2])  # grey
        # a frame of one sample at timestamp ts holds sample * a, a = float32(1 / (ts + 1)): the running mean's weight on an empty
        # frame (raygen.rgen:84-108).  One float32 product, undone here in float64: one more half-ulp
        a = np.float64(np.float32(1.0) / np.float32(ts + 1)) if ts > 0 else 1.0
        r = img[:, 0].astype(np.float64) / a / FURNACE_L
        sel = inside | outside
        assert (r[sel] > 0).all()
        k = np.zeros(len(r), np.int64)
        k[sel] = np.rint(np.log(r[sel] / E[sel]) / math.log(albedo)).astype(np.int64)
        assert (k[sel] >= 0).all() and (k[outside] == 0).all() and k.max() <= FURNACE_MAX_EVENTS
        dev = np.abs(r[sel] / (albedo ** k[sel] * E[sel]) - 1.0)
        assert (dev <= furnace_bound(k[sel]) + 5 * EPS).all(), dev.max()  # (+ the float64-to-float32 statement of E: exp of a float32 product)
        ks.append(k)
        hits += int((k[inside] == 0).sum())
        total += int(inside.sum())
    p = np.exp(-sigma_t * (d - 1e-4) / cos[inside])
    want = p.mean()
    sd = math.sqrt((p * (1.0 - p)).sum() * len(frames)) / total
    print("half-albedo furnace: share of unscattered samples %.4f over %d, free-path law %.4f, binomial sd %.4f; %.1f %% of the pixels left out"
          % (hits / total, total, want, sd, 100 * left_out))
    assert abs(hits / total - want) <= 5 * sd
    return ks


def check_furnace_bounded(img, max_events=FURNACE_MAX_EVENTS, spp=4):
    """(d) grey, albedo <= 1: no channel of any pixel exceeds L beyond the rounding of its path."""
    assert np.isfinite(img).all()
    assert img[:, :3].max() <= FURNACE_L * (1.0 + furnace_bound(max_events, spp))
