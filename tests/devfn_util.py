"""Loader of tests/devfn/libpt_devfn.so (the test-only device harness, tests/devfn/pt_devfn.hip) and of its host twins in
tests/emu/libpt_emu.so (the emu_devfn_* entry points: the same bodies, tests/devfn/devfn_bodies.h, compiled by g++).

Both sides are driven through one class, `Side`, so a test states a call once and runs it on the GPU and on the host.

The library is the tree's when the digest stamped into it (devfn_build_info(), the scheme of gsp_build_info()) is the digest of
the sources as they are now.  A missing or stale library is rebuilt where hipcc is on the path and is an error where it is
not: the GPU tests never skip over it.  GSP_DEVFN_LIB names another library file to load instead (a deliberately different
compile of the harness, to show that the tests can fail); that file is taken as it is."""
import ctypes as C
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "devfn")
LIB = os.path.join(DIR, "libpt_devfn.so")
CSRC = os.path.join(ROOT, "gpuspectral_amd", "csrc")
# what tests/devfn/Makefile hashes, in its order
DIGEST_SOURCES = (os.path.join(DIR, "pt_devfn.hip"), os.path.join(DIR, "devfn_bodies.h"), os.path.join(CSRC, "pt_math.h"),
                  os.path.join(CSRC, "pt_shading.h"), os.path.join(CSRC, "pt_trace.h"), os.path.join(CSRC, "pt_stages.h"),
                  os.path.join(ROOT, "include", "gpuspectral_pt.h"))
BAD_INDEX = -2  # devfn::kBadIndex: a vector carried an index outside its arrays; nothing was launched

vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
# name -> argument types (every entry point returns int: 0, a hipError_t, or BAD_INDEX)
SIGNATURES = {
    "math": [vp, u64] + [vp] * 6,
    "atan2": [vp, vp, u64, vp],
    "normalize": [vp, u64, vp],
    "rng": [vp, vp, u64, vp],
    "onb": [vp, vp, u64, vp],
    "helpers": [vp, vp, vp, u64, vp],
    "samplers": [vp, vp, u64, vp],
    "bsdf": [vp, vp, vp, vp, vp, vp, u64, vp, vp, vp],
    "lights": [vp, u32, u32, vp, vp, u64, vp],
    "texture": [vp, u32, vp, u64, vp, vp, vp, u64, vp],
    "envmap": [vp, u32, u32, vp, vp, u64, vp],
    "tri_tests": [vp, vp, u64, vp, vp],
    "shears": [vp, u64, vp],
    "encode_nodes": [vp, vp, u64, vp, vp],
    "node_tests": [vp, u64, vp, vp, u64, vp],
}
# the harness's own exports besides the families
EXTRA_EXPORTS = ("devfn_build_info", "devfn_run_count", "devfn_device_count", "devfn_table_layout")
REC_BYTES = (16, 8, 8, 24, 44, 16, 20, 32)


def source_digest():
    h = hashlib.sha256()
    for f in DIGEST_SOURCES:
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def product_flags():
    """The HIPFLAGS of gpuspectral_amd/csrc/Makefile without the --offload-arch, as gsp_build_info() reports them."""
    with open(os.path.join(CSRC, "Makefile")) as fh:
        line = [ln for ln in fh if ln.startswith("HIPFLAGS ?=")][0]
    return " ".join(w for w in line.split("?=", 1)[1].split() if not w.startswith("--offload-arch"))


def stamped_info(path):
    """The build-info string inside a library file, read without loading it; None if there is none."""
    if not os.path.exists(path):
        return None
    with open(path, "rb") as fh:
        m = re.search(rb"arch=(\S+) digest=([0-9a-f]{16}) flags=([^\0]*)\0", fh.read())
    return None if m is None else {"arch": m.group(1).decode(), "digest": m.group(2).decode(), "flags": m.group(3).decode()}


def ensure_built():
    """The path of a library that carries the digest of the tree's sources; builds it with hipcc if it has to, raises if it cannot."""
    info = stamped_info(LIB)
    if info is not None and info["digest"] == source_digest():
        return LIB
    if shutil.which("hipcc") is None:
        raise RuntimeError("%s is %s and hipcc is not on the path: build it with `make -C tests/devfn` (build() does)"
                           % (LIB, "missing" if info is None else "stale (digest %s, tree %s)" % (info["digest"], source_digest())))
    subprocess.check_call(["make", "-B", "-C", DIR])
    info = stamped_info(LIB)
    if info is None or info["digest"] != source_digest():
        raise RuntimeError("make -C tests/devfn left a library without the digest of the tree's sources: %r" % (info,))
    return LIB


def _ptr(a):
    return None if a is None else a.ctypes.data


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, np.float32)
    return a if shape is None else a.reshape(shape)


def _u32(a):
    return np.ascontiguousarray(a, np.uint32)


class DevfnError(RuntimeError):
    def __init__(self, what, code):
        RuntimeError.__init__(self, "%s returned %d%s" % (what, code, " (an index outside its arrays: refused before any launch)" if code == BAD_INDEX else ""))
        self.code = code


class Side:
    """The entry points of one side: prefix 'devfn_' in libpt_devfn.so (GPU), 'emu_devfn_' in libpt_emu.so (host)."""

    def __init__(self, lib, prefix, name):
        self.L, self.prefix, self.name = lib, prefix, name
        for k, args in SIGNATURES.items():
            f = getattr(lib, prefix + k)  # AttributeError: the library lacks an entry point the helper declares
            f.argtypes, f.restype = args, C.c_int

    def _call(self, k, *args):
        rc = getattr(self.L, self.prefix + k)(*args)
        if rc != 0:
            raise DevfnError(self.prefix + k, rc)

    def math(self, x):
        """x -> dict of float32 arrays: sin, cos, log, exp (det_*), sqrt (gsqrt), rcp (1 / x)."""
        x = _f32(x)
        o = [np.zeros_like(x) for _ in range(6)]
        self._call("math", _ptr(x), x.size, *[_ptr(a) for a in o])
        return dict(zip(("sin", "cos", "log", "exp", "sqrt", "rcp"), o))

    def atan2(self, y, x):
        y, x = _f32(y), _f32(x)
        o = np.zeros_like(y)
        self._call("atan2", _ptr(y), _ptr(x), y.size, _ptr(o))
        return o

    def normalize(self, v):
        v = _f32(v, (-1, 3))
        o = np.zeros_like(v)
        self._call("normalize", _ptr(v), len(v), _ptr(o))
        return o

    def rng(self, a, b):
        a, b = _u32(a), _u32(b)
        o = np.zeros((a.size, 7), np.uint32)
        self._call("rng", _ptr(a), _ptr(b), a.size, _ptr(o))
        return o

    def onb(self, n, v):
        n, v = _f32(n, (-1, 3)), _f32(v, (-1, 3))
        o = np.zeros((len(n), 15), np.float32)
        self._call("onb", _ptr(n), _ptr(v), len(n), _ptr(o))
        return o.view(np.uint32)

    def helpers(self, f, g, h):
        f, g, h = _f32(f), _f32(g), _u32(h)
        o = np.zeros((f.size, 3), np.uint32)
        self._call("helpers", _ptr(f), _ptr(g), _ptr(h), f.size, _ptr(o))
        return o

    def samplers(self, seeds, alpha):
        seeds, alpha = _u32(seeds), _f32(alpha)
        o = np.zeros((seeds.size, 8), np.float32)
        self._call("samplers", _ptr(seeds), _ptr(alpha), seeds.size, _ptr(o))
        return o.view(np.uint32)

    def table_layout(self, num):
        """(quad offsets, record offsets, image bytes) of the resident tables for `num` records per type: per type the derived
        quads in reverse order, then the records (pt_shading.h derived_of); every table starts on a 16-byte boundary."""
        quad, rec, cur = [], [], 0
        for t in range(8):
            quad.append(cur)
            cur += 16 * int(num[t])
            rec.append(cur)
            cur += (int(num[t]) * REC_BYTES[t] + 15) & ~15
        return quad, rec, cur + 16

    def bsdf(self, bsdfs, handles, wo, seeds, wi):
        """bsdfs: the eight record arrays of a scene (abi.BSDF_DTYPES).  Returns (sample words n x 9, eval words n x 5, the baked
        table image as bytes)."""
        recs = [np.ascontiguousarray(b) for b in bsdfs]
        num = np.array([len(b) for b in recs], np.uint32)
        ptrs = (vp * 8)(*[b.ctypes.data if len(b) else None for b in recs])
        handles, seeds, wo, wi = _u32(handles), _u32(seeds), _f32(wo, (-1, 3)), _f32(wi, (-1, 3))
        n = handles.size
        assert len(wo) == n and len(wi) == n and seeds.size == n
        s, e = np.zeros((n, 9), np.float32), np.zeros((n, 5), np.float32)
        image = np.zeros(self.table_layout(num)[2], np.uint8)
        self._call("bsdf", C.cast(ptrs, vp), _ptr(num), _ptr(handles), _ptr(wo), _ptr(seeds), _ptr(wi), n, _ptr(s), _ptr(e), _ptr(image))
        return s.view(np.uint32), e.view(np.uint32), image

    def lights(self, lights, pos, seeds, num_lights=None):
        """Returns (sample words n x 8, the baked records as bytes); num_lights defaults to all of `lights`."""
        baked = np.array(lights, copy=True)
        pos, seeds = _f32(pos, (-1, 3)), _u32(seeds)
        o = np.zeros((len(pos), 8), np.float32)
        self._call("lights", _ptr(baked), len(baked), len(baked) if num_lights is None else num_lights, _ptr(pos), _ptr(seeds), len(pos), _ptr(o))
        return o.view(np.uint32), baked.view(np.uint8).reshape(-1)

    def texture(self, textures, texels, decode, ids, uv):
        textures, texels, decode = np.ascontiguousarray(textures), _u32(texels), _f32(decode)
        assert decode.size == 256 and textures.dtype.itemsize == 16
        ids, uv = _u32(ids), _f32(uv, (-1, 2))
        o = np.zeros((ids.size, 3), np.float32)
        self._call("texture", _ptr(textures), len(textures), _ptr(texels), texels.size, _ptr(decode), _ptr(ids), _ptr(uv), ids.size, _ptr(o))
        return o.view(np.uint32)

    def envmap(self, env_texels, width, height, to_local, dirs):
        env, m, dirs = _f32(env_texels), _f32(to_local), _f32(dirs, (-1, 3))
        assert env.size == 4 * width * height and m.size == 16
        o = np.zeros((len(dirs), 3), np.float32)
        self._call("envmap", _ptr(env), width, height, _ptr(m), _ptr(dirs), len(dirs), _ptr(o))
        return o.view(np.uint32)

    def tri_tests(self, rays, tris):
        """-> (intersect_tri words n x 4, intersect_tri_rot words n x 4): {hit, t, u, v}."""
        rays, tris = _f32(rays, (-1, 8)), _f32(tris, (-1, 9))
        a, b = np.zeros((len(rays), 4), np.float32), np.zeros((len(rays), 4), np.float32)
        self._call("tri_tests", _ptr(rays), _ptr(tris), len(rays), _ptr(a), _ptr(b))
        return a.view(np.uint32), b.view(np.uint32)

    def shears(self, d):
        d = _f32(d, (-1, 3))
        o = np.zeros((len(d), 12), np.uint32)
        self._call("shears", _ptr(d), len(d), _ptr(o))
        return o

    def encode_nodes(self, boxes, counts):
        """-> (encode_node_w4_ref words n x 16, encode_node_w4 words n x 16)."""
        boxes, counts = _f32(boxes, (-1, 4, 6)), np.ascontiguousarray(counts, np.int32).reshape(-1, 2)
        a, b = np.zeros((len(boxes), 16), np.uint32), np.zeros((len(boxes), 16), np.uint32)
        self._call("encode_nodes", _ptr(boxes), _ptr(counts), len(boxes), _ptr(a), _ptr(b))
        return a, b

    def node_tests(self, nodes, node_idx, rays):
        nodes, node_idx, rays = _u32(nodes).reshape(-1, 16), _u32(node_idx), _f32(rays, (-1, 8))
        o = np.zeros((node_idx.size, 12), np.uint32)
        self._call("node_tests", _ptr(nodes), len(nodes), _ptr(node_idx), _ptr(rays), node_idx.size, _ptr(o))
        return o


_DEV = None


def device():
    """The GPU side.  Raises (never skips) when the library is missing or stale and cannot be rebuilt."""
    global _DEV
    if _DEV is None:
        path = os.environ.get("GSP_DEVFN_LIB") or ensure_built()
        L = C.CDLL(path)
        L.devfn_build_info.restype = C.c_char_p
        L.devfn_run_count.restype = u64
        L.devfn_table_layout.restype = u64
        L.devfn_table_layout.argtypes = [vp, vp, vp]
        _DEV = Side(L, "devfn_", "gfx950 (%s)" % os.path.basename(path))
        _DEV.path = path
    return _DEV


def build_info(side=None):
    text = (side or device()).L.devfn_build_info().decode()
    head, _, flags = text.partition(" flags=")
    info = dict(kv.split("=", 1) for kv in head.split())
    info["flags"] = flags
    return info


def host(emu):
    """The host side: conftest's `emu` fixture (tests/emu/libpt_emu.so)."""
    try:
        return Side(emu.L, "emu_devfn_", "host emu")
    except AttributeError as e:
        raise RuntimeError("tests/emu/libpt_emu.so lacks the batch twins of the device harness (%s): it is older than "
                           "tests/devfn/devfn_bodies.h -- delete it, the tests rebuild it" % e)
