"""What a ray OUGHT to cost on a given wide tree: references for the traversal WORK (node records read, triangles tested), which
the hit references cannot see -- a hit does not depend on the visiting order or on how well the running t culls.

numpy, float64 and tests/emu/trace_work_ref.cpp (a stand-alone C++ file in double, built here on first use: the per-ray walks are
too slow in Python); nothing of oracle/ or of the product is imported.  The 64-byte node record is decoded from the layout comment
at the top of gpuspectral_amd/csrc/pt_trace.h, not from node_test, and the order words are never read:

  decode_nodes   numpy: every record's four child boxes (plane = origin + q * scale), ni from the mask in bits 28..31 of order_lo,
                 unused positions (inverted boxes), child_base, tri_base - ni
  Work           per ray: the float64 brute-force hit, W_min (records a traversal that knew the hit would read) and W_sorted (the
                 textbook ordered traversal: inner children by ascending float64 entry distance)
  lattice, octant_rays, zero_component_rays: the scenes and rays of tests/test_trace_work_cpu.py and tests/test_gpu_trace_work.py
"""
import ctypes as C
import os
import subprocess

import numpy as np

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))


# ---- geometry and rays --------------------------------------------------------------------------------------------------------------
_BOX_QUADS = [((0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0)), ((0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)),
              ((0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0)), ((1, 0, 0), (1, 1, 0), (1, 1, 1), (1, 0, 1)),
              ((0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)), ((0, 1, 0), (0, 1, 1), (1, 1, 1), (1, 1, 0))]


def lattice(nx=6, ny=None, nz=None, edge=0.5, pitch=1.0):
    """nx x ny x nz separated axis-aligned boxes of the given edge, their low corners at multiples of the pitch: 12 triangles per
    box, (n, 3, 3) float32.  Behind every first hit lie up to n - 1 more boxes on the ray's line: deep occlusion."""
    ny, nz = nx if ny is None else ny, nx if nz is None else nz
    tris = []
    for q in _BOX_QUADS:
        c = np.array(q, np.float64) * edge
        tris += [c[[0, 1, 2]], c[[0, 2, 3]]]
    box = np.array(tris)  # (12, 3, 3)
    # every triangle wound so that its geometric normal (v1 - v0) x (v2 - v0) points INTO its box: as a one-sided surface seen from
    # outside it is a back face, at which a path ends -- a frame of it traces camera rays only
    n = np.cross(box[:, 1] - box[:, 0], box[:, 2] - box[:, 0])
    flip = (n * (box.mean(1) - 0.5 * edge)).sum(1) > 0
    box[flip] = box[flip][:, [0, 2, 1]]
    i, j, k = (a.ravel() for a in np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"))
    corner = np.stack([i, j, k], 1)[:, None, None, :] * pitch
    return (box[None] + corner).reshape(-1, 3, 3).astype(F)


def _rays(o, d):
    r = np.zeros((len(o), 8), F)
    r[:, 0:3], r[:, 4:7], r[:, 7] = o, d, 1e10
    return r


def octant_rays(lo, hi, octant, n=1500, seed=0):
    """n rays of one sign octant (bit a of `octant` set = the direction is negative on axis a) at the box [lo, hi]: every
    direction component has the octant's sign and magnitude >= 0.05 (drawn in 0.1 .. 1, then normalised: >= 0.07); the ray runs
    through a uniform point of the box and starts 0.05 to 0.5 box sizes before the face it enters through: outside the box, on
    the octant's side."""
    rng = np.random.RandomState(1000 * seed + octant)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    sign = np.array([-1.0 if octant >> a & 1 else 1.0 for a in range(3)])
    d = rng.uniform(0.1, 1.0, (n, 3)) * sign
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    assert (np.abs(d) >= 0.05).all()
    target = rng.uniform(lo, hi, (n, 3))
    behind = np.where(sign > 0, target - lo, hi - target)  # distance to the box face the ray enters through, per axis
    s = (behind / np.abs(d)).min(1, keepdims=True) + rng.uniform(0.05, 0.5, (n, 1)) * (hi - lo).max()
    r = _rays(target - d * s, d)
    o = r[:, 0:3].astype(np.float64)
    assert np.where(sign > 0, o < lo, o > hi).any(1).all() and (np.sign(r[:, 4:7]) == sign).all()
    return r


def zero_component_rays(lo, hi, n=1500, seed=0):
    """n rays with exactly one zero direction component -- +0.0 and -0.0 alternating, the axis cycling -- and random signs on the
    other two; they run through a uniform point of the box and start outside it, before the face they enter through."""
    rng = np.random.RandomState(7000 + seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    d = rng.uniform(0.1, 1.0, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    axis = np.arange(n) % 3
    d[np.arange(n), axis] = 0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    target = rng.uniform(lo, hi, (n, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        behind = np.where(d > 0, target - lo, hi - target) / np.abs(d)
    behind[np.arange(n), axis] = np.inf
    s = behind.min(1, keepdims=True) + rng.uniform(0.05, 0.5, (n, 1)) * (hi - lo).max()
    r = _rays(target - d * s, d)
    neg = (np.arange(n) // 3) % 2 == 1
    r[np.arange(n)[neg], 4 + axis[neg]] = F(-0.0)
    z = r[np.arange(n), 4 + axis]
    assert (z == 0).all() and (np.signbit(z) == neg).all() and ((r[:, 4:7] == 0).sum(1) == 1).all()
    return r


def work_rays(lo, hi, seed=0, per_octant=1500, zeros=1500):
    """[(label, rays)]: the eight octants, then the rays with a zero component."""
    return [("octant %d" % k, octant_rays(lo, hi, k, per_octant, seed)) for k in range(8)] + [("zero component", zero_component_rays(lo, hi, zeros, seed))]


# ---- the decoder, from the layout comment -------------------------------------------------------------------------------------------
class Tree:
    """nodes: (n, 16) uint32 records; packets: (slots, 12) float32; num_real: slots that hold a triangle (the rest is padding)."""

    def __init__(self, nodes, packets, num_real, slot_lo=None, slot_hi=None, slot_to_global=None):
        self.nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 16)
        self.packets = np.ascontiguousarray(packets, F).reshape(-1, 12)
        self.num_real = int(num_real)
        self.slot_lo, self.slot_hi, self.slot_to_global = slot_lo, slot_hi, slot_to_global

    @property
    def triangles(self):
        """(num_real, 3, 3) float32 in slot order."""
        return self.packets[:self.num_real].reshape(-1, 3, 4)[:, :, :3].copy()


def decode_nodes(nodes):
    """lo, hi: (n, 4, 3) float64 child boxes; used: (n, 4); ni, child_base, tri_base_minus_ni: (n,)."""
    w = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 16)
    origin = np.ascontiguousarray(w[:, 0:3]).view(F).astype(np.float64)
    scale = np.ascontiguousarray(w[:, [3, 14, 15]]).view(F).astype(np.float64)
    shifts = np.arange(4, dtype=np.uint32) * 8
    qlo = np.stack([(w[:, 4 + a, None] >> shifts) & 255 for a in range(3)], 2).astype(np.float64)  # (n, child, axis)
    qhi = np.stack([(w[:, 7 + a, None] >> shifts) & 255 for a in range(3)], 2).astype(np.float64)
    lo = origin[:, None, :] + qlo * scale[:, None, :]
    hi = origin[:, None, :] + qhi * scale[:, None, :]
    used = (qlo <= qhi).all(2)
    mask = w[:, 12] >> 28
    ni = ((mask >> 0) & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1) + ((mask >> 3) & 1)
    assert np.array_equal(mask, (1 << ni) - 1), "the inner positions are the first ni"
    return lo, hi, used, ni.astype(np.int64), w[:, 10].astype(np.int64), w[:, 11].astype(np.int64)


def check_decode_contains(tree):
    """No tolerance (the quantisation is outward): every decoded leaf-child box contains the padded box of its triangle slot, every
    decoded inner-child box contains the padded boxes of ALL the slots under that child, every record but the root is the child of
    exactly one position, and every real slot is the leaf child of exactly one.

    Two things that do NOT hold, measured here and returned, neither of them a defect:
      * The decode that is outward is the float32 one, origin + q * scale with ONE rounding (what the encoder verifies with an
        fma).  The real-number plane may lie up to half a float32 spacing inside the padded box (0.11 spacings on the lattice; the
        leaf pad is 84 spacings and more).  float64 holds origin + q * scale exactly, so rounding it once is that decode.
      * Decoded boxes are not NESTED: a child's own record quantises its children on the child's grid, whose last step may reach
        past the box the parent decodes for the child (by up to 0.75 % of that box on the soup).  Each box is tested on its own
        and contains the geometry under it, which is all a traversal needs; a reference must not assume nesting.
    Returns (leaf children, inner children, largest real-number cut into a padded box in float32 spacings, largest excess of a
    child's decoded children over the child's decoded box relative to that box)."""
    lo64, hi64, used, ni, child_base, tbm = decode_nodes(tree.nodes)
    lo, hi = lo64.astype(F).astype(np.float64), hi64.astype(F).astype(np.float64)
    n = len(tree.nodes)
    pos = np.arange(4)[None, :]
    inner = used & (pos < ni[:, None])
    leaf = used & (pos >= ni[:, None])
    assert (inner == (pos < ni[:, None])).all(), "an inner position is never unused"
    slot = (tbm[:, None] + pos)[leaf]
    assert np.array_equal(np.sort(slot), np.arange(tree.num_real)), "every triangle slot is the leaf child of exactly one record"
    assert (lo[leaf] <= tree.slot_lo[slot]).all() and (hi[leaf] >= tree.slot_hi[slot]).all(), "a decoded leaf box cuts into its triangle's padded box"
    spacing = np.spacing(np.maximum(np.abs(tree.slot_lo[slot]), np.abs(tree.slot_hi[slot])).astype(F)).astype(np.float64)
    cut = float(np.maximum((lo64[leaf] - tree.slot_lo[slot]) / spacing, (tree.slot_hi[slot] - hi64[leaf]) / spacing).max())
    assert cut <= 0.5
    child = (child_base[:, None] + pos)[inner]
    assert np.array_equal(np.sort(child), np.arange(1, n)) and (child > np.nonzero(inner)[0]).all(), "every record but the root is the inner child of exactly one, earlier, record"
    # the padded boxes under every record, bottom up (children come after their parent in the array)
    sub_lo, sub_hi = np.full((n, 3), np.inf), np.full((n, 3), -np.inf)
    for i in range(n - 1, -1, -1):
        for k in range(4):
            if leaf[i, k]:
                sub_lo[i], sub_hi[i] = np.minimum(sub_lo[i], tree.slot_lo[tbm[i] + k]), np.maximum(sub_hi[i], tree.slot_hi[tbm[i] + k])
            elif inner[i, k]:
                sub_lo[i], sub_hi[i] = np.minimum(sub_lo[i], sub_lo[child_base[i] + k]), np.maximum(sub_hi[i], sub_hi[child_base[i] + k])
    assert (lo[inner] <= sub_lo[child]).all() and (hi[inner] >= sub_hi[child]).all(), "a decoded inner box cuts into the geometry under it"
    big_lo, big_hi = np.where(used[:, :, None], lo, np.inf).min(1), np.where(used[:, :, None], hi, -np.inf).max(1)  # union of a record's children
    excess = np.maximum(lo[inner] - big_lo[child], big_hi[child] - hi[inner]) / np.maximum(hi[inner] - lo[inner], 1e-300)
    return int(leaf.sum()), int(inner.sum()), cut, float(excess.max())


# ---- the per-ray references ------------------------------------------------------------------------------------------------------------
_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        src, so = os.path.join(HERE, "emu", "trace_work_ref.cpp"), os.path.join(HERE, "emu", "libtrace_work_ref.so")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", so, src])
        L = C.CDLL(so)
        L.twr_decode.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 6
        L.twr_decode.restype = None
        L.twr_work.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64] + [C.c_void_p] * 6
        L.twr_work.restype = None
        _LIB = L
    return _LIB


def decode_nodes_cxx(nodes):
    """The C++ file's own decode, as decode_nodes returns it: the two must agree exactly."""
    w = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 16)
    n = len(w)
    lo, hi, used = np.zeros((n, 4, 3)), np.zeros((n, 4, 3)), np.zeros((n, 4), np.uint8)
    ni, cb, tb = np.zeros(n, np.int32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    _lib().twr_decode(w.ctypes.data, n, lo.ctypes.data, hi.ctypes.data, used.ctypes.data, ni.ctypes.data, cb.ctypes.data, tb.ctypes.data)
    return lo, hi, used.astype(bool), ni.astype(np.int64), cb.astype(np.int64), tb.astype(np.int64)


class Work:
    """Per ray: t_hit (float64; tmax for a miss), slot (-1: miss), w_min, w_sorted, tris_sorted."""

    def __init__(self, tree, rays):
        rays = np.ascontiguousarray(rays, F).reshape(-1, 8)
        n = len(rays)
        self.t_hit, self.slot = np.zeros(n), np.zeros(n, np.int64)
        self.w_min, self.w_sorted, self.tris_sorted = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        slot_sorted = np.zeros(n, np.int64)
        _lib().twr_work(tree.nodes.ctypes.data, len(tree.nodes), tree.packets.ctypes.data, tree.num_real, rays.ctypes.data, n, self.t_hit.ctypes.data,
                        self.slot.ctypes.data, self.w_min.ctypes.data, self.w_sorted.ctypes.data, self.tris_sorted.ctypes.data, slot_sorted.ctypes.data)
        # the ordered traversal is a tracer too: it must find the brute force's hit (exactly: same arithmetic on the same triangle)
        assert np.array_equal(slot_sorted, self.slot), "the ordered traversal of the decoded tree misses the brute force's hit on %d rays" % (slot_sorted != self.slot).sum()
        assert (self.w_min <= self.w_sorted).all() and (self.w_min >= 1).all()
