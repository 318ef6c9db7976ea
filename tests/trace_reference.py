"""A BVH-free geometric reference for ray/triangle hits (numpy and Python integers only; nothing of oracle/ or the product).

Three independent sources of truth:
  * brute_force: float64 Moeller-Trumbore over every triangle -- no acceleration structure, no shear;
  * voxel_solid / voxel_march: a random solid of lattice cubes and an exact integer march through it, for rays that pass exactly
    through face diagonals, lattice edges and lattice vertices;
  * closed meshes with bit-identical shared vertices (icosphere, torus, two slivers), for the "a ray from inside must hit"
    properties that need no number at all.

The same cases with their geometry arriving through an instance transform (edit_case, lattice_transform, the split scene's mover)
are what tests/test_gpu_trace_edits.py brings about by edits of a resident scene.
"""
import functools
import math
from fractions import Fraction

import numpy as np

F = np.float32

# Largest deviation of THIS module's Moeller-Trumbore formula evaluated in numpy float32 from its float64 evaluation, on the
# (clear ray, nearest triangle) pairs of soup() / soup_rays(): t in units of 2^-24 * max(|o|inf, |vertices|inf, t), barycentrics
# in units of 2^-24.  Measured and printed by tests/test_trace_reference_cpu.py::test_float32_reference_deviation_defines_the_
# tolerance, which also asserts that these constants are what it measures (rounded up).  The tolerance a tracer must meet is
# twice these: Woop's sheared test is another float32 algorithm of similar length.  Neither the oracle nor a kernel had a say.
MT_F32_T_UNITS = 56
MT_F32_BARY_UNITS = 57
TOL_T_UNITS = 2 * MT_F32_T_UNITS
TOL_BARY_UNITS = 2 * MT_F32_BARY_UNITS
UNIT = 2.0 ** -24
BARY_MARGIN = 2.0 ** -14  # a ray is "clear" of an edge when every barycentric is beyond this, one way or the other
LATTICE_TOL = 2.0 ** -10  # relative: the next lattice crossing is a lattice step away, so this is a condition, not a measurement

PLACEMENTS = {"unit": (1.0, (0.0, 0.0, 0.0)), "tiny-far": (1e-3, (100.0, 100.0, 100.0)), "huge": (1e4, (0.0, 0.0, 0.0))}
LATTICE_DIRS = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)] + [
    (1, 2, 0), (2, -1, 0), (0, 1, -2), (1, 2, 3), (-3, 1, 2), (1, -2, 4), (1, 3, 0), (3, 0, -1)]
LATTICE_PLACEMENTS = {"2^-3": (2.0 ** -3, 0.0), "1": (1.0, 0.0), "2^-10@64": (2.0 ** -10, 64.0), "2^12": (2.0 ** 12, 0.0)}


# ---- float64 (or, for the tolerance measurement, float32) Moeller-Trumbore --------------------------------------------------
def moller_trumbore(v0, v1, v2, o, d):
    """The textbook test on arrays that broadcast against each other (last axis = xyz), in the dtype of the inputs, component
    by component (no library reduction, so the float32 evaluation is the same on every machine).  Returns t, u, v with u the
    weight of v1 and v the weight of v2; a ray parallel to the plane gives inf / nan, which no comparison accepts."""

    def cross(a, b):
        return (a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0])

    def dot(a, b):  # a: array or tuple of components
        a = a if isinstance(a, tuple) else (a[..., 0], a[..., 1], a[..., 2])
        b = b if isinstance(b, tuple) else (b[..., 0], b[..., 1], b[..., 2])
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]

    e1, e2, s = v1 - v0, v2 - v0, o - v0
    p = cross(d, e2)
    q = cross(s, e1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = 1.0 / dot(e1, p) if e1.dtype == np.float64 else F(1.0) / dot(e1, p)
        return dot(e2, q) * inv, dot(s, p) * inv, dot(d, q) * inv


def brute_force(tris, rays, chunk=512):
    """tris: (n, 3, 3) float32 world-space triangles; rays: (m, 8) float32 {o, tmin, d, tmax}.  float64 Moeller-Trumbore of every
    ray against every triangle: t, u, v as (m, n) float64 arrays.  Ranges are the caller's business."""
    tris = np.asarray(tris, F).reshape(-1, 3, 3).astype(np.float64)
    rays = np.asarray(rays, F).reshape(-1, 8).astype(np.float64)
    out = [np.empty((len(rays), len(tris))) for _ in range(3)]
    for a in range(0, len(rays), chunk):
        o, d = rays[a:a + chunk, None, 0:3], rays[a:a + chunk, None, 4:7]
        for dst, val in zip(out, moller_trumbore(tris[None, :, 0], tris[None, :, 1], tris[None, :, 2], o, d)):
            dst[a:a + chunk] = val
    return tuple(out)


def inside(t, u, v, tmin, tmax):
    """Candidates of a brute_force result: in the (closed) triangle and in the (open) range."""
    with np.errstate(invalid="ignore"):
        return (u >= 0) & (v >= 0) & (u + v <= 1) & (t > tmin) & (t < tmax)


def crossing_parity(tris, points, seed=1, ndirs=3):
    """True where a float64 brute-force ray from the point crosses the mesh an odd number of times in EVERY one of `ndirs` random
    directions: the point is interior to the closed mesh as the float32 vertices state it."""
    rng = np.random.RandomState(seed)
    ok = np.ones(len(points), bool)
    for _ in range(ndirs):
        d = rng.normal(size=3)
        rays = np.zeros((len(points), 8), F)
        rays[:, 0:3], rays[:, 4:7], rays[:, 7] = points, d / np.linalg.norm(d), np.inf
        t, u, v = brute_force(tris, rays)
        ok &= inside(t, u, v, 0.0, np.inf).sum(1) % 2 == 1
    return ok


# ---- the soup of part 3 -----------------------------------------------------------------------------------------------------
def soup(n=1000, seed=31):
    rng = np.random.RandomState(seed)
    c = rng.uniform(-1, 1, (n, 1, 3))
    return (c + rng.normal(size=(n, 3, 3)) * rng.choice([0.02, 0.1, 0.5], (n, 1, 1))).astype(F)


def soup_rays(n=8000, seed=32):
    rng = np.random.RandomState(seed)
    r = np.zeros((n, 8), F)
    r[:, 0:3] = rng.uniform(-2, 2, (n, 3))
    d = rng.normal(size=(n, 3)).astype(F)
    r[:, 4:7] = d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]
    r[:, 7] = 1e10
    return r


class SoupReference:
    """The float64 answer for every ray of a soup, and which rays it is safe to hold a float32 tracer to."""

    def __init__(self, tris, rays):
        self.tris, self.rays = tris, rays
        t, u, v = brute_force(tris, rays)
        self.t, self.u, self.v = t, u, v
        w = 1.0 - u - v
        tmin, tmax = rays[:, 3:4].astype(np.float64), rays[:, 7:8].astype(np.float64)
        o_inf = np.abs(rays[:, 0:3]).max(1).astype(np.float64)[:, None]
        v_inf = np.abs(tris).reshape(len(tris), 9).max(1).astype(np.float64)[None, :]
        with np.errstate(invalid="ignore"):
            self.t_tol = TOL_T_UNITS * UNIT * np.maximum(np.maximum(o_inf, v_inf), np.abs(t))  # per pair
            lo = np.minimum(np.minimum(u, v), w)
            in_t = (t > tmin - self.t_tol) & (t < tmax + self.t_tol)  # (in range, or too close to an end of it to tell)
            self.sure_in = in_t & (lo >= BARY_MARGIN)
            unsure = in_t & ~(lo >= BARY_MARGIN) & ~(lo <= -BARY_MARGIN)
            near_end = in_t & ((np.abs(t - tmin) <= self.t_tol) | (np.abs(t - tmax) <= self.t_tol)) & (lo > -BARY_MARGIN)
        self.edge_clear = ~unsure.any(1) & ~near_end.any(1)
        tt = np.where(self.sure_in, t, np.inf)
        self.prim = np.where(self.sure_in.any(1), tt.argmin(1), -1)
        rows = np.arange(len(rays))
        best = tt[rows, np.maximum(self.prim, 0)]
        tt2 = tt.copy()
        tt2[rows, np.maximum(self.prim, 0)] = np.inf
        second = tt2.min(1)
        tol_best = self.t_tol[rows, np.maximum(self.prim, 0)]
        tol_second = self.t_tol[rows, tt2.argmin(1)]
        self.hit = self.prim >= 0
        with np.errstate(invalid="ignore"):
            self.apart = ~self.hit | ~(second - best <= tol_best + tol_second)
        self.clear = self.edge_clear & self.apart
        self.best_t = np.where(self.hit, best, np.nan)
        self.best_u = np.where(self.hit, u[rows, np.maximum(self.prim, 0)], np.nan)
        self.best_v = np.where(self.hit, v[rows, np.maximum(self.prim, 0)], np.nan)
        self.best_tol = tol_best

    def float32_deviation(self):
        """(t units, barycentric units): the float32 evaluation of moller_trumbore against the float64 one, on the nearest
        triangle of every ray that is clear of edges (a set that does not depend on the tolerance)."""
        m = self.edge_clear & self.hit
        tr, r = self.tris[self.prim[m]], self.rays[m]
        t32, u32, v32 = moller_trumbore(tr[:, 0], tr[:, 1], tr[:, 2], r[:, 0:3], r[:, 4:7])
        assert t32.dtype == np.float32
        s = np.maximum(np.maximum(np.abs(r[:, 0:3]).max(1), np.abs(tr).reshape(-1, 9).max(1)), self.best_t[m])
        dt = np.abs(t32.astype(np.float64) - self.best_t[m]) / (UNIT * s)
        db = np.maximum(np.abs(u32.astype(np.float64) - self.best_u[m]), np.abs(v32.astype(np.float64) - self.best_v[m])) / UNIT
        return float(dt.max()), float(db.max())

    def anyhit_expectation(self, tmax):
        """For any-hit rays (tmin of the rays, the given tmax): (decided, occluded).  Decided = clear of edges and no candidate
        within the tolerance of either end of the range."""
        tmin = self.rays[:, 3:4].astype(np.float64)
        tmax = np.asarray(tmax, np.float64)[:, None]
        w = 1.0 - self.u - self.v
        with np.errstate(invalid="ignore"):
            lo = np.minimum(np.minimum(self.u, self.v), w)
            maybe = lo > -BARY_MARGIN
            near = maybe & ((np.abs(self.t - tmax) <= self.t_tol) | (np.abs(self.t - tmin) <= self.t_tol))
            in_t = (self.t > tmin) & (self.t < tmax)
            unsure = in_t & maybe & ~(lo >= BARY_MARGIN)
            occ = (in_t & (lo >= BARY_MARGIN)).any(1)
        return ~near.any(1) & ~unsure.any(1), occ


@functools.lru_cache(maxsize=None)
def soup_reference():
    return SoupReference(soup(), soup_rays())


def check_against_soup(ref, hits, who):
    """The value properties of a closest-hit result on the clear rays of a SoupReference."""
    c = ref.clear
    got_hit = hits["prim"] >= 0
    assert np.array_equal(got_hit[c], ref.hit[c]), "%s: hit/miss differs from the float64 brute force on %d clear rays" % (
        who, (got_hit[c] != ref.hit[c]).sum())
    assert np.array_equal(hits["prim"][c], ref.prim[c]), "%s: another triangle than the brute force's nearest on %d clear rays" % (
        who, (hits["prim"][c] != ref.prim[c]).sum())
    m = c & ref.hit
    dt = np.abs(hits["t"][m].astype(np.float64) - ref.best_t[m]) / (ref.best_tol[m] / TOL_T_UNITS)
    db = np.maximum(np.abs(hits["u"][m].astype(np.float64) - ref.best_u[m]), np.abs(hits["v"][m].astype(np.float64) - ref.best_v[m])) / UNIT
    print("%s: %d clear hits; largest t error %.1f units (tolerance %d), largest barycentric error %.1f units (tolerance %d)"
          % (who, m.sum(), dt.max(), TOL_T_UNITS, db.max(), TOL_BARY_UNITS))
    assert dt.max() <= TOL_T_UNITS and db.max() <= TOL_BARY_UNITS
    return float(dt.max()), float(db.max())


# ---- closed meshes with bit-identical shared vertices ----------------------------------------------------------------------
def _icosphere(subdiv=3):
    p = (1.0 + 5.0 ** 0.5) / 2.0
    verts = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1),
             (-p, 0, -1), (-p, 0, 1)]
    verts = [np.array(v, np.float64) / np.linalg.norm(v) for v in verts]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdiv):
        mid, out = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                v = verts[a] + verts[b]
                verts.append(v / np.linalg.norm(v))
                mid[k] = len(verts) - 1
            return mid[k]

        for a, b, c in faces:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    return np.array(verts), np.array(faces)


def _torus(nu=32, nv=16, r_minor=0.35):
    a, b = np.meshgrid(2 * math.pi * np.arange(nu) / nu, 2 * math.pi * np.arange(nv) / nv, indexing="ij")
    verts = np.stack([np.cos(a) * (1 + r_minor * np.cos(b)), r_minor * np.sin(b), -np.sin(a) * (1 + r_minor * np.cos(b))], -1).reshape(-1, 3)
    i, j = (x.ravel() for x in np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij"))

    def idx(i, j):
        return (i % nu) * nv + (j % nv)  # indices wrap: the seam shares its vertices

    faces = np.concatenate([np.stack([idx(i, j), idx(i + 1, j), idx(i, j + 1)], 1), np.stack([idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)], 1)])
    return verts, faces


MESHES = ("icosphere", "torus", "sliver-1e-2", "sliver-1e-3")
CONVEX = ("icosphere", "sliver-1e-2", "sliver-1e-3")
_STRETCH = {"icosphere": (1, 1, 1), "torus": (1, 1, 1), "sliver-1e-2": (1, 1e-2, 1), "sliver-1e-3": (1, 1e-3, 0.2)}


def random_rotation(seed):
    q, r = np.linalg.qr(np.random.RandomState(seed).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


class ClosedMesh:
    """verts (float32, unique) + faces (indices): shared vertices are one float32 triple, whatever the placement.  `frame`
    maps a point of the mesh's own unit frame (before stretch, rotation and placement) to float64 space coordinates."""

    def __init__(self, name, placement, seed=5):
        v, self.faces = _torus() if name == "torus" else _icosphere(3)
        self.name, self.placement = name, placement
        scale, offset = PLACEMENTS[placement]
        rot, stretch = random_rotation(seed), np.array(_STRETCH[name], np.float64)
        self.frame = lambda p: (np.asarray(p, np.float64) * stretch) @ rot.T * scale + np.array(offset)
        self.verts = self.frame(v).astype(F)  # rotation BEFORE rounding: no triangle is axis-aligned
        self.centre = self.frame(np.zeros(3))
        e = np.concatenate([self.faces[:, [0, 1]], self.faces[:, [1, 2]], self.faces[:, [2, 0]]])
        self.edges = np.unique(np.sort(e, 1), axis=0)
        assert len(self.edges) * 2 == len(self.faces) * 3  # closed: every edge belongs to exactly two triangles

    @property
    def tris(self):
        return self.verts[self.faces]  # (n, 3, 3) float32

    def interior_points(self, n=8, seed=9, radius=0.3):
        """Points well inside (float32): within 0.3 of the radius around the centre, or around the torus's centre circle."""
        rng = np.random.RandomState(seed)
        off = rng.normal(size=(n, 3))
        off *= (radius * rng.uniform(0, 1, (n, 1)) ** (1 / 3)) / np.linalg.norm(off, axis=1, keepdims=True)
        if self.name == "torus":
            a = rng.uniform(0, 2 * math.pi, n)
            off = np.stack([np.cos(a), np.zeros(n), -np.sin(a)], 1) + 0.35 * off
        return self.frame(off).astype(F)


def aim_points(verts, edges, per_edge=4, seed=3):
    """Every vertex, and `per_edge` random points of every edge (float64, from float32 vertices or their float64 images)."""
    rng = np.random.RandomState(seed)
    v = np.asarray(verts, np.float64)
    s = rng.uniform(0, 1, (len(edges), per_edge, 1))
    on_edges = v[edges[:, 0]][:, None] * (1 - s) + v[edges[:, 1]][:, None] * s
    return np.concatenate([v, on_edges.reshape(-1, 3)])


def rays_towards(origins, targets, tmax=1e10):
    """(len(origins) * len(targets), 8) float32 rays; the direction is the float32-normalised float32 difference."""
    o = np.repeat(np.asarray(origins, F), len(targets), 0)
    d = np.tile(np.asarray(targets, np.float64), (len(origins), 1)).astype(F) - o
    with np.errstate(invalid="ignore"):  # (a target that rounds to the origin: the callers assert that there is none)
        d = d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]
    r = np.zeros((len(o), 8), F)
    r[:, 0:3], r[:, 4:7], r[:, 7] = o, d, tmax
    return r


def rays_from_outside(centre, targets, factor=3.0, tmax=1e10):
    """One ray per target from centre + factor * (target - centre) towards the target, and the distance |origin - centre| that the
    hit must stay below: the far side of a convex mesh lies beyond the centre, so a leak through the near side shows."""
    centre, targets = np.asarray(centre, np.float64), np.asarray(targets, np.float64)
    o = (centre + factor * (targets - centre)).astype(F)
    d = targets.astype(F) - o
    with np.errstate(invalid="ignore"):  # (a target that rounds to the origin: the callers assert that there is none)
        d = d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]
    r = np.zeros((len(o), 8), F)
    r[:, 0:3], r[:, 4:7], r[:, 7] = o, d, tmax
    return r, np.linalg.norm(o.astype(np.float64) - centre, axis=1)


def transform_points_f32(m16, p):
    """Column-major 4x4 (16 float32) times points, in float32 with the association ((m0 x + m4 y) + m8 z) + m12 -- how a float32
    renderer brings object-space vertices to the world, so equal inputs give equal outputs."""
    m, p = np.asarray(m16, F), np.asarray(p, F)
    return np.stack([((m[k] * p[..., 0] + m[4 + k] * p[..., 1]) + m[8 + k] * p[..., 2]) + m[12 + k] for k in range(3)], -1)


# ---- the lattice solid and its exact march ----------------------------------------------------------------------------------
class VoxelSolid:
    """n^3 cells, each solid with probability 1/2; the mesh is every face between a solid cell and an empty one (outside the
    lattice is empty), two triangles per face split along the diagonal from the face's low corner.  Lattice coordinates are
    integers 0..n; world = lattice * scale + offset."""

    def __init__(self, n, seed):
        self.n = n
        rng = np.random.RandomState(seed)
        self.cells = rng.rand(n, n, n) < 0.5
        pad = np.zeros((n + 2,) * 3, bool)
        pad[1:-1, 1:-1, 1:-1] = self.cells
        self._pad = pad
        self.face_tris = {}  # (axis, plane, a, b) -> first of its two triangle ids; a, b = cell coordinates on the other two axes
        tris = []
        for axis in range(3):
            oa, ob = [k for k in range(3) if k != axis]
            for plane in range(n + 1):
                for a in range(n):
                    for b in range(n):
                        lo, hi = [0, 0, 0], [0, 0, 0]
                        lo[axis], hi[axis], lo[oa], hi[oa], lo[ob], hi[ob] = plane - 1, plane, a, a, b, b
                        if self.solid(lo) == self.solid(hi):
                            continue
                        c = []
                        for da, db in ((0, 0), (1, 0), (1, 1), (0, 1)):
                            p = [0, 0, 0]
                            p[axis], p[oa], p[ob] = plane, a + da, b + db
                            c.append(p)
                        self.face_tris[(axis, plane, a, b)] = len(tris)
                        tris += [(c[0], c[1], c[2]), (c[0], c[2], c[3])]
        self.lattice_tris = np.array(tris, np.int64)  # (m, 3, 3)
        self.solid_cells = np.argwhere(self.cells)

    def solid(self, c):
        return bool(self._pad[c[0] + 1, c[1] + 1, c[2] + 1]) if all(-1 <= x <= self.n for x in c) else False

    def world_tris(self, scale, offset):
        t = (self.lattice_tris.astype(np.float64) * scale + offset).astype(F)
        assert np.array_equal(t.astype(np.float64), self.lattice_tris * scale + offset)  # exact in float32
        return t

    def world_rays(self, scale, offset, dirs=LATTICE_DIRS):
        """Every solid cell's centre x every direction (unnormalised), ordered cell-major."""
        o = (self.solid_cells + 0.5) * scale + offset
        assert np.array_equal(o.astype(F).astype(np.float64), o)
        r = np.zeros((len(o) * len(dirs), 8), F)
        r[:, 0:3] = np.repeat(o, len(dirs), 0)
        r[:, 4:7] = np.tile(np.array(dirs, F), (len(o), 1))
        r[:, 7] = 1e10
        return r


@functools.lru_cache(maxsize=None)
def voxel_solid(n, seed):
    return VoxelSolid(n, seed)


def _in_triangle_2d(p, a, b, c):
    """Closed point-in-triangle on integers."""
    def e(s, t):
        return (t[0] - s[0]) * (p[1] - s[1]) - (t[1] - s[1]) * (p[0] - s[0])

    x, y, z = e(a, b), e(b, c), e(c, a)
    return (x >= 0 and y >= 0 and z >= 0) or (x <= 0 and y <= 0 and z <= 0)


def voxel_march(solid, origin_cell, direction, max_crossings=None):
    """Exact march from the centre of `origin_cell` along the integer `direction`, in Python integers.

    Coordinates are doubled (cell centres odd, lattice planes even) and scaled by M = lcm of the direction's nonzero |components|,
    so that every meeting of the ray with a lattice plane happens at an integer step tau: the point is (O M + tau D) / (2 M) in
    lattice units and the ray parameter, in lattice units per unit of `direction`, is tau / (2 M).

    Returns the list of events (param: Fraction, point: 3 Fractions in lattice units, crossing: bool, tris: ids of the mesh
    triangles that contain the point) at which the ray meets the mesh.  crossing = the cell the ray leaves and the cell it
    enters differ in solidity, so the ray passes THROUGH the closed surface there and any watertight tracer must report it;
    otherwise the ray only touches an edge or a vertex of the mesh between two cells of equal solidity (a tracer may report the
    touch or not).  The march ends when the ray has left the lattice or after `max_crossings` crossings."""
    D = tuple(int(x) for x in direction)
    M = 1
    for x in D:
        if x:
            M = M * abs(x) // math.gcd(M, abs(x))
    O = tuple((2 * int(c) + 1) * M for c in origin_cell)
    n, two_m = solid.n, 2 * M
    steps = sorted({(M // abs(x)) * (2 * j + 1) for x in D if x for j in range(n + 1)})
    events, crossings = [], 0
    for tau in steps:
        P = tuple(O[k] + tau * D[k] for k in range(3))
        on = [P[k] % two_m == 0 for k in range(3)]
        if not any(on):
            continue
        before, after, around = [], [], []
        for k in range(3):
            if on[k]:
                m = P[k] // two_m
                before.append(m - 1 if D[k] > 0 else m)
                after.append(m if D[k] > 0 else m - 1)
                around.append((m - 1, m))
            else:
                c = P[k] // two_m  # floor
                before.append(c)
                after.append(c)
                around.append((c,))
        if any(not (-1 <= c <= n) for c in after):
            break  # beyond the lattice: nothing but empty space from here on
        hit_tris = []
        for k in range(3):
            if not on[k]:
                continue
            oa, ob = [j for j in range(3) if j != k]
            for a in around[oa]:
                for b in around[ob]:
                    first = solid.face_tris.get((k, P[k] // two_m, a, b))
                    if first is None:
                        continue
                    for tid in (first, first + 1):
                        tri = solid.lattice_tris[tid]
                        if _in_triangle_2d((P[oa], P[ob]), *[(int(v[oa]) * two_m, int(v[ob]) * two_m) for v in tri]):
                            hit_tris.append(tid)
        crossing = solid.solid(before) != solid.solid(after)
        assert hit_tris or not crossing  # a change of solidity between two cells that meet in P puts a mesh face through P
        if hit_tris:
            events.append((Fraction(tau, two_m), tuple(Fraction(p, two_m) for p in P), crossing, sorted(hit_tris)))
            crossings += crossing
            if max_crossings is not None and crossings >= max_crossings:
                break
    return events


class LatticeReference:
    """The march of every ray of VoxelSolid.world_rays, up to the second crossing, as arrays in lattice units (multiply the
    parameters by the lattice scale for world units; directions are not scaled).

    first_any: parameter of the first event of any kind; first: parameter of the first crossing; admissible[i]: {triangle id ->
    parameter} over the events up to and including the first crossing (a closest hit must be one of these); nxt / admissible_next:
    the same from the first crossing (exclusive) to the second (inclusive), nxt = nan where the ray leaves the lattice first."""

    def __init__(self, solid, dirs=LATTICE_DIRS):
        self.solid = solid
        m = len(solid.solid_cells) * len(dirs)
        self.first_any, self.first, self.nxt = np.zeros(m), np.zeros(m), np.full(m, np.nan)
        self.admissible, self.admissible_next = [], []
        self.zero_bary = 0
        i = 0
        for cell in solid.solid_cells:
            for d in dirs:
                ev = voxel_march(solid, cell, d, max_crossings=2)
                ci = [k for k, e in enumerate(ev) if e[2]]
                assert ci, "a ray from a solid cell must leave the solid"
                self.first_any[i], self.first[i] = float(ev[0][0]), float(ev[ci[0]][0])
                self.admissible.append({t: float(e[0]) for e in ev[:ci[0] + 1] for t in e[3]})
                self.zero_bary += len(ev[ci[0]][3]) > 1  # the exact crossing point lies on more than one triangle
                rest = ev[ci[0] + 1:]
                if len(ci) > 1:
                    self.nxt[i] = float(ev[ci[1]][0])
                self.admissible_next.append({t: float(e[0]) for e in rest for t in e[3]})
                i += 1


@functools.lru_cache(maxsize=None)
def lattice_reference(n, seed):
    return LatticeReference(voxel_solid(n, seed))


def check_lattice_closest(ref, hits, scale, who, admissible=None, must_hit=None):
    """Every ray hits (where `must_hit`), the reported triangle contains the exact point of an admissible event, and t is that
    event's exact parameter to within LATTICE_TOL relative."""
    admissible = ref.admissible if admissible is None else admissible
    must_hit = np.ones(len(hits), bool) if must_hit is None else must_hit
    missed = (hits["prim"] < 0) & must_hit
    assert not missed.any(), "%s: %d of %d lattice rays leak (first: ray %d)" % (who, missed.sum(), len(hits), np.nonzero(missed)[0][0])
    worst = 0.0
    for i in np.nonzero(hits["prim"] >= 0)[0]:
        want = admissible[i].get(int(hits["prim"][i]))
        assert want is not None, "%s: ray %d reports triangle %d at t = %g, which does not contain a crossing point (%s)" % (
            who, i, hits["prim"][i], hits["t"][i], admissible[i])
        rel = abs(float(hits["t"][i]) / (want * scale) - 1.0)
        worst = max(worst, rel)
        assert rel <= LATTICE_TOL, "%s: ray %d: t = %r, exact %r" % (who, i, hits["t"][i], want * scale)
    return worst


# ---- the cases both test modules run (geometry and rays only: the scene is built by the caller) -----------------------------
def instance_transform():
    """Rotated, non-uniformly scaled, mirrored (negative determinant), translated: column-major 16 float32."""
    m = np.eye(4)
    m[:3, :3] = random_rotation(11) @ np.diag([-1.0, 2.5, 0.4])
    m[:3, 3] = (0.3, -0.2, 0.1)
    return m.T.astype(F).reshape(16).copy()


class LeakCase:
    """One closed mesh at one placement, as it is (identity transform: the float32 vertices ARE the geometry) or as the object-
    space mesh of one instance under instance_transform().  inside_rays: from 8 interior origins at every vertex and 4 points of
    every edge; grazing_rays: from inside too, nearly or exactly within an axis plane through the target (an addition to the
    issue's classes; on the slivers only a few dozen survive the interior filter); outside_rays (convex, uncrumpled meshes):
    towards the same targets from beyond them, with the distance the hit must stay below.  world_tris: what the tracer sees,
    for the reference-only checks."""

    def __init__(self, name, placement, instanced):
        self.key = (name, placement, instanced)
        self._derive(ClosedMesh(name, placement), instance_transform() if instanced else None, (name, placement) in CRUMPLED)

    def _derive(self, mesh, transform, crumpled):
        """Everything but the key, from the object-space mesh, its transform (None = identity) and whether rounding has crumpled
        the world-space mesh (origins by crossing parity, no outside rays)."""
        name = mesh.name
        self.mesh, self.obj_tris, self.transform = mesh, mesh.tris, transform
        if transform is not None:
            m = self.transform.astype(np.float64).reshape(4, 4).T
            to_world = lambda p: np.asarray(p, np.float64) @ m[:3, :3].T + m[:3, 3]
            world_verts = transform_points_f32(self.transform, mesh.verts)
        else:
            to_world, world_verts = (lambda p: np.asarray(p, np.float64)), mesh.verts
        self.world_tris = world_verts[mesh.faces]
        # origins: the first 8 of a fixed sequence of candidates that the float64 brute force finds interior (odd crossing
        # parity in three directions); for a well resolved mesh those are simply the first 8
        # (the float32 points inside a crumpled sliver are few and candidates round onto each other: distinct ones, up to 8)
        cand = to_world(mesh.interior_points(n=16384 if crumpled else 8, radius=0.9 if crumpled else 0.3).astype(np.float64)).astype(F)
        if crumpled:
            cand = cand[np.sort(np.unique(cand, axis=0, return_index=True)[1])]
        self.origins = cand[crossing_parity(self.world_tris, cand)][:8]
        targets = aim_points(world_verts, mesh.edges)
        self.inside_rays = rays_towards(self.origins, targets)
        self.inside_rays = self.inside_rays[np.isfinite(self.inside_rays).all(1)]  # (a target that rounds to the origin)
        self.outside_rays = self.outside_limit = None
        self.grazing_rays = self.inside_rays[:0]
        # slab-grazing rays: the first origin moved, for every 4th target, to 1e-3 of the mesh's size off the target's x, y or z
        # plane (at scale 1e-3 around 100 that rounds INTO the plane: a zero direction component, origin on box planes), kept
        # where the float64 brute force still finds the moved origin interior
        t4 = targets[::4]
        if len(self.origins) == 0:
            return
        moved = np.repeat(self.origins[:1].astype(np.float64), len(t4), 0)
        k = np.arange(len(t4)) % 3
        moved[np.arange(len(t4)), k] = t4[np.arange(len(t4)), k] - 1e-3 * np.abs(world_verts - to_world(mesh.centre)).max()
        g = np.concatenate([rays_towards(moved[i:i + 1], t4[i:i + 1]) for i in range(len(t4))])
        self.grazing_rays = g[np.isfinite(g).all(1) & crossing_parity(self.world_tris, g[:, 0:3], ndirs=2)]
        if name in CONVEX and not crumpled:
            self.outside_rays, self.outside_limit = rays_from_outside(to_world(mesh.centre), targets)

    @property
    def instances(self):
        return [(self.obj_tris, self.transform)]


@functools.lru_cache(maxsize=None)
def leak_case(name, placement, instanced):
    return LeakCase(name, placement, instanced)


# Scale 1e-3 at (100, 100, 100) puts the slivers' thickness (2e-5 and 2e-6) at or below the spacing of float32 there (7.6e-6):
# rounding crumples them.  They are still closed, so the inside properties hold for every origin of odd crossing parity, and
# LeakCase picks its origins by that parity; what goes is convexity, and with it the outside rays
# (tests/test_trace_reference_cpu.py::test_crumpled_slivers_are_closed_but_not_convex).
CRUMPLED = [("sliver-1e-2", "tiny-far"), ("sliver-1e-3", "tiny-far")]
LEAK_CASES = [(m, p, i) for m in MESHES for p in PLACEMENTS for i in (False, True)]


def concavity_in_spacings(tris):
    """How far, in spacings of float32 at the largest coordinate, some vertex lies on the wrong side of some face plane when
    the other side holds a vertex at least as far: 0 for a convex mesh."""
    t = np.asarray(tris, np.float64)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)
    d = (t.reshape(-1, 3)[None] - t[:, :1]) @ np.ones((3, 1)) * 0  # (shape only)
    d = np.einsum("fk,fvk->fv", n, t.reshape(1, -1, 3) - t[:, :1])
    return float(np.minimum(d.max(1), -d.min(1)).max() / np.spacing(F(np.abs(t).max())))


def thickness_in_ulps(verts):
    """Smallest principal extent of a vertex cloud (its thickness), in spacings of float32 at its largest coordinate."""
    v = np.asarray(verts, np.float64)
    proj = (v - v.mean(0)) @ np.linalg.svd(v - v.mean(0), full_matrices=False)[2][-1]
    return float((proj.max() - proj.min()) / np.spacing(F(np.abs(v).max())))


# ---- cases whose geometry arrives through a transform: what an edit of the instance table leaves behind ---------------------------
def affine(linear, offset=(0.0, 0.0, 0.0)):
    """Column-major 16 float32 of x -> linear x + offset."""
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = linear, offset
    return m.T.astype(F).reshape(16).copy()


def _edit_targets():
    r = random_rotation(11)
    return {"rotated": affine(random_rotation(12)),  # (the mesh's own rotation is random_rotation(5))
            "mirrored-stretched": instance_transform(),
            "shrunk-far": affine(r * 1e-3, (100.0, 100.0, 100.0)),
            "huge": affine(r * 1e4),
            "flattened": affine(r @ np.diag([1.0, 1e-4, 1.0]), (0.5, 0.5, 0.5))}


EDIT_TARGETS = _edit_targets()
EDIT_CASES = [(m, t) for m in MESHES for t in EDIT_TARGETS]
# Cases whose world-space mesh has fewer than 4 float32 points of odd crossing parity among the 16384 candidates: nothing to shoot
# from.  A list, so that collecting the GPU tests costs nothing; tests/test_trace_reference_cpu.py::test_edit_case_origins_are_
# interior measures every case and asserts that this list is exactly the cases it finds so.
EDIT_DROPPED = []


class EditCase(LeakCase):
    """ClosedMesh(name, "unit") as the object-space mesh of one instance under EDIT_TARGETS[target]; rays as LeakCase derives
    them for its instanced case.  Whether the world-space mesh is still what its name says is measured, not looked up: it keeps
    its 8 fixed origins and (if convex by construction) its outside rays where it is more than 16 float32 spacings thick and, for
    the meshes of CONVEX, no vertex lies a spacing or more beyond a face plane.  (The torus is concave by construction, by half
    its size: the concavity figure says nothing about rounding there, and it has no outside rays to lose, so thickness alone
    decides for it.)  Otherwise the case is treated as CRUMPLED is: origins by crossing parity, no outside rays."""

    def __init__(self, name, target, transform=None):
        mesh = ClosedMesh(name, "unit")
        self.key, self.target = (name, "edit", target), target
        transform = EDIT_TARGETS[target] if transform is None else transform
        world = transform_points_f32(transform, mesh.verts)[mesh.faces]
        self.thickness, self.concavity = thickness_in_ulps(world.reshape(-1, 3)), concavity_in_spacings(world)
        self.resolved = self.thickness > 16 and (name not in CONVEX or self.concavity < 1)
        self._derive(mesh, transform, not self.resolved)


@functools.lru_cache(maxsize=None)
def edit_case(name, target):
    return EditCase(name, target)


# The split scene: the lattice (12, seed 2) at scale 1 stays where it is, a small closed mesh beside its x = 0 face is edited.
# The mover's bounding ball (radius <= SPLIT_MOVER_RADIUS around a centre within SPLIT_MOVER_WOBBLE per axis of SPLIT_MOVER_CENTRE)
# is met by NO ray of the lattice's world_rays, so check_lattice holds in the scene of both as it does for the lattice alone, and the
# origins of the mover's outside rays, 3 radii out, lie short of x = 0 (tests/test_trace_reference_cpu.py::test_split_mover_stays_
# clear_of_the_lattice_and_its_rays).  Seen from the mover the lattice fills nearly the half space x > 0 (44 % of the outside rays and
# 47 % of the inside rays have it on their line beyond the mover): a ray that leaks out of the mover on that side names a lattice
# triangle, on the other side it misses.
SPLIT_LATTICE = (12, 2)
SPLIT_MOVER_RADIUS = 0.16
SPLIT_MOVER_WOBBLE = 0.03
SPLIT_MOVER_CENTRE = (-0.6, 8.0, 4.0)


def split_mover_transform(name, step):
    """The mover's transform after `step` edits: turned by 0.37 rad per step about (1, 2, 3), scaled between 0.8 and 1.0 of its
    start, moved within the wobble.  Step 0 is the placement the scene is uploaded with."""
    axis = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    rot = np.eye(3) + math.sin(0.37 * step) * k + (1 - math.cos(0.37 * step)) * (k @ k)
    scale = SPLIT_MOVER_RADIUS / (1.35 if name == "torus" else 1.0) * (1.0 - 0.2 * ((7 * step) % 11) / 10.0)
    wobble = np.array([(3 * step) % 7 / 3.0 - 1.0, (5 * step) % 11 / 5.0 - 1.0, (2 * step) % 5 / 2.0 - 1.0]) * SPLIT_MOVER_WOBBLE
    return affine(rot * scale, np.array(SPLIT_MOVER_CENTRE) + (wobble if step else 0.0))


@functools.lru_cache(maxsize=None)
def split_mover_case(name, step):
    case = EditCase(name, "split-%d" % step, split_mover_transform(name, step))
    assert case.resolved
    return case


def lattice_transform(placement):
    """The 16 floats that bring the integer lattice to LATTICE_PLACEMENTS[placement]."""
    scale, offset = LATTICE_PLACEMENTS[placement]
    return affine(np.eye(3) * scale, (offset, offset, offset))


def lattice_tris_through_transform(solid, placement):
    """The lattice triangles in lattice units as a float32 object-space mesh, brought to the world the way a float32 renderer
    does it -- and the assertion that this IS world_tris(scale, offset), bit for bit (powers of two and small integers: every
    product and every sum is exact), which is what lets the integer march stay the reference after an edit."""
    obj = solid.lattice_tris.astype(F)
    assert np.array_equal(obj.astype(np.int64), solid.lattice_tris)
    world = transform_points_f32(lattice_transform(placement), obj)
    want = solid.world_tris(*LATTICE_PLACEMENTS[placement])
    assert world.dtype == F and np.array_equal(world.view(np.uint32), want.view(np.uint32))
    return obj, world


def check_no_leaks(case, trace, who, prim_range=None):
    """trace(rays, any_hit) -> hit records.  Returns the number of rays checked.  prim_range = (first, count): every closest
    hit must name a triangle of that range -- in a scene with other objects a ray that leaks out of the mesh hits one of them."""

    def in_range(h, what):
        if prim_range is not None:
            bad = (h["prim"] < prim_range[0]) | (h["prim"] >= prim_range[0] + prim_range[1])
            assert not bad.any(), "%s %s: %d of %d %s hit a triangle outside [%d, %d) (first: ray %d, triangle %d)" % (
                who, case.key, bad.sum(), len(bad), what, prim_range[0], prim_range[0] + prim_range[1], np.nonzero(bad)[0][0], h["prim"][bad][0])

    h = trace(case.inside_rays, False)
    bad = h["prim"] < 0
    assert not bad.any(), "%s %s: %d of %d rays from inside leak out (first: ray %d)" % (who, case.key, bad.sum(), len(bad), np.nonzero(bad)[0][0])
    in_range(h, "rays from inside")
    a = trace(case.inside_rays, True)
    assert (a["prim"] == 0).all(), "%s %s: %d shadow rays from inside are not occluded" % (who, case.key, (a["prim"] != 0).sum())
    g = trace(case.grazing_rays, False)
    assert (g["prim"] >= 0).all(), "%s %s: %d of %d slab-grazing rays from inside leak out" % (who, case.key, (g["prim"] < 0).sum(), len(g))
    in_range(g, "slab-grazing rays from inside")
    assert (trace(case.grazing_rays, True)["prim"] == 0).all(), "%s %s: slab-grazing shadow rays from inside are not occluded" % (who, case.key)
    n = len(h) + len(g)
    if case.outside_rays is not None:
        r = case.outside_rays
        h = trace(r, False)
        dist = h["t"].astype(np.float64) * np.linalg.norm(r[:, 4:7].astype(np.float64), axis=1)
        bad = (h["prim"] < 0) | ~(dist < case.outside_limit)
        assert not bad.any(), "%s %s: %d of %d rays from outside pass the near surface (first: ray %d)" % (
            who, case.key, bad.sum(), len(bad), np.nonzero(bad)[0][0])
        in_range(h, "rays from outside")
        sh = r.copy()
        sh[:, 7] = (case.outside_limit / np.linalg.norm(r[:, 4:7].astype(np.float64), axis=1)).astype(F)  # up to the centre only
        a = trace(sh, True)
        assert (a["prim"] == 0).all(), "%s %s: %d shadow rays from outside pass the near surface" % (who, case.key, (a["prim"] != 0).sum())
        n += len(r)
    return n


def check_lattice(ref, scale, offset, trace, who):
    """Lattice rays: closest hits and both ends of the range.  Returns the worst relative t error of the closest hits."""
    rays = ref.solid.world_rays(scale, offset)
    h = trace(rays, False)
    worst = check_lattice_closest(ref, h, scale, who)
    r = rays.copy()
    r[:, 7] = (ref.first * scale * (1 + LATTICE_TOL)).astype(F)
    a = trace(r, True)
    assert (a["prim"] == 0).all(), "%s: %d lattice shadow rays reaching past the crossing are not occluded" % (who, (a["prim"] != 0).sum())
    r[:, 7] = (ref.first_any * scale * (1 - LATTICE_TOL)).astype(F)
    a = trace(r, True)
    assert (a["prim"] == -1).all(), "%s: %d lattice shadow rays ending before the surface are occluded" % (who, (a["prim"] != -1).sum())
    r = rays.copy()
    r[:, 3] = (ref.first * scale * (1 + LATTICE_TOL)).astype(F)
    h2 = trace(r, False)
    check_lattice_closest(ref, h2, scale, who + " (tmin past the first crossing)", ref.admissible_next, ~np.isnan(ref.nxt))
    return worst


# ---- range consistency on slivers: what the leaf-box pad is for ---------------------------------------------------------------
# (length, width) of the slivers: aspect (longest edge)^2 / (2 area) = 2 length / width from 3e3 to 2e7, on both sides of every
# threshold a pad rule could have (the pad of oracle and k_bake grows with the aspect up to 32768 and changes form there).
SLIVER_SHAPES = [(3.0, 2e-3), (3.0, 2e-4), (3.0, 2e-5), (3.0, 6.7e-6), (3.0, 3e-6), (3.0, 3e-7), (0.3, 2e-5)]


@functools.lru_cache(maxsize=None)
def sliver_case(length, width, seed=0, n=60, per=400):
    """60 axis-aligned slivers (long axis, width axis and normal a random permutation of x, y, z: the box is thin on two axes)
    and 400 rays at interior points of each, from 0.5 to 8 away, their components along the width and the normal shrunk by
    random factors down to 1e-4: rays that graze the sliver along its length, where the float32 t of a sliver is worst."""
    rng = np.random.RandomState(seed)
    c = rng.uniform(-1, 1, (n, 3))
    perm = np.array([rng.permutation(3) for _ in range(n)])
    a, b, nn = (np.eye(3)[perm[:, k]][:, None] for k in range(3))
    tris = np.stack([c - length * a[:, 0], c + length * a[:, 0], c + width * b[:, 0]], 1).astype(F)
    s = rng.uniform(-0.9, 0.9, (n, per, 1))
    p = c[:, None] + s * length * a + rng.uniform(0.05, 0.95, (n, per, 1)) * (1 - np.abs(s)) * width * b
    d = rng.normal(size=(n, per, 3))
    d = a * (d * a).sum(2, keepdims=True) + b * (d * b).sum(2, keepdims=True) * 10.0 ** rng.uniform(-4, 0, (n, per, 1)) \
        + nn * (d * nn).sum(2, keepdims=True) * 10.0 ** rng.uniform(-4, 0, (n, per, 1))
    o = p - d / np.linalg.norm(d, axis=2, keepdims=True) * rng.uniform(0.5, 8, (n, per, 1))
    return tris, np.concatenate([rays_towards(o.reshape(-1, 3)[i:i + 1], p.reshape(-1, 3)[i:i + 1]) for i in range(n * per)])


def check_range_consistency(rays, trace, who, min_hits=0):
    """A reported hit does not depend on tmax as long as tmax lies beyond it: with tmax = t (1 + 2^-20), eight float32 spacings
    past the reported t, the closest hit is the same record bit for bit and the shadow ray is occluded.  No tolerance and no
    reference: a tracer that culls the box of a triangle whose own test reports a hit (a pad too small for the t the test
    reports) answers differently, and which of two surfaces wins then depends on the order they are met in."""
    h = trace(rays, False)
    m = h["prim"] >= 0
    assert m.sum() > min_hits, "%s: only %d of %d rays hit" % (who, m.sum(), len(rays))
    r = rays[m].copy()
    r[:, 7] = h["t"][m] * F(1 + 2.0 ** -20)
    assert (r[:, 7] > h["t"][m]).all()
    h2 = trace(r, False)
    bad = (h2["prim"] != h["prim"][m]) | (h2["t"] != h["t"][m]) | (h2["u"] != h["u"][m]) | (h2["v"] != h["v"][m])
    assert not bad.any(), "%s: %d of %d hits change or vanish when tmax shrinks to just beyond them" % (who, bad.sum(), m.sum())
    a = trace(r, True)
    assert (a["prim"] == 0).all(), "%s: %d of %d shadow rays reaching past a reported hit are free" % (who, (a["prim"] != 0).sum(), m.sum())
    return int(m.sum())
