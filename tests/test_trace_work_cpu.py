"""The product's per-ray traversal (trace_ray<false> with the product's encoder, step table and node step, on the host:
tests/emu/pt_emu.cpp emu_trace_work) against the two plain references of tests/trace_work.py, on the emulation's own tree.

Hits cannot see any of this: a flipped sign in order_key, exchanged octant bits or a far bound that never shrinks leave every hit,
frame and ray count bit-equal and only make a ray read more node records.  So the WORK is held: never less than the ideal, and --
per scene and sign octant -- no worse against the textbook exact-sort traversal than measured (profiles/trace_work_cpu.txt), with
four mutants of the product's headers shown, in this run, to fail that gate with unchanged hits.

Any-hit work is not counted here (trace_ray<true> reads no step table, which is where the counting sits); it is measured on the GPU
in tests/test_gpu_trace_work.py.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import trace_reference as R
import trace_work as W
from trace_scenes import build_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ("lattice", "materials", "soup")
GXX = ["g++", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mfma", "-mavx2", "-shared"]

# The gate of test_static_order_is_as_good_as_the_exact_sort: R = sum(nodes_per_ray) / sum(W_sorted) per (scene, octant) cell, as
# measured (profiles/trace_work_cpu.txt, printed by tests/tools/trace_work_table.py), + 0.02.  One gate for all cells -- the worst
# cell + 0.02 = 1.352 -- would let the `octhi inverted` mutant through (its worst cell is 1.33, on a scene where the product's own
# is 1.33; it moves the lattice from 1.10 to 1.25), so every cell is held to its own figure.
MEASURED_R = {
    "lattice": (1.1037, 1.1133, 1.1099, 1.1246, 1.0911, 1.1215, 1.0937, 1.1254),
    "materials": (1.0924, 1.0875, 1.1787, 1.3320, 0.9060, 1.0091, 1.0208, 1.2372),
    "soup": (1.0945, 1.1193, 1.0832, 1.1034, 1.0809, 1.1156, 1.0919, 1.0891),
}
GATE_MARGIN = 0.02


def make_scene(name):
    from gpuspectral_amd import scenes

    if name == "lattice":
        return build_scene([(W.lattice(6), None)])
    if name == "materials":
        return scenes.cornell_materials(8)
    return build_scene([(R.soup(), None)])


class EmuLib:
    """emu_trace_work / emu_tree of one build of tests/emu/pt_emu.cpp."""

    def __init__(self, so):
        from gpuspectral_amd import abi

        self.L = L = C.CDLL(so)
        L.emu_create.restype = C.c_void_p
        L.emu_create.argtypes = [C.POINTER(abi.SceneDesc)]
        L.emu_destroy.argtypes = [C.c_void_p]
        L.emu_trace_work.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.emu_tree.argtypes = [C.c_void_p] + [C.c_void_p] * 8
        L.emu_tree.restype = None

    def scene(self, sc):
        self._desc = sc.desc()
        return self.L.emu_create(C.byref(self._desc))

    def destroy(self, h):
        self.L.emu_destroy(h)

    def tree(self, h):
        p = [C.c_void_p() for _ in range(8)]
        n = [C.c_uint64() for _ in range(3)]
        self.L.emu_tree(h, C.byref(p[0]), C.byref(n[0]), C.byref(p[1]), C.byref(n[1]), C.byref(n[2]), C.byref(p[2]), C.byref(p[3]), C.byref(p[4]))

        def arr(ptr, count, dtype):
            return np.frombuffer((C.c_char * (count * np.dtype(dtype).itemsize)).from_address(ptr.value), dtype).copy()

        nn, ns, nr = n[0].value, n[1].value, n[2].value
        return W.Tree(arr(p[0], 16 * nn, np.uint32), arr(p[1], 12 * ns, np.float32), nr, arr(p[2], 3 * ns, np.float32).reshape(-1, 3).astype(np.float64),
                      arr(p[3], 3 * ns, np.float32).reshape(-1, 3).astype(np.float64), arr(p[4], ns, np.uint32))

    def trace_work(self, h, rays):
        from oracle.oracle import HIT_DT

        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        hits, nodes, tris = np.zeros(len(rays), HIT_DT), np.zeros(len(rays), np.uint32), np.zeros(len(rays), np.uint32)
        assert self.L.emu_trace_work(h, rays.ctypes.data, len(rays), 0, hits.ctypes.data, nodes.ctypes.data, tris.ctypes.data) == 0
        return hits, nodes, tris


class Case:
    """One scene on the product's emulation: its tree, the nine groups of rays, the references and the product's work."""

    def __init__(self, lib, name):
        self.name, self.sc = name, make_scene(name)
        h = lib.scene(self.sc)
        self.tree = lib.tree(h)
        t = self.tree.triangles.reshape(-1, 3).astype(np.float64)
        self.groups = W.work_rays(t.min(0), t.max(0), seed=SCENES.index(name))
        self.ref = [W.Work(self.tree, rays) for _, rays in self.groups]
        self.got = [lib.trace_work(h, rays) for _, rays in self.groups]
        lib.destroy(h)


def ratios(case, got):
    """Per group of rays: (sum nodes / sum W_sorted, sum nodes / sum W_min)."""
    return [(float(g[1].sum(dtype=np.float64) / r.w_sorted.sum(dtype=np.float64)), float(g[1].sum(dtype=np.float64) / r.w_min.sum(dtype=np.float64)))
            for g, r in zip(got, case.ref)]


@pytest.fixture(scope="module")
def product(emu):  # (the session's `emu` has built tests/emu/libpt_emu.so from the tree's sources)
    return EmuLib(os.path.join(ROOT, "tests", "emu", "libpt_emu.so"))


@pytest.fixture(scope="module")
def cases(product):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(product, name)
        return made[name]

    return get


@pytest.mark.parametrize("name", SCENES)
def test_decode_contains(cases, name):
    """The decoder written from the layout comment reads the product's records: leaf boxes contain their triangles' padded boxes,
    inner boxes the padded boxes of everything under them, the topology is a tree over all records and slots.  The C++ decode
    the per-ray references use is the same decode.  Decoded boxes are NOT nested, and the real-number plane is outward only after
    its one float32 rounding (W.check_decode_contains; figures in profiles/trace_work_cpu.txt)."""
    tree = cases(name).tree
    leaves, inner, cut, excess = W.check_decode_contains(tree)
    for a, b in zip(W.decode_nodes(tree.nodes), W.decode_nodes_cxx(tree.nodes)):
        assert np.array_equal(a, b)
    assert {"lattice": 2592, "materials": 932, "soup": 1000}[name] == tree.num_real == leaves and inner == len(tree.nodes) - 1
    print("%s: %d records, %d leaf children, %d inner children; real-number planes cut %.2f float32 spacings into a padded box; "
          "a child's decoded children exceed its decoded box by %.2e of it" % (name, len(tree.nodes), leaves, inner, max(cut, 0.0), max(excess, 0.0)))


@pytest.mark.parametrize("name", SCENES)
def test_never_less_than_the_ideal(cases, name):
    """The product's box test is looser than the exact one, and it cannot know the hit in advance: every ray reads at least the
    records whose boxes the segment up to the float64 hit enters.  No tolerance."""
    case = cases(name)
    for (label, _), ref, (_, nodes, _) in zip(case.groups, case.ref, case.got):
        bad = nodes < ref.w_min
        assert not bad.any(), "%s, %s: %d rays read fewer records than the ideal (first: ray %d, %d < %d)" % (
            name, label, bad.sum(), np.nonzero(bad)[0][0], nodes[bad][0], ref.w_min[bad][0])


@pytest.mark.parametrize("name", SCENES)
def test_same_hits(cases, name):
    """The product's hit is the float64 brute force's -- hit or miss, the triangle, and t within the tolerance of
    tests/trace_reference.py -- on the rays that its clear-winner criterion keeps (at most 2 % of a scene's rays are left out, as
    there), and the brute force of trace_work_ref.cpp names the same triangle as that one's.  (The barycentric tolerance of
    trace_reference belongs to its own rays -- it was measured on them -- and is not applied to these: the sphere's small
    triangles seen from four room sizes away give u, v a larger float32 error in any algorithm.)"""
    case = cases(name)
    world = np.zeros((case.tree.num_real, 3, 3), np.float32)
    world[case.tree.slot_to_global[:case.tree.num_real]] = case.tree.triangles  # global id order
    unclear = total = 0
    for (label, rays), ref, (hits, _, _) in zip(case.groups, case.ref, case.got):
        sr = R.SoupReference(world, rays)
        c, m = sr.clear, sr.clear & sr.hit
        unclear, total = unclear + int((~c).sum()), total + len(rays)
        assert np.array_equal(hits["prim"][c], sr.prim[c]), "%s, %s: another triangle than the brute force's nearest (or hit / miss differs) on %d clear rays" % (
            name, label, (hits["prim"][c] != sr.prim[c]).sum())
        dt = np.abs(hits["t"][m].astype(np.float64) - sr.best_t[m]) / (sr.best_tol[m] / R.TOL_T_UNITS)
        assert dt.max() <= R.TOL_T_UNITS, (name, label, dt.max())
        mine = np.where(ref.slot >= 0, case.tree.slot_to_global[np.maximum(ref.slot, 0)].astype(np.int64), -1)
        assert np.array_equal(mine[c], sr.prim[c])
        assert np.abs(ref.t_hit[m] - sr.best_t[m]).max() <= 1e-9 * np.abs(sr.best_t[m]).max()
    assert unclear <= 0.02 * total, (name, unclear, total)


def check_gate(table):
    """table: {scene: ratios(...)}.  The first eight groups are the octants; the rays with a zero component are reported only.
    Returns the cells above their gate as (scene, octant, R, gate)."""
    return [(name, k, table[name][k][0], MEASURED_R[name][k] + GATE_MARGIN) for name in SCENES for k in range(8)
            if not table[name][k][0] <= MEASURED_R[name][k] + GATE_MARGIN]


def print_table(who, table):
    for name in SCENES:
        print("%-28s %-9s R per octant : %s | zero component %.4f" % (who, name, " ".join("%.4f" % r[0] for r in table[name][:8]), table[name][8][0]))
        print("%-28s %-9s nodes / W_min: %s | zero component %.4f" % (who, name, " ".join("%.4f" % r[1] for r in table[name][:8]), table[name][8][1]))


def test_static_order_is_as_good_as_the_exact_sort(cases):
    """R = sum(nodes_per_ray) / sum(W_sorted) per scene and octant is at most what was measured + 0.02
    (profiles/trace_work_cpu.txt): the build-time order by box centres on the octant's diagonal, walked without stored entry
    distances, costs 8 to 12 % over the exact per-node distance sort with culling of stacked records on the lattice and the soup,
    and up to 33 % on the materials scene (octant 3) -- on the emulation's median-split tree; the sentence this test replaces in
    pt_trace.h claimed equality on another tree and scene."""
    table = {name: ratios(cases(name), cases(name).got) for name in SCENES}
    print_table("product", table)
    bad = check_gate(table)
    assert not bad, "cells above their gate (scene, octant, R, gate): %s" % bad


# ---- the gate sees what it is for ---------------------------------------------------------------------------------------------------
MUTANTS = {
    "order_key negated": ("return ((oct & 1 ? -cx : cx) + (oct & 2 ? -cy : cy)) + (oct & 4 ? -cz : cz);",
                          "return -(((oct & 1 ? -cx : cx) + (oct & 2 ? -cy : cy)) + (oct & 4 ? -cz : cz));"),
    "octhi inverted": ("r.octhi = r.negz;", "r.octhi = !r.negz;"),
    "octshift x and y exchanged": ("r.octshift = (r.negx ? 7u : 0u) + (r.negy ? 14u : 0u);", "r.octshift = (r.negy ? 7u : 0u) + (r.negx ? 14u : 0u);"),
    "culling never shrinks": ("node_step<ANY>(n, rb, tmin, h.t, tab, ngb, ngs, tb, tm);", "node_step<ANY>(n, rb, tmin, tmax, tab, ngb, ngs, tb, tm);"),
}


def build_mutant(tmp_path, mutant):
    """A copy of gpuspectral_amd/csrc (+ the public header and the harness) with one textual replacement in pt_trace.h, which must
    match exactly once, built into its own emulation library."""
    root = tmp_path / "tree"
    shutil.copytree(os.path.join(ROOT, "gpuspectral_amd", "csrc"), root / "gpuspectral_amd" / "csrc", ignore=shutil.ignore_patterns("build", "*.o", "*.so"))
    shutil.copytree(os.path.join(ROOT, "include"), root / "include")
    os.makedirs(root / "tests" / "emu")
    shutil.copy(os.path.join(ROOT, "tests", "emu", "pt_emu.cpp"), root / "tests" / "emu")
    old, new = MUTANTS[mutant]
    path = root / "gpuspectral_amd" / "csrc" / "pt_trace.h"
    text = path.read_text()
    assert text.count(old) == 1, "%s: the text to replace occurs %d times" % (mutant, text.count(old))
    # (the encoder's device form restates order_key inline: the harness builds its tree through the definition instead, so that the
    # ONE replacement reaches the tree; the two forms agree bit for bit, tests/test_emu_parity.py::test_node_encoder_forms_agree)
    path.write_text(text.replace(old, new))
    src = root / "tests" / "emu" / "pt_emu.cpp"
    s = src.read_text()
    assert s.count("encode_node_w4(out, wc, ni, nl, child_base, tri_base);") == 1
    src.write_text(s.replace("encode_node_w4(out, wc, ni, nl, child_base, tri_base);", "encode_node_w4_ref(out, wc, ni, nl, child_base, tri_base);"))
    so = str(tmp_path / "libpt_emu_mutant.so")
    subprocess.check_call(GXX + ["-O1", "-o", so, str(src)])
    return EmuLib(so)


def mutant_table(lib, cases, mutant):
    """The ratios of a mutant library on the cases' rays, after asserting that every hit record is the product's, bit for bit."""
    table = {}
    for name in SCENES:
        case = cases(name)
        h = lib.scene(case.sc)
        got = [lib.trace_work(h, rays) for _, rays in case.groups]
        lib.destroy(h)
        for (label, _), a, b in zip(case.groups, got, case.got):
            assert a[0].tobytes() == b[0].tobytes(), "%s: hits differ from the product's on %s, %s" % (mutant, name, label)
        table[name] = ratios(case, got)
    return table


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_the_gate_fails_on_a_mutant_with_unchanged_hits(cases, tmp_path, mutant):
    """One textual replacement in a copy of the product's pt_trace.h: every hit record stays bit-equal to the product's, and the
    gate of test_static_order_is_as_good_as_the_exact_sort fails.  Each mutant alters the visiting order or leaves a culling
    bound at its conservative start value: none can change a result."""
    lib = build_mutant(tmp_path, mutant)
    table = mutant_table(lib, cases, mutant)
    print_table(mutant, table)
    assert check_gate(table), "%s passes the gate in every cell" % mutant
    moved = max(table[name][k][0] / ratios(cases(name), cases(name).got)[k][0] for name in SCENES for k in range(8))
    assert moved >= 1.10, "%s moves no cell by 10 %% (largest: %.3f): the scenes are too weak" % (mutant, moved)
