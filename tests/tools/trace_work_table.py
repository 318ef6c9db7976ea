"""Prints profiles/trace_work_cpu.txt: the measured cells behind the gate of tests/test_trace_work_cpu.py -- the product's
emulation and its four mutants, R = sum(nodes per ray) / sum(W_sorted) and sum(nodes per ray) / sum(W_min) per scene and octant.

    python tests/tools/trace_work_table.py > profiles/trace_work_cpu.txt
"""
import os
import pathlib
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import conftest  # noqa: E402
import test_trace_work_cpu as T  # noqa: E402
import trace_work as W  # noqa: E402


def main():
    conftest.Emu()  # builds tests/emu/libpt_emu.so
    product = T.EmuLib(os.path.join(T.ROOT, "tests", "emu", "libpt_emu.so"))
    made = {name: T.Case(product, name) for name in T.SCENES}
    cases = made.__getitem__
    print("Work per ray on the CPU: trace_ray<false> of the product's headers (tests/emu/pt_emu.cpp, median-split 4-wide tree written by")
    print("encode_node_w4) against tests/trace_work.py.  8 x 1500 rays per scene and sign octant (bit a of the octant = direction negative on")
    print("axis a) + 1500 rays with one zero component.  R = sum(nodes_per_ray) / sum(W_sorted); gate per cell = product's R + %.2f." % T.GATE_MARGIN)
    print()
    for name in T.SCENES:
        c = cases(name)
        leaves, inner, cut, excess = W.check_decode_contains(c.tree)
        n = sum(len(r) for _, r in c.groups)
        print("%-9s %5d triangles, %4d records; mean per ray: product %.2f records %.2f triangles, W_sorted %.2f records %.2f triangles, W_min %.2f records"
              % (name, leaves, len(c.tree.nodes), sum(g[1].sum() for g in c.got) / n, sum(g[2].sum() for g in c.got) / n,
                 sum(r.w_sorted.sum() for r in c.ref) / n, sum(r.tris_sorted.sum() for r in c.ref) / n, sum(r.w_min.sum() for r in c.ref) / n))
        print("          real-number decoded planes cut at most %.2f float32 spacings into a padded leaf box (none after the decode's one rounding);"
              % max(cut, 0.0))
        print("          a child's decoded children reach past its own decoded box by at most %.2e of that box (decoded boxes are not nested)" % max(excess, 0.0))
    print()
    T.print_table("product", {name: T.ratios(cases(name), cases(name).got) for name in T.SCENES})
    for mutant in T.MUTANTS:
        print()
        with tempfile.TemporaryDirectory() as d:
            table = T.mutant_table(T.build_mutant(pathlib.Path(d), mutant), cases, mutant)
        T.print_table(mutant, table)
        print("%-28s hits bit-equal to the product's; cells above their gate: %d of 24" % (mutant, len(T.check_gate(table))))


if __name__ == "__main__":
    main()
