"""What a feature pass costs next to a beauty pass.

In ONE process on ONE context, on bench.py's workload (scenes.interior(1_000_000, seed=7)) at 1920x1080: interleaved repetitions
of a 16-spp gsp_render_features and a 16-spp gsp_render (each timed to completion: gsp_render_features returns complete,
gsp_render is followed by gsp_sync), for no filter and for the tent filter, and their medians.

    python tests/tools/features_probe.py [--reps 5] [--out FILE]   (default: profiles/features_cost.txt)
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "features_cost.txt"))
    a = ap.parse_args()
    assert a.reps >= 5, "at least 5 repetitions"

    import gpuspectral_amd as g
    from gpuspectral_amd import abi, scenes

    sc = scenes.interior(a.tris, seed=7)
    lines = ["feature pass vs beauty pass: scenes.interior(%d, seed=7) at %dx%d, %d spp per call, %d interleaved repetitions, one context"
             % (a.tris, a.width, a.height, a.spp, a.reps), "library " + str(g.pt.build_info())]
    with g.Context(0) as ctx:
        ctx.upload_scene(sc)
        ctx.frame_begin(a.width, a.height)
        for name, filt in (("no filter", abi.FILTER_NONE), ("tent", abi.FILTER_TENT)):
            ctx.render_features(1, 0, pixel_filter=filt)  # warm-up: allocations, first launches
            ctx.render(1, 0, pixel_filter=filt)
            ctx.sync()
            tf, tb = [], []
            for r in range(a.reps):
                ctx.frame_begin(a.width, a.height)
                t0 = time.perf_counter()
                ctx.render_features(a.spp, 0, pixel_filter=filt)
                t1 = time.perf_counter()
                ctx.render(a.spp, 0, pixel_filter=filt)
                ctx.sync()
                t2 = time.perf_counter()
                tf.append((t1 - t0) * 1e3)
                tb.append((t2 - t1) * 1e3)
            mf, mb = statistics.median(tf), statistics.median(tb)
            lines.append("%-10s features %8.2f ms (min %.2f max %.2f)   beauty %9.2f ms (min %.2f max %.2f)   features / beauty = %.4f"
                         % (name, mf, min(tf), max(tf), mb, min(tb), max(tb), mf / mb))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
