"""What a pixel filter costs on the GPU (include/gpuspectral_pt.h, "Pixel filter").

A filtered frame traces the camera rays the primary-hit memo answers for an unfiltered one, and draws two variates per sample.
On bench.py's workload (its own generator, at its resolution and samples per step) this renders, in ONE process, interleaved,
`--reps` times each after a warm-up:

    none        the default: unfiltered, memo on
    none/memo2  unfiltered with gsp_ctx_options.primary_memo = 2 (every camera ray traced): the fair baseline of a filter
    box, tent, gaussian

and writes ms per step (median, min, max, spread), the traced rays and -- from one more pass with collect_kernel_times --
the extend / shade / connect kernel time.  Two statements are checked against the run's own numbers and printed as
PASS / FAIL: filtered is not slower than none/memo2 by more than the spread the run shows.

    python tests/tools/pixel_filter_probe.py [--reps 5] [--out profiles/pixel_filter_cost.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the workload generator only: bench.make_scene)
import gpuspectral_amd as g  # noqa: E402
from gpuspectral_amd import abi  # noqa: E402

CONFIGS = [("none", "memo", abi.FILTER_NONE), ("none/memo2", "nomemo", abi.FILTER_NONE), ("box", "memo", abi.FILTER_BOX),
           ("tent", "memo", abi.FILTER_TENT), ("gaussian", "memo", abi.FILTER_GAUSSIAN)]


def step(ctx, W, H, spp, filt, **kw):
    ctx.frame_begin(W, H)
    ctx.reset_stats()
    t0 = time.perf_counter()
    ctx.render(spp=spp, pixel_filter=filt, **kw)
    ctx.sync()
    ms = (time.perf_counter() - t0) * 1e3
    return ms, ctx.stats()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixel_filter_cost.txt"))
    a = ap.parse_args()
    bargs = argparse.Namespace(scene="interior", tris=1_000_000)
    sc, what = bench.make_scene(bargs)
    W, H, SPP = 1920, 1080, 64  # bench.py's defaults
    lines = ["pixel filter cost: %s, %dx%d, %d spp per step, %d repetitions per configuration, interleaved, one process" % (what, W, H, SPP, a.reps),
             "library %s" % g.pt.build_info()]
    # two contexts on the one device, each with a quarter of its memory: the same pool size for every configuration
    ctxs = {"memo": g.Context(0, memory_share=0.25), "nomemo": g.Context(0, memory_share=0.25, primary_memo=2)}
    for c in ctxs.values():
        c.upload_scene(sc)
    for name, which, filt in CONFIGS:  # warm-up: pools, queues, memo
        step(ctxs[which], W, H, SPP, filt)
    ms = {name: [] for name, _, _ in CONFIGS}
    rays = {}
    for _ in range(a.reps):
        for name, which, filt in CONFIGS:
            t, st = step(ctxs[which], W, H, SPP, filt)
            ms[name].append(t)
            rays[name] = st
    kt = {}
    for name, which, filt in CONFIGS:
        _, st = step(ctxs[which], W, H, SPP, filt, collect_kernel_times=1)
        kt[name] = st
    lines.append("%-11s %9s %9s %9s %8s %14s %14s %14s %10s %10s %10s" % ("config", "median ms", "min ms", "max ms", "spread", "traced ext", "memoised",
                                                                    "shadow rays", "extend ms", "shade ms", "connect ms"))
    med = {}
    for name, _, _ in CONFIGS:
        v = ms[name]
        med[name] = statistics.median(v)
        st, k = rays[name], kt[name]
        lines.append("%-11s %9.2f %9.2f %9.2f %7.2f%% %14d %14d %14d %10.2f %10.2f %10.2f"
                     % (name, med[name], min(v), max(v), 100 * (max(v) - min(v)) / med[name], st["extension_rays"] - st["memoised_rays"],
                        st["memoised_rays"], st["shadow_rays"], k["extend_kernel_ms"], k["shade_kernel_ms"], k["connect_kernel_ms"]))
    spread = max((max(v) - min(v)) / statistics.median(v) for v in ms.values())
    lines.append("largest run-to-run spread of a configuration: %.2f %%" % (100 * spread))
    base = med["none/memo2"]
    ok = True
    for name in ("box", "tent", "gaussian"):
        rel = med[name] / base - 1.0
        good = rel <= spread
        ok = ok and good
        lines.append("%-9s vs none/memo2: %+.2f %%  (vs none: %+.2f %%)  %s" % (name, 100 * rel, 100 * (med[name] / med["none"] - 1.0),
                                                                            "PASS" if good else "FAIL: slower than the baseline by more than the spread"))
    lines.append("none/memo2 vs none (what the memo saves): %+.2f %%" % (100 * (base / med["none"] - 1.0)))
    for c in ctxs.values():
        c.close()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
