"""What the thin lens costs on the GPU (include/gpuspectral_pt.h, "Thin lens").

A lens frame traces the camera rays the primary-hit memo answers for a pinhole frame -- as a filtered frame does -- draws two
more variates per sample, and its camera rays start from different points of the aperture, so they are slightly less coherent.
On bench.py's workload (its own generator, at its resolution and samples per step) this renders, in ONE process, interleaved,
`--reps` times each after a warm-up:

    pinhole        the default: memo on
    pinhole/memo2  gsp_ctx_options.primary_memo = 2 (every camera ray traced)
    box            BOX pixel filter: the same memo bypass as a lens -- the comparison that matters
    lens           circular aperture, focused on what the centre pixel shows (gsp_focus_distance)
    lens+box       both

and writes ms per step (median, min, max, spread), the traced rays and -- from one more pass with collect_kernel_times -- the
extend / shade / connect kernel time.  Checked against the run's own numbers and printed as PASS / FAIL: lens is not slower than
box, and lens+box not slower than box, by more than the spread the run shows.

    python tests/tools/lens_probe.py [--reps 5] [--radius-fraction 0.01] [--out profiles/lens_cost.txt]
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

CONFIGS = [("pinhole", "memo", abi.FILTER_NONE, False), ("pinhole/memo2", "nomemo", abi.FILTER_NONE, False), ("box", "memo", abi.FILTER_BOX, False),
           ("lens", "memo", abi.FILTER_NONE, True), ("lens+box", "memo", abi.FILTER_BOX, True)]


def step(ctx, W, H, spp, filt, lens, **kw):
    if lens:
        ctx.set_lens(**lens)
    else:
        ctx.set_lens()
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
    ap.add_argument("--radius-fraction", type=float, default=0.01, help="aperture radius as a fraction of the focus distance")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lens_cost.txt"))
    a = ap.parse_args()
    bargs = argparse.Namespace(scene="interior", tris=1_000_000)
    sc, what = bench.make_scene(bargs)
    W, H, SPP = 1920, 1080, 64  # bench.py's defaults
    # two contexts on the one device, each with a quarter of its memory: the same pool size for every configuration
    ctxs = {"memo": g.Context(0, memory_share=0.25), "nomemo": g.Context(0, memory_share=0.25, primary_memo=2)}
    for c in ctxs.values():
        c.upload_scene(sc)
    D = float(ctxs["memo"].focus_distance(W, H, W / 2.0, H / 2.0))
    if not D > 0:
        D = 1.0
    the_lens = dict(radius=a.radius_fraction * D, focus_distance=D)
    lines = ["lens cost: %s, %dx%d, %d spp per step, %d repetitions per configuration, interleaved, one process" % (what, W, H, SPP, a.reps),
             "library %s" % g.pt.build_info(), "lens: autofocus on the centre pixel: focus distance %.4f, radius %.5f, circular aperture" % (D, the_lens["radius"])]
    for name, which, filt, lens in CONFIGS:  # warm-up: pools, queues, memo
        step(ctxs[which], W, H, SPP, filt, the_lens if lens else None)
    ms = {c[0]: [] for c in CONFIGS}
    rays = {}
    for _ in range(a.reps):
        for name, which, filt, lens in CONFIGS:
            t, st = step(ctxs[which], W, H, SPP, filt, the_lens if lens else None)
            ms[name].append(t)
            rays[name] = st
    kt = {}
    for name, which, filt, lens in CONFIGS:
        _, st = step(ctxs[which], W, H, SPP, filt, the_lens if lens else None, collect_kernel_times=1)
        kt[name] = st
    lines.append("%-13s %9s %9s %9s %8s %14s %14s %14s %10s %10s %10s" % ("config", "median ms", "min ms", "max ms", "spread", "traced ext", "memoised",
                                                                    "shadow rays", "extend ms", "shade ms", "connect ms"))
    med = {}
    for name, _, _, _ in CONFIGS:
        v = ms[name]
        med[name] = statistics.median(v)
        st, k = rays[name], kt[name]
        lines.append("%-13s %9.2f %9.2f %9.2f %7.2f%% %14d %14d %14d %10.2f %10.2f %10.2f"
                     % (name, med[name], min(v), max(v), 100 * (max(v) - min(v)) / med[name], st["extension_rays"] - st["memoised_rays"],
                        st["memoised_rays"], st["shadow_rays"], k["extend_kernel_ms"], k["shade_kernel_ms"], k["connect_kernel_ms"]))
    spread = max((max(v) - min(v)) / statistics.median(v) for v in ms.values())
    lines.append("largest run-to-run spread of a configuration: %.2f %%" % (100 * spread))
    base = med["box"]
    ok = True
    for name in ("lens", "lens+box"):
        rel = med[name] / base - 1.0
        good = rel <= spread
        ok = ok and good
        lines.append("%-9s vs box: %+.2f %%  (vs pinhole/memo2: %+.2f %%, vs pinhole: %+.2f %%)  %s"
                     % (name, 100 * rel, 100 * (med[name] / med["pinhole/memo2"] - 1.0), 100 * (med[name] / med["pinhole"] - 1.0),
                        "PASS" if good else "FAIL: slower than the box filter by more than the spread"))
    lines.append("pinhole/memo2 vs pinhole (what the memo saves): %+.2f %%" % (100 * (med["pinhole/memo2"] / med["pinhole"] - 1.0)))
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
