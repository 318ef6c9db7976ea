"""What a viewer pays per displayed frame, before and after the LDR film.

In ONE process on ONE context at 1920x1080, with the frame rendered and idle, interleaved repetitions of
  peek            gsp_peek alone (33 MB RGBA32F over PCIe)
  peek+host       gsp_peek + toneMapToRgb8 on the host: the path a viewer had before
  display clamp   gsp_peek_display, CLAMP + gamma 2.2 (8.3 MB RGBA8 over PCIe)
  display reinh   gsp_peek_display, REINHARD with measured luminances (k_display_stats + k_display_map)
and their medians.  --kernels-only runs the two display calls a few times and nothing else: the run to put under
`rocprofv3 --kernel-trace --stats` for the kernels' own durations; --kernel-stats CSV merges that run's kernel_stats file into
the JSON.

    python tests/tools/display_probe.py [--reps 15] [--out profiles/display_probe.json] [--kernel-stats FILE.csv]
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()

    import gpuspectral_amd as g
    from gpuspectral_amd import abi, host, scenes

    W, H = a.width, a.height
    clamp = abi.display(tonemap=abi.TONEMAP_CLAMP, gamma=2.2)
    reinhard = abi.display(tonemap=abi.TONEMAP_REINHARD, gamma=2.2)
    with g.Context(0) as ctx:
        ctx.upload_scene(scenes.cornell_materials(16))
        ctx.frame_begin(W, H)
        ctx.render(spp=a.spp)
        ctx.sync()
        if a.kernels_only:
            for _ in range(10):
                ctx.peek_display(clamp)
                ctx.peek_display(reinhard)
            return
        paths = {
            "peek": lambda: ctx.peek(),
            "peek+host": lambda: host.tone_map(ctx.peek()[0].reshape(H, W, 4)),
            "display clamp": lambda: ctx.peek_display(clamp),
            "display reinhard": lambda: ctx.peek_display(reinhard),
        }
        for f in paths.values():  # warm: staging buffers, the RGBA8 buffer, the statistics record
            f()
        times = {k: [] for k in paths}
        for _ in range(a.reps):
            for k, f in paths.items():  # interleaved
                t0 = time.perf_counter()
                f()
                times[k].append((time.perf_counter() - t0) * 1e3)
        # the Python binding allocates the output array inside the timed call (33 MB / 8.3 MB of zeros): measured apart
        alloc = {}
        for k, shape, dt in (("float frame", (W * H, 4), np.float32), ("rgba8 frame", (W * H,), np.uint32)):
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                np.zeros(shape, dt)
                ts.append((time.perf_counter() - t0) * 1e3)
            alloc[k] = statistics.median(ts)
        lum = ctx.frame_luminance()
    res = {
        "width": W, "height": H, "reps": a.reps, "library": g.pt.build_info()["digest"],
        "median_ms": {k: round(statistics.median(v), 4) for k, v in times.items()},
        "min_ms": {k: round(min(v), 4) for k, v in times.items()},
        "max_ms": {k: round(max(v), 4) for k, v in times.items()},
        "numpy_zeros_ms": {k: round(v, 4) for k, v in alloc.items()},
        "frame_luminance": lum,
    }
    if a.kernel_stats and os.path.exists(a.kernel_stats):
        rows = [r for r in csv.DictReader(open(a.kernel_stats)) if "k_display" in r.get("Name", "")]
        res["kernels"] = [{"name": r["Name"], "calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 3),
                           "min_us": round(float(r["MinNs"]) / 1e3, 3), "max_us": round(float(r["MaxNs"]) / 1e3, 3)} for r in rows]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
