"""What temporal accumulation costs next to a sample per pixel.

In ONE process on ONE context, on bench.py's workload (scenes.interior(1_000_000, seed=7)) at 1920x1080: repetitions of the viewer
loop -- gsp_frame_begin, a 1-spp gsp_render followed by gsp_sync (timed), a 1-spp gsp_render_features, gsp_temporal_accumulate
(timed; the call returns complete) -- with the camera turned by half a degree between frames, so the two timed calls are
interleaved, and their medians.  The expectation is a direction: one accumulate costs well under a tenth of one sample per pixel.

    python tests/tools/temporal_probe.py [--reps 5] [--out FILE]   (default: profiles/temporal_cost.txt)
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def turned(to_world, degrees):
    m = np.asarray(to_world, np.float64).reshape(4, 4).T
    a = np.radians(degrees)
    r = np.eye(4)
    r[0, 0], r[0, 2], r[2, 0], r[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    m[:3, :3] = r[:3, :3] @ m[:3, :3]  # about the eye: the view turns, the position stays
    return m.T.astype(np.float32).reshape(16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_cost.txt"))
    a = ap.parse_args()
    assert a.reps >= 5, "at least 5 repetitions"

    import gpuspectral_amd as g
    from gpuspectral_amd import scenes

    W, H = a.width, a.height
    sc = scenes.interior(a.tris, seed=7)
    lines = ["temporal accumulation vs one sample per pixel: scenes.interior(%d, seed=7) at %dx%d, %d interleaved repetitions, one context" % (a.tris, W, H, a.reps),
             "library " + str(g.pt.build_info())]
    with g.Context(0) as ctx:
        ctx.upload_scene(sc)
        tr, tt, length = [], [], 0.0
        for r in range(-2, a.reps):  # two warm-up frames: the history planes, first launches
            ctx.update_camera(turned(sc.to_world, 0.5 * (r + 2)), sc.fov)
            ctx.frame_begin(W, H)
            ctx.frame_sample_base(r + 2)
            t0 = time.perf_counter()
            ctx.render(1, r + 2)
            ctx.sync()
            t1 = time.perf_counter()
            ctx.render_features(1, r + 2)
            t2 = time.perf_counter()
            ctx.temporal_accumulate()
            t3 = time.perf_counter()
            if r >= 0:
                tr.append((t1 - t0) * 1e3)
                tt.append((t3 - t2) * 1e3)
        length = float(ctx.download_temporal()[..., 3].mean())
    ms, mt = statistics.median(tr), statistics.median(tt)
    lines.append("1-spp gsp_render + gsp_sync   %8.3f ms (min %.3f max %.3f)" % (ms, min(tr), max(tr)))
    lines.append("gsp_temporal_accumulate       %8.3f ms (min %.3f max %.3f)   / one sample per pixel = %.4f" % (mt, min(tt), max(tt), mt / ms))
    lines.append("mean history length after the last frame %.2f" % length)
    ok = mt < 0.1 * ms
    lines.append("one accumulate costs %s than a tenth of one sample per pixel" % ("LESS" if ok else "MORE"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
