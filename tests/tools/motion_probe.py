"""What following moved instances costs.

On bench.py's workload (scenes.interior(1_000_000, seed=7)) at 1920x1080, one context at a time runs the viewer loop with the camera
turned by half a degree between frames: gsp_frame_begin, a 1-spp gsp_render followed by gsp_sync (timed), a 1-spp
gsp_render_features, gsp_temporal_accumulate (timed; the call returns complete).  Three configurations, each with and without the
luminance moments: following off (the parent's path), following on with nothing moved, following on with 16 instances translated
before every frame (the edit itself is not timed).  Medians; no threshold.

    python tests/tools/motion_probe.py [--reps 5] [--out FILE]   (default: profiles/motion_cost.txt)
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


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_cost.txt"))
    a = ap.parse_args()
    assert a.reps >= 5, "at least 5 repetitions"

    import gpuspectral_amd as g
    from gpuspectral_amd import scenes

    W, H = a.width, a.height
    sc = scenes.interior(a.tris, seed=7)
    n = len(sc.instances)
    movers = list(range(n // 2, min(n, n // 2 + 16)))
    lines = ["moved instances: scenes.interior(%d, seed=7) (%d instances) at %dx%d, %d repetitions after two warm-up frames, one context at a time"
             % (a.tris, n, W, H, a.reps), "library " + str(g.pt.build_info()), ""]
    med = lambda v: statistics.median(v)
    base = {}
    for moments in (False, True):
        for config in ("off", "on, nothing moved", "on, %d instances moved" % len(movers)):
            t_render, t_acc, followed = [], [], 0
            with g.Context(0) as ctx:
                ctx.upload_scene(sc)
                ctx.temporal_track_moments(moments)
                ctx.temporal_follow_instances(config != "off")
                for r in range(-2, a.reps):  # two warm-up frames: the planes, first launches
                    if "instances moved" in config:
                        inst = sc.instances.copy()
                        for m in movers:
                            inst["transform"][m][12:15] += np.float32([0.01, 0.0, 0.01]) * (r + 3)
                        ctx.update_instances(inst)
                    ctx.update_camera(turned(sc.to_world, 0.5 * (r + 2)), sc.fov)
                    ctx.frame_begin(W, H)
                    ctx.frame_sample_base(r + 2)
                    ms = timed(lambda: (ctx.render(1, r + 2), ctx.sync()))
                    ctx.render_features(1, r + 2)
                    ma = timed(ctx.temporal_accumulate)
                    if r >= 0:
                        t_render.append(ms)
                        t_acc.append(ma)
                if config != "off":
                    followed = int((ctx.download_temporal_motion()[..., 3] == 2.0).sum())
                length = float(ctx.download_temporal()[..., 3].mean())
            key = "moments" if moments else "plain"
            if config == "off":
                base[key] = med(t_acc)
            lines.append("%-8s following %-26s gsp_temporal_accumulate %.3f ms (x %.2f of off; min %.3f max %.3f)   1-spp gsp_render + gsp_sync %.2f ms   "
                         "%d followed pixels, mean history length %.2f"
                         % (key, config, med(t_acc), med(t_acc) / base[key], min(t_acc), max(t_acc), med(t_render), followed, length))
            print(lines[-1], flush=True)
    lines += ["", "Wall-clock times of whole calls on the host (the accumulate returns complete); with following on the call also forms the",
              "%d records in double, copies %d bytes to the device and stores 16 more bytes per pixel." % (n, 96 * n)]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("written:", a.out)


if __name__ == "__main__":
    main()
