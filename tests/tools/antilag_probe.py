"""What the temporal anti-lag costs.

On bench.py's workload (scenes.interior(1_000_000, seed=7)) at 1920x1080, the viewer loop of tests/tools/illum_probe.py with the camera
turned by half a degree between frames and every switch on (moments, following, demodulation), so that the accumulate launches
k_temporal_reproject_illum<true, true>: gsp_frame_begin, a 1-spp gsp_render, a 1-spp gsp_render_features, gsp_temporal_accumulate
(timed; the call returns complete), gsp_temporal_antilag (timed; the call returns complete).  One context per radius, two warm-up
frames, then the repetitions.  Medians; no threshold.

The host clock gives whole calls (launches, the synchronise).  For the kernels themselves run the same program under a kernel trace, in
a run of its own (tracing slows the host):

    rocprofv3 --kernel-trace --stats -d OUT -- python tests/tools/antilag_probe.py --out ""

    python tests/tools/antilag_probe.py [--reps 5] [--out FILE]   (default: profiles/antilag_cost.txt)
"""
import argparse
import os
import statistics
import sys

import torch  # noqa: F401  first: the tracer's library then binds to the HIP runtime torch has loaded (see bench.py)

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from svgf_probe import timed, turned  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "antilag_cost.txt"))
    a = ap.parse_args()
    assert a.reps >= 5, "at least 5 repetitions"

    import gpuspectral_amd as g
    from gpuspectral_amd import abi, scenes

    W, H = a.width, a.height
    sc = scenes.interior(a.tris, seed=7)
    med = statistics.median
    lines = ["temporal anti-lag: scenes.interior(%d, seed=7) at %dx%d, moments + following + demodulation on, %d repetitions after two warm-up frames"
             % (a.tris, W, H, a.reps), "library " + str(g.pt.build_info()), ""]
    for radius in (1, 2, 3):
        t_acc, t_al = [], []
        with g.Context(0) as ctx:
            ctx.upload_scene(sc)
            ctx.temporal_track_moments(True)
            ctx.temporal_follow_instances(True)
            ctx.temporal_demodulate(True)
            al = abi.antilag(radius=radius)
            for r in range(-2, a.reps):  # two warm-up frames: the planes, first launches
                ctx.update_camera(turned(sc.to_world, 0.5 * (r + 2)), sc.fov)
                ctx.frame_begin(W, H)
                ctx.frame_sample_base(r + 2)
                ctx.render(1, r + 2)
                ctx.render_features(1, r + 2)
                ctx.sync()  # (the timed calls find nothing queued)
                ctx.download_features()
                ma = timed(ctx.temporal_accumulate)
                ml = timed(lambda: ctx.temporal_antilag(al))
                if r >= 0:
                    t_acc.append(ma)
                    t_al.append(ml)
            hist, fast = ctx.download_temporal()[..., 3], ctx.download_temporal_fast()[..., 3]
        lines.append("radius %d  gsp_temporal_accumulate %.3f ms (min %.3f max %.3f)   gsp_temporal_antilag %.3f ms (min %.3f max %.3f; x %.2f of the accumulate)   "
                     "mean length: history %.2f, fast history %.2f" % (radius, med(t_acc), min(t_acc), max(t_acc), med(t_al), min(t_al), max(t_al), med(t_al) / med(t_acc),
                                                                     float(hist.mean()), float(fast.mean())))
        print(lines[-1], flush=True)
    lines += ["", "Wall-clock times of whole calls on the host (each returns complete): two launches and a synchronise for the anti-lag, one launch and a",
              "synchronise for the accumulate."]
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
