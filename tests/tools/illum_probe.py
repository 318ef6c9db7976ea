"""What the illumination history costs.

On bench.py's workload (scenes.interior(1_000_000, seed=7)) at 1920x1080, the viewer loop with the camera turned by half a degree
between frames: gsp_frame_begin, a 1-spp gsp_render followed by gsp_sync (timed), a 1-spp gsp_render_features,
gsp_temporal_accumulate (timed; the call returns complete).

Part 1, gsp_temporal_accumulate, measured the way tests/tools/motion_probe.py measures it -- ONE context at a time, two warm-up
frames, then the repetitions -- for {plain, moments, moments + following} x {demodulation off, on}.  The off rows launch the
kernels of the parent commits (profiles/svgf_cost.txt, profiles/motion_cost.txt hold their earlier measurements).

Part 2, the filter at 5 levels into a torch tensor: for demodulation off and on, TWO contexts side by side with moments on, one that
only ever calls gsp_temporal_svgf_to_device and one that only ever calls gsp_temporal_svgf_feedback_to_device (the first level fed
back), interleaved frame by frame in alternating order, so that neither call is always the one behind the other; then
gsp_temporal_image_to_device on each.  Medians; no threshold.

    python tests/tools/illum_probe.py [--reps 5] [--out FILE]   (default: profiles/illum_cost.txt)
"""
import argparse
import os
import statistics
import sys

import torch  # first: the tracer's library then binds to the HIP runtime torch has loaded (see bench.py)

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from svgf_probe import timed, turned  # noqa: E402

MODES = ("plain", "moments", "follow")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "illum_cost.txt"))
    a = ap.parse_args()
    assert a.reps >= 5, "at least 5 repetitions"

    import gpuspectral_amd as g
    from gpuspectral_amd import scenes

    W, H = a.width, a.height
    sc = scenes.interior(a.tris, seed=7)
    lines = ["illumination history: scenes.interior(%d, seed=7) at %dx%d, %d repetitions after two warm-up frames" % (a.tris, W, H, a.reps),
             "library " + str(g.pt.build_info()), "", "gsp_temporal_accumulate, one context at a time:"]
    med = statistics.median

    def frame(ctx, r):
        ctx.update_camera(turned(sc.to_world, 0.5 * (r + 2)), sc.fov)
        ctx.frame_begin(W, H)
        ctx.frame_sample_base(r + 2)
        ms = timed(lambda: (ctx.render(1, r + 2), ctx.sync()))
        ctx.render_features(1, r + 2)
        return ms, timed(ctx.temporal_accumulate)

    renders = []
    for m in MODES:
        off = None
        for d in (False, True):
            t_acc = []
            with g.Context(0) as ctx:
                ctx.upload_scene(sc)
                ctx.temporal_track_moments(m != "plain")
                ctx.temporal_follow_instances(m == "follow")
                ctx.temporal_demodulate(d)
                for r in range(-2, a.reps):  # two warm-up frames: the planes, first launches
                    ms, ma = frame(ctx, r)
                    if r >= 0:
                        renders.append(ms)
                        t_acc.append(ma)
                length = float(ctx.download_temporal()[..., 3].mean())
            off = med(t_acc) if off is None else off
            lines.append("%-8s demodulation %-3s  gsp_temporal_accumulate %.3f ms (x %.2f of off; min %.3f max %.3f)   mean history length %.2f"
                         % (m, "on" if d else "off", med(t_acc), med(t_acc) / off, min(t_acc), max(t_acc), length))
            print(lines[-1], flush=True)
    render = med(renders)
    lines += ["1-spp gsp_render + gsp_sync of the same loops %.3f ms (median)" % render, "",
              "the filter at 5 levels, a context that only filters beside one that only feeds back, alternating order:"]
    dst = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    for d in (False, True):
        t = {"svgf": [], "feedback": [], "image": []}
        with g.Context(0) as plain, g.Context(0) as fed:
            for ctx in (plain, fed):
                ctx.upload_scene(sc)
                ctx.temporal_track_moments(True)
                ctx.temporal_demodulate(d)
            for r in range(-2, a.reps):
                for ctx in ((plain, fed) if r % 2 == 0 else (fed, plain)):
                    frame(ctx, r)
                    if ctx is plain:
                        ms = timed(lambda: ctx.temporal_svgf_to_device(dst.data_ptr(), W * H * 16, None, None))
                    else:
                        ms = timed(lambda: ctx.temporal_svgf_feedback_to_device(dst.data_ptr(), W * H * 16, None, None, 1))
                    mi = timed(lambda: ctx.temporal_image_to_device(dst.data_ptr(), W * H * 16))
                    if r >= 0:
                        t["svgf" if ctx is plain else "feedback"].append(ms)
                        t["image"].append(mi)
        for name, label in (("svgf", "gsp_temporal_svgf_to_device, 5 levels"), ("feedback", "gsp_temporal_svgf_feedback_to_device, 5 levels, 1 fed back"),
                            ("image", "gsp_temporal_image_to_device")):
            v = t[name]
            lines.append("%-58s demodulation %-3s  %.3f ms (min %.3f max %.3f)   / one sample per pixel = %.4f"
                         % (label, "on" if d else "off", med(v), min(v), max(v), med(v) / render))
            print(lines[-1], flush=True)
    lines += ["", "Wall-clock times of whole calls on the host (each returns complete).  The rows with demodulation off launch the kernels of the",
              "parent commits: profiles/svgf_cost.txt has plain 0.068 (0.067-0.075) and moments 0.085 (0.084-0.088) ms, profiles/motion_cost.txt",
              "plain 0.064 (0.064-0.071), moments 0.082 (0.081-0.085) and following with moments 0.092 (0.091-0.093) ms."]
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
