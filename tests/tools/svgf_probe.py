"""What the variance-guided filter costs.

In ONE process, on bench.py's workload (scenes.interior(1_000_000, seed=7)) at 1920x1080, two contexts on one device -- one that
tracks the luminance moments and one that does not -- run the viewer loop side by side with the camera turned by half a degree
between frames: gsp_frame_begin, a 1-spp gsp_render followed by gsp_sync (timed), a 1-spp gsp_render_features,
gsp_temporal_accumulate (timed; the call returns complete).  On the tracking context every frame then times
gsp_temporal_svgf_to_device at 1, 3 and 5 levels into a torch tensor, and gsp_download_temporal_svgf beside the unchanged
gsp_download_temporal_denoised (both with the read-back of the frame, 5 levels).  Medians; no threshold.

    python tests/tools/svgf_probe.py [--reps 5] [--out FILE]   (default: profiles/svgf_cost.txt)
"""
import argparse
import os
import statistics
import sys
import time

import torch  # first: the tracer's library then binds to the HIP runtime torch has loaded (see bench.py)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svgf_cost.txt"))
    a = ap.parse_args()
    assert a.reps >= 5, "at least 5 repetitions"

    import gpuspectral_amd as g
    from gpuspectral_amd import abi, scenes

    W, H = a.width, a.height
    sc = scenes.interior(a.tris, seed=7)
    lines = ["variance-guided filter: scenes.interior(%d, seed=7) at %dx%d, %d interleaved repetitions, two contexts on one device" % (a.tris, W, H, a.reps),
             "library " + str(g.pt.build_info())]
    dst = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    t = {k: [] for k in ("render", "acc", "acc_m", "svgf1", "svgf3", "svgf5", "dl_plain", "dl_svgf")}
    with g.Context(0) as on, g.Context(0) as off:
        for ctx in (on, off):
            ctx.upload_scene(sc)
        on.temporal_track_moments(True)
        for r in range(-2, a.reps):  # two warm-up frames: the planes, first launches
            rec = r >= 0
            for ctx in (off, on):
                ctx.update_camera(turned(sc.to_world, 0.5 * (r + 2)), sc.fov)
                ctx.frame_begin(W, H)
                ctx.frame_sample_base(r + 2)
                ms = timed(lambda: (ctx.render(1, r + 2), ctx.sync()))
                ctx.render_features(1, r + 2)
                ma = timed(ctx.temporal_accumulate)
                if rec:
                    t["render"].append(ms)
                    t["acc_m" if ctx is on else "acc"].append(ma)
            for it in (1, 3, 5):
                ms = timed(lambda: on.temporal_svgf_to_device(dst.data_ptr(), W * H * 16, abi.denoise(iterations=it), None))
                if rec:
                    t["svgf%d" % it].append(ms)
            for key, call in (("dl_plain", on.download_temporal_denoised), ("dl_svgf", on.download_temporal_svgf)):
                ms = timed(call)
                if rec:
                    t[key].append(ms)
        length = float(on.download_temporal()[..., 3].mean())
    med = {k: statistics.median(v) for k, v in t.items()}
    row = lambda name, k: "%-58s %8.3f ms (min %.3f max %.3f)   / one sample per pixel = %.4f" % (name, med[k], min(t[k]), max(t[k]), med[k] / med["render"])
    lines += [row("1-spp gsp_render + gsp_sync", "render"), row("gsp_temporal_accumulate, moments off (unchanged kernel)", "acc"),
              row("gsp_temporal_accumulate, moments on", "acc_m"), row("gsp_temporal_svgf_to_device, 1 level", "svgf1"),
              row("gsp_temporal_svgf_to_device, 3 levels", "svgf3"), row("gsp_temporal_svgf_to_device, 5 levels", "svgf5"),
              row("gsp_download_temporal_denoised, 5 levels, with read-back", "dl_plain"), row("gsp_download_temporal_svgf, 5 levels, with read-back", "dl_svgf"),
              "moments on / off: %.3f; variance-guided / plain filter with read-back: %.3f" % (med["acc_m"] / med["acc"], med["dl_svgf"] / med["dl_plain"]),
              "mean history length after the last frame %.2f" % length]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
