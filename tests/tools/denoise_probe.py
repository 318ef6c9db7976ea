"""What the denoiser costs next to a sample per pixel.

In ONE process on ONE context, on bench.py's workload (scenes.interior(1_000_000, seed=7)) at 1920x1080, with a 4-spp frame and its
feature planes in place: interleaved repetitions of gsp_denoise_to_device at 1, 3 and 5 iterations (into a device buffer of the
caller's; the call returns complete) and of a 1-spp gsp_render followed by gsp_sync, and their medians.  The requirement is a
direction: five levels cost less than one sample per pixel.

    python tests/tools/denoise_probe.py [--reps 7] [--out FILE]   (default: profiles/denoise_cost.txt)
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_cost.txt"))
    a = ap.parse_args()
    assert a.reps >= 5, "at least 5 repetitions"

    import gpuspectral_amd as g
    from gpuspectral_amd import abi, scenes

    W, H = a.width, a.height
    sc = scenes.interior(a.tris, seed=7)
    lines = ["denoiser vs one sample per pixel: scenes.interior(%d, seed=7) at %dx%d, %d interleaved repetitions, one context" % (a.tris, W, H, a.reps),
             "library " + str(g.pt.build_info())]
    hip = C.CDLL("libamdhip64.so")
    dptr = C.c_void_p()
    nbytes = W * H * 16
    assert hip.hipMalloc(C.byref(dptr), C.c_size_t(nbytes)) == 0
    try:
        with g.Context(0) as ctx:
            ctx.upload_scene(sc)
            ctx.frame_begin(W, H)
            ctx.render(4, 0)
            ctx.render_features(4, 0)
            ctx.sync()
            its = (1, 3, 5)
            for it in its:  # warm-up: the scratch planes, first launches
                ctx.denoise_to_device(dptr.value, nbytes, abi.denoise(iterations=it))
            ctx.render(1, 4)
            ctx.sync()
            td = {it: [] for it in its}
            ts = []
            for r in range(a.reps):
                for it in its:  # interleaved
                    d = abi.denoise(iterations=it)
                    t0 = time.perf_counter()
                    ctx.denoise_to_device(dptr.value, nbytes, d)
                    td[it].append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                ctx.render(1, 5 + r)
                ctx.sync()
                ts.append((time.perf_counter() - t0) * 1e3)
            ms = statistics.median(ts)
            lines.append("1-spp gsp_render + gsp_sync   %8.3f ms (min %.3f max %.3f)" % (ms, min(ts), max(ts)))
            for it in its:
                m = statistics.median(td[it])
                lines.append("gsp_denoise_to_device, %d level%s %8.3f ms (min %.3f max %.3f)   / one sample per pixel = %.4f"
                             % (it, " " if it == 1 else "s", m, min(td[it]), max(td[it]), m / ms))
            ok = statistics.median(td[5]) < ms
            lines.append("five levels cost %s than one sample per pixel" % ("LESS" if ok else "MORE"))
    finally:
        hip.hipFree(dptr)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
