"""Adaptive sampling (ABI 9) on the GPU: what it saves and what it costs.

For the bench workload (scenes.interior(1M, seed=7) at 1920x1080) and scenes.cornell_materials(96) at 1024x1024:
  * uniform N spp against adaptive with the same maximum: wall time (render + sync) and stats.samples
  * the mean relative luminance error of both against a high-spp uniform render of the same scene
  * the per-round overhead: adaptive with a threshold so small that (almost) nothing stops, against uniform at equal spp,
    from stats.render_seconds

    python scripts/adaptive_probe.py [--spp 64] [--ref-spp 4096] [--thresholds 0.05,0.1,0.2,0.3] [--out profiles/adaptive_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gpuspectral_amd as g  # noqa: E402
from gpuspectral_amd import scenes  # noqa: E402


def lum(img):
    c = np.asarray(img, np.float64).reshape(-1, 4)
    return 0.2126 * c[:, 0] + 0.7152 * c[:, 1] + 0.0722 * c[:, 2]


def rel_err(img, ref):
    y, r = lum(img), lum(ref)
    return float(np.mean(np.abs(y - r) / np.maximum(r, 1e-3)))


def run(ctx, W, H, spp, **adaptive):
    ctx.frame_begin(W, H)
    ctx.reset_stats()
    t0 = time.perf_counter()
    ctx.render(spp=spp, **adaptive)
    ctx.sync()
    wall = time.perf_counter() - t0
    st = ctx.stats()
    return ctx.download_compact(), wall, st


def probe(name, sc, W, H, args):
    out = {"scene": name, "resolution": [W, H], "spp": args.spp, "ref_spp": args.ref_spp}
    with g.Context(0) as ctx:
        ctx.upload_scene(sc)
        run(ctx, W, H, 8)  # warm-up: pool, queues, memo ...
        run(ctx, W, H, 8, adaptive_threshold=0.1, adaptive_min_spp=4, adaptive_step=4)  # ... and the adaptive buffers
        ref, wall, _ = run(ctx, W, H, args.ref_spp)
        out["ref_seconds"] = wall
        img, wall, st = run(ctx, W, H, args.spp)
        out["uniform"] = {"wall_s": wall, "render_seconds": st["render_seconds"], "samples": st["samples"],
                          "extension_rays": st["extension_rays"], "rel_err": rel_err(img, ref)}
        out["adaptive"] = []
        for t in args.thresholds:
            img, wall, st = run(ctx, W, H, args.spp, adaptive_threshold=t)
            _, spp = ctx.pixel_stats()
            out["adaptive"].append({"threshold": t, "wall_s": wall, "render_seconds": st["render_seconds"], "samples": st["samples"],
                                    "samples_share": st["samples"] / float(W * H * args.spp), "extension_rays": st["extension_rays"],
                                    "rounds": st["adaptive_rounds"], "active_after": st["adaptive_active_pixels"],
                                    "spp_histogram": {int(k): int(v) for k, v in zip(*np.unique(spp, return_counts=True))},
                                    "rel_err": rel_err(img, ref)})
        # per-round overhead: nothing (or almost nothing) stops, so the same samples are taken in rounds that drain
        img, wall_u, st_u = run(ctx, W, H, args.spp)
        img, wall_a, st_a = run(ctx, W, H, args.spp, adaptive_threshold=1e-12)
        rounds = max(1, st_a["adaptive_rounds"])
        out["round_overhead"] = {"uniform_render_seconds": st_u["render_seconds"], "adaptive_render_seconds": st_a["render_seconds"],
                                 "rounds": rounds, "samples_uniform": st_u["samples"], "samples_adaptive": st_a["samples"],
                                 "per_round_ms": 1e3 * (st_a["render_seconds"] - st_u["render_seconds"]) / rounds}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--thresholds", default="0.05,0.1,0.2,0.3")
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_probe.json"))
    args = ap.parse_args()
    args.thresholds = [float(x) for x in args.thresholds.split(",")]
    res = {"library": g.pt.build_info(), "runs": []}
    for name, make, W, H in (("bench workload: scenes.interior(%d, seed=7)" % args.tris, lambda: scenes.interior(args.tris, seed=7), 1920, 1080),
                             ("scenes.cornell_materials(96)", lambda: scenes.cornell_materials(96), 1024, 1024)):
        r = probe(name, make(), W, H, args)
        res["runs"].append(r)
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
