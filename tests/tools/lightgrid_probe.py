"""tests/tools/lightgrid_probe.py -- the measurements of DESIGN.md section 31 on one GPU: `staircase2` with built-in shapes under
--light-sampling power --estimator textbook, with and without the light grid.

    python tests/tools/lightgrid_probe.py [out.txt]

Reports, with the grid off and on, alternating in the same process: ms per sample (host clock around gsp_render + gsp_sync at
1280 x 720, after a warm-up frame of each mode; median and range over the repeats), the k_shade share of the step (the library's
per-kernel event times, in a pass of their own), MSE against a 16 384-spp textbook frame at equal spp and at equal time (320 x 180,
independent timestamp ranges), the table image bytes and the host time of the grid build."""
import os
import sys
import tarfile
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, SPP = 1280, 720, 16
RW, RH, REF_SPP, TEST_SPP = 320, 180, 16384, 16
REPEATS = 5


def staircase2(tmp):
    g = os.path.join(ROOT, "tests", "golden", "ref_scenes")
    with tarfile.open(os.path.join(g, "staircase2.tar.xz")) as t:
        t.extractall(tmp)
    from gpuspectral_amd import host

    return host.Scene(os.path.join(tmp, "staircase2", "scene.xml"), builtin_shapes=True).arrays()


def timed(ctx, spp, ts0, **kw):
    ctx.reset_stats()
    t = time.perf_counter()
    ctx.render(spp=spp, first_timestamp=ts0, **kw)
    ctx.sync()
    return (time.perf_counter() - t) * 1e3, ctx.stats()


def main():
    import gpuspectral_amd as g

    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout

    def say(s=""):
        print(s, file=out, flush=True)
        if out is not sys.stdout:
            print(s, flush=True)

    with tempfile.TemporaryDirectory() as tmp:
        sc = staircase2(tmp)
    n = len(sc.lights)
    say("staircase2 --builtin-shapes: %d triangles, %d light triangles; power pick, textbook estimator, clamp default" % (len(sc.positions) // 3, n))
    with g.Context(0) as ctx:
        ctx.set_light_sampling("power")
        ctx.set_estimator("textbook")
        ctx.upload_scene(sc)
        # ---- host cost of the switch under the resident scene: repack + upload without / with the grid build
        t_on, t_off = [], []
        for _ in range(REPEATS):
            t = time.perf_counter(); ctx.set_light_grid(True); t_on.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter(); ctx.set_light_grid(False); t_off.append((time.perf_counter() - t) * 1e3)
        ctx.set_light_grid(True)
        on, res, (lo, hi) = ctx.light_grid()
        cells = res[0] * res[1] * res[2]
        grid_bytes = 64 + cells * (n + 1) * 16
        say("auto resolution %d x %d x %d = %d cells over [%s] .. [%s]" % (res + (cells, ", ".join("%.3f" % x for x in lo), ", ".join("%.3f" % x for x in hi))))
        say("table image: %d bytes in front of the grid (lights, pick table, tail; BSDF tables aside) + %d bytes of grid (%.2f MB)"
            % (n * 80 + 16, grid_bytes, grid_bytes / 2 ** 20))
        say("gsp_set_light_grid under the resident scene, %d repeats: on %.1f ms median (%.1f .. %.1f), off %.1f ms median (%.1f .. %.1f): the host build of the grid is the difference, %.1f ms"
            % (REPEATS, np.median(t_on), min(t_on), max(t_on), np.median(t_off), min(t_off), max(t_off), np.median(t_on) - np.median(t_off)))
        # ---- time per sample, alternating, one warm-up frame per mode
        ms = {False: [], True: []}
        share = {False: [], True: []}
        for mode in (False, True):
            ctx.set_light_grid(mode)
            ctx.frame_begin(W, H)
            timed(ctx, SPP, 0)
        for r in range(REPEATS):
            for mode in (False, True):
                ctx.set_light_grid(mode)
                ctx.frame_begin(W, H)
                dt, st = timed(ctx, SPP, 0)
                ms[mode].append(dt / SPP)
        for r in range(3):  # the kernel split in passes of their own (event timing serialises the launches)
            for mode in (False, True):
                ctx.set_light_grid(mode)
                ctx.frame_begin(W, H)
                dt, st = timed(ctx, SPP, 0, collect_kernel_times=1)
                tot = st["extend_kernel_ms"] + st["shade_kernel_ms"] + st["connect_kernel_ms"]
                share[mode].append((st["shade_kernel_ms"], st["shade_kernel_ms"] / tot, st["shade_kernel_ms"] * 1e6 / st["shaded_vertices"], st["shadow_rays"]))
        for mode in (False, True):
            a = np.array(share[mode])
            say("%s  %d x %d, %d spp: %.3f ms per sample median (%.3f .. %.3f over %d); k_shade %.2f ms = %.1f %% of extend + shade + connect, %.3f ns per vertex; %d shadow rays"
                % ("grid " if mode else "power", W, H, SPP, np.median(ms[mode]), min(ms[mode]), max(ms[mode]), REPEATS, np.median(a[:, 0]), 100 * np.median(a[:, 1]),
                   np.median(a[:, 2]), int(a[0, 3])))
        ratio = float(np.median(ms[True]) / np.median(ms[False]))
        say("time per sample, grid / power: %.3f" % ratio)
        # ---- MSE against a long textbook frame (power pick: the two converge to the same image), equal spp and equal time
        ctx.set_light_grid(False)
        ctx.frame_begin(RW, RH)
        ctx.frame_sample_base(1 << 20)  # (other random numbers than the frames under test; folded as the frame's own samples 0, 1, ...)
        ctx.render(spp=REF_SPP, first_timestamp=1 << 20)
        ref = ctx.download().reshape(-1, 4)[:, :3].astype(np.float64)
        eq_time_spp = max(1, int(round(TEST_SPP / ratio)))
        rows = {}
        for name, mode, spp in (("power", False, TEST_SPP), ("grid, equal spp", True, TEST_SPP), ("grid, equal time", True, eq_time_spp)):
            ctx.set_light_grid(mode)
            errs = []
            for r in range(REPEATS):
                ctx.frame_begin(RW, RH)
                ctx.frame_sample_base(r * 64)
                ctx.render(spp=spp, first_timestamp=r * 64)
                img = ctx.download().reshape(-1, 4)[:, :3].astype(np.float64)
                errs.append(float(((img - ref) ** 2).mean()))
            rows[name] = errs
            say("%-17s %d x %d, %2d spp: MSE against %d spp  %.5g median (%.5g .. %.5g over %d)" % (name, RW, RH, spp, REF_SPP, np.median(errs), min(errs), max(errs), REPEATS))
        say("MSE power / grid: equal spp %.3f, equal time %.3f" % (np.median(rows["power"]) / np.median(rows["grid, equal spp"]),
                                                                  np.median(rows["power"]) / np.median(rows["grid, equal time"])))
        ctx.set_light_grid(True)
        ctx.frame_begin(RW, RH)
        ctx.frame_sample_base(1 << 21)
        ctx.render(spp=1024, first_timestamp=1 << 21)
        long_grid = ctx.download().reshape(-1, 4)[:, :3].astype(np.float64)
        say("frame mean: %d spp power %s, 1024 spp grid %s" % (REF_SPP, np.round(ref.mean(0), 5), np.round(long_grid.mean(0), 5)))


if __name__ == "__main__":
    main()
