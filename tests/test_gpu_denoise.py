"""The denoiser on the GPU (include/gpuspectral_pt.h, "Denoiser"): k_denoise_prepare / k_denoise_atrous against the same text run
on the host (csrc/pt_denoise.h through tests/emu/denoise_emu.cpp, itself checked against a float64 restatement in
tests/test_denoise_cpu.py).  gsp_download_denoised equals the emulation applied to gsp_download + gsp_download_features BIT FOR
BIT: both fetch paths of the kernel (LDS for steps 1 and 2, global memory above), ragged tiles, steps beyond the frame."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from denoise_util import INF, DenoiseEmu, same
from display_util import DisplayEmu
from temporal_util import refusals

pytestmark = pytest.mark.gpu

TENT = 2
LENS = dict(radius=0.08, focus_distance=5.0, blades=0, rotation=0.0)
ITERATIONS = (1, 3, 5, 8)
# the defaults, one term off at a time, all terms off
PARAMS = {"defaults": {}, "no-color": dict(sigma_color=INF), "no-normal": dict(sigma_normal=INF), "no-depth": dict(sigma_depth=INF),
          "no-albedo": dict(sigma_albedo=INF), "all-off": dict(sigma_color=INF, sigma_normal=INF, sigma_depth=INF, sigma_albedo=INF)}
SPP = 4


@pytest.fixture(scope="module")
def emu():
    return DenoiseEmu()


@pytest.fixture(scope="module")
def scenes_(cornell, materials_scene):
    return {"cornell": cornell, "materials": materials_scene}


@pytest.fixture(scope="module")
def rigs(scenes_):
    """Per scene: one context with the scene uploaded, shared by the cases below."""
    import gpuspectral_amd as g

    made = {}

    def get(name):
        if name not in made:
            made[name] = g.Context(0)
            made[name].upload_scene(scenes_[name])
        return made[name]

    yield get
    for ctx in made.values():
        ctx.close()


def begin(ctx, w, h, filt=0, lens=None, spp=SPP):
    ctx.set_lens(**(lens or {}))
    ctx.frame_begin(w, h)
    ctx.render(spp, 0, pixel_filter=filt)
    ctx.render_features(spp, 0, pixel_filter=filt)


def check(ctx, emu, combos, what):
    """download_denoised == the emulation of (download, download_features), for every (iterations, parameter set) of combos."""
    from gpuspectral_amd import abi

    c = ctx.download()
    a, g, _ = ctx.download_features()
    for it, name in combos:
        d = abi.denoise(iterations=it, **PARAMS[name])
        got = ctx.download_denoised(d)
        want = emu.run(d, c, a, g)
        bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
        assert bad == 0, "%s, %d iterations, %s: %d of %d words differ" % (what, it, name, bad, got.size)
    return c, a, g


ALL = [(it, name) for it in ITERATIONS for name in PARAMS]


@pytest.mark.parametrize("scene", ["cornell", "materials"])
@pytest.mark.parametrize("size", [(33, 17), (96, 64), (5, 3), (1, 1)])
def test_download_denoised_equals_the_emulation(rigs, emu, scene, size):
    from gpuspectral_amd import abi

    ctx = rigs(scene)
    begin(ctx, *size)
    c, _, _ = check(ctx, emu, ALL, "%s %dx%d" % ((scene,) + size))
    assert same(ctx.download(), c)  # the frame is left alone
    assert same(ctx.download_denoised(None), ctx.download_denoised(abi.denoise(iterations=5)))  # NULL = every default


def test_several_tiles_and_a_ragged_last_tile(rigs, emu):
    """300 x 200: ten tiles of 32 across (the last one 12 wide), 25 of 8 down; every level, both fetch paths."""
    ctx = rigs("cornell")
    begin(ctx, 300, 200)
    check(ctx, emu, [(1, "defaults"), (3, "defaults"), (5, "defaults"), (8, "defaults"), (8, "all-off"), (3, "no-color")], "cornell 300x200")


@pytest.mark.parametrize("scene,size,filt,lens", [("cornell", (96, 64), TENT, None), ("materials", (33, 17), TENT, None), ("cornell", (96, 64), 0, LENS)],
                         ids=["cornell-tent", "materials-tent", "cornell-lens"])
def test_filtered_and_defocused_inputs(rigs, emu, scene, size, filt, lens):
    ctx = rigs(scene)
    try:
        begin(ctx, *size, filt=filt, lens=lens)
        check(ctx, emu, [(it, "defaults") for it in ITERATIONS] + [(5, "all-off")], "%s %s" % (scene, "lens" if lens else "tent"))
    finally:
        ctx.set_lens()


def test_nan_and_inf_in_the_frame(rigs, emu):
    from gpuspectral_amd import abi

    W, H = 64, 32
    ctx = rigs("cornell")
    begin(ctx, W, H, spp=2)
    a = ctx.download_compact().copy()
    rng = np.random.default_rng(5)
    for value in (np.nan, np.inf, -np.inf):
        a[rng.integers(0, W * H, 30), rng.integers(0, 3, 30)] = value
    a[7] = np.nan
    a[8, :3] = np.inf
    ctx.upload_accum(a)
    c, _, _ = check(ctx, emu, [(it, "defaults") for it in ITERATIONS] + [(5, "all-off")], "NaN / Inf frame")
    assert same(c.reshape(-1, 4), a)
    out = ctx.download_denoised(abi.denoise()).reshape(-1, 4)
    bad = ~np.isfinite(a[:, :3]).all(1)
    assert bad.sum() > 40 and same(out[bad], a[bad])  # a non-finite pixel leaves the filter as it came
    assert np.isfinite(out[~bad]).all()  # ... and reaches no neighbour


def test_adaptive_frame(rigs, emu):
    ctx = rigs("cornell")
    ctx.set_lens()
    ctx.frame_begin(64, 48)
    ctx.render(spp=64, adaptive_threshold=0.05)
    ctx.render_features(4, 0)
    assert ctx.stats()["adaptive_rounds"] > 0
    check(ctx, emu, [(it, "defaults") for it in ITERATIONS], "adaptive frame")


def test_frame_state_is_untouched_by_a_denoise_call(scenes_):
    """A denoise call between the two render calls of a frame against a gsp_download in the same place (both complete the queued
    samples first): the same image, pixel statistics and gsp_stats; the feature planes and -- in a frame without adaptive
    sampling -- the image also equal those of the frame with nothing between the calls."""
    import gpuspectral_amd as g

    w, h = 96, 64
    out = {}
    for between in ("nothing", "download", "denoise"):
        for adaptive in (False, True):
            with g.Context(0) as ctx:
                ctx.upload_scene(scenes_["cornell"])
                ctx.frame_begin(w, h)
                kw = dict(adaptive_threshold=0.05, adaptive_min_spp=4, adaptive_step=4) if adaptive else {}
                ctx.render(4, 0, **kw)
                ctx.render_features(2, 0, pixel_filter=TENT)
                if between == "download":
                    ctx.download()
                elif between == "denoise":
                    ctx.download_denoised(None)
                    ctx.download_denoised_display(None, None)
                ctx.render(4, 4, **kw)
                rec = dict(img=ctx.download(), feat=ctx.download_features(), stats=ctx.stats())
                if adaptive:
                    rec["px"] = ctx.pixel_stats()
                out[between, adaptive] = rec
    for adaptive in (False, True):
        plain, dl, dn = (out[k, adaptive] for k in ("nothing", "download", "denoise"))
        assert same(dl["img"], dn["img"]) and (adaptive or same(plain["img"], dn["img"]))
        for p, q in zip(plain["feat"], dn["feat"]):
            assert np.array_equal(p.view(np.uint32), q.view(np.uint32))
        if adaptive:
            assert same(dl["px"][0], dn["px"][0]) and np.array_equal(dl["px"][1], dn["px"][1])
        skip = ("render_seconds", "extend_kernel_ms", "shade_kernel_ms", "connect_kernel_ms", "bvh_build_ms", "device_bytes")
        for k, v in dl["stats"].items():
            if k not in skip:
                assert dn["stats"][k] == v, k
        assert dn["stats"]["device_bytes"] == dl["stats"]["device_bytes"] + 4 * 16 * w * h + 4 * w * h  # four scratch planes + the RGBA8 frame


_TORCH_CHILD = """
import sys
import torch  # first: the tracer's library then binds to the HIP runtime torch has loaded (see bench.py)
import numpy as np
sys.path.insert(0, sys.argv[1])
import gpuspectral_amd as g
from gpuspectral_amd import abi, scenes
W, H = 96, 64
with g.Context(0) as ctx:
    ctx.upload_scene(scenes.cornell_materials(8))
    ctx.frame_begin(W, H)
    ctx.render(spp=3)
    ctx.render_features(3)
    for d in (None, abi.denoise(iterations=3, sigma_color=float("inf"))):
        want = ctx.download_denoised(d).reshape(-1)
        for off in (0, 1):  # floats: the second destination is not 16-byte aligned and goes through the context's own buffer
            t = torch.zeros(W * H * 4 + 8, dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            ctx.denoise_to_device(t.data_ptr() + 4 * off, W * H * 16, d)
            back = t.cpu().numpy()
            assert np.array_equal(back[off:off + W * H * 4].view(np.uint32), want.view(np.uint32)) and not back[:off].any() and not back[off + W * H * 4:].any()
    t = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda:0")
    try:
        ctx.denoise_to_device(t.data_ptr(), W * H * 16 - 4, None)
        raise SystemExit("a destination of the wrong size was accepted")
    except g.GspError as e:
        assert "destination too small" in str(e), e
    assert not t.cpu().numpy().any()
print("torch tensor ok")
"""


def test_denoise_to_device_torch_tensor():
    """Into a torch tensor, in a process of its own: torch has to be imported before the library is loaded (bench.py does the same)."""
    r = subprocess.run([sys.executable, "-c", _TORCH_CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "torch tensor ok" in r.stdout, r.stdout + r.stderr


def test_download_denoised_display(rigs, emu):
    """The LDR film of the DENOISED frame, statistics included: byte for byte the display emulation of the denoised buffer."""
    from gpuspectral_amd import abi

    demu = DisplayEmu()
    ctx = rigs("cornell")
    begin(ctx, 96, 64)
    dn = abi.denoise(iterations=3)
    den = ctx.download_denoised(dn)
    for name, d in (("clamp", abi.display()), ("aces", abi.display(tonemap=abi.TONEMAP_ACES)), ("reinhard measured", abi.display(tonemap=abi.TONEMAP_REINHARD)),
                    ("NULL", None)):
        got = ctx.download_denoised_display(dn, d)
        assert np.array_equal(got.reshape(-1), demu.map(d, den.reshape(-1, 4))), name
    r = abi.display(tonemap=abi.TONEMAP_REINHARD)
    assert not np.array_equal(ctx.download_denoised_display(dn, r), ctx.download_display(r))  # not the accumulate buffer's film


def test_validation(rigs, scenes_):
    import gpuspectral_amd as g
    from gpuspectral_amd import abi

    with g.Context(0) as ctx:
        with pytest.raises(g.GspError, match="gsp_frame_begin"):
            ctx.download_denoised(None)  # no frame
        ctx.upload_scene(scenes_["cornell"])
        # the order of the refusals, two broken conditions per call (temporal_util.refusals): first without a frame ...
        buf = np.zeros((16, 16, 4), np.float32).ctypes.data
        bad_dn, tone = C.byref(abi.denoise(iterations=9)), C.byref(abi.display(tonemap=7))
        names = ("gsp_download_denoised", "gsp_denoise_to_device", "gsp_download_denoised_display")
        null, frame, share, feats = (dict((n, n + t) for n in names) for t in (
            ": null output pointer", " needs gsp_frame_begin first",
            ": the frame was begun with pixel_ids; a share has no neighbours (use gsp_multi_download_denoised)",
            " needs a gsp_render_features call since gsp_frame_begin"))
        n0, n1, n2 = names
        refusals(ctx, [(n0, (bad_dn, None), null[n0]), (n0, (bad_dn, buf), frame[n0]),
                       (n1, (bad_dn, None, 0), null[n1]), (n1, (bad_dn, 16, 0), frame[n1]),
                       (n2, (None, tone, None), "tonemap"), (n2, (bad_dn, None, None), null[n2]), (n2, (bad_dn, None, buf), frame[n2])])
        # ... in a share's frame without a feature pass ...
        ctx.frame_begin(16, 16, pixel_ids=g.pt.tile_partition(16, 16, 0, 2))
        refusals(ctx, [(n0, (None, buf), share[n0]), (n1, (None, 16, 4), "destination too small"), (n1, (None, None, 0), null[n1]),
                       (n1, (None, 16, 1 << 20), share[n1]), (n2, (None, None, None), null[n2]), (n2, (None, None, buf), share[n2])])
        ctx.frame_begin(16, 16)
        ctx.render(1)
        # ... in a full frame without one, and with one
        refusals(ctx, [(n0, (bad_dn, buf), feats[n0]), (n1, (bad_dn, 16, 1 << 20), feats[n1]), (n2, (bad_dn, None, buf), feats[n2])])
        ctx.render_features(1)
        refusals(ctx, [(n1, (bad_dn, 16, 4), "destination too small"), (n2, (bad_dn, tone, buf), "tonemap"),
                       (n2, (bad_dn, None, buf), "iterations")])
        ctx.frame_begin(16, 16)
        ctx.render(1)
        with pytest.raises(g.GspError, match="gsp_render_features"):
            ctx.download_denoised(None)  # no feature pass in this frame
        ctx.download_features()  # (a download allocates the planes; it is not a feature pass)
        with pytest.raises(g.GspError, match="gsp_render_features"):
            ctx.download_denoised_display(None, None)
        ctx.render_features(1)
        for bad, word in ((abi.denoise(iterations=9), "iterations"), (abi.denoise(sigma_color=-1.0), "sigma_color"),
                          (abi.denoise(sigma_normal=float("nan")), "sigma_normal"), (abi.denoise(sigma_depth=-0.5), "sigma_depth"),
                          (abi.denoise(sigma_albedo=-INF), "sigma_albedo")):
            with pytest.raises(g.GspError, match=word):
                ctx.download_denoised(bad)
            with pytest.raises(g.GspError, match=word):
                ctx.download_denoised_display(bad, None)
        with pytest.raises(g.GspError, match="tonemap"):
            ctx.download_denoised_display(None, abi.display(tonemap=7))
        assert ctx._L.gsp_download_denoised(ctx._h, None, None) == 1 and "null output" in ctx._L.gsp_last_error(ctx._h).decode()
        assert ctx._L.gsp_denoise_to_device(ctx._h, None, None, 1 << 20) == 1 and "null output" in ctx._L.gsp_last_error(ctx._h).decode()
        ctx.download_denoised(None)
        ctx.frame_begin(16, 16)  # a new frame: the planes are stale again
        with pytest.raises(g.GspError, match="gsp_render_features"):
            ctx.download_denoised(None)
        ctx.frame_begin(16, 16, pixel_ids=g.pt.tile_partition(16, 16, 0, 2))
        ctx.render_features(1)
        with pytest.raises(g.GspError, match="pixel_ids"):
            ctx.download_denoised(None)


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
def test_multi_equals_the_single_context(rigs, scenes_, devices):
    """Repeated device indices: several shares on one GPU.  The gathered frame's denoised image equals the single context's."""
    import gpuspectral_amd as g
    from gpuspectral_amd import abi

    W, H = 96, 80
    ctx = rigs("cornell")
    begin(ctx, W, H, filt=TENT)
    with g.MultiContext(devices) as m:
        m.upload_scene(scenes_["cornell"])
        m.frame_begin(W, H)
        m.render(SPP, 0, pixel_filter=TENT)
        with pytest.raises(g.GspError, match="gsp_multi_render_features"):
            m.download_denoised(None)
        m.render_features(SPP, 0, pixel_filter=TENT)
        for d in (None, abi.denoise(iterations=8), abi.denoise(iterations=2, sigma_albedo=INF)):
            assert same(m.download_denoised(d), ctx.download_denoised(d))
        assert same(m.download(), ctx.download())  # (the gather's frame buffer still serves the plain download)
        a, g_, _ = m.download_features()
        assert same(a, ctx.download_features()[0]) and same(g_, ctx.download_features()[1])
        with pytest.raises(g.GspError, match="iterations"):
            m.download_denoised(abi.denoise(iterations=12))


def test_host_layer(emu):
    """The C++ host layer: PathTracer::renderFeatures / downloadDenoised / downloadDenoisedDisplay."""
    from conftest import CORNELL_XML
    from gpuspectral_amd import abi, host

    W, H = 48, 40
    sc = host.Scene(CORNELL_XML)
    pt = host.PathTracer(W, H)
    try:
        pt.render(sc, 4)
        pt.render_features(sc, 4)
        c = pt.download()
        a, g = pt.download_features()
        for d in (None, abi.denoise(iterations=3, sigma_normal=INF)):
            den = pt.download_denoised(d)
            assert same(den, emu.run(d, c, a, g))
            disp = abi.display(tonemap=abi.TONEMAP_ACES)
            assert np.array_equal(pt.download_denoised_display(d, disp).reshape(-1), DisplayEmu().map(disp, den.reshape(-1, 4)))
        assert same(pt.download(), c)
    finally:
        pt.close()


# ---- CLI ------------------------------------------------------------------------------------------------------------------
def _run_cli(args):
    import os

    lib = os.path.join(ROOT, "gpuspectral_amd", "lib")
    env = dict(os.environ, LD_LIBRARY_PATH=lib + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([os.path.join(lib, "gsp_render")] + args, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_cli_denoise(rigs, tmp_path):
    """--denoise writes download_denoised (PFM, and with --ldr the film of the denoised frame as a PNG); without it every file and
    every printed line is what it is with it, less the denoiser's own."""
    import os
    import re

    from conftest import CORNELL_XML
    from gpuspectral_amd import abi, host
    from oracle import mitsuba_loader as ml

    W, H, S = 64, 48, 4
    t = tmp_path
    plain = _run_cli(["--filter", "tent", CORNELL_XML, str(t / "a.pfm"), str(W), str(H), str(S)])
    with_dn = _run_cli(["--filter", "tent", "--denoise", str(t / "b.dn.pfm"), "--denoise-iterations", "3", "--denoise-sigma", "0,0.4,inf,0", "--ldr", str(t / "b.png"),
                        "--tonemap", "aces", CORNELL_XML, str(t / "b.pfm"), str(W), str(H), str(S)])
    multi = _run_cli(["--filter", "tent", "--denoise", str(t / "c.dn.pfm"), CORNELL_XML, str(t / "c.pfm"), str(W), str(H), str(S), "0,0"])
    assert sorted(os.listdir(str(t))) == ["a.pfm", "a.pfm.ppm", "b.dn.pfm", "b.dn.png", "b.pfm", "b.pfm.ppm", "b.png", "c.dn.pfm", "c.pfm", "c.pfm.ppm"]
    for name in ("b", "c"):
        assert open(str(t / "a.pfm"), "rb").read() == open(str(t / (name + ".pfm")), "rb").read()
        assert open(str(t / "a.pfm.ppm"), "rb").read() == open(str(t / (name + ".pfm.ppm")), "rb").read()
    strip = lambda s: [re.sub(r"in [0-9.]+ s: .*", "", l) for l in s.splitlines()]  # (the timing line's figures vary)
    assert "denoised" not in plain and strip(plain) == [l for l in strip(with_dn) if not l.startswith("denoised: ")]
    assert "denoised: 3 levels" in with_dn and "denoised: 5 levels" in multi
    ctx = rigs("cornell")
    ctx.set_lens()
    ctx.frame_begin(W, H)
    ctx.render(S, 0, pixel_filter=TENT)
    ctx.render_features(S, 0, pixel_filter=TENT)
    d = abi.denoise(iterations=3, sigma_normal=0.4, sigma_depth=INF)
    pfm = lambda path: np.asarray(ml.read_pfm(str(path)), np.float32).reshape(H, W, -1)[::-1, :, :3]  # (writePfm and read_pfm: rows bottom to top)
    assert same(pfm(t / "b.dn.pfm"), ctx.download_denoised(d)[..., :3])
    assert np.array_equal(host.decode_png(open(str(t / "b.dn.png"), "rb").read())[::-1], ctx.download_denoised_display(d, abi.display(tonemap=abi.TONEMAP_ACES)))
    assert same(pfm(t / "c.dn.pfm"), ctx.download_denoised(None)[..., :3])
