"""LDR film (include/gpuspectral_pt.h, "LDR film") on the GPU.

k_display_map / k_display_stats against the same text run on the host (csrc/pt_display.h through tests/emu/display_emu.cpp):
gsp_download_display equals the emulation applied to gsp_download BYTE FOR BYTE and gsp_frame_luminance equals it integer for
integer, for every tonemap x encode x exposure, on full frames, pixel_ids shares, adaptive frames and frames with NaN / Inf; the
peek variants; the gathered frame of gsp_multi; the CLI's PNG."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import CORNELL_XML, ROOT
from display_util import COMBOS, DisplayEmu, combo_display

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def demu():
    return DisplayEmu()


@pytest.fixture()
def ctx():
    import gpuspectral_amd as g

    c = g.Context(0)
    yield c
    c.close()


def _all_displays():
    from gpuspectral_amd import abi

    out = [("%s %s %+.1f" % c, combo_display(abi, *c)) for c in COMBOS]
    out.append(("reinhard key burn", abi.display(tonemap=abi.TONEMAP_REINHARD, gamma=2.2, key=0.36, burn=0.5)))
    out.append(("reinhard supplied", abi.display(tonemap=abi.TONEMAP_REINHARD, log_avg_luminance=0.4, max_luminance=20.0)))
    out.append(("NULL", None))
    return out


def _check_frame(ctx, demu, owned=None):
    """Every display on the context's current frame: download_display == emulation(download), statistics integer for integer."""
    hdr = ctx.download()
    H, W = hdr.shape[:2]
    compact = hdr.reshape(-1, 4) if owned is None else hdr.reshape(-1, 4)[owned]
    lum = ctx.frame_luminance()
    want_lum = demu.stats(compact)
    print("frame %dx%d: S = %d, n = %d, Lavg = %.9g, Lmax = %.9g" % (W, H, lum["log_sum_q20"], lum["pixels"], lum["log_avg"], lum["max"]))
    assert lum == want_lum
    assert ctx.frame_luminance(drain=False) == want_lum  # an idle context: the buffer as it stands is the drained one
    for name, d in _all_displays():
        got = ctx.download_display(d).reshape(-1)
        want = np.zeros(W * H, np.uint32)
        if owned is None:
            want[:] = demu.map(d, compact)
        else:
            want[owned] = demu.map(d, compact)  # unowned pixels are 0
        bad = int((got != want).sum())
        assert bad == 0, "%s: %d of %d words differ" % (name, bad, W * H)
    return hdr


@pytest.mark.parametrize("size", [(96, 64), (33, 17)])  # (the second: a pixel count that is not a multiple of four)
def test_cornell(ctx, demu, cornell, size):
    ctx.upload_scene(cornell)
    ctx.frame_begin(*size)
    ctx.render(spp=8)
    hdr = _check_frame(ctx, demu)
    assert np.array_equal(ctx.download(), hdr)  # the display calls leave the frame alone


def test_materials(ctx, demu, materials_scene):
    ctx.upload_scene(materials_scene)
    ctx.frame_begin(80, 80)
    ctx.render(spp=6)
    _check_frame(ctx, demu)


def test_large_frame_goes_through_the_staging_buffers(ctx, demu, cornell):
    """640x480 RGBA8 = 1.2 MB: above the one-copy limit of the read-back (1 MiB), so the staged path runs."""
    from gpuspectral_amd import abi

    ctx.upload_scene(cornell)
    ctx.frame_begin(640, 480)
    ctx.render(spp=1)
    hdr = ctx.download().reshape(-1, 4)
    for d in (None, abi.display(tonemap=abi.TONEMAP_REINHARD, gamma=2.2)):
        assert np.array_equal(ctx.download_display(d).reshape(-1), demu.map(d, hdr))
    assert ctx.frame_luminance() == demu.stats(hdr)


def test_pixel_ids_share(ctx, demu, cornell):
    import gpuspectral_amd as g

    W, H = 96, 64
    ctx.upload_scene(cornell)
    for rank, world in ((1, 3), (0, 2)):
        ids = g.pt.tile_partition(W, H, rank, world)
        ctx.frame_begin(W, H, pixel_ids=ids)
        ctx.render(spp=4)
        _check_frame(ctx, demu, owned=ids)
        words, _ = ctx.peek_display(None)
        assert np.array_equal(words, ctx.download_display(None).reshape(-1)[ids])


def test_share_statistics_add_up(ctx, demu, cornell):
    """S, n and Lmax of the shares of a frame sum / max to the whole frame's, exactly."""
    import gpuspectral_amd as g

    W, H, world = 96, 64, 3
    ctx.upload_scene(cornell)
    ctx.frame_begin(W, H)
    ctx.render(spp=4)
    whole = ctx.frame_luminance()
    parts = []
    for r in range(world):
        ctx.frame_begin(W, H, pixel_ids=g.pt.tile_partition(W, H, r, world))
        ctx.render(spp=4)
        parts.append(ctx.frame_luminance())
    assert sum(p["log_sum_q20"] for p in parts) == whole["log_sum_q20"] and sum(p["pixels"] for p in parts) == whole["pixels"] == W * H
    assert max(p["max"] for p in parts) == whole["max"]


def test_adaptive_frame(ctx, demu, cornell):
    ctx.upload_scene(cornell)
    ctx.frame_begin(64, 48)
    ctx.render(spp=64, adaptive_threshold=0.05)
    assert ctx.stats()["adaptive_rounds"] > 0
    _check_frame(ctx, demu)


def test_nan_and_inf_in_the_frame(ctx, demu, cornell):
    W, H = 64, 32
    ctx.upload_scene(cornell)
    ctx.frame_begin(W, H)
    ctx.render(spp=2)
    a = ctx.download_compact().copy()
    rng = np.random.default_rng(5)
    for value in (np.nan, np.inf, -np.inf, -1.0, 1e30):
        a[rng.integers(0, W * H, 40), rng.integers(0, 3, 40)] = value
    a[7] = np.nan
    a[8, :3] = np.inf
    ctx.upload_accum(a)
    hdr = _check_frame(ctx, demu)
    assert np.array_equal(hdr.reshape(-1, 4).view(np.uint32), a.view(np.uint32))
    lum = ctx.frame_luminance()
    assert lum["pixels"] == int(np.isfinite(a[:, :3]).all(1).sum()) < W * H
    w = ctx.download_display(None).reshape(-1)
    assert w[7] == 0xFF000000 and w[8] == 0xFFFFFFFF  # NaN -> 0, +Inf saturates


def test_peek_display_idle_equals_download_display(ctx, demu, cornell):
    from gpuspectral_amd import abi

    ctx.upload_scene(cornell)
    ctx.frame_begin(96, 64)
    ctx.render(spp=5)
    ctx.sync()
    for name, d in _all_displays()[::4] + [("reinhard", abi.display(tonemap=1))]:
        words, folded = ctx.peek_display(d)
        assert folded == 5 and np.array_equal(words, ctx.download_display(d).reshape(-1)), name


def test_peek_display_while_rendering(ctx, demu, cornell):
    """No drain: the words are the display of SOME prefix of the samples, the one gsp_peek_display reports."""
    from gpuspectral_amd import abi

    W, H = 64, 48
    d = abi.display(tonemap=abi.TONEMAP_ACES, gamma=2.2)
    ctx.upload_scene(cornell)
    ctx.frame_begin(W, H)
    refs = {0: np.zeros((W * H, 4), np.float32)}
    for k in range(1, 7):
        ctx.render(spp=1, first_timestamp=k - 1)
        refs[k] = ctx.download_compact().copy()
    ctx.frame_begin(W, H)
    for k in range(6):
        ctx.render(spp=1, first_timestamp=k, timestamps_in_flight=1)
        words, folded = ctx.peek_display(d)
        assert 0 <= folded <= k + 1 and np.array_equal(words, demu.map(d, refs[folded])), (k, folded)
    assert np.array_equal(ctx.download_display(d).reshape(-1), demu.map(d, refs[6]))


def test_peek_display_to_device(ctx, demu, cornell):
    """Plain device memory (hipMalloc), 16-byte aligned and not."""
    import ctypes as C

    import gpuspectral_amd as g
    from gpuspectral_amd import abi

    W, H = 96, 64
    n = W * H
    ctx.upload_scene(cornell)
    ctx.frame_begin(W, H)
    ctx.render(spp=3)
    ctx.sync()
    hip = C.CDLL("libamdhip64.so")
    dptr = C.c_void_p()
    nbytes = (n + 8) * 4
    assert hip.hipMalloc(C.byref(dptr), C.c_size_t(nbytes)) == 0
    try:
        for d in (None, abi.display(tonemap=abi.TONEMAP_REINHARD, gamma=2.2, exposure=1.5)):
            want = ctx.download_display(d).reshape(-1)
            for offset in (0, 1):  # words: the second destination is not 16-byte aligned and goes through the context's own buffer
                assert hip.hipMemset(dptr, 0, C.c_size_t(nbytes)) == 0
                folded = ctx.peek_display_to_device(dptr.value + 4 * offset, n * 4, d)
                back = np.zeros(n + 8, np.uint32)
                assert hip.hipMemcpy(C.c_void_p(back.ctypes.data), dptr, C.c_size_t(nbytes), 2) == 0  # hipMemcpyDeviceToHost
                assert folded == 3 and np.array_equal(back[offset:offset + n], want) and not back[:offset].any() and not back[offset + n:].any()
        with pytest.raises(g.GspError, match="destination too small"):
            ctx.peek_display_to_device(dptr.value, n * 4 - 4, None)
    finally:
        hip.hipFree(dptr)


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
    ctx.sync()
    for d in (None, abi.display(tonemap=abi.TONEMAP_REINHARD, gamma=2.2, exposure=1.5), abi.display(tonemap=abi.TONEMAP_ACES)):
        want = ctx.download_display(d).reshape(-1)
        t = torch.zeros(W * H + 4, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        folded = ctx.peek_display_to_device(t.data_ptr(), W * H * 4, d)
        back = t.cpu().numpy().view(np.uint32)
        assert folded == 3 and np.array_equal(back[:W * H], want) and not back[W * H:].any()
        assert (back[:W * H] >> 24 == 255).all() and len(np.unique(back[:W * H])) > 16
print("torch tensor ok")
"""


def test_peek_display_to_device_torch_tensor():
    """Into a torch tensor, in a process of its own: torch has to be imported before the library is loaded (bench.py does the same)."""
    import sys

    r = subprocess.run([sys.executable, "-c", _TORCH_CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "torch tensor ok" in r.stdout, r.stdout + r.stderr


def test_invalid_display_is_refused(ctx, cornell):
    import gpuspectral_amd as g
    from gpuspectral_amd import abi

    with pytest.raises(g.GspError):
        ctx.download_display(None)  # no frame yet
    ctx.upload_scene(cornell)
    ctx.frame_begin(16, 16)
    for bad, word in ((abi.display(tonemap=9), "tonemap"), (abi.display(gamma=-2.0), "gamma"), (abi.display(exposure=float("nan")), "exposure"),
                      (abi.display(tonemap=1, burn=2.0), "burn")):
        with pytest.raises(g.GspError, match=word):
            ctx.download_display(bad)
        with pytest.raises(g.GspError, match=word):
            ctx.peek_display(bad)
    # gsp_peek_display_to_device asks for the room before it looks at the display (a device destination that is never written)
    assert ctx._L.gsp_peek_display_to_device(ctx._h, C.byref(abi.display(tonemap=9)), 16, 4 * 256 - 4, None) == 1
    assert ctx._L.gsp_last_error(ctx._h).decode() == "destination too small"
    assert (ctx.download_display(None) == 0xFF000000).all()  # a frame without samples: black, alpha 255
    assert ctx.frame_luminance()["pixels"] == 256


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
def test_multi_download_display(ctx, demu, cornell, devices):
    """Repeated device indices: several shares on one GPU.  The gathered frame's display equals the single context's."""
    import gpuspectral_amd as g
    from gpuspectral_amd import abi

    W, H = 96, 80
    ctx.upload_scene(cornell)
    ctx.frame_begin(W, H)
    ctx.render(spp=4)
    with g.MultiContext(devices) as m:
        m.upload_scene(cornell)
        m.frame_begin(W, H)
        m.render(spp=4)
        assert np.array_equal(m.download(), ctx.download())
        for name, d in _all_displays()[::3] + [("reinhard", abi.display(tonemap=1))]:
            assert np.array_equal(m.download_display(d), ctx.download_display(d)), name
        with pytest.raises(g.GspError, match="tonemap"):
            m.download_display(abi.display(tonemap=5))


def test_host_layer_download_display(demu):
    from gpuspectral_amd import abi, host

    W, H = 48, 40
    sc = host.Scene(CORNELL_XML, read_film=True)
    pt = host.PathTracer(W, H)
    try:
        pt.render(sc, 4)
        hdr = pt.download().reshape(-1, 4)
        ldr, d = sc.film
        assert ldr and np.array_equal(pt.download_display(d).reshape(-1), demu.map(d, hdr))  # the scene's film: clamp, gamma 2.2
        d2 = abi.display(tonemap=abi.TONEMAP_ACES)
        assert np.array_equal(pt.download_display(d2).reshape(-1), demu.map(d2, hdr))
    finally:
        pt.close()


# ---- CLI ------------------------------------------------------------------------------------------------------------------
def _run_cli(args):
    lib = os.path.join(ROOT, "gpuspectral_amd", "lib")
    env = dict(os.environ, LD_LIBRARY_PATH=lib + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([os.path.join(lib, "gsp_render")] + args, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_cli_ldr_png(ctx, demu, cornell, tmp_path):
    from gpuspectral_amd import abi, host

    W, H, SPP = 64, 48, 4
    plain, with_png, png = str(tmp_path / "a.pfm"), str(tmp_path / "b.pfm"), str(tmp_path / "b.png")
    out_plain = _run_cli([CORNELL_XML, plain, str(W), str(H), str(SPP)])
    _run_cli(["--ldr", png, "--tonemap", "reinhard:0.36:0.25", "--exposure", "0.5", "--gamma", "2.2", CORNELL_XML, with_png, str(W), str(H), str(SPP)])
    assert open(plain, "rb").read() == open(with_png, "rb").read()  # the PFM does not change ...
    assert open(plain + ".ppm", "rb").read() == open(with_png + ".ppm", "rb").read()  # ... nor the preview
    assert not os.path.exists(str(tmp_path / "a.png")) and sorted(os.listdir(str(tmp_path))) == ["a.pfm", "a.pfm.ppm", "b.pfm", "b.pfm.ppm", "b.png"]
    assert "triangles" in out_plain
    ctx.upload_scene(cornell)
    ctx.frame_begin(W, H)
    ctx.render(spp=SPP)
    d = abi.display(tonemap=abi.TONEMAP_REINHARD, key=0.36, burn=0.25, exposure=0.5, gamma=2.2)
    want = ctx.download_display(d)
    got = host.decode_png(open(png, "rb").read())[::-1]  # (decodePng hands the rows back bottom-up)
    assert got.shape == (H, W) and np.array_equal(got, want)
    # --scene-film: the Cornell scene's ldrfilm (gamma 2.2, clamp); a flag overrides one value
    png2, png3 = str(tmp_path / "c.png"), str(tmp_path / "d.png")
    _run_cli(["--ldr", png2, "--scene-film", CORNELL_XML, str(tmp_path / "c.pfm"), str(W), str(H), str(SPP)])
    assert np.array_equal(host.decode_png(open(png2, "rb").read())[::-1], ctx.download_display(abi.display(gamma=2.2)))
    _run_cli(["--ldr", png3, "--scene-film", "--tonemap", "aces", CORNELL_XML, str(tmp_path / "d.pfm"), str(W), str(H), str(SPP)])
    assert np.array_equal(host.decode_png(open(png3, "rb").read())[::-1], ctx.download_display(abi.display(tonemap=abi.TONEMAP_ACES, gamma=2.2)))
    # several shares: the gathered frame
    png4 = str(tmp_path / "e.png")
    _run_cli(["--ldr", png4, CORNELL_XML, str(tmp_path / "e.pfm"), str(W), str(H), str(SPP), "0,0"])
    assert np.array_equal(host.decode_png(open(png4, "rb").read())[::-1], ctx.download_display(None))
