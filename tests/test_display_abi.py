"""LDR film without a GPU: gsp_display / gsp_luminance against the C header (ABI still 9), the validation and struct_size rule of
gsp_*_display (the library's own resolve_display, compiled for the host in tests/emu/display_emu.cpp), and the CLI flags."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT
from display_util import DisplayEmu


@pytest.fixture(scope="module")
def demu():
    return DisplayEmu()


def test_structs_match_header(tmp_path):
    from gpuspectral_amd import abi

    fields = ["struct_size", "tonemap", "exposure", "gamma", "key", "burn", "log_avg_luminance", "max_luminance"]
    lfields = ["log_sum_q20", "pixels", "log_avg", "max"]
    body = ('printf("%zu %zu ", sizeof(gsp_display), sizeof(gsp_luminance));'
            + "".join('printf("%%zu ", offsetof(gsp_display, %s));' % f for f in fields)
            + "".join('printf("%%zu ", offsetof(gsp_luminance, %s));' % f for f in lfields)
            + 'printf("%d %u %u %u\\n", GSP_ABI_VERSION, GSP_TONEMAP_CLAMP, GSP_TONEMAP_REINHARD, GSP_TONEMAP_ACES);')
    protos = ("int (*a)(gsp_context*, int, gsp_luminance*) = gsp_frame_luminance;"
              "int (*b)(gsp_context*, const gsp_display*, uint32_t*) = gsp_download_display;"
              "int (*c)(gsp_context*, const gsp_display*, uint32_t*, uint32_t*) = gsp_peek_display;"
              "int (*d)(gsp_context*, const gsp_display*, void*, uint64_t, uint32_t*) = gsp_peek_display_to_device;"
              "int (*e)(gsp_multi*, const gsp_display*, uint32_t*) = gsp_multi_download_display; (void)a; (void)b; (void)c; (void)d; (void)e;")
    head = '#include <stdio.h>\n#include <stddef.h>\n#include "gpuspectral_pt.h"\nint main(){'
    src = tmp_path / "d.c"
    src.write_text(head + protos + "return 0;}\n")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "d.o")])  # the prototypes
    src2 = tmp_path / "d2.c"
    src2.write_text(head + body + "return 0;}\n")
    exe = tmp_path / "d2"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src2), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert vals[0] == C.sizeof(abi.Display) == 32 and vals[1] == C.sizeof(abi.Luminance) == 24
    assert vals[2:10] == [getattr(abi.Display, f).offset for f in fields] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert vals[10:14] == [getattr(abi.Luminance, f).offset for f in lfields] == [0, 8, 16, 20]
    assert vals[14] == abi.GSP_ABI_VERSION == 9
    assert vals[15:18] == [abi.TONEMAP_CLAMP, abi.TONEMAP_REINHARD, abi.TONEMAP_ACES] == [0, 1, 2]
    assert abi.display().struct_size == 32


def test_abi_version_still_9_and_exports_exist():
    from gpuspectral_amd import pt

    L = pt.load()
    assert L.gsp_abi_version() == 9
    for name in ("gsp_frame_luminance", "gsp_download_display", "gsp_peek_display", "gsp_peek_display_to_device", "gsp_multi_download_display"):
        assert name in pt.EXPORTS and getattr(L, name)


def test_null_context_is_invalid():
    import numpy as np

    from gpuspectral_amd import abi, pt

    L = pt.load()
    d = abi.display()
    out = np.zeros(4, np.uint32)
    lum = abi.Luminance()
    assert L.gsp_frame_luminance(None, 1, C.byref(lum)) == 1  # GSP_ERR_INVALID
    assert L.gsp_download_display(None, C.byref(d), out.ctypes.data) == 1
    assert L.gsp_peek_display(None, C.byref(d), out.ctypes.data, None) == 1
    assert L.gsp_peek_display_to_device(None, C.byref(d), out.ctypes.data, 16, None) == 1
    assert L.gsp_multi_download_display(None, C.byref(d), out.ctypes.data) == 1
    assert not out.any()


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("fields,word", [
    (dict(tonemap=3), "tonemap"), (dict(tonemap=0xFFFFFFFF), "tonemap"),
    (dict(exposure=NAN), "exposure"), (dict(exposure=INF), "exposure"), (dict(exposure=-INF), "exposure"), (dict(exposure=65.0), "exposure"),
    (dict(gamma=-1.0), "gamma"), (dict(gamma=NAN), "gamma"), (dict(gamma=INF), "gamma"),
    (dict(tonemap=1, key=-0.1), "key"), (dict(tonemap=1, key=1.5), "key"), (dict(tonemap=1, key=NAN), "key"),
    (dict(tonemap=1, burn=-0.1), "burn"), (dict(tonemap=1, burn=1.1), "burn"), (dict(tonemap=1, burn=NAN), "burn"),
    (dict(tonemap=1, log_avg_luminance=-1.0), "log_avg_luminance"), (dict(tonemap=1, log_avg_luminance=NAN), "log_avg_luminance"),
    (dict(tonemap=1, log_avg_luminance=INF), "log_avg_luminance"),
    (dict(tonemap=1, max_luminance=-1.0), "max_luminance"), (dict(tonemap=1, max_luminance=NAN), "max_luminance"),
    (dict(tonemap=1, max_luminance=INF), "max_luminance"),
])
def test_validation_errors(demu, fields, word):
    from gpuspectral_amd import abi

    out, err = demu.resolve(abi.display(**fields))
    assert out is None and word in err, err


@pytest.mark.parametrize("fields", [
    dict(), dict(tonemap=2), dict(tonemap=1), dict(gamma=2.2), dict(exposure=-64.0), dict(exposure=64.0), dict(tonemap=1, key=1.0, burn=1.0),
    dict(tonemap=1, key=0.18, burn=0.0, log_avg_luminance=0.5, max_luminance=12.0), dict(tonemap=2, gamma=1.0, exposure=1.5),
])
def test_valid_displays(demu, fields):
    from gpuspectral_amd import abi

    out, err = demu.resolve(abi.display(**fields))
    assert err is None and out.struct_size == 32
    assert out.tonemap == fields.get("tonemap", 0) and out.gamma == C.c_float(fields.get("gamma", 0.0)).value


def test_null_and_zeroed_are_clamp_srgb(demu):
    from gpuspectral_amd import abi

    for d in (None, abi.Display()):
        out, err = demu.resolve(d)
        assert err is None
        assert (out.tonemap, out.exposure, out.gamma, out.key, out.burn, out.log_avg_luminance, out.max_luminance) == (0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    k = demu.consts(None, [[0.5, 0.5, 0.5, 1.0]])
    assert (k["tonemap"], k["srgb"], float(k["exposure_scale"])) == (0, 1, 1.0)


def test_struct_size_rule(demu):
    """A shorter struct reads its missing fields as 0; a longer one is read up to the fields this library knows."""
    from gpuspectral_amd import abi

    full = abi.display(tonemap=1, exposure=1.0, gamma=2.2, key=0.5, burn=0.25, log_avg_luminance=0.3, max_luminance=9.0)
    full.struct_size = abi.Display.key.offset  # a host whose header ends behind gamma
    out, err = demu.resolve(full)
    assert err is None and (out.tonemap, out.exposure, out.gamma) == (1, 1.0, C.c_float(2.2).value)
    assert (out.key, out.burn, out.log_avg_luminance, out.max_luminance) == (0.0, 0.0, 0.0, 0.0)
    full.struct_size = abi.Display.exposure.offset  # tonemap alone
    out, err = demu.resolve(full)
    assert err is None and (out.tonemap, out.exposure, out.gamma) == (1, 0.0, 0.0)
    full.struct_size = 0  # the zeroed struct's own size field: everything 0
    out, err = demu.resolve(full)
    assert err is None and (out.tonemap, out.gamma) == (0, 0.0)
    full.struct_size = 400  # a newer host
    out, err = demu.resolve(full)
    assert err is None and (out.key, out.burn, out.max_luminance) == (0.5, 0.25, 9.0) and out.struct_size == 32
    bad = abi.display(tonemap=7)
    bad.struct_size = abi.Display.tonemap.offset  # the bad field lies beyond the struct: not read
    assert demu.resolve(bad)[1] is None


def test_resolved_constants(demu):
    """2^exposure, 1/gamma, scale and invWp2 are formed in double and rounded to float once."""
    import numpy as np

    from gpuspectral_amd import abi

    px = [[0.5, 0.5, 0.5, 1.0]]
    k = demu.consts(abi.display(exposure=1.5, gamma=2.2), px)
    assert k["exposure_scale"] == np.float32(2.0 ** float(np.float32(1.5))) and k["inv_gamma"] == np.float32(1.0 / float(np.float32(2.2))) and k["srgb"] == 0
    k = demu.consts(abi.display(tonemap=1, key=0.36, burn=0.5, log_avg_luminance=0.25, max_luminance=8.0), px)
    key, lavg, lmax, burn = (float(np.float32(v)) for v in (0.36, 0.25, 8.0, 0.5))
    scale = key / lavg
    assert k["scale"] == np.float32(scale) and k["inv_wp2"] == np.float32(1.0 / ((lmax * scale) ** 2 * (1.0 - burn) ** 4))
    k = demu.consts(abi.display(tonemap=1, log_avg_luminance=0.25, max_luminance=8.0), px)
    assert k["scale"] == np.float32(0.18 / 0.25)  # key 0 = 0.18
    k = demu.consts(abi.display(tonemap=1), np.zeros((0, 4), np.float32))
    assert (float(k["scale"]), float(k["inv_wp2"])) == (1.0, 0.0)  # a frame without a finite pixel
    k = demu.consts(abi.display(tonemap=1), np.zeros((5, 4), np.float32))
    assert float(k["inv_wp2"]) == 0.0 and float(k["scale"]) == 1.0  # an all-black frame: Lmax = 0


# ---- CLI ------------------------------------------------------------------------------------------------------------------
def _cli():
    lib = os.path.join(ROOT, "gpuspectral_amd", "lib")
    exe = os.path.join(lib, "gsp_render")
    assert os.path.exists(exe), "host CLI not built (make -C gpuspectral_amd/host)"
    return exe, dict(os.environ, LD_LIBRARY_PATH=lib + ":" + os.environ.get("LD_LIBRARY_PATH", ""))


def test_cli_usage_names_the_film_flags():
    exe, env = _cli()
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    for tok in ("--ldr out.png", "--tonemap clamp|aces|reinhard[:key[:burn]]", "--exposure E", "--gamma G|srgb", "--scene-film"):
        assert tok in r.stderr, tok
    for tok in ("--dormant-features", "--filter none|box|tent[:r]|gaussian[:s]", "--scene-filter", "--aperture R", "--scene-lens", "scene.xml out.pfm",
                "[width height spp [device | d0,d1,...]]"):
        assert tok in r.stderr, tok


@pytest.mark.parametrize("flags", [
    ["--ldr", "o.png"], ["--ldr", "o.png", "--tonemap", "aces"], ["--ldr", "o.png", "--tonemap", "clamp", "--gamma", "2.2"],
    ["--ldr", "o.png", "--tonemap", "reinhard"], ["--ldr", "o.png", "--tonemap", "reinhard:0.36"], ["--ldr", "o.png", "--tonemap", "reinhard:0.36:0.5"],
    ["--ldr", "o.png", "--exposure", "-1.5"], ["--ldr", "o.png", "--gamma", "srgb"], ["--ldr", "o.png", "--scene-film"],
    ["--tonemap", "aces", "--exposure", "1", "--ldr", "o.png"],
])
def test_cli_parses_film_flags(tmp_path, flags):
    """A bad device list is reported AFTER the options, so reaching it means the options were accepted."""
    exe, env = _cli()
    r = subprocess.run([exe] + flags + [str(tmp_path / "none.xml"), str(tmp_path / "x.pfm"), "8", "8", "1", "abc"], env=env, capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 2 and "unknown option" not in r.stderr and "gsp_render: bad " + "device list" in r.stderr, r.stderr
    assert r.stderr.count("gsp_render: bad") == 1, r.stderr


@pytest.mark.parametrize("flags,word", [
    (["--ldr", "o.png", "--tonemap", "filmic"], "bad tonemap"), (["--ldr", "o.png", "--tonemap", ""], "bad tonemap"),
    (["--ldr", "o.png", "--tonemap", "aces:0.5"], "bad tonemap"), (["--ldr", "o.png", "--tonemap", "reinhard:"], "bad tonemap"),
    (["--ldr", "o.png", "--tonemap", "reinhard:0"], "bad tonemap"), (["--ldr", "o.png", "--tonemap", "reinhard:2"], "bad tonemap"),
    (["--ldr", "o.png", "--tonemap", "reinhard:0.2:1.5"], "bad tonemap"), (["--ldr", "o.png", "--tonemap", "reinhard:0.2:x"], "bad tonemap"),
    (["--ldr", "o.png", "--exposure", "x"], "bad exposure"), (["--ldr", "o.png", "--exposure", "nan"], "bad exposure"),
    (["--ldr", "o.png", "--exposure", "100"], "bad exposure"), (["--ldr", "o.png", "--gamma", "0"], "bad gamma"),
    (["--ldr", "o.png", "--gamma", "-2.2"], "bad gamma"), (["--ldr", "o.png", "--gamma", "linear"], "bad gamma"),
    (["--tonemap", "aces"], "need --ldr"), (["--exposure", "1"], "need --ldr"), (["--gamma", "2.2"], "need --ldr"), (["--scene-film"], "need --ldr"),
])
def test_cli_rejects_bad_film_flags(tmp_path, flags, word):
    exe, env = _cli()
    r = subprocess.run([exe] + flags + [str(tmp_path / "none.xml"), str(tmp_path / "x.pfm"), "8", "8", "1", "abc"], env=env, capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 2 and word in r.stderr and "bad device list" not in r.stderr, r.stderr
