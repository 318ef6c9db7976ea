"""Temporal anti-aliasing without a GPU: the five prototypes and the struct of "Temporal anti-aliasing" against the C header (ABI still 9,
the existing parameter structs unchanged), the exports, the NULL-handle returns, the Python and host bindings, and the CLI flags."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = ("gsp_temporal_taa", "gsp_temporal_taa_from_device", "gsp_download_taa", "gsp_download_taa_display", "gsp_taa_display_to_device")
METHODS = ("temporal_taa", "temporal_taa_from_device", "download_taa", "download_taa_display", "taa_display_to_device")


def test_prototypes_and_struct_match_the_header(tmp_path):
    from gpuspectral_amd import abi

    protos = ("int (*a)(gsp_context*, const gsp_taa*, const gsp_display*, const float*) = gsp_temporal_taa;"
              "int (*b)(gsp_context*, const gsp_taa*, const gsp_display*, const void*, uint64_t) = gsp_temporal_taa_from_device;"
              "int (*c)(gsp_context*, float*) = gsp_download_taa;"
              "int (*d)(gsp_context*, uint32_t*) = gsp_download_taa_display;"
              "int (*e)(gsp_context*, void*, uint64_t) = gsp_taa_display_to_device;"
              "(void)a; (void)b; (void)c; (void)d; (void)e;")
    head = '#include <stdio.h>\n#include <stddef.h>\n#include "gpuspectral_pt.h"\nint main(){'
    src = tmp_path / "t.c"
    src.write_text(head + protos + "return 0;}\n")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])  # the prototypes
    src2 = tmp_path / "t2.c"
    src2.write_text(head + 'printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(gsp_taa), offsetof(gsp_taa, struct_size), offsetof(gsp_taa, alpha), '
                    "offsetof(gsp_taa, sigma_clip), sizeof(gsp_temporal), sizeof(gsp_svgf), sizeof(gsp_denoise), sizeof(gsp_antilag), sizeof(gsp_display), "
                    "GSP_ABI_VERSION);return 0;}\n")
    exe = tmp_path / "t2"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src2), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    T = abi.Taa
    assert vals[:4] == [C.sizeof(T), T.struct_size.offset, T.alpha.offset, T.sigma_clip.offset] == [12, 0, 4, 8]
    assert vals[4:9] == [C.sizeof(abi.Temporal), C.sizeof(abi.Svgf), C.sizeof(abi.Denoise), C.sizeof(abi.Antilag), C.sizeof(abi.Display)] == [20, 12, 24, 16, 32]
    assert vals[9] == abi.GSP_ABI_VERSION == 9
    t = abi.taa(0.25, 1.5)
    assert (t.struct_size, t.alpha, t.sigma_clip) == (12, 0.25, 1.5)
    z = abi.taa()
    assert (z.struct_size, z.alpha, z.sigma_clip) == (12, 0.0, 0.0)


def test_abi_version_still_9_and_exports_exist():
    from gpuspectral_amd import pt

    L = pt.load()
    assert L.gsp_abi_version() == 9
    for name in SYMBOLS:
        assert name in pt.EXPORTS and getattr(L, name)
    for name in METHODS:
        assert callable(getattr(pt.Context, name))


def test_host_bindings_exist():
    from gpuspectral_amd import host

    L = host.load()
    for name in METHODS:
        assert getattr(L, "gsph_pathtracer_" + name) and callable(getattr(host.PathTracer, name))
    with open(os.path.join(ROOT, "gpuspectral_amd", "host", "PathTracer.h")) as fh:
        text = fh.read()
    for name in ("temporalTaa", "temporalTaaFromDevice", "downloadTaa", "downloadTaaDisplay", "taaDisplayToDevice"):
        assert name + "(" in text, name


def test_null_handles_are_invalid():
    """The refusals that need no GPU: a NULL context is GSP_ERR_INVALID and nothing is written."""
    from gpuspectral_amd import abi, pt

    L = pt.load()
    out = np.zeros(16, np.float32)
    words = np.zeros(16, np.uint32)
    assert L.gsp_temporal_taa(None, None, None, None) == 1  # GSP_ERR_INVALID
    assert L.gsp_temporal_taa(None, C.byref(abi.taa(alpha=2.0)), None, out.ctypes.data) == 1
    assert L.gsp_temporal_taa_from_device(None, None, None, None, 0) == 1
    assert L.gsp_download_taa(None, out.ctypes.data) == 1
    assert L.gsp_download_taa_display(None, words.ctypes.data) == 1
    assert L.gsp_taa_display_to_device(None, words.ctypes.data, 64) == 1
    assert not out.any() and not words.any()


def test_the_header_states_the_section_and_its_limits():
    with open(os.path.join(ROOT, "include", "gpuspectral_pt.h")) as fh:
        text = fh.read()
    assert text.index("Temporal anti-aliasing.") > text.index("Temporal anti-lag.")  # the section follows it
    for word in ("X.y = (0.25f*r + 0.5f*g) + 0.25f*b", "X.co = 0.5f*r - 0.5f*b", "X.cg = (-0.25f*r + 0.5f*g) - 0.25f*b", "t = y - cg;  r = t + co;  g = y + cg;  b = t - co",
                 "Neighbourhood box.", "n += 1.0f;  s1.k += X_q.k;  s2.k += X_q.k * X_q.k", "lo.k = m.k - sigma_clip * sd.k", "taa_valid", "sw < 0.01f", "sw2 < 0.01f",
                 "read from the OLDER D plane", "o.k = c.k + (X_p.k - c.k) * alpha", "steps 5-6 of \"LDR film\" on D'.rgb",
                 "a viewer should pass fixed\n *     log_avg_luminance / max_luminance", "fetched bilinearly", "Catmull-Rom", "Disocclusion is handled by V.z",
                 "deforming meshes and gsp_multi_* variants"):
        assert word in text, word
    top = text[:text.index("status codes")]
    for name in SYMBOLS:
        assert name in top, name  # the ABI-9 list
    with open(os.path.join(ROOT, "gpuspectral_amd", "csrc", "Makefile")) as fh:
        assert "pt_taa.h" in fh.read()  # the digest of gsp_build_info covers the new header
    from gpuspectral_amd import pt

    assert "pt_taa.h" in pt.DIGEST_SOURCES


# ---- CLI ------------------------------------------------------------------------------------------------------------------
def _cli():
    lib = os.path.join(ROOT, "gpuspectral_amd", "lib")
    exe = os.path.join(lib, "gsp_render")
    assert os.path.exists(exe), "host CLI not built (make -C gpuspectral_amd/host)"
    return exe, dict(os.environ, LD_LIBRARY_PATH=lib + ":" + os.environ.get("LD_LIBRARY_PATH", ""))


def _run(tmp_path, flags, devices="abc"):
    exe, env = _cli()
    return subprocess.run([exe] + flags + [str(tmp_path / "none.xml"), str(tmp_path / "x.pfm"), "8", "8", "1", devices], env=env, capture_output=True,
                          text=True, timeout=60)


TEMPORAL = ["--temporal", "o.pfm", "--temporal-frames", "3"]
FOLLOW = TEMPORAL + ["--temporal-follow"]


def test_cli_usage_names_the_flags():
    exe, env = _cli()
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "[--taa out.png [--taa-alpha A] [--taa-sigma S]]" in r.stderr


@pytest.mark.parametrize("flags", [
    FOLLOW + ["--taa", "t.png"], FOLLOW + ["--taa", "t.png", "--taa-alpha", "1", "--taa-sigma", "0.5"],
    ["--taa-alpha", "0.05", "--taa", "t.png", "--svgf", "s.pfm", "--svgf-feedback", "1", "--temporal-demodulate", "--temporal-antilag"] + FOLLOW,
    FOLLOW + ["--taa", "t.png", "--tonemap", "aces", "--exposure", "1", "--gamma", "2.2"],  # (the display flags serve --taa without --ldr)
])
def test_cli_parses_the_flags(tmp_path, flags):
    """A bad device list is reported AFTER the options, so reaching it means the options were accepted."""
    r = _run(tmp_path, flags)
    assert r.returncode == 2 and "unknown option" not in r.stderr and "gsp_render: bad device list" in r.stderr, r.stderr
    assert r.stderr.count("gsp_render: bad") == 1, r.stderr


@pytest.mark.parametrize("flags,word", [
    (["--taa", "t.png"], "--taa needs --temporal out.pfm and --temporal-follow"), (TEMPORAL + ["--taa", "t.png"], "--taa needs --temporal out.pfm and --temporal-follow"),
    (FOLLOW + ["--taa-alpha", "0.5"], "need --taa out.png"), (FOLLOW + ["--taa-sigma", "1"], "need --taa out.png"),
    (FOLLOW + ["--taa", "t.png", "--taa-alpha", "0"], "bad taa alpha"), (FOLLOW + ["--taa", "t.png", "--taa-alpha", "1.5"], "bad taa alpha"),
    (FOLLOW + ["--taa", "t.png", "--taa-alpha", "x"], "bad taa alpha"), (FOLLOW + ["--taa", "t.png", "--taa-alpha", "nan"], "bad taa alpha"),
    (FOLLOW + ["--taa", "t.png", "--taa-sigma", "0"], "bad taa sigma"), (FOLLOW + ["--taa", "t.png", "--taa-sigma", "-2"], "bad taa sigma"),
    (FOLLOW + ["--taa", "t.png", "--taa-sigma", "inf"], "bad taa sigma"),
    (["--tonemap", "aces"], "need --ldr out.png"),  # (unchanged where neither --ldr nor --taa is given)
])
def test_cli_rejects_bad_flags(tmp_path, flags, word):
    r = _run(tmp_path, flags)
    assert r.returncode == 2 and word in r.stderr and "bad device list" not in r.stderr, r.stderr
