"""The illumination history without a GPU: the five prototypes of "Illumination history" against the C header (ABI still 9, the three
parameter structs unchanged), the exports, the NULL-handle returns, the Python and host bindings, and the CLI flags."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = ("gsp_temporal_demodulate", "gsp_download_temporal_image", "gsp_temporal_image_to_device", "gsp_temporal_svgf_feedback",
           "gsp_temporal_svgf_feedback_to_device")
METHODS = ("temporal_demodulate", "download_temporal_image", "temporal_image_to_device", "temporal_svgf_feedback", "temporal_svgf_feedback_to_device")


def test_prototypes_and_structs_match_the_header(tmp_path):
    from gpuspectral_amd import abi

    protos = ("int (*a)(gsp_context*, int) = gsp_temporal_demodulate;"
              "int (*b)(gsp_context*, float*) = gsp_download_temporal_image;"
              "int (*c)(gsp_context*, void*, uint64_t) = gsp_temporal_image_to_device;"
              "int (*d)(gsp_context*, const gsp_denoise*, const gsp_svgf*, uint32_t, float*) = gsp_temporal_svgf_feedback;"
              "int (*e)(gsp_context*, const gsp_denoise*, const gsp_svgf*, uint32_t, void*, uint64_t) = gsp_temporal_svgf_feedback_to_device;"
              "(void)a; (void)b; (void)c; (void)d; (void)e;")
    head = '#include <stdio.h>\n#include <stddef.h>\n#include "gpuspectral_pt.h"\nint main(){'
    src = tmp_path / "t.c"
    src.write_text(head + protos + "return 0;}\n")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])  # the prototypes
    src2 = tmp_path / "t2.c"
    src2.write_text(head + 'printf("%zu %zu %zu %d\\n", sizeof(gsp_temporal), sizeof(gsp_svgf), sizeof(gsp_denoise), GSP_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "t2"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src2), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert vals[:3] == [C.sizeof(abi.Temporal), C.sizeof(abi.Svgf), C.sizeof(abi.Denoise)] == [20, 12, 24]  # no existing struct changed
    assert vals[3] == abi.GSP_ABI_VERSION == 9


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
    for name in ("temporalDemodulate", "downloadTemporalImage", "temporalImageToDevice", "temporalSvgfFeedback", "temporalSvgfFeedbackToDevice"):
        assert name + "(" in text, name


def test_null_handles_are_invalid():
    from gpuspectral_amd import pt

    L = pt.load()
    out = np.zeros(16, np.float32)
    assert L.gsp_temporal_demodulate(None, 1) == 1  # GSP_ERR_INVALID
    assert L.gsp_download_temporal_image(None, out.ctypes.data) == 1
    assert L.gsp_temporal_image_to_device(None, out.ctypes.data, 64) == 1
    assert L.gsp_temporal_svgf_feedback(None, None, None, 1, out.ctypes.data) == 1
    assert L.gsp_temporal_svgf_feedback_to_device(None, None, None, 1, out.ctypes.data, 64) == 1
    assert not out.any()


def test_the_header_states_the_section_and_its_limits():
    with open(os.path.join(ROOT, "include", "gpuspectral_pt.h")) as fh:
        text = fh.read()
    for word in ("Illumination history.", "fed back already", "upper bound", "temporal gradients (A-SVGF)", "separate direct and indirect histories"):
        assert word in text, word
    top = text[:text.index("status codes")]
    for name in SYMBOLS:
        assert name in top, name  # the ABI-9 list
    with open(os.path.join(ROOT, "gpuspectral_amd", "csrc", "Makefile")) as fh:
        assert "pt_illum.h" in fh.read()  # the digest of gsp_build_info covers the new header


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


def test_cli_usage_names_the_flags():
    exe, env = _cli()
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "[--temporal-demodulate] [--svgf-feedback LEVELS]" in r.stderr


@pytest.mark.parametrize("flags", [
    TEMPORAL + ["--temporal-demodulate"], TEMPORAL + ["--svgf", "s.pfm", "--svgf-feedback", "1"],
    ["--svgf-feedback", "5", "--temporal-demodulate", "--svgf", "s.pfm", "--temporal-follow"] + TEMPORAL,
])
def test_cli_parses_the_flags(tmp_path, flags):
    """A bad device list is reported AFTER the options, so reaching it means the options were accepted."""
    r = _run(tmp_path, flags)
    assert r.returncode == 2 and "unknown option" not in r.stderr and "gsp_render: bad device list" in r.stderr, r.stderr
    assert r.stderr.count("gsp_render: bad") == 1, r.stderr


@pytest.mark.parametrize("flags,word", [
    (["--temporal-demodulate"], "--temporal-demodulate needs --temporal"),
    (TEMPORAL + ["--svgf", "s.pfm", "--svgf-feedback", "0"], "bad svgf feedback"), (TEMPORAL + ["--svgf", "s.pfm", "--svgf-feedback", "9"], "bad svgf feedback"),
    (TEMPORAL + ["--svgf", "s.pfm", "--svgf-feedback", "x"], "bad svgf feedback"), (TEMPORAL + ["--svgf", "s.pfm", "--svgf-feedback", "1.5"], "bad svgf feedback"),
])
def test_cli_rejects_bad_flags(tmp_path, flags, word):
    r = _run(tmp_path, flags)
    assert r.returncode == 2 and word in r.stderr and "bad device list" not in r.stderr, r.stderr


def test_cli_feedback_without_svgf_exits_1_with_its_message(tmp_path):
    r = _run(tmp_path, TEMPORAL + ["--svgf-feedback", "1"], devices="0")
    assert r.returncode == 1 and "--svgf-feedback needs --svgf" in r.stderr, r.stderr
