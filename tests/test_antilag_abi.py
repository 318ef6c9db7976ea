"""The temporal anti-lag without a GPU: the three prototypes and the struct of "Temporal anti-lag" against the C header (ABI still 9, the
existing parameter structs unchanged), the exports, the NULL-handle returns, the Python and host bindings, and the CLI flags."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = ("gsp_temporal_antilag", "gsp_download_temporal_fast", "gsp_temporal_fast_to_device")
METHODS = ("temporal_antilag", "download_temporal_fast", "temporal_fast_to_device")


def test_prototypes_and_struct_match_the_header(tmp_path):
    from gpuspectral_amd import abi

    protos = ("int (*a)(gsp_context*, const gsp_antilag*) = gsp_temporal_antilag;"
              "int (*b)(gsp_context*, float*) = gsp_download_temporal_fast;"
              "int (*c)(gsp_context*, void*, uint64_t) = gsp_temporal_fast_to_device;"
              "(void)a; (void)b; (void)c;")
    head = '#include <stdio.h>\n#include <stddef.h>\n#include "gpuspectral_pt.h"\nint main(){'
    src = tmp_path / "t.c"
    src.write_text(head + protos + "return 0;}\n")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])  # the prototypes
    src2 = tmp_path / "t2.c"
    src2.write_text(head + 'printf("%zu %zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(gsp_antilag), offsetof(gsp_antilag, struct_size), '
                    "offsetof(gsp_antilag, fast_history), offsetof(gsp_antilag, radius), offsetof(gsp_antilag, sigma_scale), sizeof(gsp_temporal), sizeof(gsp_svgf), "
                    "sizeof(gsp_denoise), GSP_ABI_VERSION);return 0;}\n")
    exe = tmp_path / "t2"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src2), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    A = abi.Antilag
    assert vals[:5] == [C.sizeof(A), A.struct_size.offset, A.fast_history.offset, A.radius.offset, A.sigma_scale.offset] == [16, 0, 4, 8, 12]
    assert vals[5:8] == [C.sizeof(abi.Temporal), C.sizeof(abi.Svgf), C.sizeof(abi.Denoise)] == [20, 12, 24]  # no existing struct changed
    assert vals[8] == abi.GSP_ABI_VERSION == 9
    al = abi.antilag(3, 1, 1.5)
    assert (al.struct_size, al.fast_history, al.radius, al.sigma_scale) == (16, 3, 1, 1.5)
    z = abi.antilag()
    assert (z.struct_size, z.fast_history, z.radius, z.sigma_scale) == (16, 0, 0, 0.0)


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
    for name in ("temporalAntilag", "downloadTemporalFast", "temporalFastToDevice"):
        assert name + "(" in text, name


def test_null_handles_are_invalid():
    """The refusals that need no GPU: a NULL context is GSP_ERR_INVALID and nothing is written."""
    from gpuspectral_amd import abi, pt

    L = pt.load()
    out = np.zeros(16, np.float32)
    assert L.gsp_temporal_antilag(None, None) == 1  # GSP_ERR_INVALID
    assert L.gsp_temporal_antilag(None, C.byref(abi.antilag(radius=9))) == 1
    assert L.gsp_download_temporal_fast(None, out.ctypes.data) == 1
    assert L.gsp_temporal_fast_to_device(None, out.ctypes.data, 64) == 1
    assert not out.any()


def test_the_header_states_the_section_and_its_limits():
    with open(os.path.join(ROOT, "include", "gpuspectral_pt.h")) as fh:
        text = fh.read()
    assert text.index("Temporal anti-lag.") > text.index("Illumination history.")  # the section follows it
    for word in ("Step A, the fast history.", "Step B, the clamp", "fast_valid", "M is not clamped", "Values whose square overflows float32 are outside the domain",
                 "min(fast_history, max_history)", "n < 2 radius + 1"):
        assert word in text, word
    top = text[:text.index("status codes")]
    for name in SYMBOLS:
        assert name in top, name  # the ABI-9 list
    with open(os.path.join(ROOT, "gpuspectral_amd", "csrc", "Makefile")) as fh:
        assert "pt_antilag.h" in fh.read()  # the digest of gsp_build_info covers the new header
    from gpuspectral_amd import pt

    assert "pt_antilag.h" in pt.DIGEST_SOURCES


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
    assert r.returncode == 2 and "[--temporal-antilag [--antilag-fast N] [--antilag-radius R] [--antilag-sigma S]]" in r.stderr


@pytest.mark.parametrize("flags", [
    TEMPORAL + ["--temporal-antilag"], TEMPORAL + ["--temporal-antilag", "--antilag-fast", "64", "--antilag-radius", "3", "--antilag-sigma", "0.5"],
    ["--antilag-radius", "1", "--temporal-antilag", "--svgf", "s.pfm", "--svgf-feedback", "1", "--temporal-demodulate", "--temporal-follow"] + TEMPORAL,
])
def test_cli_parses_the_flags(tmp_path, flags):
    """A bad device list is reported AFTER the options, so reaching it means the options were accepted."""
    r = _run(tmp_path, flags)
    assert r.returncode == 2 and "unknown option" not in r.stderr and "gsp_render: bad device list" in r.stderr, r.stderr
    assert r.stderr.count("gsp_render: bad") == 1, r.stderr


@pytest.mark.parametrize("flags,word", [
    (["--temporal-antilag"], "--temporal-antilag needs --temporal"),
    (TEMPORAL + ["--antilag-fast", "3"], "need --temporal-antilag"), (TEMPORAL + ["--antilag-radius", "1"], "need --temporal-antilag"),
    (TEMPORAL + ["--antilag-sigma", "1"], "need --temporal-antilag"),
    (TEMPORAL + ["--temporal-antilag", "--antilag-fast", "0"], "bad antilag fast history"), (TEMPORAL + ["--temporal-antilag", "--antilag-fast", "65"], "bad antilag fast history"),
    (TEMPORAL + ["--temporal-antilag", "--antilag-fast", "x"], "bad antilag fast history"), (TEMPORAL + ["--temporal-antilag", "--antilag-radius", "4"], "bad antilag radius"),
    (TEMPORAL + ["--temporal-antilag", "--antilag-radius", "1.5"], "bad antilag radius"), (TEMPORAL + ["--temporal-antilag", "--antilag-sigma", "0"], "bad antilag sigma"),
    (TEMPORAL + ["--temporal-antilag", "--antilag-sigma", "-2"], "bad antilag sigma"), (TEMPORAL + ["--temporal-antilag", "--antilag-sigma", "inf"], "bad antilag sigma"),
])
def test_cli_rejects_bad_flags(tmp_path, flags, word):
    r = _run(tmp_path, flags)
    assert r.returncode == 2 and word in r.stderr and "bad device list" not in r.stderr, r.stderr
