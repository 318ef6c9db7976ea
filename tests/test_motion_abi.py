"""Moved instances without a GPU: the three prototypes of "Temporal accumulation: moved instances" against the C header (ABI still 9,
gsp_temporal still 20 bytes), the exports, the NULL-handle returns, and the CLI flags."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = ("gsp_temporal_follow_instances", "gsp_download_temporal_motion", "gsp_temporal_motion_to_device")


def test_prototypes_and_structs_match_the_header(tmp_path):
    from gpuspectral_amd import abi

    protos = ("int (*a)(gsp_context*, int) = gsp_temporal_follow_instances;"
              "int (*b)(gsp_context*, float*) = gsp_download_temporal_motion;"
              "int (*c)(gsp_context*, void*, uint64_t) = gsp_temporal_motion_to_device;"
              "(void)a; (void)b; (void)c;")
    head = '#include <stdio.h>\n#include <stddef.h>\n#include "gpuspectral_pt.h"\nint main(){'
    src = tmp_path / "t.c"
    src.write_text(head + protos + "return 0;}\n")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])  # the prototypes
    src2 = tmp_path / "t2.c"
    src2.write_text(head + 'printf("%zu %zu %zu %zu %d\\n", sizeof(gsp_temporal), sizeof(gsp_svgf), sizeof(gsp_denoise), sizeof(gsp_instance), GSP_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "t2"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src2), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert vals[:3] == [C.sizeof(abi.Temporal), C.sizeof(abi.Svgf), C.sizeof(abi.Denoise)] == [20, 12, 24]  # no existing struct changed
    assert vals[3] == abi.INSTANCE_DT.itemsize == 92
    assert vals[4] == abi.GSP_ABI_VERSION == 9


def test_abi_version_still_9_and_exports_exist():
    from gpuspectral_amd import pt

    L = pt.load()
    assert L.gsp_abi_version() == 9
    for name in SYMBOLS:
        assert name in pt.EXPORTS and getattr(L, name)
    for name in ("temporal_follow_instances", "download_temporal_motion", "temporal_motion_to_device"):
        assert callable(getattr(pt.Context, name))


def test_null_handles_are_invalid():
    from gpuspectral_amd import pt

    L = pt.load()
    out = np.zeros(16, np.float32)
    assert L.gsp_temporal_follow_instances(None, 1) == 1  # GSP_ERR_INVALID
    assert L.gsp_download_temporal_motion(None, out.ctypes.data) == 1
    assert L.gsp_temporal_motion_to_device(None, out.ctypes.data, 64) == 1
    assert not out.any()


def test_the_header_no_longer_defers_motion_vectors():
    for path in (os.path.join(ROOT, "include", "gpuspectral_pt.h"), os.path.join(ROOT, "DESIGN.md")):
        with open(path) as fh:
            text = fh.read()
        assert "motion vectors are a later change" not in text and "have no motion vectors" not in text, path


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


def test_cli_usage_names_the_follow_flags():
    exe, env = _cli()
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "[--temporal-follow [--temporal-move INST,DX,DY,DZ] [--motion out.pfm]]" in r.stderr


@pytest.mark.parametrize("flags", [
    FOLLOW, FOLLOW + ["--temporal-move", "6,0.1,0,-0.05"], ["--motion", "v.pfm", "--temporal-move", "0,1e-3,2,3"] + FOLLOW,
    FOLLOW + ["--motion", "v.pfm", "--svgf", "s.pfm"],
])
def test_cli_parses_follow_flags(tmp_path, flags):
    """A bad device list is reported AFTER the options, so reaching it means the options were accepted."""
    r = _run(tmp_path, flags)
    assert r.returncode == 2 and "unknown option" not in r.stderr and "gsp_render: bad device list" in r.stderr, r.stderr
    assert r.stderr.count("gsp_render: bad") == 1, r.stderr


@pytest.mark.parametrize("flags,word", [
    (["--temporal-follow"], "--temporal-follow needs --temporal"),
    (TEMPORAL + ["--temporal-move", "1,0,0,0"], "need --temporal-follow"), (TEMPORAL + ["--motion", "v.pfm"], "need --temporal-follow"),
    (FOLLOW + ["--temporal-move", "1,0,0"], "bad temporal move"), (FOLLOW + ["--temporal-move", "-1,0,0,0"], "bad temporal move"),
    (FOLLOW + ["--temporal-move", "x,0,0,0"], "bad temporal move"), (FOLLOW + ["--temporal-move", "1,0,0,0,0"], "bad temporal move"),
    (FOLLOW + ["--temporal-move", "1,0,nan,0"], "bad temporal move"), (FOLLOW + ["--temporal-move", "1,0,inf,0"], "bad temporal move"),
    (FOLLOW + ["--temporal-move", "1 0 0 0"], "bad temporal move"),
])
def test_cli_rejects_bad_follow_flags(tmp_path, flags, word):
    r = _run(tmp_path, flags)
    assert r.returncode == 2 and word in r.stderr and "bad device list" not in r.stderr, r.stderr
