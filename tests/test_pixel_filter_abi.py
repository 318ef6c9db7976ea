"""Pixel filter without a GPU: the two new fields' layout against the C header (ABI still 9), their defaults, the CLI flags."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT


def test_pixel_filter_fields_match_header(tmp_path):
    from gpuspectral_amd import abi

    src = tmp_path / "pf.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "gpuspectral_pt.h"\n'
        "int main(){printf(\"%zu %zu %zu %zu %zu %d %u %u %u %u\\n\",sizeof(gsp_render_params),"
        "offsetof(gsp_render_params,pixel_filter),offsetof(gsp_render_params,pixel_filter_param),"
        "sizeof(((gsp_render_params*)0)->pixel_filter),sizeof(((gsp_render_params*)0)->pixel_filter_param),"
        "GSP_ABI_VERSION,GSP_FILTER_NONE,GSP_FILTER_BOX,GSP_FILTER_TENT,GSP_FILTER_GAUSSIAN);return 0;}\n"
    )
    exe = tmp_path / "pf"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert vals[0] == C.sizeof(abi.RenderParams)
    # the two fields are the LAST of the struct, right behind the adaptive ones
    assert vals[1] == abi.RenderParams.pixel_filter.offset == abi.RenderParams.adaptive_step.offset + 4
    assert vals[2] == abi.RenderParams.pixel_filter_param.offset == vals[1] + 4
    assert vals[2] + 4 == vals[0]
    assert vals[3] == 4 and vals[4] == 4
    assert vals[5] == abi.GSP_ABI_VERSION == 9
    assert vals[6:10] == [abi.FILTER_NONE, abi.FILTER_BOX, abi.FILTER_TENT, abi.FILTER_GAUSSIAN] == [0, 1, 2, 3]


def test_abi_version_still_9():
    from gpuspectral_amd import pt

    assert pt.load().gsp_abi_version() == 9


def test_default_render_params_leave_filter_off():
    from gpuspectral_amd import abi, pt

    p = abi.RenderParams()
    p.pixel_filter, p.pixel_filter_param = 3, 7.0
    pt.load().gsp_default_render_params(C.byref(p))
    assert (p.pixel_filter, p.pixel_filter_param) == (0, 0.0)
    assert p.struct_size == C.sizeof(abi.RenderParams)
    q = abi.default_render_params(4, 2)
    assert (q.pixel_filter, q.pixel_filter_param) == (0, 0.0)
    assert q.struct_size == C.sizeof(abi.RenderParams)


def _cli():
    lib = os.path.join(ROOT, "gpuspectral_amd", "lib")
    exe = os.path.join(lib, "gsp_render")
    assert os.path.exists(exe), "host CLI not built (make -C gpuspectral_amd/host)"
    return exe, dict(os.environ, LD_LIBRARY_PATH=lib + ":" + os.environ.get("LD_LIBRARY_PATH", ""))


def test_cli_usage_names_filter():
    exe, env = _cli()
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "--filter none|box|tent[:r]|gaussian[:s]" in r.stderr and "--scene-filter" in r.stderr
    # every token the usage line had before is still there
    for tok in ("--dormant-features", "--builtin-shapes", "--no-nee", "--memory-share F", "--pool-paths N", "--adaptive T",
                "--adaptive-min N", "--adaptive-step N", "scene.xml out.pfm"):
        assert tok in r.stderr, tok


@pytest.mark.parametrize("value", ["tent:1.5", "tent", "box", "gaussian:0.75", "gaussian", "none"])
def test_cli_parses_filter(tmp_path, value):
    """The flag is parsed: a bad device list is reported AFTER the options, so reaching it means the option was accepted."""
    exe, env = _cli()
    r = subprocess.run([exe, "--filter", value, "--scene-filter", str(tmp_path / "none.xml"), str(tmp_path / "x.pfm"), "8", "8", "1", "abc"],
                       env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "unknown option" not in r.stderr and "bad filter" not in r.stderr and "bad device list" in r.stderr, r.stderr


@pytest.mark.parametrize("value", ["mitchell", "tent:", "tent:x", "tent:-1", "box:2", "none:1", ""])
def test_cli_rejects_bad_filter(tmp_path, value):
    exe, env = _cli()
    r = subprocess.run([exe, "--filter", value, str(tmp_path / "none.xml"), str(tmp_path / "x.pfm"), "8", "8", "1", "abc"],
                       env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "bad filter" in r.stderr and "bad device list" not in r.stderr, r.stderr
