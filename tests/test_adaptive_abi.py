"""Adaptive sampling (ABI 9) without a GPU: the new fields' layout against the C header, their defaults, the CLI flags."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import CORNELL_XML, ROOT


def test_adaptive_fields_match_header(tmp_path):
    from gpuspectral_amd import abi

    src = tmp_path / "ad.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "gpuspectral_pt.h"\n'
        "int main(){printf(\"%zu %zu %zu %zu %zu %zu %zu %d\\n\",sizeof(gsp_render_params),"
        "offsetof(gsp_render_params,adaptive_threshold),offsetof(gsp_render_params,adaptive_min_spp),"
        "offsetof(gsp_render_params,adaptive_step),sizeof(gsp_stats),offsetof(gsp_stats,adaptive_rounds),"
        "offsetof(gsp_stats,adaptive_active_pixels),GSP_ABI_VERSION);"
        "printf(\"%.17g\\n\",(double)GSP_ADAPTIVE_LUMINANCE_FLOOR);return 0;}\n"
    )
    exe = tmp_path / "ad"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split()
    vals = [int(x) for x in out[:8]]
    assert vals[0] == C.sizeof(abi.RenderParams)
    assert vals[1] == abi.RenderParams.adaptive_threshold.offset == abi.RenderParams.disable_nee.offset + 4
    assert vals[2] == abi.RenderParams.adaptive_min_spp.offset
    assert vals[3] == abi.RenderParams.adaptive_step.offset
    assert vals[4] == C.sizeof(abi.Stats)
    assert vals[5] == abi.Stats.adaptive_rounds.offset == abi.Stats.scene_splits.offset + 8
    assert vals[6] == abi.Stats.adaptive_active_pixels.offset
    assert vals[7] == abi.GSP_ABI_VERSION == 9
    assert float(out[8]) == abi.ADAPTIVE_LUMINANCE_FLOOR


def test_default_render_params_leave_adaptive_off():
    from gpuspectral_amd import abi, pt

    p = abi.RenderParams()
    for f in ("adaptive_threshold", "adaptive_min_spp", "adaptive_step"):
        setattr(p, f, 7)
    pt.load().gsp_default_render_params(C.byref(p))
    assert (p.adaptive_threshold, p.adaptive_min_spp, p.adaptive_step) == (0.0, 0, 0)
    q = abi.default_render_params(4, 2)
    assert (q.adaptive_threshold, q.adaptive_min_spp, q.adaptive_step) == (0.0, 0, 0)


def test_cli_usage_names_adaptive(tmp_path):
    lib = os.path.join(ROOT, "gpuspectral_amd", "lib")
    exe = os.path.join(lib, "gsp_render")
    if not os.path.exists(exe):
        pytest.skip("host CLI not built")
    env = dict(os.environ, LD_LIBRARY_PATH=lib + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--adaptive T" in r.stderr and "--adaptive-min N" in r.stderr and "--adaptive-step N" in r.stderr
    # the flags are parsed (a missing scene is reported after them, not as an unknown option)
    r = subprocess.run([exe, "--adaptive", "0.05", "--adaptive-min", "8", "--adaptive-step", "8", str(tmp_path / "none.xml"),
                        str(tmp_path / "x.pfm"), "8", "8", "1", "abc"], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "unknown option" not in r.stderr and "bad device list" in r.stderr, r.stderr
    assert os.path.exists(CORNELL_XML)
