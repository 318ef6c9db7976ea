"""The estimator mode without a GPU: the two constants and the two new exports against the C header (ABI still 9, no struct
changed), the header's section, the layout rule of the table image, the Python names, the host library's entry point and the CLI
flag."""
import ctypes as C
import os
import subprocess

import pytest

import estimator_util as eu
from conftest import ROOT

SYMBOLS = ("gsp_set_estimator", "gsp_multi_set_estimator")


def test_constants_and_prototypes_match_header(tmp_path):
    from gpuspectral_amd import abi

    src = tmp_path / "est.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "gpuspectral_pt.h"\n'
        'int main(){printf("%d %u %u %zu %zu %zu\\n",GSP_ABI_VERSION,(unsigned)GSP_ESTIMATOR_REFERENCE,(unsigned)GSP_ESTIMATOR_TEXTBOOK,'
        "sizeof(gsp_render_params),sizeof(gsp_light_pick),sizeof(gsp_triangle_light));"
        "int (*a)(gsp_context*, uint32_t) = gsp_set_estimator; int (*b)(gsp_multi*, uint32_t) = gsp_multi_set_estimator; return !(a && b);}\n")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "est.o")])  # the prototypes
    src2 = tmp_path / "est2.c"
    src2.write_text(src.read_text().split("int (*a)")[0] + "return 0;}\n")
    exe = tmp_path / "est2"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src2), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert vals[0] == abi.GSP_ABI_VERSION == 9
    assert vals[1:3] == [abi.ESTIMATOR_REFERENCE, abi.ESTIMATOR_TEXTBOOK] == [0, 1]
    assert vals[3] == C.sizeof(abi.RenderParams) and vals[4] == abi.LIGHT_PICK_DT.itemsize == 16 and vals[5] == abi.LIGHT_DT.itemsize  # no struct changed


def test_abi_version_still_9_and_exports_exist():
    from gpuspectral_amd import pt

    L = pt.load()
    assert L.gsp_abi_version() == 9
    for name in SYMBOLS:
        assert name in pt.EXPORTS and getattr(L, name)


def test_null_context_is_invalid():
    from gpuspectral_amd import pt

    L = pt.load()
    assert L.gsp_set_estimator(None, 1) == 1  # GSP_ERR_INVALID
    assert L.gsp_multi_set_estimator(None, 1) == 1


def test_mode_names():
    from gpuspectral_amd import abi

    assert abi.estimator_mode("reference") == 0 and abi.estimator_mode("textbook") == 1 and abi.estimator_mode(1) == 1
    assert abi.estimator_mode(7) == 7  # (a number goes through: the library refuses it)
    with pytest.raises(ValueError):
        abi.estimator_mode("unbiased")


def test_header_section_holds_the_rule_and_the_digest_covers_the_new_unit():
    with open(os.path.join(ROOT, "include", "gpuspectral_pt.h")) as fh:
        text = fh.read()
    top = text[:text.index("status codes")]
    for name in SYMBOLS:
        assert name in top, name  # the ABI-9 list
    sec = text[text.index(" * Estimator:"):text.index("int gsp_set_estimator")]
    for phrase in ("CONTEXT STATE", "survives", "GSP_ERR_INVALID", "power_heuristic(lightPdf, lb.pdf)", "max(.., 0.01)", "countEmitted == 0 and wasDelta == 0",
                   "0.5 * |length(cross(v2 - v0, v1 - v0))|", "((t * t) / (|dot(-rayDir, N)| * A)) * p_sel", "isLight ? power_heuristic(lastPdf, hitPdf) : 1",
                   "1.0f / (float)num_lights", "(0.2126f * r + 0.7152f * g) + 0.0722f * b", "w_hit * inv_sum_w", "trailing 16-byte", "(1 + d_i) / (n * 2^32)",
                   "EVERY EMISSIVE TRIANGLE IS ONE LIGHT RECORD", "carries lastPdf", "gsp_render_params.clamp", "#define GSP_ESTIMATOR_REFERENCE 0u",
                   "#define GSP_ESTIMATOR_TEXTBOOK 1u"):
        assert phrase in sec, phrase
    with open(os.path.join(ROOT, "gpuspectral_amd", "csrc", "Makefile")) as fh:
        assert "pt_render_textbook.hip" in fh.read()  # the digest of gsp_build_info covers the unit of the <EST> kernels
    from gpuspectral_amd import pt

    assert "pt_render_textbook.hip" in pt.DIGEST_SOURCES


@pytest.mark.parametrize("n", [0, 1, 3, 130])
def test_trailing_record_exists_only_with_both_modes_on(n):
    """The layout rule pack_tables applies (pt_lightpick.h light_pick_table_bytes / light_pick_tail_bytes): the bytes of the light
    records and what follows them.  Every combination but power + textbook is what it was before the estimator mode existed: nothing
    behind the records under the uniform pick, 16 bytes per light under the power pick."""
    emu = eu.EstimatorEmu()
    rec = 64 * n
    assert emu.light_image_bytes(n, eu.UNIFORM, eu.REFERENCE) == rec
    assert emu.light_image_bytes(n, eu.UNIFORM, eu.TEXTBOOK) == rec
    assert emu.light_image_bytes(n, eu.POWER, eu.REFERENCE) == rec + 16 * n
    assert emu.light_image_bytes(n, eu.POWER, eu.TEXTBOOK) == rec + 16 * n + (16 if n else 0)


def test_python_layers_name_the_feature():
    from gpuspectral_amd import host, pt

    for cls in (pt.Context, pt.MultiContext):
        assert callable(getattr(cls, "set_estimator"))
    assert callable(host.PathTracer.set_estimator)


# ---- the C++ host ------------------------------------------------------------------------------------------------------------------
def test_host_library_exports_the_setter():
    from gpuspectral_amd import host

    assert host.load().gsph_pathtracer_set_estimator


def test_cxx_host_compiles_against_the_setters(tmp_path):
    src = tmp_path / "host.cpp"
    src.write_text(
        '#include "PathTracer.h"\nusing namespace GPUSpectral;\n'
        "void (PathTracer::*a)(uint32_t) = &PathTracer::setEstimator;\n"
        "void (MultiGpuPathTracer::*b)(uint32_t) = &MultiGpuPathTracer::setEstimator;\n"
        "int main() { return !(a && b); }\n")
    host = os.path.join(ROOT, "gpuspectral_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", host, "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "host.o")])
    with open(os.path.join(host, "integration", "PathTracerHip.h")) as fh:
        assert "void setEstimator(uint32_t mode) { check(gsp_set_estimator(ctx, mode)); }" in fh.read()


# ---- CLI -----------------------------------------------------------------------------------------------------------------------------
def _cli():
    lib = os.path.join(ROOT, "gpuspectral_amd", "lib")
    exe = os.path.join(lib, "gsp_render")
    assert os.path.exists(exe), "host CLI not built (make -C gpuspectral_amd/host)"
    return exe, dict(os.environ, LD_LIBRARY_PATH=lib + ":" + os.environ.get("LD_LIBRARY_PATH", ""))


def _run(tmp_path, flags, devices="abc"):
    exe, env = _cli()
    return subprocess.run([exe] + flags + [str(tmp_path / "none.xml"), str(tmp_path / "x.pfm"), "8", "8", "1", devices], env=env, capture_output=True,
                          text=True, timeout=60)


def test_cli_usage_names_the_flag():
    exe, env = _cli()
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "[--estimator reference|textbook]" in r.stderr


@pytest.mark.parametrize("value", ["reference", "textbook"])
def test_cli_parses_the_flag(tmp_path, value):
    """A bad device list is reported AFTER the options, so reaching it means the option was accepted."""
    r = _run(tmp_path, ["--estimator", value])
    assert r.returncode == 2 and "unknown option" not in r.stderr and "gsp_render: bad device list" in r.stderr, r.stderr


def test_cli_rejects_an_unknown_mode(tmp_path):
    r = _run(tmp_path, ["--estimator", "unbiased"])
    assert r.returncode == 2 and "--estimator: reference or textbook" in r.stderr and "bad device list" not in r.stderr, r.stderr
