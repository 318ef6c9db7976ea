"""Light selection without a GPU: gsp_light_pick, the mode constants and the three new exports against the C header (ABI still 9,
no struct changed), the Python names, the host library's entry points and the CLI flag."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT

SYMBOLS = ("gsp_set_light_sampling", "gsp_download_light_pick", "gsp_multi_set_light_sampling")


def test_struct_constants_and_prototypes_match_header(tmp_path):
    from gpuspectral_amd import abi

    src = tmp_path / "lights.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "gpuspectral_pt.h"\n'
        'int main(){printf("%zu %zu %zu %zu %zu %d %u %u %zu %zu\\n",sizeof(gsp_light_pick),offsetof(gsp_light_pick,threshold),offsetof(gsp_light_pick,alias),'
        "offsetof(gsp_light_pick,pmf_self),offsetof(gsp_light_pick,pmf_alias),GSP_ABI_VERSION,(unsigned)GSP_LIGHTS_UNIFORM,(unsigned)GSP_LIGHTS_POWER,"
        "sizeof(gsp_triangle_light),sizeof(gsp_render_params));"
        "int (*a)(gsp_context*, uint32_t) = gsp_set_light_sampling; int (*b)(gsp_context*, gsp_light_pick*, uint32_t, uint32_t*) = gsp_download_light_pick;"
        "int (*c)(gsp_multi*, uint32_t) = gsp_multi_set_light_sampling; return !(a && b && c);}\n"
    )
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "lights.o")])  # the prototypes
    src2 = tmp_path / "lights2.c"
    src2.write_text(src.read_text().split("int (*a)")[0] + "return 0;}\n")
    exe = tmp_path / "lights2"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src2), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert vals[0] == abi.LIGHT_PICK_DT.itemsize == 16
    assert vals[1:5] == [abi.LIGHT_PICK_DT.fields[k][1] for k in ("threshold", "alias", "pmf_self", "pmf_alias")] == [0, 4, 8, 12]
    assert vals[5] == abi.GSP_ABI_VERSION == 9
    assert vals[6:8] == [abi.LIGHTS_UNIFORM, abi.LIGHTS_POWER] == [0, 1]
    assert vals[8] == abi.LIGHT_DT.itemsize == 64  # (a multiple of 16: the pick table behind the records starts on a 16-byte boundary)
    assert vals[9] == C.sizeof(abi.RenderParams)  # no struct changed


def test_abi_version_still_9_and_exports_exist():
    from gpuspectral_amd import pt

    L = pt.load()
    assert L.gsp_abi_version() == 9
    for name in SYMBOLS:
        assert name in pt.EXPORTS and getattr(L, name)


def test_null_context_is_invalid():
    from gpuspectral_amd import pt

    L = pt.load()
    n = C.c_uint32(7)
    assert L.gsp_set_light_sampling(None, 1) == 1  # GSP_ERR_INVALID
    assert L.gsp_download_light_pick(None, None, 0, C.byref(n)) == 1
    assert L.gsp_multi_set_light_sampling(None, 1) == 1


def test_mode_names():
    from gpuspectral_amd import abi

    assert abi.light_sampling_mode("uniform") == 0 and abi.light_sampling_mode("power") == 1 and abi.light_sampling_mode(1) == 1
    assert abi.light_sampling_mode(7) == 7  # (a number goes through: the library refuses it)
    with pytest.raises(ValueError):
        abi.light_sampling_mode("brightest")


def test_header_section_and_digest_cover_the_feature():
    with open(os.path.join(ROOT, "include", "gpuspectral_pt.h")) as fh:
        text = fh.read()
    top = text[:text.index("status codes")]
    for name in SYMBOLS:
        assert name in top, name  # the ABI-9 list
    sec = text[text.index(" * Light selection:"):text.index("int gsp_set_light_sampling")]
    for phrase in ("CONTEXT STATE", "Vose", "ascending", "round(s'_j * 2^32)", "0xffffffff", "(uint64)r * num_lights", "EXPECTED", "2^-33 / n", "textbook"):
        assert phrase in sec, phrase
    with open(os.path.join(ROOT, "gpuspectral_amd", "csrc", "Makefile")) as fh:
        assert "pt_lightpick.h" in fh.read()  # the digest of gsp_build_info covers the new header
    from gpuspectral_amd import pt

    assert "pt_lightpick.h" in pt.DIGEST_SOURCES


def test_python_layers_name_the_feature():
    from gpuspectral_amd import host, pt

    for cls in (pt.Context, pt.MultiContext):
        assert callable(getattr(cls, "set_light_sampling"))
    assert callable(pt.Context.download_light_pick)
    assert callable(host.PathTracer.set_light_sampling) and callable(host.PathTracer.download_light_pick)


# ---- the C++ host ------------------------------------------------------------------------------------------------------------------
def test_host_library_exports_the_setter():
    from gpuspectral_amd import host

    L = host.load()
    assert L.gsph_pathtracer_set_light_sampling and L.gsph_pathtracer_download_light_pick


def test_cxx_host_compiles_against_the_setters(tmp_path):
    """PathTracer / MultiGpuPathTracer::setLightSampling as a C++ caller sees them; the integration header (which builds only inside
    the viewer's tree) names its setter."""
    src = tmp_path / "host.cpp"
    src.write_text(
        '#include "PathTracer.h"\nusing namespace GPUSpectral;\n'
        "void (PathTracer::*a)(uint32_t) = &PathTracer::setLightSampling;\n"
        "std::vector<gsp_light_pick> (PathTracer::*b)() = &PathTracer::downloadLightPick;\n"
        "void (MultiGpuPathTracer::*c)(uint32_t) = &MultiGpuPathTracer::setLightSampling;\n"
        "int main() { return !(a && b && c); }\n")
    host = os.path.join(ROOT, "gpuspectral_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", host, "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "host.o")])
    with open(os.path.join(host, "integration", "PathTracerHip.h")) as fh:
        assert "void setLightSampling(uint32_t mode) { check(gsp_set_light_sampling(ctx, mode)); }" in fh.read()


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
    assert r.returncode == 2 and "[--light-sampling uniform|power]" in r.stderr


@pytest.mark.parametrize("value", ["uniform", "power"])
def test_cli_parses_the_flag(tmp_path, value):
    """A bad device list is reported AFTER the options, so reaching it means the option was accepted."""
    r = _run(tmp_path, ["--light-sampling", value])
    assert r.returncode == 2 and "unknown option" not in r.stderr and "gsp_render: bad device list" in r.stderr, r.stderr


def test_cli_rejects_an_unknown_mode(tmp_path):
    r = _run(tmp_path, ["--light-sampling", "brightest"])
    assert r.returncode == 2 and "--light-sampling: uniform or power" in r.stderr and "bad device list" not in r.stderr, r.stderr
