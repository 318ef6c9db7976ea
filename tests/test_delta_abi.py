"""Delta lights without a GPU: gsp_delta_light, the kind constants and the two new exports against the C header (ABI still 9, no
struct changed), the Python names, the digest lists and the build files."""
import ctypes as C
import os
import subprocess

from conftest import ROOT

SYMBOLS = ("gsp_set_delta_lights", "gsp_multi_set_delta_lights")
FIELDS = ("position", "kind", "direction", "cos_cutoff", "intensity", "cos_beam", "extent", "reserved")


def test_struct_constants_and_prototypes_match_header(tmp_path):
    from gpuspectral_amd import abi

    src = tmp_path / "delta.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "gpuspectral_pt.h"\n'
        'int main(){printf("%zu %zu %d %u %u %u %zu",sizeof(gsp_delta_light),sizeof(gsp_triangle_light),GSP_ABI_VERSION,(unsigned)GSP_LIGHT_POINT,'
        "(unsigned)GSP_LIGHT_SPOT,(unsigned)GSP_LIGHT_DIRECTIONAL,sizeof(gsp_render_params));"
        + "".join('printf(" %%zu",offsetof(gsp_delta_light,%s));' % f for f in FIELDS)
        + "int (*a)(gsp_context*, const gsp_delta_light*, uint32_t) = gsp_set_delta_lights;"
        "int (*b)(gsp_multi*, const gsp_delta_light*, uint32_t) = gsp_multi_set_delta_lights; return !(a && b);}\n"
    )
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "delta.o")])  # the prototypes
    src2 = tmp_path / "delta2.c"
    src2.write_text(src.read_text().split("int (*a)")[0] + "return 0;}\n")
    exe = tmp_path / "delta2"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src2), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert vals[0] == C.sizeof(abi.DeltaLight) == 64 and vals[1] == abi.LIGHT_DT.itemsize == 64
    assert vals[2] == abi.GSP_ABI_VERSION == 9
    assert vals[3:6] == [abi.LIGHT_POINT, abi.LIGHT_SPOT, abi.LIGHT_DIRECTIONAL] == [1, 2, 3]
    assert vals[6] == C.sizeof(abi.RenderParams)  # no struct changed
    assert vals[7:] == [getattr(abi.DeltaLight, f).offset for f in FIELDS] == [0, 12, 16, 28, 32, 44, 48, 52]


def test_abi_version_still_9_and_exports_exist():
    from gpuspectral_amd import pt

    L = pt.load()
    assert L.gsp_abi_version() == 9
    for name in SYMBOLS:
        assert name in pt.EXPORTS and getattr(L, name)


def test_null_context_is_invalid():
    from gpuspectral_amd import abi, pt

    L = pt.load()
    arr = abi.delta_light_array([abi.point_light((0, 1, 0), (1, 1, 1))])
    assert L.gsp_set_delta_lights(None, arr, 1) == 1  # GSP_ERR_INVALID
    assert L.gsp_multi_set_delta_lights(None, arr, 1) == 1


def test_constructors_fill_the_record():
    from gpuspectral_amd import abi

    s = abi.spot_light((1, 2, 3), (0, -1, 0), (4, 5, 6), 0.5, 0.75)
    assert (list(s.position), s.kind, list(s.direction), s.cos_cutoff, list(s.intensity), s.cos_beam, s.extent, list(s.reserved)) == (
        [1, 2, 3], 2, [0, -1, 0], 0.5, [4, 5, 6], 0.75, 0.0, [0, 0, 0])
    d = abi.directional_light((0, -1, 0), (1, 2, 3), 7.0)
    assert d.kind == 3 and d.extent == 7.0 and list(d.intensity) == [1, 2, 3]
    assert abi.delta_light_array([]) is None and abi.delta_light_array(None) is None
    assert len(abi.delta_light_array([s, d, abi.point_light((0, 0, 0), (1, 1, 1))])) == 3


def test_header_section_digest_and_build_files_cover_the_feature():
    from gpuspectral_amd import pt

    text = open(os.path.join(ROOT, "include", "gpuspectral_pt.h")).read()
    assert "Delta lights:" in text and "NOT Mitsuba's ramp" in text and "DARK under it" in text
    for f in ("pt_render_delta.hip", "pt_deltalight.h"):
        assert f in pt.DIGEST_SOURCES
        assert f in open(os.path.join(ROOT, "gpuspectral_amd", "csrc", "Makefile")).read()
    assert "pt_render_delta.hip" in open(os.path.join(ROOT, "scripts", "build_variant.sh")).read()
    assert pt.build_info()["digest"] == pt.source_digest()


def test_valu_mix_names_the_all_false_instantiation():
    """scripts/valu_mix.py finds k_shade by a substring of the mangled name: seven template flags now, all false, and nothing behind them"""
    import importlib.util

    spec = importlib.util.spec_from_file_location("valu_mix", os.path.join(ROOT, "scripts", "valu_mix.py"))
    vm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(vm)
    assert vm.RENDER_KERNELS["k_shade"] == "k_shade" + "I" + "Lb0E" * 7
    # (csrc/Makefile ran it over the device assembly of this build: it found exactly that kernel, or the build would have failed)
    import json

    rec = json.load(open(os.path.join(ROOT, "gpuspectral_amd", "lib", "valu_mix.json")))
    assert rec["kernels"]["k_shade"]["valu_instructions_static"] > 1000
