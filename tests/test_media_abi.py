"""Interior media without a GPU: gsp_medium, the handle macro and the two new exports against the C header (ABI still 9, no
struct changed)."""
import ctypes as C
import os
import subprocess

from conftest import ROOT

HANDLES = [(0, 0, 0), (1, 3, 1), (7, 0xFFFF, 4095), (1, 0, 4095), (5, 17, 2048), (2, 65535, 1)]


def test_medium_struct_macro_and_prototypes_match_header(tmp_path):
    from gpuspectral_amd import abi

    prints = "".join('printf("%%u\\n", (unsigned)GSP_BSDF_HANDLE_MEDIUM(%d, %d, %d));' % h for h in HANDLES)
    src = tmp_path / "media.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "gpuspectral_pt.h"\n'
        'int main(){printf("%zu %zu %zu %zu %d %u\\n",sizeof(gsp_medium),offsetof(gsp_medium,sigma_a),offsetof(gsp_medium,reserved),'
        "sizeof(gsp_instance),GSP_ABI_VERSION,(unsigned)GSP_MAX_MEDIA);" + prints +
        "int (*a)(gsp_context*, const gsp_medium*, uint32_t) = gsp_set_media; int (*b)(gsp_multi*, const gsp_medium*, uint32_t) = gsp_multi_set_media;"
        " return !(a && b);}\n"
    )
    obj = tmp_path / "media.o"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(obj)])  # the prototypes
    src2 = tmp_path / "media2.c"
    src2.write_text(src.read_text().split("int (*a)")[0] + "return 0;}\n")
    exe = tmp_path / "media2"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src2), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().split("\n")
    vals = [int(x) for x in lines[0].split()]
    assert vals[0] == C.sizeof(abi.Medium) == 16
    assert vals[1:3] == [abi.Medium.sigma_a.offset, abi.Medium.reserved.offset] == [0, 12]
    assert vals[3] == abi.INSTANCE_DT.itemsize == 92
    assert vals[4] == abi.GSP_ABI_VERSION == 9
    assert vals[5] == abi.MAX_MEDIA == 4095
    got = [int(x) for x in lines[1:1 + len(HANDLES)]]
    assert got == [abi.bsdf_handle(*h) for h in HANDLES]


def test_handle_bit_layout():
    from gpuspectral_amd import abi

    for t, i, k in HANDLES:
        h = abi.bsdf_handle(t, i, k)
        assert h < (1 << 31)  # bit 31 of the baked material word is `twofaced`
        assert ((h >> 16) & 7, h & 0xFFFF, (h >> 19) & 0xFFF) == (t, i, k)
        assert abi.bsdf_handle(t, i) == h & 0x0007FFFF  # without a medium: the handle of every scene so far
    assert abi.bsdf_handle(1, 2, 3) == (1 << 16) | 2 | (3 << 19)


def test_abi_version_still_9_and_exports_exist():
    from gpuspectral_amd import pt

    L = pt.load()
    assert L.gsp_abi_version() == 9
    for name in ("gsp_set_media", "gsp_multi_set_media"):
        assert name in pt.EXPORTS and getattr(L, name)


def test_null_context_is_invalid():
    from gpuspectral_amd import abi, pt

    L = pt.load()
    arr = abi.media_array([(1.0, 2.0, 3.0)])
    assert L.gsp_set_media(None, arr, 1) == 1  # GSP_ERR_INVALID
    assert L.gsp_multi_set_media(None, arr, 1) == 1


def test_media_array():
    from gpuspectral_amd import abi

    assert abi.media_array(None) is None and abi.media_array([]) is None
    arr = abi.media_array([(0.5, 0.2, 0.4), (250, 1000, 1000)])
    assert len(arr) == 2 and list(arr[1].sigma_a) == [250.0, 1000.0, 1000.0] and arr[0].reserved == 0.0
