"""Thin lens without a GPU: gsp_lens against the C header (ABI still 9), gsp_set_lens's validation and struct_size rule (the
library's own resolve_lens, compiled for the host in tests/emu/lens_emu.cpp), the CLI flags, the loader's readLens option."""
import ctypes as C
import math
import os
import subprocess

import pytest

from conftest import CORNELL_XML, ROOT
from lens_util import LensEmu


@pytest.fixture(scope="module")
def lemu():
    return LensEmu()


def test_lens_struct_matches_header(tmp_path):
    from gpuspectral_amd import abi

    src = tmp_path / "lens.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "gpuspectral_pt.h"\n'
        "int main(){printf(\"%zu %zu %zu %zu %zu %zu %d\\n\",sizeof(gsp_lens),offsetof(gsp_lens,struct_size),offsetof(gsp_lens,radius),"
        "offsetof(gsp_lens,focus_distance),offsetof(gsp_lens,blades),offsetof(gsp_lens,rotation),GSP_ABI_VERSION);"
        "int (*a)(gsp_context*, const gsp_lens*) = gsp_set_lens; int (*b)(gsp_multi*, const gsp_lens*) = gsp_multi_set_lens;"
        "int (*c)(gsp_context*, uint32_t, uint32_t, float, float, float*) = gsp_focus_distance; return !(a && b && c);}\n"
    )
    obj = tmp_path / "lens.o"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(obj)])  # the prototypes
    src2 = tmp_path / "lens2.c"
    src2.write_text(src.read_text().split("int (*a)")[0] + "return 0;}\n")
    exe = tmp_path / "lens2"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src2), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert vals[0] == C.sizeof(abi.Lens) == 20
    assert vals[1:6] == [abi.Lens.struct_size.offset, abi.Lens.radius.offset, abi.Lens.focus_distance.offset, abi.Lens.blades.offset,
                         abi.Lens.rotation.offset] == [0, 4, 8, 12, 16]
    assert vals[6] == abi.GSP_ABI_VERSION == 9
    assert abi.lens().struct_size == 20


def test_abi_version_still_9_and_exports_exist():
    from gpuspectral_amd import pt

    L = pt.load()
    assert L.gsp_abi_version() == 9
    for name in ("gsp_set_lens", "gsp_multi_set_lens", "gsp_focus_distance"):
        assert name in pt.EXPORTS and getattr(L, name)


def test_null_context_is_invalid():
    from gpuspectral_amd import abi, pt

    L = pt.load()
    l = abi.lens(0.1, 2.0)
    assert L.gsp_set_lens(None, C.byref(l)) == 1  # GSP_ERR_INVALID
    assert L.gsp_multi_set_lens(None, C.byref(l)) == 1
    out = C.c_float(7.0)
    assert L.gsp_focus_distance(None, 8, 8, 1.0, 1.0, C.byref(out)) == 1 and out.value == 7.0


@pytest.mark.parametrize("lens,word", [
    (dict(radius=-0.1, focus_distance=1.0), "radius"),
    (dict(radius=float("nan"), focus_distance=1.0), "radius"),
    (dict(radius=float("inf"), focus_distance=1.0), "radius"),
    (dict(radius=0.1, focus_distance=0.0), "focus_distance"),
    (dict(radius=0.1, focus_distance=-2.0), "focus_distance"),
    (dict(radius=0.1, focus_distance=float("nan")), "focus_distance"),
    (dict(radius=0.1, focus_distance=float("inf")), "focus_distance"),
    (dict(radius=0.1, focus_distance=1.0, blades=1), "blades"),
    (dict(radius=0.1, focus_distance=1.0, blades=2), "blades"),
    (dict(radius=0.1, focus_distance=1.0, blades=17), "blades"),
    (dict(radius=0.0, blades=2), "blades"),
    (dict(radius=0.1, focus_distance=1.0, rotation=float("nan")), "rotation"),
    (dict(radius=0.1, focus_distance=1.0, rotation=float("inf")), "rotation"),
])
def test_validation_errors(lemu, lens, word):
    out, err = lemu.resolve(lens)
    assert out is None and word in err, err


@pytest.mark.parametrize("lens", [
    dict(), dict(radius=0.0, focus_distance=0.0), dict(radius=0.0, focus_distance=-1.0, blades=5, rotation=1.0),
    dict(radius=0.1, focus_distance=3.0), dict(radius=0.1, focus_distance=3.0, blades=3), dict(radius=0.1, focus_distance=3.0, blades=16, rotation=-7.5),
])
def test_valid_lenses(lemu, lens):
    out, err = lemu.resolve(lens)
    assert err is None and out.struct_size == 20
    assert out.radius == C.c_float(lens.get("radius", 0.0)).value and out.blades == lens.get("blades", 0)


def test_null_is_the_pinhole(lemu):
    out, err = lemu.resolve(None)
    assert err is None and (out.radius, out.focus_distance, out.blades, out.rotation) == (0.0, 0.0, 0, 0.0)


def test_struct_size_rule(lemu):
    """A shorter struct means zeros for the fields it does not have; a struct_size below the field itself is refused."""
    from gpuspectral_amd import abi

    full = abi.lens(0.1, 3.0, 6, 0.5)
    full.struct_size = abi.Lens.blades.offset  # a host whose header ends behind focus_distance
    out, err = lemu.resolve(full)
    assert err is None and (out.radius, out.focus_distance, out.blades, out.rotation) == (C.c_float(0.1).value, 3.0, 0, 0.0)
    full.struct_size = abi.Lens.focus_distance.offset  # radius alone: radius > 0 without a focus distance
    out, err = lemu.resolve(full)
    assert out is None and "focus_distance" in err
    full.struct_size = abi.Lens.radius.offset  # struct_size alone: the pinhole
    out, err = lemu.resolve(full)
    assert err is None and out.radius == 0.0
    full.struct_size = 400  # a newer host: the fields this library knows
    out, err = lemu.resolve(full)
    assert err is None and (out.blades, out.rotation) == (6, 0.5) and out.struct_size == 20
    for bad in (0, 3):
        full.struct_size = bad
        out, err = lemu.resolve(full)
        assert out is None and "struct_size" in err


def test_resolved_constants(lemu, cornell):
    """s = focus_distance / zplane in float32, formed once; a pinhole leaves every lens constant 0 whatever the other fields."""
    import numpy as np

    W, H = 96, 64
    c = lemu.consts(cornell, W, H, dict(radius=0.05, focus_distance=4.5, blades=7, rotation=0.25))
    zplane = np.float32(max(W, H) / 2.0) / np.float32(math.tan(np.float32(cornell.fov) / np.float32(2.0)))
    assert abs(float(c["zplane"]) - float(zplane)) <= float(np.spacing(zplane))  # (tanf of the C library against numpy's)
    assert c["s"] == np.float32(4.5) / c["zplane"]
    assert (c["radius"], c["focus"], c["blades"], c["rotation"]) == (np.float32(0.05), 4.5, 7.0, 0.25)
    z = lemu.consts(cornell, W, H, dict(radius=0.0, focus_distance=4.5, blades=7, rotation=0.25))
    assert not any(float(z[k]) for k in ("radius", "focus", "s", "blades", "rotation"))


# ---- CLI ------------------------------------------------------------------------------------------------------------------
def _cli():
    lib = os.path.join(ROOT, "gpuspectral_amd", "lib")
    exe = os.path.join(lib, "gsp_render")
    assert os.path.exists(exe), "host CLI not built (make -C gpuspectral_amd/host)"
    return exe, dict(os.environ, LD_LIBRARY_PATH=lib + ":" + os.environ.get("LD_LIBRARY_PATH", ""))


def test_cli_usage_names_the_lens_flags():
    exe, env = _cli()
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    for tok in ("--aperture R", "--focus-distance D", "--focus-pixel X,Y", "--blades N[:rot_deg]", "--scene-lens"):
        assert tok in r.stderr, tok
    # every token the usage line had before is still there
    for tok in ("--dormant-features", "--builtin-shapes", "--no-nee", "--memory-share F", "--pool-paths N", "--adaptive T",
                "--adaptive-min N", "--adaptive-step N", "--filter none|box|tent[:r]|gaussian[:s]", "--scene-filter", "scene.xml out.pfm",
                "[width height spp [device | d0,d1,...]]"):
        assert tok in r.stderr, tok


@pytest.mark.parametrize("flags", [
    ["--aperture", "0.1", "--focus-distance", "4.5"], ["--aperture", "0.1", "--focus-pixel", "12,20.5"], ["--aperture", "0", "--scene-lens"],
    ["--aperture", "0.1", "--scene-lens"], ["--aperture", "0.1", "--focus-distance", "3", "--blades", "6"],
    ["--aperture", "0.1", "--focus-distance", "3", "--blades", "5:36"], ["--blades", "0"], ["--scene-lens"], ["--focus-distance", "2"],
])
def test_cli_parses_lens_flags(tmp_path, flags):
    """A bad device list is reported AFTER the options, so reaching it means the options were accepted."""
    exe, env = _cli()
    r = subprocess.run([exe] + flags + [str(tmp_path / "none.xml"), str(tmp_path / "x.pfm"), "8", "8", "1", "abc"], env=env, capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 2 and "unknown option" not in r.stderr and "gsp_render: bad " + "device list" in r.stderr, r.stderr
    assert r.stderr.count("gsp_render: bad") == 1, r.stderr


@pytest.mark.parametrize("flags,word", [
    (["--aperture", "-1"], "bad aperture"), (["--aperture", "x"], "bad aperture"), (["--aperture", "nan"], "bad aperture"),
    (["--aperture", ""], "bad aperture"), (["--focus-distance", "0"], "bad focus distance"), (["--focus-distance", "-3"], "bad focus distance"),
    (["--focus-distance", "inf"], "bad focus distance"), (["--focus-pixel", "12"], "bad focus pixel"), (["--focus-pixel", "a,b"], "bad focus pixel"),
    (["--focus-pixel", "3,"], "bad focus pixel"), (["--blades", "2"], "bad blades"), (["--blades", "17"], "bad blades"),
    (["--blades", "six"], "bad blades"), (["--blades", "6:"], "bad blades"), (["--blades", "6:x"], "bad blades"),
    (["--aperture", "0.1"], "--aperture needs"),
])
def test_cli_rejects_bad_lens_flags(tmp_path, flags, word):
    exe, env = _cli()
    r = subprocess.run([exe] + flags + [str(tmp_path / "none.xml"), str(tmp_path / "x.pfm"), "8", "8", "1", "abc"], env=env, capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 2 and word in r.stderr and "bad device list" not in r.stderr, r.stderr


# ---- loader ---------------------------------------------------------------------------------------------------------------
def _scene_xml(tmp_path, sensor_type, props):
    """The Cornell scene with another sensor plugin and extra sensor properties (a small XML written here; meshes linked)."""
    text = open(CORNELL_XML).read()
    assert '<sensor type="perspective" >' in text
    d = tmp_path / "scene"
    d.mkdir()
    for f in os.listdir(os.path.dirname(CORNELL_XML)):
        if f != "scene.xml":
            os.symlink(os.path.join(os.path.dirname(CORNELL_XML), f), str(d / f))
    extra = "".join('\n\t\t<float name="%s" value="%s" />' % kv for kv in props)
    (d / "scene.xml").write_text(text.replace('<sensor type="perspective" >', '<sensor type="%s" >%s' % (sensor_type, extra)))
    return str(d / "scene.xml")


def _scene_bytes(s):
    a = s.arrays()
    return b"".join([a.positions.tobytes(), a.normals.tobytes(), a.instances.tobytes(), a.lights.tobytes(), a.to_world.tobytes()])


@pytest.mark.parametrize("names", [("aperture_radius", "focus_distance"), ("apertureRadius", "focusDistance")])
def test_loader_reads_thinlens(tmp_path, names):
    from gpuspectral_amd import host

    path = _scene_xml(tmp_path, "thinlens", [(names[0], "0.125"), (names[1], "5.5")])
    with_l = host.Scene(path, read_lens=True)
    assert with_l.lens == (0.125, 5.5, 0, 0.0)
    without = host.Scene(path)
    assert without.lens == (0.0, 0.0, 0, 0.0)  # default: the sensor plugin is ignored, as in the reference
    # nothing else changes: geometry, lights, camera and warnings are those of the perspective scene
    plain = host.Scene(CORNELL_XML)
    assert _scene_bytes(with_l) == _scene_bytes(without) == _scene_bytes(plain) and with_l.warnings == without.warnings == plain.warnings


def test_loader_perspective_sensor_has_no_lens(tmp_path):
    from gpuspectral_amd import host

    assert host.Scene(CORNELL_XML, read_lens=True).lens == (0.0, 0.0, 0, 0.0)
    path = _scene_xml(tmp_path, "perspective", [("aperture_radius", "0.125"), ("focus_distance", "5.5")])
    assert host.Scene(path, read_lens=True).lens == (0.0, 0.0, 0, 0.0)  # only a thinlens sensor has an aperture


@pytest.mark.parametrize("props,word", [
    ([("aperture_radius", "-0.1"), ("focus_distance", "5")], "aperture_radius"),
    ([("aperture_radius", "0.1")], "focus_distance"),
    ([("aperture_radius", "0.1"), ("focus_distance", "0")], "focus_distance"),
    ([("aperture_radius", "0.1"), ("focus_distance", "-4")], "focus_distance"),
])
def test_loader_refuses_invalid_lens(tmp_path, props, word):
    from gpuspectral_amd import host

    path = _scene_xml(tmp_path, "thinlens", props)
    with pytest.raises(host.GspError) as e:
        host.Scene(path, read_lens=True)
    assert word in str(e.value)
    assert host.Scene(path).lens == (0.0, 0.0, 0, 0.0)  # without the option the values are not even looked at


def test_scene_set_lens_roundtrip():
    from gpuspectral_amd import host

    s = host.Scene(CORNELL_XML)
    s.set_lens(0.25, 3.0, 6, 0.5)
    assert s.lens == (0.25, 3.0, 6, 0.5)
