"""The light grid's interface: gsp_light_grid and the three new exports against the C header (ABI still 9, no struct changed), the
Python names, the digest lists and the build files -- without a GPU; and, on one, what the setter accepts and refuses: validation,
the two prerequisites in both call orders, the exclusion with environment sampling in both call orders, the cap, and the round trip
of gsp_get_light_grid."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = ("gsp_set_light_grid", "gsp_get_light_grid", "gsp_multi_set_light_grid")
FIELDS = ("enabled", "resolution", "reserved")
GSP_ERR_INVALID, GSP_ERR_NOMEM = 1, 3


def test_struct_and_prototypes_match_header(tmp_path):
    from gpuspectral_amd import abi

    src = tmp_path / "grid.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "gpuspectral_pt.h"\n'
        'int main(){printf("%zu %d %zu %zu %zu",sizeof(gsp_light_grid),GSP_ABI_VERSION,sizeof(gsp_render_params),sizeof(gsp_delta_light),sizeof(gsp_envmap_sampling));'
        + "".join('printf(" %%zu",offsetof(gsp_light_grid,%s));' % f for f in FIELDS)
        + "int (*a)(gsp_context*, const gsp_light_grid*) = gsp_set_light_grid;"
        "int (*b)(gsp_context*, gsp_light_grid*, float*) = gsp_get_light_grid;"
        "int (*c)(gsp_multi*, const gsp_light_grid*) = gsp_multi_set_light_grid; return !(a && b && c);}\n"
    )
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "grid.o")])  # the prototypes
    src2 = tmp_path / "grid2.c"
    src2.write_text(src.read_text().split("int (*a)")[0] + "return 0;}\n")
    exe = tmp_path / "grid2"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src2), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert vals[0] == C.sizeof(abi.LightGrid) == 32
    assert vals[1] == abi.GSP_ABI_VERSION == 9
    assert vals[2] == C.sizeof(abi.RenderParams) and vals[3] == C.sizeof(abi.DeltaLight) and vals[4] == C.sizeof(abi.EnvmapSampling)  # no struct changed
    assert vals[5:] == [getattr(abi.LightGrid, f).offset for f in FIELDS] == [0, 4, 16]


def test_abi_version_still_9_and_exports_exist():
    from gpuspectral_amd import pt

    L = pt.load()
    assert L.gsp_abi_version() == 9
    for name in SYMBOLS:
        assert name in pt.EXPORTS and getattr(L, name)
    assert hasattr(pt.Context, "set_light_grid") and hasattr(pt.Context, "light_grid") and hasattr(pt.MultiContext, "set_light_grid")


def test_null_context_is_invalid():
    from gpuspectral_amd import abi, pt

    L = pt.load()
    s = abi.light_grid()
    assert L.gsp_set_light_grid(None, C.byref(s)) == GSP_ERR_INVALID
    assert L.gsp_get_light_grid(None, C.byref(s), None) == GSP_ERR_INVALID
    assert L.gsp_multi_set_light_grid(None, C.byref(s)) == GSP_ERR_INVALID


def test_mode_2_of_light_sampling_is_still_unknown():
    """The grid is a switch of its own, not a third value of gsp_set_light_sampling."""
    from gpuspectral_amd import abi

    assert set(abi.LIGHT_SAMPLING_NAMES.values()) == {abi.LIGHTS_UNIFORM, abi.LIGHTS_POWER} == {0, 1}


def test_header_section_digest_and_build_files_cover_the_feature():
    from gpuspectral_amd import pt

    text = open(os.path.join(ROOT, "include", "gpuspectral_pt.h")).read()
    assert "Light grid:" in text and "WHICH POINT NAMES THE CELL" in text and "a p_sel per cell is a follow-up" in text
    for f in ("pt_render_lightgrid.hip", "pt_lightgrid.h"):
        assert f in pt.DIGEST_SOURCES
        assert f in open(os.path.join(ROOT, "gpuspectral_amd", "csrc", "Makefile")).read()
    assert "pt_render_lightgrid.hip" in open(os.path.join(ROOT, "scripts", "build_variant.sh")).read()
    assert pt.build_info()["digest"] == pt.source_digest()
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "lightgrid.mk" in entry and "set_light_grid" in entry


# ---- on a device: what the setter accepts and refuses ------------------------------------------------------------------------------------
def _ctx(power=True, textbook=True):
    import gpuspectral_amd as g

    ctx = g.Context(0)
    if power:
        ctx.set_light_sampling("power")
    if textbook:
        ctx.set_estimator("textbook")
    return ctx


def _raw(ctx, enabled, resolution=(0, 0, 0), reserved=(0, 0, 0, 0)):
    from gpuspectral_amd import abi, pt

    s = abi.LightGrid(enabled, (C.c_uint32 * 3)(*resolution), (C.c_uint32 * 4)(*reserved))
    return pt.load().gsp_set_light_grid(ctx._h, C.byref(s))


def _error_of(fn):
    with pytest.raises(RuntimeError) as e:
        fn()
    return str(e.value)


@pytest.mark.gpu
def test_validation_errors_leave_the_state_unchanged():
    import lights_util as lu

    sc = lu.room_scene(3)
    with _ctx() as ctx:
        ctx.upload_scene(sc)
        ctx.set_light_grid(True, (4, 2, 4))
        before = ctx.light_grid()
        assert before[0] and before[1] == (4, 2, 4)
        assert _raw(ctx, 1, (0, 0, 0), (0, 0, 0, 7)) == GSP_ERR_INVALID      # reserved
        assert _raw(ctx, 1, (65, 1, 1)) == GSP_ERR_INVALID                   # above 64
        assert _raw(ctx, 1, (4, 0, 4)) == GSP_ERR_INVALID                    # mixed zero / non-zero
        assert _raw(ctx, 1, (0, 3, 0)) == GSP_ERR_INVALID
        assert ctx.light_grid() == before
        assert "reserved" in _error_of(lambda: ctx._check(_raw(ctx, 1, (0, 0, 0), (1, 0, 0, 0)), "gsp_set_light_grid"))
        assert _raw(ctx, 0, (99, 0, 7), (5, 5, 5, 5)) == 0                   # enabled == 0: nothing else is read
        assert ctx.light_grid() == (False, (0, 0, 0), ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)))


@pytest.mark.gpu
def test_prerequisites_are_reported_in_both_call_orders():
    """As gsp_set_envmap_sampling reports its own: the setter first is refused and names the call that must come first; leaving a
    prerequisite with the grid on is refused by THAT call; off again, both modes are free."""
    with _ctx(power=False, textbook=True) as ctx:
        msg = _error_of(lambda: ctx.set_light_grid(True))
        assert "GSP_LIGHTS_POWER" in msg and "gsp_set_light_sampling first" in msg
    with _ctx(power=True, textbook=False) as ctx:
        msg = _error_of(lambda: ctx.set_light_grid(True))
        assert "GSP_ESTIMATOR_TEXTBOOK" in msg and "gsp_set_estimator first" in msg
    with _ctx() as ctx:
        ctx.set_light_grid(True)
        assert "light grid is on" in _error_of(lambda: ctx.set_estimator("reference"))
        assert "light grid is on" in _error_of(lambda: ctx.set_light_sampling("uniform"))
        ctx.set_estimator("textbook")      # (the state is unchanged: both still hold, the grid still on)
        ctx.set_light_sampling("power")
        ctx.set_light_grid(False)
        ctx.set_estimator("reference")     # off: both modes are free again
        ctx.set_light_sampling("uniform")


def ctx_error(ctx):
    from gpuspectral_amd import pt

    return pt.load().gsp_last_error(ctx._h).decode()


@pytest.mark.gpu
def test_environment_sampling_excludes_the_grid_in_both_call_orders():
    with _ctx() as ctx:
        ctx.set_envmap_sampling(True, 2.0)
        msg = _error_of(lambda: ctx.set_light_grid(True))
        assert "envmap sampling is on" in msg and "per cell" in msg
        ctx.set_envmap_sampling(False)
        ctx.set_light_grid(True)
        msg = _error_of(lambda: ctx.set_envmap_sampling(True, 2.0))
        assert "light grid is on" in msg and "per cell" in msg
        ctx.set_light_grid(False)
        ctx.set_envmap_sampling(True, 2.0)


@pytest.mark.gpu
def test_get_light_grid_round_trip_and_the_cap():
    import lightgrid_util as gu
    import lights_util as lu

    emu = gu.GridEmu()
    sc3, sc40 = lu.room_scene(3), lu.room_scene(40)
    b3 = emu.scene(sc3).bounds()
    with _ctx() as ctx:
        assert ctx.light_grid()[0] is False            # no scene, no switch
        ctx.set_light_grid(True)                       # auto, before the scene: nothing resident yet
        assert ctx.light_grid()[0] is False
        ctx.upload_scene(sc3)
        on, res, (lo, hi) = ctx.light_grid()
        assert on and res == emu.resolve(b3, 3) and np.array_equal(np.float32(lo + hi), b3)
        ctx.set_light_grid(True, (8, 2, 8))            # another resolution under the resident scene: repacked
        assert ctx.light_grid()[:2] == (True, (8, 2, 8))
        ctx.update_tables(sc3)                         # context state: it survives gsp_update_tables ...
        assert ctx.light_grid()[:2] == (True, (8, 2, 8))
        ctx.upload_scene(sc40)                         # ... and gsp_upload_scene
        assert ctx.light_grid()[:2] == (True, (8, 2, 8))
        # 64^3 cells * 40 lights is beyond 2^20 entries: GSP_ERR_NOMEM from the setter, the resident grid stays
        assert _raw(ctx, 1, (64, 64, 64)) == GSP_ERR_NOMEM and "2^20" in ctx_error(ctx)
        assert ctx.light_grid()[:2] == (True, (8, 2, 8))
        ctx.set_light_grid(False)
        assert ctx.light_grid()[0] is False
        # ... and from gsp_upload_scene when the switch came first
        ctx.upload_scene(sc3)
        ctx.set_light_grid(True, (64, 64, 64))         # 2^18 * 3 fits
        assert ctx.light_grid()[:2] == (True, (64, 64, 64))
        with pytest.raises(RuntimeError, match="2\\^20"):
            ctx.upload_scene(sc40)


@pytest.mark.gpu
def test_multi_context_forwards_the_switch():
    import lightgrid_util as gu
    import lights_util as lu
    from gpuspectral_amd import pt

    sc = lu.room_scene(3)
    ref = gu.GridEmu().scene(sc).render(16, 12, 2, grid=(4, 2, 4))[0]
    with pt.MultiContext([0, 0]) as m:
        m.set_light_sampling("power")
        m.set_estimator("textbook")
        m.set_light_grid(True, (4, 2, 4))
        m.upload_scene(sc)
        m.frame_begin(16, 12)
        m.render(spp=2)
        m.gather()
        img = m.download().reshape(-1, 4)
    assert gu.same(img, ref)


# ---- C++ host and CLI, without a device ------------------------------------------------------------------------------------------------
def test_host_classes_carry_the_option(tmp_path):
    src = tmp_path / "host.cpp"
    src.write_text(
        '#include "PathTracer.h"\nusing namespace GPUSpectral;\n'
        "void (PathTracer::*a)(bool, uint32_t, uint32_t, uint32_t) = &PathTracer::setLightGrid;\n"
        "void (MultiGpuPathTracer::*b)(bool, uint32_t, uint32_t, uint32_t) = &MultiGpuPathTracer::setLightGrid;\n"
        "int main() { return !(a && b); }\n")
    host = os.path.join(ROOT, "gpuspectral_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", host, "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "host.o")])
    with open(os.path.join(host, "integration", "PathTracerHip.h")) as fh:
        assert "void setLightGrid(bool enabled" in fh.read()


def _cli():
    lib = os.path.join(ROOT, "gpuspectral_amd", "lib")
    exe = os.path.join(lib, "gsp_render")
    assert os.path.exists(exe), "host CLI not built (make -C gpuspectral_amd/host)"
    return exe, dict(os.environ, LD_LIBRARY_PATH=lib + ":" + os.environ.get("LD_LIBRARY_PATH", ""))


def test_cli_usage_names_the_flag():
    exe, env = _cli()
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "[--light-grid [NX,NY,NZ]]" in r.stderr


@pytest.mark.parametrize("flags", [["--light-grid"], ["--light-grid", "8,2,8"], ["--light-grid", "--no-nee"]])
def test_cli_parses_the_flag_with_and_without_a_resolution(tmp_path, flags):
    """A bad device list is reported AFTER the options, so reaching it means the option was accepted (and, without a resolution, that
    the scene path behind the flag was not taken for one)."""
    exe, env = _cli()
    r = subprocess.run([exe] + flags + [str(tmp_path / "none.xml"), str(tmp_path / "x.pfm"), "8", "8", "1", "abc"], env=env, capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2 and "unknown option" not in r.stderr and "gsp_render: bad device list" in r.stderr, r.stderr
