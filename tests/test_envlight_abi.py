"""The environment light's interface: gsp_envmap_sampling, the kind constant and the two new exports against the C header (ABI still
9, no struct changed), the Python names, the digest lists and the build files -- without a GPU; and, on one, what the setter accepts
and refuses: the estimator in both orders, a frame that is no rotation, the extent, the count of gsp_download_light_pick."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = ("gsp_set_envmap_sampling", "gsp_multi_set_envmap_sampling")
FIELDS = ("enabled", "extent", "reserved")


def test_struct_constant_and_prototypes_match_header(tmp_path):
    from gpuspectral_amd import abi

    src = tmp_path / "env.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "gpuspectral_pt.h"\n'
        'int main(){printf("%zu %d %u %zu %zu",sizeof(gsp_envmap_sampling),GSP_ABI_VERSION,(unsigned)GSP_LIGHT_ENVIRONMENT,sizeof(gsp_render_params),sizeof(gsp_delta_light));'
        + "".join('printf(" %%zu",offsetof(gsp_envmap_sampling,%s));' % f for f in FIELDS)
        + "int (*a)(gsp_context*, const gsp_envmap_sampling*) = gsp_set_envmap_sampling;"
        "int (*b)(gsp_multi*, const gsp_envmap_sampling*) = gsp_multi_set_envmap_sampling; return !(a && b);}\n"
    )
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "env.o")])  # the prototypes
    src2 = tmp_path / "env2.c"
    src2.write_text(src.read_text().split("int (*a)")[0] + "return 0;}\n")
    exe = tmp_path / "env2"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src2), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert vals[0] == C.sizeof(abi.EnvmapSampling) == 16
    assert vals[1] == abi.GSP_ABI_VERSION == 9
    assert vals[2] == abi.LIGHT_ENVIRONMENT == 4 and abi.LIGHT_ENVIRONMENT not in (abi.LIGHT_POINT, abi.LIGHT_SPOT, abi.LIGHT_DIRECTIONAL)
    assert vals[3] == C.sizeof(abi.RenderParams) and vals[4] == C.sizeof(abi.DeltaLight)  # no struct changed
    assert vals[5:] == [getattr(abi.EnvmapSampling, f).offset for f in FIELDS] == [0, 4, 8]


def test_abi_version_still_9_and_exports_exist():
    from gpuspectral_amd import pt

    L = pt.load()
    assert L.gsp_abi_version() == 9
    for name in SYMBOLS:
        assert name in pt.EXPORTS and getattr(L, name)
    assert hasattr(pt.Context, "set_envmap_sampling") and hasattr(pt.MultiContext, "set_envmap_sampling")


def test_null_context_is_invalid():
    from gpuspectral_amd import abi, pt

    L = pt.load()
    s = abi.EnvmapSampling(1, 2.0, (C.c_uint32 * 2)(0, 0))
    assert L.gsp_set_envmap_sampling(None, C.byref(s)) == 1  # GSP_ERR_INVALID
    assert L.gsp_multi_set_envmap_sampling(None, C.byref(s)) == 1


def test_header_section_digest_and_build_files_cover_the_feature():
    from gpuspectral_amd import pt

    text = open(os.path.join(ROOT, "include", "gpuspectral_pt.h")).read()
    assert "Environment light:" in text and "lengthens the path's random stream by one draw" in text and "no Jacobian term" in text
    for f in ("pt_render_envlight.hip", "pt_envlight.h"):
        assert f in pt.DIGEST_SOURCES
        assert f in open(os.path.join(ROOT, "gpuspectral_amd", "csrc", "Makefile")).read()
    assert "pt_render_envlight.hip" in open(os.path.join(ROOT, "scripts", "build_variant.sh")).read()
    assert pt.build_info()["digest"] == pt.source_digest()
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "envlight.mk" in entry and "set_envmap_sampling" in entry


def test_gsp_set_delta_lights_keeps_rejecting_the_internal_kind():
    import delta_util as du
    from gpuspectral_amd import abi

    l = abi.point_light((0, 1, 0), (1, 1, 1))
    l.kind = abi.LIGHT_ENVIRONMENT
    err, _ = du.DeltaEmu().check([l])
    assert err and "kind" in err


# ---- on a device: what the setter accepts and refuses ------------------------------------------------------------------------------------
def _ctx():
    import gpuspectral_amd as g

    return g.Context(0)


def _sky():
    import textured

    return textured.decorate(textured.open_scene(6), seed=3, textures=False)


@pytest.mark.gpu
def test_the_reference_estimator_is_refused_in_both_orders():
    with _ctx() as ctx:
        with pytest.raises(RuntimeError):
            ctx.set_envmap_sampling(True, 2.0)            # the new setter first: the context runs the reference estimator
        ctx.set_estimator("textbook")
        ctx.set_envmap_sampling(True, 2.0)
        with pytest.raises(RuntimeError):
            ctx.set_estimator("reference")                # gsp_set_estimator second: the switch is on
        ctx.set_estimator("textbook")                     # (the state is unchanged: still textbook, still on)
        ctx.upload_scene(_sky())
        ctx.set_light_sampling("power")
        n_on = len(ctx.download_light_pick())
        ctx.set_envmap_sampling(False)
        ctx.set_estimator("reference")                    # off: the reference estimator is free again
        assert len(ctx.download_light_pick()) == n_on - 1


@pytest.mark.gpu
def test_extent_and_reserved_are_validated_and_leave_the_state_unchanged():
    from gpuspectral_amd import abi, pt

    L = pt.load()
    with _ctx() as ctx:
        ctx.set_estimator("textbook")
        ctx.set_light_sampling("power")
        ctx.upload_scene(_sky())
        ctx.set_envmap_sampling(True, 2.0)
        before = ctx.download_light_pick()
        for extent in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(RuntimeError):
                ctx.set_envmap_sampling(True, extent)
        s = abi.EnvmapSampling(1, 2.0, (C.c_uint32 * 2)(0, 5))
        assert L.gsp_set_envmap_sampling(ctx._h, C.byref(s)) == 1
        assert np.array_equal(before, ctx.download_light_pick())
        s = abi.EnvmapSampling(0, float("nan"), (C.c_uint32 * 2)(9, 9))  # enabled == 0: nothing else is read
        assert L.gsp_set_envmap_sampling(ctx._h, C.byref(s)) == 0
        assert len(ctx.download_light_pick()) == len(before) - 1


@pytest.mark.gpu
def test_a_frame_that_is_no_rotation_is_refused_whichever_call_comes_second():
    sc = _sky()
    sc.env_to_local = (np.asarray(sc.env_to_local, np.float32) * np.float32(1.01)).astype(np.float32)  # a uniform scale: no rotation
    with _ctx() as ctx:
        ctx.set_estimator("textbook")
        ctx.upload_scene(sc)                               # fine with the switch off
        ctx.frame_begin(8, 8)
        ctx.render(spp=1)
        with pytest.raises(RuntimeError):
            ctx.set_envmap_sampling(True, 2.0)             # the setter second
        ctx.frame_begin(8, 8)
        ctx.render(spp=1)                                  # (the state is unchanged: the scene still renders)
        good = _sky()
        ctx.upload_scene(good)
        ctx.set_envmap_sampling(True, 2.0)
        with pytest.raises(RuntimeError):
            ctx.upload_scene(sc)                           # the upload second


@pytest.mark.gpu
def test_download_light_pick_counts_the_record_last_and_the_record_carries_its_mass():
    import envlight_util as eu
    from gpuspectral_amd import abi

    sc = _sky()
    point = [abi.point_light((0.0, 2.0, 0.0), (1.0, 1.0, 1.0))]
    emu = eu.EnvEmu()
    with _ctx() as ctx:
        ctx.set_estimator("textbook")
        ctx.set_light_sampling("power")
        ctx.set_delta_lights(point)
        ctx.upload_scene(sc)
        n = len(ctx.download_light_pick())
        assert n == len(sc.lights) + 1
        ctx.set_envmap_sampling(True, 2.5)
        table = ctx.download_light_pick()
        assert len(table) == n + 1
        want = emu.light_pick(sc.lights, point, emu.power_weight(sc.env_texels, 2.5))
        assert np.array_equal(table, want)                 # triangles, the point light, the environment record LAST
        ctx.upload_scene(sc)                               # context state: it survives gsp_upload_scene ...
        assert np.array_equal(ctx.download_light_pick(), want)
        ctx.update_tables(sc)                              # ... and gsp_update_tables
        assert np.array_equal(ctx.download_light_pick(), want)
        bare = _sky()
        bare.env_texels = None
        ctx.upload_scene(bare)                             # no map: inert
        assert len(ctx.download_light_pick()) == n


@pytest.mark.gpu
def test_multi_context_forwards_the_switch():
    import envlight_util as eu
    from gpuspectral_amd import pt

    sc = _sky()
    ref = eu.EnvEmu().scene(sc).render(16, 12, 2, env=2.0)[0]
    with pt.MultiContext([0, 0]) as m:
        m.set_estimator("textbook")
        m.set_envmap_sampling(True, 2.0)
        m.upload_scene(sc)
        m.frame_begin(16, 12)
        m.render(spp=2)
        m.gather()
        img = m.download().reshape(-1, 4)
    assert eu.same(img, ref)
