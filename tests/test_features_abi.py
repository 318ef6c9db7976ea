"""Feature buffers, the C side without a GPU: the header's prototypes through gcc, the exports of the built library, and the
argument checks that need no device (include/gpuspectral_pt.h, "Feature buffers")."""
import os
import subprocess

from conftest import ROOT

PROTOTYPES = r"""
#include "gpuspectral_pt.h"
/* the header's prototypes, assigned to pointers of the documented types: a changed signature does not compile */
int (*p1)(gsp_context*, const gsp_render_params*) = gsp_render_features;
int (*p2)(gsp_context*, float*, float*, uint32_t*) = gsp_download_features;
int (*p3)(gsp_context*, void*, void*, void*, uint64_t) = gsp_copy_features_to_device;
int (*p4)(gsp_multi*, const gsp_render_params*) = gsp_multi_render_features;
int (*p5)(gsp_multi*, float*, float*, uint32_t*) = gsp_multi_download_features;
/* no struct has changed: the ABI version and the sizes the earlier tests pin stay */
_Static_assert(GSP_ABI_VERSION == 9, "new exports only");
_Static_assert(sizeof(gsp_render_params) == 60, "gsp_render_params");
"""


def test_prototypes_compile_as_c(tmp_path):
    src = tmp_path / "features_abi.c"
    src.write_text(PROTOTYPES)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "features_abi.o")])


def test_exports_and_null_arguments():
    import gpuspectral_amd as g
    from gpuspectral_amd import abi, pt
    import ctypes as C

    L = pt.load()
    for name in ("gsp_render_features", "gsp_download_features", "gsp_copy_features_to_device", "gsp_multi_render_features", "gsp_multi_download_features"):
        assert name in pt.EXPORTS and hasattr(L, name)
    p = abi.default_render_params()
    assert L.gsp_render_features(None, C.byref(p)) == 1  # GSP_ERR_INVALID
    assert L.gsp_download_features(None, None, None, None) == 1
    assert L.gsp_copy_features_to_device(None, None, None, None, 0) == 1
    assert L.gsp_multi_render_features(None, C.byref(p)) == 1
    assert L.gsp_multi_download_features(None, None, None, None) == 1
    assert g.abi.GSP_ABI_VERSION == 9


# ---- CLI ------------------------------------------------------------------------------------------------------------------
def _cli():
    lib = os.path.join(ROOT, "gpuspectral_amd", "lib")
    exe = os.path.join(lib, "gsp_render")
    assert os.path.exists(exe), "host CLI not built (make -C gpuspectral_amd/host)"
    return exe, dict(os.environ, LD_LIBRARY_PATH=lib + ":" + os.environ.get("LD_LIBRARY_PATH", ""))


def test_cli_usage_names_the_feature_flags():
    exe, env = _cli()
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--features PREFIX [--feature-spp N]" in r.stderr
    for tok in ("--ldr out.png", "--aperture R", "--filter none|box|tent[:r]|gaussian[:s]", "scene.xml out.pfm"):  # what was there stays
        assert tok in r.stderr, tok


def test_cli_feature_flag_errors(tmp_path):
    exe, env = _cli()
    tail = [str(tmp_path / "none.xml"), str(tmp_path / "x.pfm"), "8", "8", "1", "abc"]
    for flags, word in ((["--feature-spp", "4"], "--feature-spp needs --features PREFIX"),
                        (["--features", "p", "--feature-spp", "0"], "a sample count of at least 1"),
                        (["--features", "p", "--feature-spp", "x"], "a sample count of at least 1")):
        r = subprocess.run([exe] + flags + tail, env=env, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and word in r.stderr, (flags, r.stderr)
    # accepted flags reach the device list, which is reported after the options
    r = subprocess.run([exe, "--features", str(tmp_path / "f"), "--feature-spp", "3"] + tail, env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "gsp_render: bad " + "device list" in r.stderr, r.stderr
