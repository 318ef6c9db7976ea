"""The denoiser without a GPU: gsp_denoise against the C header (ABI still 9), the prototypes, the NULL-handle returns, the
validation and struct_size rule of gsp_*_denoised* (the library's own resolve_denoise, compiled for the host in
tests/emu/denoise_emu.cpp), and the CLI flags."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from denoise_util import INF, DenoiseEmu, inv_sigma2

NAN = float("nan")


@pytest.fixture(scope="module")
def emu():
    return DenoiseEmu()


def test_struct_matches_header(tmp_path):
    from gpuspectral_amd import abi

    fields = ["struct_size", "iterations", "sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo"]
    body = ('printf("%zu ", sizeof(gsp_denoise));' + "".join('printf("%%zu ", offsetof(gsp_denoise, %s));' % f for f in fields)
            + 'printf("%d\\n", GSP_ABI_VERSION);')
    protos = ("int (*a)(gsp_context*, const gsp_denoise*, float*) = gsp_download_denoised;"
              "int (*b)(gsp_context*, const gsp_denoise*, void*, uint64_t) = gsp_denoise_to_device;"
              "int (*c)(gsp_context*, const gsp_denoise*, const gsp_display*, uint32_t*) = gsp_download_denoised_display;"
              "int (*d)(gsp_multi*, const gsp_denoise*, float*) = gsp_multi_download_denoised; (void)a; (void)b; (void)c; (void)d;")
    head = '#include <stdio.h>\n#include <stddef.h>\n#include "gpuspectral_pt.h"\nint main(){'
    src = tmp_path / "d.c"
    src.write_text(head + protos + "return 0;}\n")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "d.o")])  # the prototypes
    src2 = tmp_path / "d2.c"
    src2.write_text(head + body + "return 0;}\n")
    exe = tmp_path / "d2"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src2), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert vals[0] == C.sizeof(abi.Denoise) == 24
    assert vals[1:7] == [getattr(abi.Denoise, f).offset for f in fields] == [0, 4, 8, 12, 16, 20]
    assert vals[7] == abi.GSP_ABI_VERSION == 9
    assert abi.denoise().struct_size == 24


def test_abi_version_still_9_and_exports_exist():
    from gpuspectral_amd import pt

    L = pt.load()
    assert L.gsp_abi_version() == 9
    for name in ("gsp_download_denoised", "gsp_denoise_to_device", "gsp_download_denoised_display", "gsp_multi_download_denoised"):
        assert name in pt.EXPORTS and getattr(L, name)


def test_null_handles_are_invalid():
    from gpuspectral_amd import abi, pt

    L = pt.load()
    d = abi.denoise()
    out = np.zeros(16, np.float32)
    assert L.gsp_download_denoised(None, C.byref(d), out.ctypes.data) == 1  # GSP_ERR_INVALID
    assert L.gsp_denoise_to_device(None, C.byref(d), out.ctypes.data, 64) == 1
    assert L.gsp_download_denoised_display(None, C.byref(d), None, out.ctypes.data) == 1
    assert L.gsp_multi_download_denoised(None, C.byref(d), out.ctypes.data) == 1
    assert not out.any()


@pytest.mark.parametrize("fields,word", [
    (dict(iterations=9), "iterations"), (dict(iterations=0xFFFFFFFF), "iterations"),
    (dict(sigma_color=-1.0), "sigma_color"), (dict(sigma_color=NAN), "sigma_color"), (dict(sigma_color=-INF), "sigma_color"),
    (dict(sigma_normal=-0.3), "sigma_normal"), (dict(sigma_normal=NAN), "sigma_normal"),
    (dict(sigma_depth=-1e-9), "sigma_depth"), (dict(sigma_depth=NAN), "sigma_depth"),
    (dict(sigma_albedo=-2.0), "sigma_albedo"), (dict(sigma_albedo=NAN), "sigma_albedo"),
])
def test_validation_errors(emu, fields, word):
    from gpuspectral_amd import abi

    out, err = emu.resolve(abi.denoise(**fields))
    assert out is None and word in err, err


@pytest.mark.parametrize("fields", [
    dict(), dict(iterations=1), dict(iterations=8), dict(sigma_color=INF), dict(sigma_normal=INF, sigma_depth=INF, sigma_albedo=INF),
    dict(iterations=3, sigma_color=0.25, sigma_normal=0.7, sigma_depth=0.013, sigma_albedo=2.0), dict(sigma_depth=1e-30),
])
def test_valid_parameters_and_constants(emu, fields):
    """Defaults fill the zero fields; 1 / sigma^2 is formed in double and rounded to float once; +Inf gives 0."""
    from gpuspectral_amd import abi

    out, err = emu.resolve(abi.denoise(**fields))
    assert err is None and out["iterations"] == (fields.get("iterations") or 5)
    for key, name, dflt in (("inv_sc2", "sigma_color", 0.5), ("inv_sn2", "sigma_normal", 0.3), ("inv_sz2", "sigma_depth", 0.05), ("inv_sa2", "sigma_albedo", 0.1)):
        sigma = float(np.float32(fields.get(name, 0.0)))
        assert float(out[key]) == inv_sigma2(sigma, dflt), key
        assert np.isfinite(out[key])
    if "sigma_color" in fields and fields["sigma_color"] == INF:
        assert float(out["inv_sc2"]) == 0.0


def test_null_and_zeroed_are_the_defaults(emu):
    from gpuspectral_amd import abi

    want = emu.resolve(abi.denoise(iterations=5, sigma_color=0.5, sigma_normal=0.3, sigma_depth=0.05, sigma_albedo=0.1))[0]
    for d in (None, abi.Denoise(), abi.denoise()):
        out, err = emu.resolve(d)
        assert err is None and out == want
    assert (want["iterations"], float(want["inv_sc2"]), float(want["inv_sz2"])) == (5, 4.0, 400.0)


def test_struct_size_rule(emu):
    """A shorter struct reads its missing fields as 0 (= their defaults); a longer one is read up to the fields this library knows."""
    from gpuspectral_amd import abi

    full = abi.denoise(iterations=3, sigma_color=1.0, sigma_normal=2.0, sigma_depth=4.0, sigma_albedo=8.0)
    full.struct_size = abi.Denoise.sigma_depth.offset  # a host whose header ends behind sigma_normal
    out, err = emu.resolve(full)
    assert err is None and (out["iterations"], float(out["inv_sc2"]), float(out["inv_sn2"]), float(out["inv_sz2"]), float(out["inv_sa2"])) == (3, 1.0, 0.25, 400.0, 100.0)
    full.struct_size = abi.Denoise.sigma_color.offset  # iterations alone
    out, err = emu.resolve(full)
    assert err is None and (out["iterations"], float(out["inv_sc2"])) == (3, 4.0)
    full.struct_size = 0  # the zeroed struct's own size field: everything default
    out, err = emu.resolve(full)
    assert err is None and out == emu.resolve(None)[0]
    full.struct_size = 400  # a newer host
    out, err = emu.resolve(full)
    assert err is None and (float(out["inv_sz2"]), float(out["inv_sa2"])) == (0.0625, 0.015625)
    bad = abi.denoise(sigma_albedo=-1.0)
    bad.struct_size = abi.Denoise.sigma_albedo.offset  # the bad field lies beyond the struct: not read
    assert emu.resolve(bad)[1] is None


# ---- CLI ------------------------------------------------------------------------------------------------------------------
def _cli():
    lib = os.path.join(ROOT, "gpuspectral_amd", "lib")
    exe = os.path.join(lib, "gsp_render")
    assert os.path.exists(exe), "host CLI not built (make -C gpuspectral_amd/host)"
    return exe, dict(os.environ, LD_LIBRARY_PATH=lib + ":" + os.environ.get("LD_LIBRARY_PATH", ""))


def test_cli_usage_names_the_denoise_flags():
    exe, env = _cli()
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "[--denoise out.pfm [--denoise-iterations N] [--denoise-sigma c,n,z,a]]" in r.stderr


@pytest.mark.parametrize("flags", [
    ["--denoise", "o.pfm"], ["--denoise", "o.pfm", "--denoise-iterations", "8"], ["--denoise-sigma", "0.5,0.3,0.05,0.1", "--denoise", "o.pfm"],
    ["--denoise", "o.pfm", "--denoise-sigma", "inf,0,inf,2", "--denoise-iterations", "1"], ["--denoise", "o.pfm", "--ldr", "o.png", "--features", "f"],
])
def test_cli_parses_denoise_flags(tmp_path, flags):
    """A bad device list is reported AFTER the options, so reaching it means the options were accepted."""
    exe, env = _cli()
    r = subprocess.run([exe] + flags + [str(tmp_path / "none.xml"), str(tmp_path / "x.pfm"), "8", "8", "1", "abc"], env=env, capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 2 and "unknown option" not in r.stderr and "gsp_render: bad device list" in r.stderr, r.stderr
    assert r.stderr.count("gsp_render: bad") == 1, r.stderr


@pytest.mark.parametrize("flags,word", [
    (["--denoise", "o.pfm", "--denoise-iterations", "0"], "bad denoise iterations"), (["--denoise", "o.pfm", "--denoise-iterations", "9"], "bad denoise iterations"),
    (["--denoise", "o.pfm", "--denoise-iterations", "x"], "bad denoise iterations"), (["--denoise", "o.pfm", "--denoise-sigma", "1,2,3"], "bad denoise sigma"),
    (["--denoise", "o.pfm", "--denoise-sigma", "1,2,3,4,5"], "bad denoise sigma"), (["--denoise", "o.pfm", "--denoise-sigma", "1,-2,3,4"], "bad denoise sigma"),
    (["--denoise", "o.pfm", "--denoise-sigma", "1,nan,3,4"], "bad denoise sigma"), (["--denoise", "o.pfm", "--denoise-sigma", ""], "bad denoise sigma"),
    (["--denoise-iterations", "3"], "need --denoise"), (["--denoise-sigma", "1,1,1,1"], "need --denoise"),
])
def test_cli_rejects_bad_denoise_flags(tmp_path, flags, word):
    exe, env = _cli()
    r = subprocess.run([exe] + flags + [str(tmp_path / "none.xml"), str(tmp_path / "x.pfm"), "8", "8", "1", "abc"], env=env, capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 2 and word in r.stderr and "bad device list" not in r.stderr, r.stderr
