"""The variance-guided filter without a GPU: gsp_svgf against the C header (ABI still 9; gsp_denoise and gsp_temporal as they
were), the five prototypes, the NULL-handle returns, the validation and struct_size rule (the library's own resolve_svgf, compiled
for the host in tests/emu/svgf_emu.cpp), and the CLI flags."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from svgf_util import SvgfEmu

NAN = float("nan")
INF = float("inf")
SYMBOLS = ("gsp_temporal_track_moments", "gsp_download_temporal_moments", "gsp_download_temporal_svgf", "gsp_temporal_svgf_to_device",
           "gsp_download_temporal_svgf_display")


@pytest.fixture(scope="module")
def emu():
    return SvgfEmu()


def test_struct_matches_header(tmp_path):
    from gpuspectral_amd import abi

    fields = ["struct_size", "min_history", "sigma_variance"]
    body = ('printf("%zu ", sizeof(gsp_svgf));' + "".join('printf("%%zu ", offsetof(gsp_svgf, %s));' % f for f in fields)
            + 'printf("%zu %zu %d\\n", sizeof(gsp_denoise), sizeof(gsp_temporal), GSP_ABI_VERSION);')
    protos = ("int (*a)(gsp_context*, int) = gsp_temporal_track_moments;"
              "int (*b)(gsp_context*, float*) = gsp_download_temporal_moments;"
              "int (*c)(gsp_context*, const gsp_denoise*, const gsp_svgf*, float*) = gsp_download_temporal_svgf;"
              "int (*d)(gsp_context*, const gsp_denoise*, const gsp_svgf*, void*, uint64_t) = gsp_temporal_svgf_to_device;"
              "int (*e)(gsp_context*, const gsp_denoise*, const gsp_svgf*, const gsp_display*, uint32_t*) = gsp_download_temporal_svgf_display;"
              "(void)a; (void)b; (void)c; (void)d; (void)e;")
    head = '#include <stdio.h>\n#include <stddef.h>\n#include "gpuspectral_pt.h"\nint main(){'
    src = tmp_path / "t.c"
    src.write_text(head + protos + "return 0;}\n")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])  # the prototypes
    src2 = tmp_path / "t2.c"
    src2.write_text(head + body + "return 0;}\n")
    exe = tmp_path / "t2"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src2), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert vals[0] == C.sizeof(abi.Svgf) == 12
    assert vals[1:4] == [getattr(abi.Svgf, f).offset for f in fields] == [0, 4, 8]
    assert vals[4:6] == [C.sizeof(abi.Denoise), C.sizeof(abi.Temporal)] == [24, 20]  # the structs beside it did not change
    assert vals[6] == abi.GSP_ABI_VERSION == 9
    assert abi.svgf().struct_size == 12


def test_abi_version_still_9_and_exports_exist():
    from gpuspectral_amd import pt

    L = pt.load()
    assert L.gsp_abi_version() == 9
    for name in SYMBOLS:
        assert name in pt.EXPORTS and getattr(L, name)


def test_null_handles_are_invalid():
    from gpuspectral_amd import pt

    L = pt.load()
    out = np.zeros(16, np.float32)
    assert L.gsp_temporal_track_moments(None, 1) == 1  # GSP_ERR_INVALID
    assert L.gsp_download_temporal_moments(None, out.ctypes.data) == 1
    assert L.gsp_download_temporal_svgf(None, None, None, out.ctypes.data) == 1
    assert L.gsp_temporal_svgf_to_device(None, None, None, out.ctypes.data, 64) == 1
    assert L.gsp_download_temporal_svgf_display(None, None, None, None, out.ctypes.data) == 1
    assert not out.any()


@pytest.mark.parametrize("denoise,fields,word", [
    ({}, dict(min_history=1), "min_history"), ({}, dict(min_history=65537), "min_history"), ({}, dict(min_history=0xFFFFFFFF), "min_history"),
    ({}, dict(sigma_variance=-0.5), "sigma_variance"), ({}, dict(sigma_variance=NAN), "sigma_variance"), ({}, dict(sigma_variance=-INF), "sigma_variance"),
    (dict(iterations=9), {}, "iterations"), (dict(sigma_color=-1.0), {}, "sigma_color"), (dict(sigma_normal=NAN), {}, "sigma_normal"),
    (dict(sigma_depth=-1.0), {}, "sigma_depth"), (dict(sigma_albedo=-INF), {}, "sigma_albedo"),
])
def test_validation_errors(emu, denoise, fields, word):
    """gsp_svgf's own fields, and every field of the gsp_denoise beside it -- sigma_color too, which the filter does not use."""
    from gpuspectral_amd import abi

    out, err = emu.resolve(abi.denoise(**denoise), abi.svgf(**fields))
    assert out is None and word in err, err


@pytest.mark.parametrize("fields", [dict(), dict(min_history=2), dict(min_history=65536), dict(sigma_variance=INF), dict(sigma_variance=1e-6),
                                    dict(min_history=9, sigma_variance=2.5)])
def test_valid_parameters_and_constants(emu, fields):
    from gpuspectral_amd import abi

    out, err = emu.resolve(abi.denoise(iterations=3, sigma_normal=0.5, sigma_color=123.0), abi.svgf(**fields))
    assert err is None
    assert float(out["min_history"]) == float(fields.get("min_history") or 4)
    s = fields.get("sigma_variance") or 4.0
    assert out["lum_on"] == (0 if np.isinf(s) else 1)
    if out["lum_on"]:
        assert out["sigma_v"] == np.float32(s)
    assert out["iterations"] == 3 and out["inv_sn2"] == np.float32(4.0) and out["inv_sz2"] == np.float32(1.0 / (0.05 * 0.05)) and out["inv_sa2"] == np.float32(1.0 / (0.1 * 0.1))


def test_null_and_zeroed_are_the_defaults(emu):
    from gpuspectral_amd import abi

    want = emu.resolve(abi.denoise(iterations=5, sigma_normal=0.3, sigma_depth=0.05, sigma_albedo=0.1), abi.svgf(min_history=4, sigma_variance=4.0))[0]
    for d in (None, abi.Denoise(), abi.denoise()):
        for s in (None, abi.Svgf(), abi.svgf()):
            out, err = emu.resolve(d, s)
            assert err is None and out == want
    assert float(want["min_history"]) == 4.0 and want["sigma_v"] == np.float32(4.0) and want["lum_on"] == 1


def test_struct_size_rule(emu):
    """A shorter struct reads its missing fields as 0 (= their defaults); a longer one is read up to the fields this library knows."""
    from gpuspectral_amd import abi

    full = abi.svgf(min_history=7, sigma_variance=0.5)
    full.struct_size = abi.Svgf.sigma_variance.offset  # a host whose header ends behind min_history
    out, err = emu.resolve(None, full)
    assert err is None and (float(out["min_history"]), out["sigma_v"]) == (7.0, np.float32(4.0))
    full.struct_size = 0  # the zeroed struct's own size field: everything default
    out, err = emu.resolve(None, full)
    assert err is None and out == emu.resolve(None, None)[0]
    full.struct_size = 400  # a newer host
    out, err = emu.resolve(None, full)
    assert err is None and (float(out["min_history"]), out["sigma_v"]) == (7.0, np.float32(0.5))
    bad = abi.svgf(sigma_variance=-3.0)
    bad.struct_size = abi.Svgf.sigma_variance.offset  # the bad field lies beyond the struct: not read
    assert emu.resolve(None, bad)[1] is None


# ---- CLI ------------------------------------------------------------------------------------------------------------------
def _cli():
    lib = os.path.join(ROOT, "gpuspectral_amd", "lib")
    exe = os.path.join(lib, "gsp_render")
    assert os.path.exists(exe), "host CLI not built (make -C gpuspectral_amd/host)"
    return exe, dict(os.environ, LD_LIBRARY_PATH=lib + ":" + os.environ.get("LD_LIBRARY_PATH", ""))


def _run(tmp_path, flags, devices="abc"):
    exe, env = _cli()
    return subprocess.run([exe] + flags + [str(tmp_path / "none.xml"), str(tmp_path / "x.pfm"), "8", "8", "1", devices], env=env, capture_output=True,
                          text=True, timeout=60)


TEMPORAL = ["--temporal", "o.pfm", "--temporal-frames", "3"]


def test_cli_usage_names_the_svgf_flags():
    exe, env = _cli()
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "[--svgf out.pfm [--svgf-sigma S] [--svgf-min-history N]]" in r.stderr


@pytest.mark.parametrize("flags", [
    TEMPORAL + ["--svgf", "s.pfm"], ["--svgf", "s.pfm", "--svgf-sigma", "2.5", "--svgf-min-history", "2"] + TEMPORAL,
    TEMPORAL + ["--svgf", "s.pfm", "--svgf-sigma", "inf", "--denoise", "d.pfm", "--denoise-iterations", "3"],
])
def test_cli_parses_svgf_flags(tmp_path, flags):
    """A bad device list is reported AFTER the options, so reaching it means the options were accepted."""
    r = _run(tmp_path, flags)
    assert r.returncode == 2 and "unknown option" not in r.stderr and "gsp_render: bad device list" in r.stderr, r.stderr
    assert r.stderr.count("gsp_render: bad") == 1, r.stderr


@pytest.mark.parametrize("flags,word", [
    (["--svgf", "s.pfm"], "--svgf needs --temporal"), (["--svgf", "s.pfm", "--denoise", "d.pfm"], "--svgf needs --temporal"),
    (TEMPORAL + ["--svgf-sigma", "2"], "need --svgf"), (TEMPORAL + ["--svgf-min-history", "4"], "need --svgf"),
    (TEMPORAL + ["--svgf", "s.pfm", "--svgf-sigma", "0"], "bad svgf sigma"), (TEMPORAL + ["--svgf", "s.pfm", "--svgf-sigma", "-1"], "bad svgf sigma"),
    (TEMPORAL + ["--svgf", "s.pfm", "--svgf-sigma", "nan"], "bad svgf sigma"), (TEMPORAL + ["--svgf", "s.pfm", "--svgf-sigma", "4x"], "bad svgf sigma"),
    (TEMPORAL + ["--svgf", "s.pfm", "--svgf-min-history", "1"], "bad svgf min history"),
    (TEMPORAL + ["--svgf", "s.pfm", "--svgf-min-history", "65537"], "bad svgf min history"),
    (TEMPORAL + ["--svgf", "s.pfm", "--svgf-min-history", "four"], "bad svgf min history"),
])
def test_cli_rejects_bad_svgf_flags(tmp_path, flags, word):
    r = _run(tmp_path, flags)
    assert r.returncode == 2 and word in r.stderr and "bad device list" not in r.stderr, r.stderr
