"""Temporal accumulation without a GPU: gsp_temporal against the C header (ABI still 9), the six prototypes, the NULL-handle
returns, the validation and struct_size rule of gsp_temporal_accumulate (the library's own resolve_temporal, compiled for the host
in tests/emu/temporal_emu.cpp), and the CLI flags."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from temporal_util import FLT_MIN, TemporalEmu

NAN = float("nan")
INF = float("inf")
SYMBOLS = ("gsp_temporal_accumulate", "gsp_temporal_reset", "gsp_download_temporal", "gsp_temporal_to_device", "gsp_download_temporal_denoised",
           "gsp_download_temporal_denoised_display", "gsp_frame_sample_base")


@pytest.fixture(scope="module")
def emu():
    return TemporalEmu()


def test_struct_matches_header(tmp_path):
    from gpuspectral_amd import abi

    fields = ["struct_size", "max_history", "alpha", "depth_tolerance", "normal_min"]
    body = ('printf("%zu ", sizeof(gsp_temporal));' + "".join('printf("%%zu ", offsetof(gsp_temporal, %s));' % f for f in fields)
            + 'printf("%d\\n", GSP_ABI_VERSION);')
    protos = ("int (*a)(gsp_context*, const gsp_temporal*) = gsp_temporal_accumulate;"
              "int (*b)(gsp_context*) = gsp_temporal_reset;"
              "int (*c)(gsp_context*, float*) = gsp_download_temporal;"
              "int (*d)(gsp_context*, void*, uint64_t) = gsp_temporal_to_device;"
              "int (*e)(gsp_context*, const gsp_denoise*, float*) = gsp_download_temporal_denoised;"
              "int (*f)(gsp_context*, const gsp_denoise*, const gsp_display*, uint32_t*) = gsp_download_temporal_denoised_display;"
              "int (*g)(gsp_context*, uint32_t) = gsp_frame_sample_base;"
              "(void)a; (void)b; (void)c; (void)d; (void)e; (void)f; (void)g;")
    head = '#include <stdio.h>\n#include <stddef.h>\n#include "gpuspectral_pt.h"\nint main(){'
    src = tmp_path / "t.c"
    src.write_text(head + protos + "return 0;}\n")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])  # the prototypes
    src2 = tmp_path / "t2.c"
    src2.write_text(head + body + "return 0;}\n")
    exe = tmp_path / "t2"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src2), "-o", str(exe)])
    vals = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert vals[0] == C.sizeof(abi.Temporal) == 20
    assert vals[1:6] == [getattr(abi.Temporal, f).offset for f in fields] == [0, 4, 8, 12, 16]
    assert vals[6] == abi.GSP_ABI_VERSION == 9
    assert abi.temporal().struct_size == 20


def test_abi_version_still_9_and_exports_exist():
    from gpuspectral_amd import pt

    L = pt.load()
    assert L.gsp_abi_version() == 9
    for name in SYMBOLS:
        assert name in pt.EXPORTS and getattr(L, name)


def test_null_handles_are_invalid():
    from gpuspectral_amd import abi, pt

    L = pt.load()
    t = abi.temporal()
    out = np.zeros(16, np.float32)
    assert L.gsp_temporal_accumulate(None, C.byref(t)) == 1  # GSP_ERR_INVALID
    assert L.gsp_temporal_reset(None) == 1
    assert L.gsp_frame_sample_base(None, 3) == 1
    assert L.gsp_download_temporal(None, out.ctypes.data) == 1
    assert L.gsp_temporal_to_device(None, out.ctypes.data, 64) == 1
    assert L.gsp_download_temporal_denoised(None, None, out.ctypes.data) == 1
    assert L.gsp_download_temporal_denoised_display(None, None, None, out.ctypes.data) == 1
    assert not out.any()


@pytest.mark.parametrize("fields,word", [
    (dict(max_history=65537), "max_history"), (dict(max_history=0xFFFFFFFF), "max_history"),
    (dict(alpha=-0.1), "alpha"), (dict(alpha=1.0000001), "alpha"), (dict(alpha=NAN), "alpha"), (dict(alpha=INF), "alpha"),
    (dict(depth_tolerance=-1e-9), "depth_tolerance"), (dict(depth_tolerance=NAN), "depth_tolerance"), (dict(depth_tolerance=-INF), "depth_tolerance"),
    (dict(normal_min=-1.5), "normal_min"), (dict(normal_min=1.0000001), "normal_min"), (dict(normal_min=NAN), "normal_min"),
])
def test_validation_errors(emu, fields, word):
    from gpuspectral_amd import abi

    out, err = emu.resolve(abi.temporal(**fields))
    assert out is None and word in err, err


@pytest.mark.parametrize("fields", [
    dict(), dict(max_history=1), dict(max_history=65536), dict(alpha=1.0), dict(alpha=FLT_MIN), dict(depth_tolerance=INF), dict(normal_min=-1.0),
    dict(normal_min=1.0), dict(max_history=7, alpha=0.35, depth_tolerance=0.013, normal_min=0.5),
])
def test_valid_parameters_and_constants(emu, fields):
    """Defaults fill the zero fields; the defaults are formed in double and rounded to float once; a given value passes as it is."""
    from gpuspectral_amd import abi

    out, err = emu.resolve(abi.temporal(**fields))
    assert err is None
    assert float(out["max_history"]) == float(fields.get("max_history") or 32)
    for key, dflt in (("alpha", 0.2), ("depth_tolerance", 0.02), ("normal_min", 0.9)):
        assert out[key] == np.float32(fields.get(key) or dflt), key


def test_null_and_zeroed_are_the_defaults(emu):
    from gpuspectral_amd import abi

    want = emu.resolve(abi.temporal(max_history=32, alpha=0.2, depth_tolerance=0.02, normal_min=0.9))[0]
    for t in (None, abi.Temporal(), abi.temporal()):
        out, err = emu.resolve(t)
        assert err is None and out == want
    assert float(want["max_history"]) == 32.0 and want["alpha"] == np.float32(0.2)


def test_struct_size_rule(emu):
    """A shorter struct reads its missing fields as 0 (= their defaults); a longer one is read up to the fields this library knows."""
    from gpuspectral_amd import abi

    full = abi.temporal(max_history=5, alpha=0.5, depth_tolerance=0.25, normal_min=0.125)
    full.struct_size = abi.Temporal.depth_tolerance.offset  # a host whose header ends behind alpha
    out, err = emu.resolve(full)
    assert err is None and [float(out[k]) for k in ("max_history", "alpha", "depth_tolerance", "normal_min")] == [5.0, 0.5, float(np.float32(0.02)), float(np.float32(0.9))]
    full.struct_size = abi.Temporal.alpha.offset  # max_history alone
    out, err = emu.resolve(full)
    assert err is None and (float(out["max_history"]), out["alpha"]) == (5.0, np.float32(0.2))
    full.struct_size = 0  # the zeroed struct's own size field: everything default
    out, err = emu.resolve(full)
    assert err is None and out == emu.resolve(None)[0]
    full.struct_size = 400  # a newer host
    out, err = emu.resolve(full)
    assert err is None and [float(out[k]) for k in ("max_history", "alpha", "depth_tolerance", "normal_min")] == [5.0, 0.5, 0.25, 0.125]
    bad = abi.temporal(normal_min=-3.0)
    bad.struct_size = abi.Temporal.normal_min.offset  # the bad field lies beyond the struct: not read
    assert emu.resolve(bad)[1] is None


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


def test_cli_usage_names_the_temporal_flags():
    exe, env = _cli()
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "[--temporal out.pfm --temporal-frames N [--temporal-orbit DEG]]" in r.stderr


@pytest.mark.parametrize("flags", [
    ["--temporal", "o.pfm", "--temporal-frames", "4"], ["--temporal-frames", "2", "--temporal-orbit", "-2.5", "--temporal", "o.pfm"],
    ["--temporal", "o.pfm", "--temporal-frames", "1", "--temporal-orbit", "0", "--denoise", "d.pfm"],
])
def test_cli_parses_temporal_flags(tmp_path, flags):
    """A bad device list is reported AFTER the options, so reaching it means the options were accepted."""
    r = _run(tmp_path, flags)
    assert r.returncode == 2 and "unknown option" not in r.stderr and "gsp_render: bad device list" in r.stderr, r.stderr
    assert r.stderr.count("gsp_render: bad") == 1, r.stderr


@pytest.mark.parametrize("flags,word", [
    (["--temporal", "o.pfm", "--temporal-frames", "0"], "bad temporal frames"), (["--temporal", "o.pfm", "--temporal-frames", "x"], "bad temporal frames"),
    (["--temporal", "o.pfm", "--temporal-frames", "100001"], "bad temporal frames"),
    (["--temporal", "o.pfm", "--temporal-frames", "3", "--temporal-orbit", "nan"], "bad temporal orbit"),
    (["--temporal", "o.pfm", "--temporal-frames", "3", "--temporal-orbit", "2deg"], "bad temporal orbit"),
    (["--temporal", "o.pfm", "--temporal-frames", "3", "--temporal-orbit", "400"], "bad temporal orbit"),
    (["--temporal-frames", "3"], "need --temporal"), (["--temporal-orbit", "2"], "need --temporal"), (["--temporal", "o.pfm"], "needs --temporal-frames"),
])
def test_cli_rejects_bad_temporal_flags(tmp_path, flags, word):
    r = _run(tmp_path, flags)
    assert r.returncode == 2 and word in r.stderr and "bad device list" not in r.stderr, r.stderr


def test_cli_temporal_is_single_device(tmp_path):
    r = _run(tmp_path, ["--temporal", "o.pfm", "--temporal-frames", "3"], devices="0,1")
    assert r.returncode == 2 and "--temporal needs a single device" in r.stderr, r.stderr
