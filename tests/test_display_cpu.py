"""LDR film without a GPU: the library's per-pixel code (csrc/pt_display.h compiled for the host, tests/emu/display_emu.cpp) against a
float64 numpy restatement of the header's "LDR film" section; the frame statistics; the Reinhard operator's properties; the PNG
writer; the loader's readFilm option.

Byte agreement.  The transform's float32 error is ~1e-6 of a code value, so the emulation and the float64 restatement can only
disagree where a value sits on a rounding threshold: no byte may differ by more than 1, and at most 1e-4 of the bytes may differ at
all.  Measured with det_expf / det_logf (profiles/display_cpu_check.txt; `python tests/test_display_cpu.py` rewrites it)."""
import os
import struct
import zlib

import numpy as np
import pytest

from conftest import CORNELL_XML, GOLDEN, ROOT
from display_util import COMBOS, TONEMAPS, DisplayEmu, bytes64, combo_display, stats64, unpack

MAX_SHARE = 1e-4  # of the bytes; a condition of the design, not a measurement


@pytest.fixture(scope="module")
def demu():
    return DisplayEmu()


def _rgba(rgb):
    rgb = np.asarray(rgb, np.float32)
    return np.concatenate([rgb, np.ones(rgb.shape[:-1] + (1,), np.float32)], -1)


def _datasets():
    rng = np.random.default_rng(20261017)
    n = 1 << 16
    t = np.linspace(0.0, 1.0, n, dtype=np.float32)
    ramps = np.concatenate([np.stack([t, t, t], 1), np.stack([t * 4, t[::-1], t * t], 1), np.stack([t * 0.01, t * 16, t * 0.3], 1)])  # linear, crossing, dark / bright
    hdr = np.exp(rng.normal(-1.0, 2.0, (1 << 18, 3))).astype(np.float32)  # log-normal radiance over ~8 decades
    hdr[rng.random(len(hdr)) < 0.02] = 0.0  # black pixels
    hdr[::97, 1] *= -1.0  # negative channels (step 1)
    cornell = np.load(os.path.join(GOLDEN, "cornell_128_1spp.npy")).reshape(-1, 3)
    return {"ramps": _rgba(ramps), "random HDR": _rgba(hdr), "cornell 128 1spp (oracle)": _rgba(cornell)}


DATA = _datasets()


def _compare(demu, rgba, tonemap, gamma, exposure, **kw):
    """(bytes that differ, largest difference, bytes) between the emulation and the float64 restatement."""
    from gpuspectral_amd import abi

    d = combo_display(abi, tonemap, gamma, exposure, **kw)
    got = unpack(demu.map(d, rgba))
    assert (got[..., 3] == 255).all()
    st = demu.stats(rgba)
    want = bytes64(rgba, TONEMAPS[tonemap], d.gamma, exposure, key=kw.get("key", 0.0), burn=kw.get("burn", 0.0),
                   lavg=st["log_avg"] if st["pixels"] else None, lmax=st["max"])
    diff = np.abs(got[..., :3].astype(np.int32) - want.astype(np.int32))
    return int((diff != 0).sum()), int(diff.max()), diff.size


@pytest.mark.parametrize("tonemap,gamma,exposure", COMBOS)
@pytest.mark.parametrize("name", list(DATA))
def test_emulation_matches_float64_header(demu, name, tonemap, gamma, exposure):
    bad, worst, n = _compare(demu, DATA[name], tonemap, gamma, exposure)
    print("%s %s %s %+.1f: %d of %d bytes differ (share %.2e), largest difference %d" % (name, tonemap, gamma, exposure, bad, n, bad / n, worst))
    assert worst <= 1
    assert bad <= MAX_SHARE * n


def test_reinhard_key_and_burn_match_float64_header(demu):
    for key, burn in ((0.36, 0.0), (0.09, 0.5), (1.0, 1.0)):
        bad, worst, n = _compare(demu, DATA["random HDR"], "reinhard", "srgb", 0.0, key=key, burn=burn)
        assert worst <= 1 and bad <= MAX_SHARE * n, (key, burn, bad, worst)


def measure_shares(demu, pixels=1 << 21):
    """The share of differing bytes on `pixels` log-normal HDR pixels (3 x as many values), per tonemap and encode, exposure 0."""
    rng = np.random.default_rng(7)
    rgba = _rgba(np.exp(rng.normal(-1.0, 2.0, (pixels, 3))).astype(np.float32))
    rows = []
    for tonemap in TONEMAPS:
        for gamma in ("gamma2.2", "srgb"):
            bad, worst, n = _compare(demu, rgba, tonemap, gamma, 0.0)
            rows.append((tonemap, gamma, bad, n, worst))
    return rows


def test_share_on_six_million_values(demu):
    for tonemap, gamma, bad, n, worst in measure_shares(demu):
        print("%-8s %-8s %d of %d bytes differ: share %.2e, largest difference %d" % (tonemap, gamma, bad, n, bad / n, worst))
        assert n >= 6_000_000 and worst <= 1 and bad <= MAX_SHARE * n


def test_special_values(demu):
    """Step 1 and step 4 on what a float64 restatement cannot say: NaN and negative channels are 0, +Inf saturates, under every curve."""
    from gpuspectral_amd import abi

    inf, nan = np.float32(np.inf), np.float32(np.nan)
    px = np.array([[nan, 0.5, -1.0, 1], [inf, 0.0, -inf, 1], [0, 0, 0, 1], [1, 1, 1, 1], [1e30, 1e-30, 100, nan]], np.float32)
    for tonemap in (abi.TONEMAP_CLAMP, abi.TONEMAP_ACES):
        for gamma in (0.0, 2.2):
            b = unpack(demu.map(abi.display(tonemap=tonemap, gamma=gamma), px))
            assert b[0, 0] == 0 and b[0, 2] == 0 and b[0, 1] > 0
            assert tuple(b[1]) == (255, 0, 0, 255) and tuple(b[2]) == (0, 0, 0, 255)
            assert (b[3, :3] >= (255 if tonemap == abi.TONEMAP_CLAMP else 200)).all()
            assert b[4, 0] == 255 and b[4, 1] == 0 and b[4, 2] == 255 and b[4, 3] == 255
    b = unpack(demu.map(abi.display(tonemap=abi.TONEMAP_REINHARD), px))
    assert tuple(b[2]) == (0, 0, 0, 255) and b[0, 0] == 0 and b[0, 2] == 0  # Y == 0 is black; sanitised channels stay 0
    assert (b[..., 3] == 255).all()


# ---- frame statistics -------------------------------------------------------------------------------------------------------
def test_statistics_are_partition_independent(demu):
    """S, n and Lmax of a frame equal the sum, sum and max over any gsp_tile_partition of it, exactly (an integer sum and a max)."""
    from gpuspectral_amd import pt

    W, H = 200, 136
    rng = np.random.default_rng(3)
    frame = _rgba(np.exp(rng.normal(-1.0, 2.0, (W * H, 3))).astype(np.float32))
    frame[rng.integers(0, W * H, 50), 0] = np.nan
    whole = demu.stats(frame)
    assert whole["pixels"] == W * H - len(np.unique(np.nonzero(np.isnan(frame[:, 0]))[0]))
    for world, tile in ((2, 32), (3, 32), (5, 16), (7, 8)):
        parts = [demu.stats(frame[pt.tile_partition(W, H, r, world, tile)]) for r in range(world)]
        S, n, mx = sum(p["log_sum_q20"] for p in parts), sum(p["pixels"] for p in parts), max(p["max"] for p in parts)
        assert (S, n, mx) == (whole["log_sum_q20"], whole["pixels"], whole["max"])
        assert demu.combine(S, n, mx) == whole
    perm = rng.permutation(W * H)
    assert demu.stats(frame[perm]) == whole  # ... and of the order


def test_log_average_against_float64(demu):
    """|log Lavg - mean(log(Y + 1e-3))| <= 2^-21 (each q is rounded to a multiple of 2^-20: half a step) + 2^-21 (det_logf, ~1 ulp of a
    value below 8) + 6 * 2^-24 (the float32 roundings of Y -- two products' sums --, of Y + 1e-3 and of Lavg itself, relative, i.e.
    absolute in log units).  Lmax is the float32 luminance: within 3 * 2^-24 relative of the float64 one."""
    bound = 2.0 ** -21 + 2.0 ** -21 + 6 * 2.0 ** -24
    for name, rgba in DATA.items():
        st = demu.stats(rgba)
        lavg, lmax, n = stats64(rgba)
        assert st["pixels"] == n
        err = abs(np.log(st["log_avg"]) - np.log(lavg))
        print("%s: Lavg %.9g vs %.9g (log error %.2e, bound %.2e), Lmax %.9g vs %.9g" % (name, st["log_avg"], lavg, err, bound, st["max"], lmax))
        assert err <= bound
        assert abs(st["max"] - lmax) <= 3 * 2.0 ** -24 * lmax


def test_non_finite_pixels_are_excluded(demu):
    rgba = DATA["cornell 128 1spp (oracle)"].copy()
    clean = demu.stats(rgba)
    dirty = np.concatenate([rgba, np.array([[np.nan, 1, 1, 1], [1, np.inf, 1, 1], [1, 1, -np.inf, 1]], np.float32)])
    assert demu.stats(dirty) == clean
    assert demu.stats(np.full((4, 4), np.nan, np.float32)) == dict(log_sum_q20=0, pixels=0, log_avg=0.0, max=0.0)
    neg = demu.stats(np.array([[-2.0, -3.0, -1.0, 1.0]], np.float32))  # negative channels count as 0 (step 1)
    assert neg["pixels"] == 1 and neg["max"] == 0.0 and abs(neg["log_avg"] - 1e-3) < 1e-9


# ---- Reinhard -----------------------------------------------------------------------------------------------------------------
def test_reinhard_white_point(demu):
    """burn = 0: the pixel holding Lmax maps to luminance 1 before the encode.  In exact arithmetic Lp * invWp2 = 1 / Lp there, so
    Y' = (Lp + 1) / (1 + Lp) = 1.  In float32: scale and invWp2 are each rounded once (2 x 2^-24 relative), then Lp, Lp * invWp2,
    1 + ., the product, 1 + Lp and the quotient round once each (6 x 2^-24): |Y' - 1| <= 8 * 2^-24."""
    from gpuspectral_amd import abi

    for name, rgba in DATA.items():
        st = demu.stats(rgba)
        yp = demu.reinhard_luma(abi.display(tonemap=abi.TONEMAP_REINHARD), rgba, st["max"])
        print("%s: Y'(Lmax) = %.9g" % (name, yp))
        assert abs(yp - 1.0) <= 8 * 2.0 ** -24
        # a burn > 0 lowers the white point: the same pixel is beyond 1
        assert demu.reinhard_luma(abi.display(tonemap=abi.TONEMAP_REINHARD, burn=0.5), rgba, st["max"]) > 1.0


def test_reinhard_is_monotone(demu):
    from gpuspectral_amd import abi

    rgba = DATA["random HDR"]
    Y = np.geomspace(1e-5, 1e5, 2400)  # steps of 1 %: far above the rounding of a float32
    for d in (abi.display(tonemap=1), abi.display(tonemap=1, burn=0.8), abi.display(tonemap=1, key=0.9, log_avg_luminance=2.0, max_luminance=3.0)):
        yp = np.array([demu.reinhard_luma(d, rgba, y) for y in Y])
        assert (np.diff(yp) > 0).all()


def test_supplied_luminances_bypass_the_measurement(demu):
    from gpuspectral_amd import abi

    d = abi.display(tonemap=1, log_avg_luminance=0.4, max_luminance=20.0)
    a, b = DATA["random HDR"][:4096], DATA["ramps"][:4096]
    ka, kb = demu.consts(d, a), demu.consts(d, b)
    assert ka == kb and ka["scale"] == np.float32(0.18 / float(np.float32(0.4)))
    both = np.concatenate([a, b])
    assert np.array_equal(demu.map(d, both)[:4096], demu.map(d, a))  # a pixel's bytes do not depend on the rest of the frame
    m = abi.display(tonemap=1)
    assert demu.consts(m, a) != demu.consts(m, b)  # measured: they do
    half = abi.display(tonemap=1, log_avg_luminance=0.4)  # one supplied, one measured
    assert demu.consts(half, a)["scale"] == ka["scale"] and demu.consts(half, a)["inv_wp2"] != ka["inv_wp2"]


# ---- PNG writer ----------------------------------------------------------------------------------------------------------------
def _png_chunks(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, out = 8, []
    while pos < len(data):
        (ln,) = struct.unpack(">I", data[pos:pos + 4])
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + ln]
        assert zlib.crc32(kind + body) == struct.unpack(">I", data[pos + 8 + ln:pos + 12 + ln])[0], "CRC-32 of chunk %r" % kind
        out.append((kind, body))
        pos += 12 + ln
    return out


def _png_images():
    rng = np.random.default_rng(11)
    y, x = np.mgrid[0:97, 0:131]
    grad = ((x * 255 // 130) | ((y * 255 // 96) << 8) | ((((x + y) // 2) % 256) << 16) | ((x % 256) << 24)).astype(np.uint32)
    return {
        "gradient 131x97": grad,
        "noise 17x33": rng.integers(0, 2 ** 32, (33, 17), dtype=np.uint32),  # defeats LZ77
        "1x1": np.array([[0x12345678]], np.uint32),
        "1x5": rng.integers(0, 2 ** 32, (5, 1), dtype=np.uint32),
        "posterised 400x300": (rng.integers(0, 4, (300, 400), dtype=np.uint32) * 0x00405060) | 0xFF000000,  # long matches, far distances
        "flat 70x3": np.full((3, 70), 0x80FF00FF, np.uint32),
    }


PNG_IMAGES = _png_images()


@pytest.mark.parametrize("alpha", [False, True])
@pytest.mark.parametrize("name", list(PNG_IMAGES))
def test_png_round_trip(name, alpha):
    from gpuspectral_amd import host

    img = PNG_IMAGES[name]
    data = host.encode_png(img, alpha)
    dec = host.decode_png(data)
    assert np.array_equal(dec[::-1], img | np.uint32(0xFF000000))  # decodePng: rows bottom-up, A = 255
    # ... and through an independent inflate: the stream, its Adler-32 (zlib checks it) and the scanline filters
    chunks = _png_chunks(data)
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    bpp = 4 if alpha else 3
    assert (w, h, depth, ctype, comp, filt, lace) == (img.shape[1], img.shape[0], 8, 6 if alpha else 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, 1 + w * bpp)
    rows = np.zeros((h, w * bpp), np.uint8)
    for r in range(h):
        f, line = raw[r, 0], raw[r, 1:].astype(np.int64)
        assert f in (0, 1, 2)  # None / Sub / Up
        if f == 1:
            line = line.reshape(w, bpp).cumsum(0).reshape(-1)
        elif f == 2:
            line = line + (rows[r - 1] if r else 0)
        rows[r] = line % 256
    want = unpack(img)[..., :bpp].reshape(h, w * bpp)
    assert np.array_equal(rows, want)


@pytest.mark.parametrize("alpha", [False, True])
def test_png_round_trip_pil(tmp_path, alpha):
    Image = pytest.importorskip("PIL.Image")
    from gpuspectral_amd import host

    for name, img in PNG_IMAGES.items():
        path = str(tmp_path / ("%s_%d.png" % (name.split()[0], alpha)))
        host.write_png(path, img, alpha)
        with Image.open(path) as im:
            assert im.mode == ("RGBA" if alpha else "RGB")
            got = np.asarray(im)
        assert np.array_equal(got, unpack(img)[..., :4 if alpha else 3]), name


def test_png_compresses_a_smooth_gradient():
    from gpuspectral_amd import host

    img = PNG_IMAGES["gradient 131x97"]
    assert len(host.encode_png(img, False)) < img.size * 3 // 4
    assert len(host.encode_png(PNG_IMAGES["posterised 400x300"], False)) < PNG_IMAGES["posterised 400x300"].size * 3 // 2


def test_png_refuses_an_empty_image():
    from gpuspectral_amd import host

    with pytest.raises(host.GspError):
        host.encode_png(np.zeros((0, 4), np.uint32))


# ---- loader ----------------------------------------------------------------------------------------------------------------------
def _film_xml(tmp_path, film_type="ldrfilm", gamma="2.2", extra=()):
    text = open(CORNELL_XML).read()
    assert '<film type="ldrfilm" >' in text and '<float name="gamma" value="2.2" />' in text
    d = tmp_path / "scene"
    d.mkdir()
    for f in os.listdir(os.path.dirname(CORNELL_XML)):
        if f != "scene.xml":
            os.symlink(os.path.join(os.path.dirname(CORNELL_XML), f), str(d / f))
    props = "".join('\n\t\t\t<%s name="%s" value="%s" />' % p for p in extra)
    text = text.replace('<film type="ldrfilm" >', '<film type="%s" >%s' % (film_type, props))
    text = text.replace('<float name="gamma" value="2.2" />', '<float name="gamma" value="%s" />' % gamma if gamma is not None else "")
    (d / "scene.xml").write_text(text)
    return str(d / "scene.xml")


def _scene_bytes(s):
    a = s.arrays()
    return b"".join([a.positions.tobytes(), a.normals.tobytes(), a.instances.tobytes(), a.lights.tobytes(), a.to_world.tobytes()])


def _film(d):
    return (d.tonemap, d.gamma, d.exposure, d.key, d.burn)


def test_loader_reads_the_shipped_film():
    from gpuspectral_amd import abi, host

    ldr, d = host.Scene(CORNELL_XML, read_film=True).film
    assert ldr and _film(d) == (abi.TONEMAP_CLAMP, np.float32(2.2), 0.0, 0.0, 0.0) and d.struct_size == 32
    off = host.Scene(CORNELL_XML)
    ldr, d = off.film
    assert not ldr and _film(d) == (0, 0.0, 0.0, 0.0, 0.0)  # default: the film is ignored, as in the reference
    on = host.Scene(CORNELL_XML, read_film=True)
    assert _scene_bytes(on) == _scene_bytes(off) and on.warnings == off.warnings and on.pixel_filter == off.pixel_filter == (0, 0.0)


def test_loader_reads_film_variants(tmp_path):
    from gpuspectral_amd import abi, host

    p = _film_xml(tmp_path, gamma="-1", extra=[("float", "exposure", "1.5"), ("string", "tonemapMethod", "reinhard"), ("float", "key", "0.36"), ("float", "burn", "0.25")])
    ldr, d = host.Scene(p, read_film=True).film
    assert ldr and _film(d) == (abi.TONEMAP_REINHARD, 0.0, 1.5, np.float32(0.36), 0.25)  # gamma -1 = sRGB = 0
    assert not host.Scene(p).film[0]


def test_loader_film_defaults_and_gamma_method(tmp_path):
    from gpuspectral_amd import abi, host

    p = _film_xml(tmp_path, gamma=None, extra=[("string", "tonemapMethod", "gamma")])
    ldr, d = host.Scene(p, read_film=True).film
    assert ldr and _film(d) == (abi.TONEMAP_CLAMP, 0.0, 0.0, 0.0, 0.0)  # Mitsuba's defaults: sRGB, exposure 0


def test_loader_other_film_type_warns(tmp_path):
    from gpuspectral_amd import host

    p = _film_xml(tmp_path, film_type="hdrfilm")
    s = host.Scene(p, read_film=True)
    ldr, d = s.film
    assert not ldr and _film(d) == (0, 0.0, 0.0, 0.0, 0.0)
    assert any("hdrfilm" in w for w in s.warnings)
    assert not any("hdrfilm" in w for w in host.Scene(p).warnings)  # with the option off the film is not even looked at


@pytest.mark.parametrize("gamma,extra,word", [
    ("-3", [], "gamma"), ("2.2", [("float", "exposure", "100")], "exposure"), ("2.2", [("float", "key", "2")], "key"),
    ("2.2", [("float", "burn", "-1")], "burn"), ("2.2", [("string", "tonemapMethod", "filmic")], "tonemapMethod"),
])
def test_loader_refuses_invalid_film(tmp_path, gamma, extra, word):
    from gpuspectral_amd import host

    p = _film_xml(tmp_path, gamma=gamma, extra=extra)
    with pytest.raises(host.GspError) as e:
        host.Scene(p, read_film=True)
    assert word in str(e.value)
    host.Scene(p)  # without the option the values are not looked at


if __name__ == "__main__":
    # rewrites profiles/display_cpu_check.txt
    lines = ["LDR film, CPU check: bytes on which the host emulation of csrc/pt_display.h (det_expf / det_logf, float32) and the float64",
             "restatement of the header (tests/display_util.py bytes64) differ; 2^21 log-normal HDR pixels = 6 291 456 values, exposure 0.",
             "Condition (tests/test_display_cpu.py): no difference above 1, share of differing bytes <= 1e-4.", ""]
    for tonemap, gamma, bad, n, worst in measure_shares(DisplayEmu()):
        lines.append("%-8s %-8s %4d of %d bytes differ: share %.2e, largest difference %d" % (tonemap, gamma, bad, n, bad / n, worst))
    with open(os.path.join(ROOT, "profiles", "display_cpu_check.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
