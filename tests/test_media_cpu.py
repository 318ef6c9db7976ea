"""Interior media without a GPU (include/gpuspectral_pt.h, "Interior media"): the product's shade_vertex<.., MED = true> compiled for
the host (tests/emu/media_emu.cpp) against an analytic slab, against the frame without media, and its validation."""
import numpy as np
import pytest

import media_util as mu

SLAB_W = 32  # silhouette-edge pixels: 4.7 % of the frame at 32 x 32 (3.1 % at 48 x 48); the cap is 8 %
SLAB_SPP = 8


@pytest.fixture(scope="module")
def emu():
    return mu.MediaEmu()


@pytest.fixture(scope="module")
def slab(emu):
    """(frame without media, frame with SLAB_SIGMA on the box, expected, inside, outside), rendered once."""
    plain, _ = emu.scene(mu.slab_scene()).render(SLAB_W, SLAB_W, SLAB_SPP)
    img, _ = emu.scene(mu.slab_scene(1)).render(SLAB_W, SLAB_W, SLAB_SPP, media=[mu.SLAB_SIGMA])
    return (plain, img) + mu.slab_reference(SLAB_W, SLAB_W)


@pytest.fixture(scope="module")
def cornell():
    from gpuspectral_amd import scenes

    return scenes.cornell_materials(16)


def test_slab_reference_geometry_leaves_out_few_pixels():
    """The classes come from the reference geometry alone; the silhouette-edge pixels are the only ones left out, under 8 %."""
    _, inside, outside = mu.slab_reference(SLAB_W, SLAB_W)
    assert not (inside & outside).any()
    assert inside.sum() >= 100 and outside.sum() >= 100
    assert (~(inside | outside)).mean() <= 0.08


def test_slab_without_media_is_a_pass_through(slab):
    plain = slab[0]
    assert np.abs(plain[:, :3] - np.float32(mu.SLAB_EMISSION)).max() <= 1e-6  # (the index-matched box changes nothing: 4.8e-7)


def test_slab_matches_beer_lambert(slab):
    """L_c * exp(-sigma_c * 0.5 / cos(theta)), float64, relative tolerance 1e-5: the float32 rounding of sigma * t <= 4 and one
    ulp of the exponential stay below 2e-6, the rest is margin for the re-derived direction.  Measured: 4.7e-7 / 1.8e-6 / 3.9e-6
    (r / g / b).  The segment inside the box starts 1e-4 below the front face (rayhit.rchit:793), so its t alone is short by
    1e-4 / cos: sigma = 4 would turn that into 4e-4.  The vertex that sends the path inside absorbs that piece (the header's
    "entry piece"); this check is what holds it to the physical length."""
    plain, img, expected, inside, outside = slab
    rel = np.abs(img[inside, :3].astype(np.float64) - expected[inside]) / expected[inside]
    print("slab: largest relative error per channel against L exp(-sigma 0.5 / cos):", rel.max(0))
    assert rel.max() <= 1e-5


def test_slab_entry_piece_is_what_closes_the_gap(slab):
    """Without the entry piece the frame would sit at the traced length (0.5 - 1e-4) / cos: it must NOT (more than 1e-5 away in
    the strongest channel), or the piece is not being applied."""
    plain, img, _, inside, outside = slab
    short, _, _ = mu.slab_reference(SLAB_W, SLAB_W, thickness=0.5 - 1e-4)
    rel = np.abs(img[inside, :3].astype(np.float64) - short[inside]) / short[inside]
    assert rel[:, 2].min() > 1e-4


def test_slab_pixels_outside_the_silhouette_keep_their_bits(slab):
    plain, img, _, inside, outside = slab
    assert mu.same(img[outside], plain[outside])
    assert (img[inside, :3] < plain[inside, :3]).all()


def test_slab_twofaced_box_attenuates_on_the_unflipped_normal(emu, slab):
    """twofaced = 1 flips N and SN on a back-face hit (rayhit.rchit:698-707); the medium's test is made before that flip, so the
    two-sided box attenuates exactly as the one-sided one.  (With the flipped normal no vertex would ever be a back face.)"""
    plain, img, _, inside, outside = slab
    two, _ = emu.scene(mu.slab_scene(1, twofaced=True)).render(SLAB_W, SLAB_W, SLAB_SPP, media=[mu.SLAB_SIGMA])
    expected, _, _ = mu.slab_reference(SLAB_W, SLAB_W)
    rel = np.abs(two[inside, :3].astype(np.float64) - expected[inside]) / expected[inside]
    assert rel.max() <= 1e-5
    assert mu.same(two[outside], plain[outside])


def test_zero_sigma_equals_no_media_bit_for_bit(emu, cornell):
    """exp(-0) = 1 exactly: sigma_a = 0 on every glass object leaves the image and the ray counts of the frame without media."""
    glass = mu.glass_instances(cornell)
    assert len(glass) >= 1
    ref, st_ref = emu.scene(cornell).render(24, 24, 2)
    img, st = emu.scene(mu.with_medium(cornell, glass, 1)).render(24, 24, 2, media=[(0.0, 0.0, 0.0)])
    assert mu.same(img, ref)
    assert st == st_ref


def test_medium_only_darkens(emu, cornell):
    """Without Russian roulette and without the firefly clamp a medium changes no path; it scales non-negative contributions by
    factors <= 1, and every float32 operation behind it is monotone.  So no channel of no pixel grows, some pixel darkens, and a
    pixel whose paths never met a back face of the glass sphere (the emulation's path log) keeps its bits."""
    glass = mu.glass_instances(cornell)
    kw = dict(max_depth=6, rr_start_depth=6, clamp=float("inf"))
    ref, st_ref, log_ref = emu.scene(cornell).render(32, 32, 2, log=True, **kw)
    img, st, log = emu.scene(mu.with_medium(cornell, glass, 1)).render(32, 32, 2, media=[(1.0, 3.0, 5.0)], log=True, **kw)
    assert st == st_ref  # the same paths
    assert not log_ref.any() and log.any()  # (without medium numbers no triangle names one)
    assert (img[:, :3] <= ref[:, :3]).all()
    assert (img[:, :3] < ref[:, :3]).any()
    untouched = log == 0
    assert untouched.any() and mu.same(img[untouched], ref[untouched])
    assert (img[~untouched, :3] < ref[~untouched, :3]).any()


def test_weights_steer_russian_roulette(emu, cornell):
    """With the default Russian roulette the attenuated weight enters q: a strong absorber ends paths earlier."""
    glass = mu.glass_instances(cornell)
    _, st_ref = emu.scene(cornell).render(32, 32, 2)
    _, st = emu.scene(mu.with_medium(cornell, glass, 1)).render(32, 32, 2, media=[(50.0, 50.0, 50.0)])
    assert st["extension_rays"] < st_ref["extension_rays"]


def test_set_media_validation(emu):
    assert emu.check(None) is None and emu.check([]) is None
    assert emu.check([(0.0, 0.0, 0.0), (250.0, 1000.0, 1000.0)]) is None
    for bad in ([(-1.0, 0, 0)], [(0, float("nan"), 0)], [(0, 0, float("inf"))], [(-0.0, 1.0, 1.0), (1.0, 1.0, -1e-30)]):
        assert "finite and >= 0" in emu.check(bad)
    assert emu.check([(1.0, 1.0, 1.0)] * 4095) is None
    assert "4095" in emu.check([(1.0, 1.0, 1.0)] * 4096)


def test_a_medium_number_above_the_count_is_refused(emu, cornell):
    sc = mu.with_medium(cornell, mu.glass_instances(cornell), 2)
    s = emu.scene(sc)
    assert emu.L.media_emu_max_number(s.h) == 2
    with pytest.raises(ValueError):
        s.render(8, 8, 1, media=[(1.0, 1.0, 1.0)])
    with pytest.raises(ValueError):
        s.render(8, 8, 1)
