"""LoadOptions::readScattering without a GPU: sigmaS, or sigmaT with albedo, and the <phase> child of a shape's interior medium
become Scene::mediaScattering, parallel to Scene::media; the option implies readMedia; without it the loader is what it was."""
import os

import numpy as np

from test_media_loader import medium_numbers, same_scene_bytes, write_media_xml

SCATTER_XML = """<?xml version="1.0" encoding="utf-8"?>
<scene version="0.5.0">
  <sensor type="perspective">
    <float name="fov" value="35"/>
    <transform name="toWorld"><matrix value="-1 0 0 0 0 1 0 1 0 0 -1 6.8 0 0 0 1"/></transform>
  </sensor>
  <bsdf type="diffuse" id="Grey"><rgb name="reflectance" value="0.6, 0.6, 0.6"/></bsdf>
  <bsdf type="dielectric" id="Glass"><float name="intIOR" value="1.5"/><float name="extIOR" value="1"/></bsdf>
  <medium type="homogeneous" id="Milk">
    <rgb name="sigmaT" value="4, 4, 8"/>
    <rgb name="albedo" value="0.5, 0.75, 1"/>
    <float name="scale" value="0.5"/>
    <phase type="hg"><float name="g" value="0.6"/></phase>
  </medium>
  <shape type="rectangle">
    <transform name="toWorld"><matrix value="3 0 0 0 0 0 3 0 0 -3 0 0 0 0 0 1"/></transform>
    <ref id="Grey"/>
  </shape>
  <shape type="rectangle">
    <transform name="toWorld"><matrix value="0.5 0 0 0 0 0 -0.5 2.5 0 0.5 0 0 0 0 0 1"/></transform>
    <ref id="Grey"/>
    <emitter type="area"><rgb name="radiance" value="17, 12, 4"/></emitter>
  </shape>
  <shape type="cube">
    <transform name="toWorld"><matrix value="0.3 0 0 -1.2 0 0.3 0 0.31 0 0 0.3 0 0 0 0 1"/></transform>
    <ref id="Glass"/>
    <medium type="homogeneous" name="interior"><rgb name="sigmaS" value="1, 2, 4"/><rgb name="sigmaA" value="1, 2, 3"/></medium>
  </shape>
  <shape type="cube">
    <transform name="toWorld"><matrix value="0.3 0 0 -0.4 0 0.3 0 0.31 0 0 0.3 0 0 0 0 1"/></transform>
    <ref id="Glass"/>
    <ref name="interior" id="Milk"/>
  </shape>
  <shape type="cube">
    <transform name="toWorld"><matrix value="0.3 0 0 0.4 0 0.3 0 0.31 0 0 0.3 0 0 0 0 1"/></transform>
    <ref id="Glass"/>
    <medium type="homogeneous" name="interior"><rgb name="sigmaA" value="1, 2, 3"/></medium>
  </shape>
  <shape type="cube">
    <transform name="toWorld"><matrix value="0.3 0 0 1.2 0 0.3 0 0.31 0 0 0.3 0 0 0 0 1"/></transform>
    <ref id="Glass"/>
    <medium type="homogeneous" name="interior">
      <rgb name="sigmaS" value="1, 2, 4"/><rgb name="sigmaA" value="1, 2, 3"/>
      <phase type="rayleigh"/>
    </medium>
  </shape>
  <shape type="cube">
    <transform name="toWorld"><matrix value="0.2 0 0 0 0 0.2 0 0.21 0 0 0.2 1.2 0 0 0 1"/></transform>
    <ref id="Glass"/>
    <medium type="homogeneous" name="interior">
      <rgb name="sigmaS" value="1, 2, 4"/><rgb name="sigmaA" value="1, 2, 3"/>
      <phase type="isotropic"/>
    </medium>
  </shape>
</scene>
"""


def write_scatter_xml(dirpath):
    path = os.path.join(str(dirpath), "scatter_scene.xml")
    with open(path, "w") as fh:
        fh.write(SCATTER_XML)
    return path


def test_inline_ref_sigma_t_albedo_hg_and_an_unknown_phase(tmp_path):
    from gpuspectral_amd import host

    xml = write_scatter_xml(tmp_path)
    sc = host.Scene(xml, read_scattering=True)
    # inline sigmaS + sigmaA (no phase: g = 0); <ref> to sigmaT (4, 4, 8), albedo (0.5, 0.75, 1), scale 0.5, hg 0.6; a pure absorber
    assert sc.media.tolist() == [[1.0, 2.0, 3.0], [1.0, 0.5, 0.0], [1.0, 2.0, 3.0]]
    assert np.array_equal(sc.media_scattering, np.float32([[1, 2, 4, 0], [1, 1.5, 4, 0.6], [0, 0, 0, 0]]))
    # floor, light, inline, <ref>, the absorber (an entry of its own: its pair differs), rayleigh and isotropic (both share the inline entry)
    assert medium_numbers(sc.arrays()).tolist() == [0, 0, 1, 2, 3, 1, 1]
    plain = host.Scene(xml)
    new = [w for w in sc.warnings if w not in plain.warnings]
    assert new == ["unsupported phase function 'rayleigh' replaced by isotropic"]
    assert sc.add_scattering_medium((1, 0.5, 0), (1, 1.5, 4), 0.6) == 2 and sc.add_medium((1, 2, 3)) == 3
    assert sc.add_scattering_medium((1, 0.5, 0), (1, 1.5, 4), 0.5) == 4 and len(sc.media_scattering) == 4


def test_without_the_option_the_loader_is_what_it_was(tmp_path):
    from gpuspectral_amd import host

    xml = write_scatter_xml(tmp_path)
    plain, media = host.Scene(xml), host.Scene(xml, read_media=True)
    assert len(plain.media) == 0 and len(plain.media_scattering) == 0 and not medium_numbers(plain.arrays()).any()
    assert media.media.tolist() == [[1.0, 2.0, 3.0]] and len(media.media_scattering) == 0
    assert medium_numbers(media.arrays()).tolist() == [0, 0, 0, 0, 1, 0, 0]
    assert sum("scattering medium skipped" in w for w in media.warnings) == 4


def test_read_scattering_implies_read_media_and_keeps_the_absorbers(tmp_path):
    """The scene of test_media_loader.py: its one scattering medium is no longer skipped; everything else is what readMedia reads."""
    from gpuspectral_amd import host

    xml = write_media_xml(tmp_path)
    a, b = host.Scene(xml, read_media=True), host.Scene(xml, read_scattering=True)
    assert b.media.tolist() == a.media.tolist() + [[1.0, 2.0, 3.0]]
    assert np.array_equal(b.media_scattering, np.float32([[0, 0, 0, 0], [0, 0, 0, 0], [1, 1, 1, 0]]))
    assert medium_numbers(b.arrays()).tolist() == [0, 0, 1, 2, 1, 3, 0, 0]
    assert [w for w in a.warnings if w not in b.warnings] == ["scattering medium skipped (sigmaS / albedo != 0: only pure absorbers are supported)"]
    assert [w for w in b.warnings if w not in a.warnings] == []


def test_reference_scenes_are_unchanged_by_the_option(living_room_xml, staircase2_xml):
    from gpuspectral_amd import host

    for xml in (living_room_xml, staircase2_xml):
        a, b = host.Scene(xml, read_media=True), host.Scene(xml, read_scattering=True)
        assert same_scene_bytes(a.arrays(), b.arrays()) and np.array_equal(a.media, b.media)
        assert len(b.media_scattering) == 0 and a.warnings == b.warnings
