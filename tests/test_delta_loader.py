"""LoadOptions::readEmitters without a GPU: top-level point / spot / directional emitters become Scene::deltaLights; without the option
the loader is what it was, warning included."""
import math
import os

import numpy as np

from test_media_loader import same_scene_bytes

HEAD = """<?xml version="1.0" encoding="utf-8"?>
<scene version="0.5.0">
  <sensor type="perspective">
    <float name="fov" value="35"/>
    <transform name="toWorld"><matrix value="-1 0 0 0 0 1 0 1 0 0 -1 6.8 0 0 0 1"/></transform>
  </sensor>
  <bsdf type="diffuse" id="Grey"><rgb name="reflectance" value="0.6, 0.6, 0.6"/></bsdf>
  <shape type="rectangle">
    <transform name="toWorld"><matrix value="3 0 0 1 0 0 3 0 0 -3 0 2 0 0 0 1"/></transform>
    <ref id="Grey"/>
  </shape>
"""
# the floor: rect.obj (|x|, |y| <= 1, z = 0) under that matrix: x in [-2, 4], y = 0, z in [-1, 5]: half the diagonal = sqrt(72) / 2
FLOOR_EXTENT = math.sqrt(72.0) / 2.0

DEFAULTS = HEAD + """
  <emitter type="point"><point name="position" x="0.5" y="2" z="-1"/><rgb name="intensity" value="10, 20, 30"/></emitter>
  <emitter type="spot">
    <transform name="toWorld"><matrix value="1 0 0 0.25 0 0 -1 3 0 1 0 0.5 0 0 0 1"/></transform>
    <rgb name="intensity" value="5, 5, 5"/>
  </emitter>
  <emitter type="directional"><vector name="direction" x="0" y="-2" z="0"/><rgb name="irradiance" value="1, 2, 3"/></emitter>
  <emitter type="constant"><rgb name="radiance" value="1, 1, 1"/></emitter>
</scene>
"""

TO_WORLD = HEAD + """
  <emitter type="point">
    <transform name="toWorld"><matrix value="1 0 0 0.5 0 1 0 2 0 0 1 -1 0 0 0 1"/></transform>
    <rgb name="intensity" value="10, 20, 30"/>
  </emitter>
  <emitter type="point">
    <transform name="toWorld"><matrix value="1 0 0 9 0 1 0 9 0 0 1 9 0 0 0 1"/></transform>
    <point name="position" x="0.5" y="2" z="-1"/>
    <rgb name="intensity" value="10, 20, 30"/>
  </emitter>
  <emitter type="directional">
    <transform name="toWorld"><matrix value="1 0 0 0 0 0 -1 0 0 1 0 0 0 0 0 1"/></transform>
    <rgb name="irradiance" value="1, 2, 3"/>
  </emitter>
</scene>
"""

SCALE = HEAD + """
  <emitter type="point"><point name="position" x="0.5" y="2" z="-1"/><rgb name="intensity" value="10, 20, 30"/><float name="scale" value="0.5"/></emitter>
  <emitter type="spot">
    <transform name="toWorld"><matrix value="1 0 0 0.25 0 0 -1 3 0 1 0 0.5 0 0 0 1"/></transform>
    <rgb name="intensity" value="5, 5, 5"/><float name="scale" value="4"/>
    <float name="cutoffAngle" value="40"/><float name="beamWidth" value="10"/>
  </emitter>
  <emitter type="directional"><vector name="direction" x="3" y="0" z="-4"/><rgb name="irradiance" value="1, 2, 3"/><float name="scale" value="2"/></emitter>
</scene>
"""


def write_xml(dirpath, text, name="emitters.xml"):
    path = os.path.join(str(dirpath), name)
    with open(path, "w") as fh:
        fh.write(text)
    return path


def fields(l):
    return dict(position=list(l.position), kind=l.kind, direction=list(l.direction), cos_cutoff=l.cos_cutoff, intensity=list(l.intensity),
                cos_beam=l.cos_beam, extent=l.extent, reserved=list(l.reserved))


def f32(x):
    return float(np.float32(x))


def test_defaults(tmp_path):
    from gpuspectral_amd import abi, host

    sc = host.Scene(write_xml(tmp_path, DEFAULTS), read_emitters=True)
    p, s, d = [fields(l) for l in sc.delta_lights]
    assert p == dict(position=[0.5, 2.0, -1.0], kind=abi.LIGHT_POINT, direction=[0, 0, 0], cos_cutoff=0.0, intensity=[10, 20, 30], cos_beam=0.0, extent=0.0,
                     reserved=[0, 0, 0])
    # the spot: position = the translation, axis = the image of +z = (0, -1, 0); cutoff 20 degrees, beam 3 / 4 of it
    assert s["position"] == [0.25, 3.0, 0.5] and s["kind"] == abi.LIGHT_SPOT and s["direction"] == [0.0, -1.0, 0.0] and s["intensity"] == [5, 5, 5]
    assert s["cos_cutoff"] == f32(math.cos(math.radians(20.0))) and s["cos_beam"] == f32(math.cos(math.radians(15.0)))
    assert d["kind"] == abi.LIGHT_DIRECTIONAL and d["direction"] == [0.0, -1.0, 0.0] and d["intensity"] == [1, 2, 3]
    assert d["extent"] == f32(FLOOR_EXTENT)
    # another emitter type keeps today's warning, and the three that were read lose theirs
    plain = host.Scene(write_xml(tmp_path, DEFAULTS))
    warn = "top-level emitter (envmap) ignored, as in the reference (Loader.cpp:338-346)"
    assert plain.warnings.count(warn) == 4 and sc.warnings.count(warn) == 1
    # the library accepts what the loader made
    from delta_util import DeltaEmu

    assert DeltaEmu().check(sc.delta_lights)[0] is None


def test_to_world_against_position(tmp_path):
    from gpuspectral_amd import host

    a = host.Scene(write_xml(tmp_path, DEFAULTS), read_emitters=True).delta_lights
    b = host.Scene(write_xml(tmp_path, TO_WORLD, "b.xml"), read_emitters=True).delta_lights
    assert fields(b[0]) == fields(a[0])  # the translation of toWorld is the position
    assert fields(b[1]) == fields(a[0])  # ... and an explicit position wins
    assert fields(b[2]) == fields(a[2])  # the image of +z is the direction


def test_scale_and_the_spot_angles(tmp_path):
    from gpuspectral_amd import host

    p, s, d = [fields(l) for l in host.Scene(write_xml(tmp_path, SCALE), read_emitters=True).delta_lights]
    assert p["intensity"] == [5, 10, 15] and s["intensity"] == [20, 20, 20] and d["intensity"] == [2, 4, 6]
    assert s["cos_cutoff"] == f32(math.cos(math.radians(40.0))) and s["cos_beam"] == f32(math.cos(math.radians(10.0)))
    assert d["direction"] == [f32(0.6), 0.0, f32(-0.8)]


def test_without_the_option_the_loader_is_what_it_was(tmp_path, living_room_xml):
    from gpuspectral_amd import host

    xml = write_xml(tmp_path, DEFAULTS)
    plain = host.Scene(xml)
    assert plain.delta_lights == []
    on = host.Scene(xml, read_emitters=True)
    assert same_scene_bytes(plain.arrays(), on.arrays())
    a, b = host.Scene(living_room_xml), host.Scene(living_room_xml, read_emitters=True)
    assert same_scene_bytes(a.arrays(), b.arrays()) and a.warnings == b.warnings and b.delta_lights == []


def test_set_delta_lights_round_trip(tmp_path):
    from gpuspectral_amd import abi, host

    sc = host.Scene(write_xml(tmp_path, HEAD + "</scene>\n"))
    assert sc.delta_lights == []
    sc.set_delta_lights([abi.point_light((1, 2, 3), (4, 5, 6))])
    assert [fields(l) for l in sc.delta_lights] == [fields(abi.point_light((1, 2, 3), (4, 5, 6)))]
    sc.set_delta_lights(None)
    assert sc.delta_lights == []
