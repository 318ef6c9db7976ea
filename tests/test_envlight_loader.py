"""LoadOptions::sampleEnvmap and the render program's --env-sampling without a GPU: the switch and the radius of the scene's bounds in
Scene::envmapSampling; without the option the loader is what it was; the option beside an explicit reference estimator is an error."""
import os
import subprocess

from conftest import ROOT
from test_delta_loader import FLOOR_EXTENT, HEAD, write_xml
from test_media_loader import same_scene_bytes

GSP_RENDER = os.path.join(ROOT, "gpuspectral_amd", "lib", "gsp_render")


def test_the_option_sets_the_switch_and_the_radius_of_the_bounds(tmp_path):
    from gpuspectral_amd import host

    xml = write_xml(tmp_path, HEAD + "</scene>\n")
    plain = host.Scene(xml)
    assert plain.envmap_sampling == (False, 0.0)
    on = host.Scene(xml, sample_envmap=True)
    enabled, extent = on.envmap_sampling
    assert enabled and abs(extent - FLOOR_EXTENT) < 1e-5
    assert same_scene_bytes(plain.arrays(), on.arrays()) and plain.warnings == on.warnings  # nothing else changes


def test_set_envmap_sampling_round_trip(tmp_path):
    from gpuspectral_amd import host

    sc = host.Scene(write_xml(tmp_path, HEAD + "</scene>\n"))
    sc.set_envmap_sampling(True, 2.5)
    assert sc.envmap_sampling == (True, 2.5)
    sc.set_envmap_sampling(False)
    assert sc.envmap_sampling[0] is False


def test_env_sampling_beside_an_explicit_reference_estimator_is_an_error(tmp_path):
    xml = write_xml(tmp_path, HEAD + "</scene>\n")
    out = subprocess.run([GSP_RENDER, "--estimator", "reference", "--env-sampling", xml, str(tmp_path / "o.pfm"), "8", "8", "1"], capture_output=True, text=True)
    assert out.returncode != 0 and "--env-sampling needs the textbook estimator" in out.stderr
    out = subprocess.run([GSP_RENDER, "--env-extent", "2", xml, str(tmp_path / "o.pfm"), "8", "8", "1"], capture_output=True, text=True)
    assert out.returncode != 0 and "--env-extent needs --env-sampling" in out.stderr
    out = subprocess.run([GSP_RENDER, "--env-sampling", "--env-extent", "0", xml, str(tmp_path / "o.pfm")], capture_output=True, text=True)
    assert out.returncode == 2 and "--env-extent R" in out.stderr
    usage = subprocess.run([GSP_RENDER], capture_output=True, text=True).stderr
    assert "[--env-sampling [--env-extent R]]" in usage
