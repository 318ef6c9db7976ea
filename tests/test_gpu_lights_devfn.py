"""sample_light_power (gpuspectral_amd/csrc/pt_shading.h) on the GPU against its host compile, vector by vector, the way
tests/test_gpu_devfn.py holds the other device functions: the same body (tests/devfn/lights_bodies.h) compiled for gfx950
(tests/devfn/lights_devfn.hip) and by g++ (tests/emu/lights_emu.cpp), compared word for word."""
import numpy as np
import pytest

import lights_util as lu

pytestmark = pytest.mark.gpu

N = 4096


def _vectors(lights, seed):
    rng = np.random.RandomState(seed)
    pos = rng.uniform(-1.0, 1.0, (N, 3)).astype(np.float32) * np.float32([1.0, 1.0, 1.0]) + np.float32([0.0, 0.9, 0.0])
    pos[:16] = lights["positions"][np.arange(16) % len(lights), 0, :3]  # in a light's own plane, at its corner: grazing cosines and tiny distances
    seeds = rng.randint(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32)
    seeds[:4] = (0, 1, 0xFFFFFFFF, 0x80000000)
    return pos, seeds


@pytest.mark.parametrize("n", [1, 3, 130])
def test_sample_light_power_gpu_equals_host(n):
    emu, dev = lu.LightsEmu(), lu.LightsDevice()
    lights = lu.room_scene(n).lights
    pos, seeds = _vectors(lights, 17 + n)
    want, table = emu.devfn_power(lights, pos, seeds)
    got, table_dev = dev.devfn_power(lights, pos, seeds)
    assert table.tobytes() == table_dev.tobytes() == emu.build(lights).tobytes()
    bad = np.flatnonzero((want != got).any(1))
    assert len(bad) == 0, "%d of %d vectors differ (first: %d: host %s, device %s)" % (len(bad), N, bad[0], want[bad[0]], got[bad[0]])
    if n > 1:
        assert len(np.unique(want[:, 6])) > N // 2  # (the vectors do reach many lights and pdfs)


def test_the_harness_carries_the_tree_digest():
    assert lu.devfn_stamped_digest(lu.devfn_ensure_built()) == lu.devfn_source_digest()
