"""spot_falloff and sample_delta_light (gpuspectral_amd/csrc/pt_deltalight.h) on the GPU against their host compile, vector by vector,
the way tests/test_gpu_scatter_devfn.py holds pt_medium.h: the same bodies (tests/devfn/delta_bodies.h) compiled for gfx950
(tests/devfn/delta_devfn.hip) and by g++ (tests/emu/delta_emu.cpp), compared word for word on the vectors of tests/test_delta_cpu.py."""
import numpy as np
import pytest

import delta_util as du

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def both():
    return du.DeltaEmu(), du.DeltaDevice()


def test_spot_falloff_gpu_equals_host(both):
    emu, dev = both
    v = du.falloff_vectors()
    want, got = emu.spot_falloff(*v), dev.spot_falloff(*v)
    bad = np.flatnonzero(want.view(np.uint32) != got.view(np.uint32))
    assert len(bad) == 0, "%d of %d vectors differ (first: %d: host %r, device %r)" % (len(bad), len(want), bad[0], want[bad[0]], got[bad[0]])


def test_sample_delta_light_gpu_equals_host(both):
    emu, dev = both
    v = du.sample_vectors()
    want, got = emu.sample_delta_light(*v), dev.sample_delta_light(*v)
    bad = np.flatnonzero((want.view(np.uint32) != got.view(np.uint32)).any(1))
    assert len(bad) == 0, "%d of %d vectors differ (first: %d: host %s, device %s)" % (len(bad), len(want), bad[0], want[bad[0]], got[bad[0]])
    assert (want[:, 7] == 0).any() and np.isinf(want[:, 7]).any()


def test_the_harness_carries_the_tree_digest():
    assert du.devfn_stamped_digest(du.devfn_ensure_built()) == du.devfn_source_digest()
