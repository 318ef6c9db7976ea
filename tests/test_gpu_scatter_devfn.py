"""sample_hg, hg_pdf and medium_event (gpuspectral_amd/csrc/pt_medium.h) on the GPU against their host compile, vector by vector,
the way tests/test_gpu_lights_devfn.py holds sample_light_power: the same bodies (tests/devfn/medium_bodies.h) compiled for gfx950
(tests/devfn/medium_devfn.hip) and by g++ (tests/emu/scatter_emu.cpp), compared word for word on the vectors of
tests/test_scatter_cpu.py."""
import numpy as np
import pytest

import scatter_util as su

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def both():
    return su.ScatterEmu(), su.MediumDevice()


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def test_sample_hg_and_hg_pdf_gpu_equal_host(both):
    emu, dev = both
    v = [np.concatenate(x) for x in zip(*[su.hg_vectors(g) for g in su.HG_GS])]
    want, got = emu.sample_hg(*v), dev.sample_hg(*v)
    bad = np.flatnonzero((want[0].view(np.uint32) != got[0].view(np.uint32)).any(1) | (want[1].view(np.uint32) != got[1].view(np.uint32)))
    assert len(bad) == 0, "%d of %d vectors differ (first: %d: host %s %s, device %s %s)" % (len(bad), len(v[1]), bad[0], want[0][bad[0]], want[1][bad[0]],
                                                                                             got[0][bad[0]], got[1][bad[0]])
    cos = (1.0 - 2.0 * v[2].astype(np.float64)).astype(np.float32)
    assert _same(emu.hg_pdf(v[1], cos), dev.hg_pdf(v[1], cos))


def test_medium_event_gpu_equals_host(both):
    emu, dev = both
    v = su.event_vectors()
    want, got = emu.medium_event(*v), dev.medium_event(*v)
    bad = np.flatnonzero((want.view(np.uint32) != got.view(np.uint32)).any(1))
    assert len(bad) == 0, "%d of %d vectors differ (first: %d: host %s, device %s)" % (len(bad), len(want), bad[0], want[bad[0]], got[bad[0]])
    assert (want[:, 0] == 1).any() and (want[:, 0] == 0).any()


def test_the_harness_carries_the_tree_digest():
    assert su.devfn_stamped_digest(su.devfn_ensure_built()) == su.devfn_source_digest()
