"""The device functions of pt_lightgrid.h on the GPU (tests/devfn/lightgrid_devfn.hip) against the host compile of the same bodies
(tests/devfn/lightgrid_bodies.h through tests/emu/lightgrid_emu.cpp), word for word: the cell lookup, the pick and the emitter-hit
pdf over a few thousand positions and draws -- cell faces, points outside the box, NaN and infinities among them."""
import numpy as np
import pytest

import lightgrid_util as gu
import lights_util as lu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emu():
    return gu.GridEmu()


@pytest.fixture(scope="module")
def dev():
    return gu.GridDevice()


def _cases(emu):
    """(name, scene, Grid, delta): the 40-light room at 8 x 2 x 8, the 3-light room at 5 x 1 x 3 with two delta lights, and the floor
    under 16 lights at 8 x 2 x 8."""
    from gpuspectral_amd import abi

    delta = [abi.point_light((0.3, 1.2, 0.2), (0.8, 0.7, 0.5)), abi.directional_light((0.0, -0.8, 0.6), (0.3, 0.3, 0.4), 2.0)]
    out = []
    for name, sc, res, d in (("room 40", lu.room_scene(40), (8, 2, 8), None), ("room 3 + delta", lu.room_scene(3), (5, 1, 3), delta),
                             ("floor", gu.floor_under_lights(equal=True, area=1e-2), (8, 2, 8), None)):
        b = emu.scene(sc).bounds()
        out.append((name, sc, b, emu.build(b, res, sc.lights, d)))
    return out


@pytest.fixture(scope="module")
def cases(emu):
    return _cases(emu)


def test_device_harness_is_the_trees():
    assert gu.devfn_stamped_digest(gu.devfn_ensure_built()) == gu.devfn_source_digest()


def test_cell_lookup(emu, dev, cases):
    for name, _, b, g in cases:
        pos = gu.probe_positions(b, g.res, random=3000)
        hc, hx = emu.cell(g, pos)
        dc, dx = dev.cell(g, pos)
        assert np.array_equal(hc, dc) and np.array_equal(hx, dx), name
        assert (hc == gu.NO_CELL).sum() > 100 and (hc != gu.NO_CELL).sum() > 100, name
        assert len(np.unique(hc)) > g.cells // 2, name


def test_pick(emu, dev, cases):
    rng = np.random.RandomState(9)
    for name, _, b, g in cases:
        pos = gu.probe_positions(b, g.res, random=3000)
        r = rng.randint(0, 2 ** 32, len(pos), dtype=np.uint64).astype(np.uint32)
        r[:4] = (0, 1, 0xFFFFFFFF, 0x80000000)
        hk, hp = emu.pick(g, pos, r)
        dk, dp = dev.pick(g, pos, r)
        assert np.array_equal(hk, dk) and np.array_equal(hp.view(np.uint32), dp.view(np.uint32)), name
        assert (hk < g.n).all()


def test_hit_pmf(emu, dev, cases):
    """The hit triangles: the scene's own light triangles (what a ray can hit), and among them one of zero area, one of NaN emission
    and one seen from behind."""
    rng = np.random.RandomState(4)
    for name, sc, b, g in cases:
        pos = gu.probe_positions(b, g.res, random=3000)
        li = rng.randint(0, len(sc.lights), len(pos))
        tris = np.concatenate([sc.lights["positions"][li][:, :, :3].reshape(-1, 9), sc.lights["radiance"][li][:, :3]], 1).astype(np.float32)
        tris[0, 3:9] = tris[0, 0:3].tolist() * 2  # no area
        tris[1, 9] = np.nan
        tris[2, 3:6], tris[2, 6:9] = tris[2, 6:9].copy(), tris[2, 3:6].copy()  # turned round
        h = emu.hit_pmf(g, pos, tris)
        d = dev.hit_pmf(g, pos, tris)
        assert np.array_equal(h.view(np.uint32), d.view(np.uint32)), name
        assert np.isfinite(h).all() and (h >= 0.0).all() and (h > 0.0).sum() > len(h) // 2, name
