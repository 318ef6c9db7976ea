"""The device functions of pt_envlight.h on the GPU (tests/devfn/envlight_devfn.hip) against the host compile of the same bodies
(tests/emu/envlight_emu.cpp), bit for bit: the shared radiance-and-density function and the sampler, with the poles, u at the wrap,
NaN directions and a 1 x 1 map."""
import numpy as np
import pytest

import envlight_util as eu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sides():
    return eu.EnvEmu(), eu.EnvDevice()


def directions(n=20000, seed=4):
    """World directions: random unit vectors; the map's poles and the wrap of u (local -z side, x = +-0), exact and a hair beside; not
    normalised, zero, huge and NaN vectors."""
    rng = np.random.RandomState(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    A = eu.rot3(eu.TO_LOCAL)
    special = np.array([[0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1e-8, 0, 1], [-1e-8, 0, 1], [1e-8, 1, 0], [0, 1, 1e-20], [1, 0, 0], [-1, 0, 0]], np.float64)
    d[:len(special)] = special @ A  # (local -> world: the product applies to_local to these)
    d = d.astype(np.float32)
    d[20] = (0.0, 0.0, 0.0)
    d[21] = (np.nan, 0.3, 0.1)
    d[22] = (np.nan, np.nan, np.nan)
    d[23] = (3e19, -3e19, 1e19)
    d[24] = (np.inf, 0.0, 1.0)
    d[25:45] *= np.float32(7.5)
    return d


@pytest.mark.parametrize("size", eu.MAP_SIZES, ids=lambda s: "%dx%d" % s)
def test_env_eval_matches_the_host_bit_for_bit(sides, size):
    emu, dev = sides
    env = eu.random_map(*size)
    cw, ch, table, _ = emu.cells(env)
    for to_local in (eu.TO_LOCAL, np.eye(4, dtype=np.float32).ravel()):  # (identity: the special directions hit the poles and the wrap exactly)
        rec = emu.record(to_local, cw, ch, 0.25)
        d = directions()
        host, device = emu.env_eval(env, to_local, table, rec, d), dev.env_eval(env, to_local, table, rec, d)
        for a, b in zip(host, device):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert (host[2] < cw * ch).all()


@pytest.mark.parametrize("size", eu.MAP_SIZES, ids=lambda s: "%dx%d" % s)
def test_sample_env_light_matches_the_host_bit_for_bit(sides, size):
    emu, dev = sides
    env = eu.random_map(*size)
    cw, ch, table, _ = emu.cells(env)
    rec = emu.record(eu.TO_LOCAL, cw, ch, 0.25)
    rng = np.random.RandomState(8)
    n = 20000
    r2 = rng.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    e1, e2 = rng.uniform(0, 1, n).astype(np.float32), rng.uniform(0, 1, n).astype(np.float32)
    r2[:4] = (0, 0xFFFFFFFF, 0x80000000, 1)
    e1[:8] = (0.0, 0.0, np.float32(1.0) - np.float32(2.0 ** -24), np.float32(1.0) - np.float32(2.0 ** -24), 0.5, 0.5, 0.0, 0.25)  # the wrap and the cell borders
    e2[:8] = (0.0, np.float32(1.0) - np.float32(2.0 ** -24), 0.0, np.float32(1.0) - np.float32(2.0 ** -24), 0.0, 0.5, 0.5, 0.0)   # the poles
    host = emu.sample_env_light(env, eu.TO_LOCAL, table, rec, (r2, e1, e2))
    device = dev.sample_env_light(env, eu.TO_LOCAL, table, rec, (r2, e1, e2))
    for a, b in zip(host, device):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
