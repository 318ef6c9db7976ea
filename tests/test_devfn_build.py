"""The test-only device harness (tests/devfn) as it is shipped, checked without a GPU: it is the tree's, it is compiled as the
product is, it exports what the helper declares, and it refuses every out-of-range index on the host before anything is launched."""

import numpy as np
import pytest

import devfn_util


@pytest.fixture(scope="module")
def dev():
    return devfn_util.device()


def test_library_exports_what_the_helper_declares(dev):
    for k in devfn_util.SIGNATURES:
        assert hasattr(dev.L, "devfn_" + k), k
    for k in devfn_util.EXTRA_EXPORTS:
        assert hasattr(dev.L, k), k
    with open(dev.path, "rb") as fh:  # never linked against (or naming) the product library
        assert b"libgpuspectral_pt" not in fh.read()


def test_library_is_compiled_as_the_product_is(dev):
    import gpuspectral_amd as g

    info = devfn_util.build_info(dev)
    prod = g.pt.build_info()
    assert info["flags"] == prod["flags"] == devfn_util.product_flags()
    assert info["arch"] == prod["arch"] == "gfx950"
    assert info["digest"] == devfn_util.source_digest()
    assert devfn_util.stamped_info(dev.path) == info
    # the layout the helper computes is the one the library uses
    num = np.array([3, 0, 5, 1, 7, 2, 65536, 4], np.uint32)
    q, r = np.zeros(8, np.uint64), np.zeros(8, np.uint64)
    total = dev.L.devfn_table_layout(num.ctypes.data, q.ctypes.data, r.ctypes.data)
    assert (list(q), list(r), total) == dev.table_layout(num)
    assert all(int(x) % 16 == 0 for x in r)


def _refused(call):
    with pytest.raises(devfn_util.DevfnError) as e:
        call()
    assert e.value.code == devfn_util.BAD_INDEX


def test_out_of_range_indices_are_refused_before_any_launch(dev):
    from gpuspectral_amd import abi

    before = dev.L.devfn_run_count()
    bsdfs = [np.zeros(2, dt) for dt in abi.BSDF_DTYPES]
    bsdfs[5] = np.zeros(0, abi.BSDF_DTYPES[5])
    wo = np.array([[0, 0, 1]], np.float32)
    for h in (abi.bsdf_handle(0, 2), abi.bsdf_handle(7, 0xFFFF), abi.bsdf_handle(5, 0), 8 << 16, 0xFFFF0000):
        _refused(lambda: dev.bsdf(bsdfs, [h], wo, [1], wo))  # record index, empty table, BSDF type
    lights = np.zeros(3, abi.LIGHT_DT)
    _refused(lambda: dev.lights(lights, wo, [1], num_lights=4))  # more lights than records
    tex = np.zeros(2, abi.TEXTURE_DT)
    tex[0], tex[1] = (2, 2, 0), (1, 1, 4)
    texels, dec, uv = np.zeros(5, np.uint32), np.zeros(256, np.float32), np.zeros((1, 2), np.float32)
    _refused(lambda: dev.texture(tex, texels, dec, [2], uv))  # texture id
    bad = tex.copy()
    bad[1] = (2, 1, 4)  # a texture that reaches past the texel array
    _refused(lambda: dev.texture(bad, texels, dec, [0], uv))
    bad[1] = (0, 1, 4)  # an empty texture (wrap_index would divide by zero)
    _refused(lambda: dev.texture(bad, texels, dec, [0], uv))
    _refused(lambda: dev.envmap(np.zeros(0, np.float32), 0, 0, np.eye(4, dtype=np.float32), wo))
    boxes = np.zeros((1, 4, 6), np.float32)
    for cnt in ((3, 2), (-1, 1), (0, 5)):
        _refused(lambda: dev.encode_nodes(boxes, [cnt]))  # child counts
    _refused(lambda: dev.node_tests(np.zeros((2, 16), np.uint32), [2], np.zeros((1, 8), np.float32)))  # node index
    assert dev.L.devfn_run_count() == before  # nothing got as far as a hipMalloc


def test_host_twins_refuse_the_same(emu):
    from gpuspectral_amd import abi

    hst = devfn_util.host(emu)
    bsdfs = [np.zeros(1, dt) for dt in abi.BSDF_DTYPES]
    wo = np.array([[0, 0, 1]], np.float32)
    _refused(lambda: hst.bsdf(bsdfs, [abi.bsdf_handle(3, 1)], wo, [1], wo))
    _refused(lambda: hst.lights(np.zeros(1, abi.LIGHT_DT), wo, [1], num_lights=2))
    _refused(lambda: hst.encode_nodes(np.zeros((1, 4, 6), np.float32), [(4, 1)]))
