"""Feature buffers on the GPU (include/gpuspectral_pt.h, "Feature buffers"): gsp_render_features / gsp_download_features against
the host emulation of the same code (tests/emu/features_emu.cpp, itself checked against an independent composition in
tests/test_features_cpu.py) -- bit for bit, all three planes."""
import copy
import subprocess
import sys

import numpy as np
import pytest

import features_util as fu
import textured
from conftest import ROOT

pytestmark = pytest.mark.gpu

TENT = 2
LENS = dict(radius=0.08, focus_distance=5.0, blades=0, rotation=0.0)
CAMERAS = {"pinhole": (0, None), "tent": (TENT, None), "lens": (0, LENS), "tent+lens": (TENT, LENS)}
FRAMES = {"cornell": (96, 64), "cornell-odd": (33, 17), "materials": (96, 80), "textured": (64, 48)}


@pytest.fixture(scope="module")
def femu():
    return fu.FeaturesEmu()


@pytest.fixture(scope="module")
def scenes_(cornell, materials_scene):
    return {"cornell": cornell, "cornell-odd": cornell, "materials": materials_scene,
            "textured": textured.decorate(copy.deepcopy(materials_scene), seed=5, envmap=False)}


@pytest.fixture(scope="module")
def rigs(femu, scenes_):
    """Per scene: one context with the scene uploaded and the emulation's scene, shared by the cases below."""
    import gpuspectral_amd as g

    made = {}

    def get(name):
        if name not in made:
            ctx = g.Context(0)
            ctx.upload_scene(scenes_[name])
            made[name] = (ctx, femu.scene(scenes_[name]))
        return made[name]

    yield get
    for ctx, _ in made.values():
        ctx.close()


def set_lens(ctx, lens):
    ctx.set_lens(**(lens or {}))


def assert_planes(got, want, what=""):
    for name, a, b in zip(("albedo", "geom", "ids"), got, want):
        assert fu.same(a, b), "%s %s: %d of %d words differ" % (what, name, int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum()), a.size)


@pytest.mark.parametrize("camera", list(CAMERAS))
@pytest.mark.parametrize("scene", list(FRAMES))
def test_download_equals_the_emulation(rigs, scene, camera):
    ctx, emu = rigs(scene)
    w, h = FRAMES[scene]
    filt, lens = CAMERAS[camera]
    set_lens(ctx, lens)
    try:
        for spp in (1, 5):
            for t0 in (0, 5):
                ctx.frame_begin(w, h)
                ctx.render_features(spp, t0, pixel_filter=filt)
                want = fu.full(emu.render(w, h, spp, lens=lens, first_timestamp=t0, pixel_filter=filt), w, h)
                assert_planes(ctx.download_features(), want, "%s %s spp %d t0 %d" % (scene, camera, spp, t0))
                assert (want[2][..., 3] == spp).all()
    finally:
        set_lens(ctx, None)


def test_five_samples_equal_two_plus_three_and_frame_begin_clears(rigs):
    ctx, emu = rigs("cornell")
    w, h = FRAMES["cornell"]
    ctx.frame_begin(w, h)
    ctx.render_features(5, 0, pixel_filter=TENT)
    whole = ctx.download_features()
    ctx.frame_begin(w, h)
    cleared = ctx.download_features()
    assert not any(p.any() for p in cleared), "gsp_frame_begin clears the planes"
    ctx.render_features(2, 0, pixel_filter=TENT)
    ctx.render_features(3, 2, pixel_filter=TENT)
    assert_planes(ctx.download_features(), whole)
    a, _, i = ctx.download_features(geom=False)  # a NULL pointer is skipped
    assert _ is None and fu.same(a, whole[0]) and np.array_equal(i, whole[2])


def test_two_pixel_id_shares_reassemble_the_frame(rigs):
    ctx, emu = rigs("cornell")
    w, h = 33, 17
    want = fu.full(emu.render(w, h, 3, pixel_filter=TENT), w, h)
    ids = np.arange(w * h, dtype=np.uint32)
    total = [np.zeros_like(p) for p in want]
    for share in (ids[ids % 3 == 0], ids[ids % 3 != 0]):
        ctx.frame_begin(w, h, pixel_ids=share)
        ctx.render_features(3, 0, pixel_filter=TENT)
        got = ctx.download_features()
        mask = np.zeros(w * h, bool)
        mask[share] = True
        for t, p in zip(total, got):
            assert not p.reshape(-1, 4)[~mask].any(), "unowned pixels are 0"
            t += p
    assert_planes(total, want)


def test_two_lanes(scenes_, rigs):
    import gpuspectral_amd as g

    _, emu = rigs("materials")
    w, h = 33, 17
    with g.Context(0, lanes=2) as ctx:
        ctx.upload_scene(scenes_["materials"])
        ctx.frame_begin(w, h)
        ctx.render_features(3, 0, pixel_filter=TENT)
        assert_planes(ctx.download_features(), fu.full(emu.render(w, h, 3, pixel_filter=TENT), w, h))


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
def test_multi_equals_the_single_context(scenes_, rigs, devices):
    import gpuspectral_amd as g

    _, emu = rigs("materials")
    w, h = 96, 80
    with g.MultiContext(devices) as m:
        m.upload_scene(scenes_["materials"])
        m.set_lens(**LENS)
        m.frame_begin(w, h)
        m.render_features(3, 0, pixel_filter=TENT)
        assert_planes(m.download_features(), fu.full(emu.render(w, h, 3, lens=LENS, pixel_filter=TENT), w, h))


def test_beauty_frame_is_untouched_by_a_feature_call(scenes_):
    """Image, pixel statistics and the memo counters of a frame, with and without a feature call between its render calls."""
    import gpuspectral_amd as g

    w, h = 96, 64
    out = []
    for with_features in (False, True):
        for adaptive in (False, True):
            with g.Context(0) as ctx:
                ctx.upload_scene(scenes_["cornell"])
                ctx.frame_begin(w, h)
                kw = dict(adaptive_threshold=0.05, adaptive_min_spp=4, adaptive_step=4) if adaptive else {}
                ctx.render(4, 0, **kw)
                if with_features:
                    ctx.render_features(2, 0, pixel_filter=TENT)
                ctx.render(4, 4, **kw)
                img = ctx.download()
                st = ctx.stats()
                rec = [img, np.array([st["memoised_rays"], st["memo_build_rays"], st["extension_rays"], st["shadow_rays"], st["samples"]])]
                if adaptive:
                    rec += list(ctx.pixel_stats())
                out.append(rec)
    for plain, feat in zip(out[:2], out[2:]):
        for a, b in zip(plain, feat):
            assert fu.same(a, b) if a.dtype == np.float32 else np.array_equal(a, b)


def test_features_after_an_instance_edit_with_samples_in_flight(scenes_, femu):
    """gsp_update_instances moves one box while samples are in flight (the library may split the scene into two trees, refit into
    its ring or drain: scene_splits is printed): the features are those of a fresh upload of the edited scene."""
    import gpuspectral_amd as g

    sc = scenes_["cornell"]
    w, h = 96, 64
    inst = sc.instances.copy()
    k = int(np.flatnonzero(inst["vertex_count"] == inst["vertex_count"].max())[0])
    inst["transform"][k][12] += 0.2  # glm memory order: the translation's x
    inst["transform"][k][13] += 0.1
    edited = copy.deepcopy(sc)
    edited.instances = inst
    want = fu.full(femu.scene(edited).render(w, h, 3, pixel_filter=TENT), w, h)
    assert not fu.same(want[1], fu.full(femu.scene(sc).render(w, h, 3, pixel_filter=TENT), w, h)[1]), "the edit is visible"
    with g.Context(0) as ctx:
        ctx.upload_scene(sc)
        ctx.frame_begin(w, h)
        ctx.render(8)  # (returns with paths in flight)
        ctx.update_instances(inst)
        ctx.render_features(3, 0, pixel_filter=TENT)
        got = ctx.download_features()
        print("scene_splits", ctx.stats()["scene_splits"])
    assert_planes(got, want)
    with g.Context(0) as ctx:
        ctx.upload_scene(edited)
        ctx.frame_begin(w, h)
        ctx.render_features(3, 0, pixel_filter=TENT)
        assert_planes(ctx.download_features(), got)


def test_features_after_a_table_edit_with_samples_in_flight(scenes_, femu):
    """gsp_update_tables halves every diffuse reflectance while samples are in flight (they keep their version of the tables, no
    drain): the feature call waits for nothing and reads the newest tables."""
    import gpuspectral_amd as g

    sc = scenes_["cornell"]
    w, h = 96, 64
    edited = copy.deepcopy(sc)
    bs = [b.copy() for b in edited.bsdfs]
    bs[0]["reflectance"] = bs[0]["reflectance"] * np.float32(0.5)
    edited.bsdfs = bs
    want = fu.full(femu.scene(edited).render(w, h, 3, pixel_filter=TENT), w, h)
    assert not fu.same(want[0], fu.full(femu.scene(sc).render(w, h, 3, pixel_filter=TENT), w, h)[0]), "the edit is visible"
    with g.Context(0) as ctx:
        ctx.upload_scene(sc)
        ctx.frame_begin(w, h)
        ctx.render(8)  # (returns with paths in flight)
        ctx.update_tables(edited)
        ctx.render_features(3, 0, pixel_filter=TENT)
        got = ctx.download_features()
        assert ctx.stats()["scene_drains"] == 0
    assert_planes(got, want)


def test_validation(rigs, scenes_):
    import gpuspectral_amd as g

    with g.Context(0) as ctx:
        with pytest.raises(g.GspError, match="needs gsp_upload_scene and gsp_frame_begin"):
            ctx.render_features(1)
        ctx.upload_scene(scenes_["cornell"])
        with pytest.raises(g.GspError, match="needs gsp_upload_scene and gsp_frame_begin"):
            ctx.render_features(1)
        ctx.frame_begin(8, 8)
        with pytest.raises(g.GspError, match="spp must be at least 1"):
            ctx.render_features(0)
        with pytest.raises(g.GspError, match="not a GSP_FILTER"):
            ctx.render_features(1, pixel_filter=9)
        with pytest.raises(g.GspError, match="pixel_filter_param"):
            ctx.render_features(1, pixel_filter=TENT, pixel_filter_param=-1.0)
        ctx.render_features(1, adaptive_threshold=0.5, max_depth=100000)  # (fields the call ignores)
        assert (ctx.download_features()[2][..., 3] == 1).all()


_TORCH_CHILD = """
import sys
import torch  # first: the tracer's library then binds to the HIP runtime torch has loaded (see bench.py)
import numpy as np
sys.path.insert(0, sys.argv[1])
import gpuspectral_amd as g
from gpuspectral_amd import scenes
W, H = 96, 64
with g.Context(0) as ctx:
    ctx.upload_scene(scenes.cornell_materials(8))
    ctx.frame_begin(W, H)
    ctx.render_features(3, 0, pixel_filter=2)
    want = ctx.download_features()
    t = [torch.zeros(W * H * 4 + 4, dtype=torch.int32, device="cuda:0") for _ in range(3)]
    torch.cuda.synchronize()
    ctx.copy_features_to_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), W * H * 16)
    for x, w in zip(t, want):
        back = x.cpu().numpy().view(np.uint32)
        assert np.array_equal(back[:W * H * 4], w.reshape(-1).view(np.uint32)) and not back[W * H * 4:].any()
    try:
        ctx.copy_features_to_device(t[0].data_ptr(), None, None, W * H * 16 - 4)
        raise SystemExit("a short destination was accepted")
    except g.GspError as e:
        assert "destination too small" in str(e)
print("torch tensors ok")
"""


def test_copy_features_to_device_torch_tensors():
    """Into torch tensors, in a process of its own: torch has to be imported before the library is loaded."""
    r = subprocess.run([sys.executable, "-c", _TORCH_CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "torch tensors ok" in r.stdout, r.stdout + r.stderr


def test_cli_pfm_files_equal_the_binding(rigs, tmp_path):
    import os

    from conftest import CORNELL_XML
    from oracle import mitsuba_loader as ml

    ctx, _ = rigs("cornell")
    w, h, spp, fspp = 64, 48, 2, 3
    lib = os.path.join(ROOT, "gpuspectral_amd", "lib")
    env = dict(os.environ, LD_LIBRARY_PATH=lib + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    prefix = str(tmp_path / "feat")
    args = ["--filter", "tent", "--features", prefix, "--feature-spp", str(fspp), CORNELL_XML, str(tmp_path / "a.pfm"), str(w), str(h), str(spp)]
    r = subprocess.run([os.path.join(lib, "gsp_render")] + args, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "features: 3 samples per pixel" in r.stdout, r.stdout + r.stderr
    plain = subprocess.run([os.path.join(lib, "gsp_render")] + args[6:], env=env, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "features" not in plain.stdout
    ctx.frame_begin(w, h)
    ctx.render_features(fspp, 0, pixel_filter=TENT)
    a, g, _ = ctx.download_features()
    depth = np.repeat(g[..., 3:4], 3, axis=2)
    for name, want in (("albedo", a[..., :3]), ("normal", g[..., :3]), ("depth", depth)):
        got = np.asarray(ml.read_pfm(prefix + "." + name + ".pfm"), np.float32).reshape(h, w, -1)[:, :, :3]
        assert fu.same(got[::-1], want), name  # (writePfm and read_pfm: rows bottom to top, as the beauty PFM)
    for name in ("albedo", "normal"):
        assert open(prefix + "." + name + ".png", "rb").read(8) == b"\x89PNG\r\n\x1a\n"
