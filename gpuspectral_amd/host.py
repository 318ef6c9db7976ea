"""ctypes binding of libgpuspectral_host.so: the C++ host layer (Scene, loadScene, PathTracer).

The classes here only forward to the C++ objects a C++ caller would use
(gpuspectral_amd/host/*.h); see those headers for the reference citations.
"""
import ctypes as C
import os

import numpy as np

from . import abi
from .pt import GspError

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib_path():
    return os.path.join(_HERE, "lib", "libgpuspectral_host.so")


def load():
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise GspError("host library %s not found: build it with `make -C gpuspectral_amd/host`" % path)
    L = C.CDLL(path)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.gsph_last_error.restype = C.c_char_p
    L.gsph_load_scene.restype = vp
    L.gsph_load_scene.argtypes = [C.c_char_p, C.c_char_p]
    L.gsph_load_scene_ex.restype = vp
    L.gsph_load_scene_ex.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    L.gsph_load_scene_opts.restype = vp
    L.gsph_load_scene_opts.argtypes = [C.c_char_p, C.c_char_p, C.c_uint]
    L.gsph_load_bitmap.argtypes = [C.c_char_p, C.POINTER(u32), C.POINTER(u32), vp]
    L.gsph_load_hdr_bitmap.argtypes = [C.c_char_p, C.POINTER(u32), C.POINTER(u32), vp]
    L.gsph_scene_free.argtypes = [vp]
    L.gsph_scene_free.restype = None
    L.gsph_scene_desc.restype = C.POINTER(abi.SceneDesc)
    L.gsph_scene_desc.argtypes = [vp]
    L.gsph_scene_num_warnings.restype = u32
    L.gsph_scene_num_warnings.argtypes = [vp]
    L.gsph_scene_warning.restype = C.c_char_p
    L.gsph_scene_warning.argtypes = [vp, u32]
    L.gsph_scene_num_materials.restype = u32
    L.gsph_scene_num_materials.argtypes = [vp]
    L.gsph_scene_num_objects.restype = u32
    L.gsph_scene_num_objects.argtypes = [vp]
    L.gsph_scene_set_camera.argtypes = [vp, vp, C.c_float]
    L.gsph_scene_set_transform.argtypes = [vp, u32, vp]
    L.gsph_scene_set_object_material.argtypes = [vp, u32, vp, C.c_int]
    L.gsph_scene_set_diffuse_reflectance.argtypes = [vp, u32, vp]
    L.gsph_scene_make_object_rough_conductor.argtypes = [vp, u32, vp, vp, C.c_float]
    L.gsph_scene_reflatten.argtypes = [vp]
    L.gsph_pathtracer_render_files_same_slot.argtypes = [vp, C.POINTER(C.c_char_p), C.c_char_p, u32, u32, vp, vp]
    L.gsph_tracker_remember.argtypes = [vp]
    L.gsph_scene_pixel_filter.restype = u32
    L.gsph_scene_pixel_filter.argtypes = [vp, C.POINTER(C.c_float)]
    L.gsph_scene_lens.restype = None
    L.gsph_scene_lens.argtypes = [vp, C.POINTER(C.c_float * 4)]
    L.gsph_scene_set_lens.restype = None
    L.gsph_scene_set_lens.argtypes = [vp, C.c_float, C.c_float, u32, C.c_float]
    L.gsph_scene_media.restype = u32
    L.gsph_scene_media.argtypes = [vp, vp]
    L.gsph_scene_media_scattering.restype = u32
    L.gsph_scene_media_scattering.argtypes = [vp, vp]
    L.gsph_scene_delta_lights.restype = u32
    L.gsph_scene_delta_lights.argtypes = [vp, vp]
    L.gsph_scene_set_delta_lights.restype = None
    L.gsph_scene_set_delta_lights.argtypes = [vp, C.POINTER(abi.DeltaLight), u32]
    L.gsph_scene_envmap_sampling.restype = u32
    L.gsph_scene_envmap_sampling.argtypes = [vp, C.POINTER(C.c_float)]
    L.gsph_scene_set_envmap_sampling.restype = None
    L.gsph_scene_set_envmap_sampling.argtypes = [vp, u32, C.c_float]
    L.gsph_scene_add_scattering_medium.restype = u32
    L.gsph_scene_add_scattering_medium.argtypes = [vp, vp, vp, C.c_float]
    L.gsph_scene_object_medium.restype = u32
    L.gsph_scene_object_medium.argtypes = [vp, u32]
    L.gsph_scene_add_medium.restype = u32
    L.gsph_scene_add_medium.argtypes = [vp, vp]
    L.gsph_scene_set_object_medium.argtypes = [vp, u32, u32]
    L.gsph_tracker_diff.argtypes = [vp]
    L.gsph_tracker_probe.argtypes = [vp, vp]
    L.gsph_pathtracer_create.restype = vp
    L.gsph_pathtracer_create.argtypes = [u32, u32, C.c_int, vp, u64]
    L.gsph_pathtracer_free.argtypes = [vp]
    L.gsph_pathtracer_free.restype = None
    L.gsph_pathtracer_create_render_pass.argtypes = [vp, vp]
    L.gsph_pathtracer_render.argtypes = [vp, vp, u32]
    L.gsph_pathtracer_set_params.argtypes = [vp, C.POINTER(abi.RenderParams)]
    L.gsph_pathtracer_timestamp.argtypes = [vp]
    L.gsph_pathtracer_reset.argtypes = [vp]
    L.gsph_pathtracer_download.argtypes = [vp, vp, u64]
    L.gsph_pathtracer_stats.argtypes = [vp, C.POINTER(abi.Stats)]
    L.gsph_write_pfm.argtypes = [C.c_char_p, vp, u32, u32]
    L.gsph_write_ppm.argtypes = [C.c_char_p, vp, u32, u32, C.c_int]
    L.gsph_tone_map.argtypes = [vp, u32, u32, C.c_int, vp]
    L.gsph_scene_film.argtypes = [vp, C.POINTER(abi.Display)]
    L.gsph_write_png.argtypes = [C.c_char_p, vp, u32, u32, C.c_int]
    L.gsph_encode_png.argtypes = [vp, u32, u32, C.c_int, vp, C.POINTER(u64)]
    L.gsph_decode_png.argtypes = [vp, u64, C.POINTER(u32), C.POINTER(u32), vp]
    L.gsph_pathtracer_set_display.argtypes = [vp, C.POINTER(abi.Display)]
    L.gsph_pathtracer_download_display.argtypes = [vp, vp, u64]
    L.gsph_pathtracer_render_features.argtypes = [vp, vp, C.c_uint32]
    L.gsph_pathtracer_download_features.argtypes = [vp, vp, vp, u64]
    L.gsph_pathtracer_download_denoised.argtypes = [vp, C.POINTER(abi.Denoise), vp, u64]
    L.gsph_pathtracer_download_denoised_display.argtypes = [vp, C.POINTER(abi.Denoise), vp, u64]
    L.gsph_pathtracer_next_frame.argtypes = [vp]
    L.gsph_pathtracer_temporal_accumulate.argtypes = [vp, C.POINTER(abi.Temporal)]
    L.gsph_pathtracer_temporal_reset.argtypes = [vp]
    L.gsph_pathtracer_download_temporal.argtypes = [vp, vp, u64]
    L.gsph_pathtracer_download_temporal_denoised.argtypes = [vp, C.POINTER(abi.Denoise), vp, u64]
    L.gsph_pathtracer_temporal_track_moments.argtypes = [vp, C.c_int]
    L.gsph_pathtracer_download_temporal_moments.argtypes = [vp, vp, u64]
    L.gsph_pathtracer_download_temporal_svgf.argtypes = [vp, C.POINTER(abi.Denoise), C.POINTER(abi.Svgf), vp, u64]
    L.gsph_pathtracer_temporal_follow_instances.argtypes = [vp, C.c_int]
    L.gsph_pathtracer_set_light_sampling.argtypes = [vp, u32]
    L.gsph_pathtracer_set_estimator.argtypes = [vp, u32]
    L.gsph_pathtracer_set_light_grid.argtypes = [vp, u32, u32, u32, u32]
    L.gsph_pathtracer_download_light_pick.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.gsph_pathtracer_download_temporal_motion.argtypes = [vp, vp, u64]
    L.gsph_pathtracer_temporal_demodulate.argtypes = [vp, C.c_int]
    L.gsph_pathtracer_download_temporal_image.argtypes = [vp, vp, u64]
    L.gsph_pathtracer_temporal_image_to_device.argtypes = [vp, vp, u64]
    L.gsph_pathtracer_temporal_svgf_feedback.argtypes = [vp, C.POINTER(abi.Denoise), C.POINTER(abi.Svgf), C.c_uint32, vp, u64]
    L.gsph_pathtracer_temporal_svgf_feedback_to_device.argtypes = [vp, C.POINTER(abi.Denoise), C.POINTER(abi.Svgf), C.c_uint32, vp, u64]
    L.gsph_pathtracer_temporal_antilag.argtypes = [vp, C.POINTER(abi.Antilag)]
    L.gsph_pathtracer_download_temporal_fast.argtypes = [vp, vp, u64]
    L.gsph_pathtracer_temporal_fast_to_device.argtypes = [vp, vp, u64]
    L.gsph_pathtracer_temporal_taa.argtypes = [vp, C.POINTER(abi.Taa), C.POINTER(abi.Display), vp, u64]
    L.gsph_pathtracer_temporal_taa_from_device.argtypes = [vp, C.POINTER(abi.Taa), C.POINTER(abi.Display), vp, u64]
    L.gsph_pathtracer_download_taa.argtypes = [vp, vp, u64]
    L.gsph_pathtracer_download_taa_display.argtypes = [vp, vp, u64]
    L.gsph_pathtracer_taa_display_to_device.argtypes = [vp, vp, u64]
    _LIB = L
    return L


def _err(L):
    return L.gsph_last_error().decode(errors="replace")


def _view(ptr, count, dtype):
    if not ptr or count == 0:
        return np.zeros(0, dtype)
    buf = (C.c_char * (count * np.dtype(dtype).itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype, count=count).copy()


class Scene:
    """A C++ GPUSpectral::Scene produced by loadScene (S/engine/Loader.cpp:253-349)."""

    def __init__(self, path, asset_dir=None, dormant_features=False, srgb_textures=True, builtin_shapes=False, read_filter=False,
                 read_lens=False, read_film=False, read_media=False, read_scattering=False, read_emitters=False, sample_envmap=False):
        """dormant_features: LoadOptions::dormantFeatures (textures / environment map); builtin_shapes:
        LoadOptions::builtinShapes (`disk` and `sphere` shapes are built instead of skipped); the defaults are
        the reference's behaviour.  read_filter: LoadOptions::readFilter (the film's <rfilter> becomes `pixel_filter`, which
        PathTracer.render applies unless its params name a filter of their own).  read_lens: LoadOptions::readLens (a `thinlens`
        sensor's aperture_radius / focus_distance become the camera's lens, which PathTracer hands to the device).  read_film:
        LoadOptions::readFilm (an ldrfilm's gamma / exposure / tonemapMethod / key / burn become `film`).  read_media:
        LoadOptions::readMedia (the shapes' <medium name="interior"> become `media` and the objects' medium numbers: coloured glass).
        read_scattering: LoadOptions::readScattering (implies read_media; sigmaS / albedo and the hg phase become `media_scattering`).
        read_emitters: LoadOptions::readEmitters (top-level point / spot / directional emitters become `delta_lights`).
        sample_envmap: LoadOptions::sampleEnvmap (`envmap_sampling` = on, with the radius of the scene's bounds as its extent)."""
        self._L = load()
        ad = asset_dir.encode() if asset_dir else None
        if builtin_shapes or read_filter or read_lens or read_film or read_media or read_scattering or read_emitters or sample_envmap:
            self._h = self._L.gsph_load_scene_opts(path.encode(), ad, (1 if dormant_features else 0) | (2 if srgb_textures else 0) |
                                                   (4 if builtin_shapes else 0) | (8 if read_filter else 0) | (16 if read_lens else 0) |
                                                   (32 if read_film else 0) | (64 if read_media else 0) |
                                                   (128 if read_scattering else 0) | (256 if read_emitters else 0) | (512 if sample_envmap else 0))
        elif dormant_features:
            self._h = self._L.gsph_load_scene_ex(path.encode(), ad, 1, 1 if srgb_textures else 0)
        else:
            self._h = self._L.gsph_load_scene(path.encode(), ad)
        if not self._h:
            raise GspError("loadScene(%s): %s" % (path, _err(self._L)))

    def close(self):
        if getattr(self, "_h", None):
            self._L.gsph_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def warnings(self):
        return [self._L.gsph_scene_warning(self._h, i).decode() for i in range(self._L.gsph_scene_num_warnings(self._h))]

    @property
    def pixel_filter(self):
        """(abi.FILTER_*, parameter) the loader read from the film's <rfilter>; (0, 0.0) without read_filter."""
        param = C.c_float(0.0)
        f = self._L.gsph_scene_pixel_filter(self._h, C.byref(param))
        return int(f), float(param.value)

    @property
    def lens(self):
        """(aperture radius, focus distance, blades, rotation) of the scene's camera; all 0 without read_lens / set_lens."""
        out = (C.c_float * 4)()
        self._L.gsph_scene_lens(self._h, C.byref(out))
        return float(out[0]), float(out[1]), int(out[2]), float(out[3])

    @property
    def film(self):
        """(an ldrfilm was read, abi.Display of Scene::film); (False, clamp + sRGB) without read_film."""
        d = abi.Display()
        ldr = self._L.gsph_scene_film(self._h, C.byref(d))
        return bool(ldr), d

    @property
    def media(self):
        """Scene::media as an (n, 3) float32 array of absorption coefficients; empty without read_media / add_medium."""
        n = self._L.gsph_scene_media(self._h, None)
        out = np.zeros((n, 3), np.float32)
        if n:
            self._L.gsph_scene_media(self._h, out.ctypes.data)
        return out

    @property
    def media_scattering(self):
        """Scene::mediaScattering as an (n, 4) float32 array (sigma_s, g), parallel to `media`; empty while no medium scatters."""
        n = self._L.gsph_scene_media_scattering(self._h, None)
        out = np.zeros((n, 4), np.float32)
        if n:
            self._L.gsph_scene_media_scattering(self._h, out.ctypes.data)
        return out

    @property
    def delta_lights(self):
        """Scene::deltaLights as a list of abi.DeltaLight; empty without read_emitters / set_delta_lights."""
        n = self._L.gsph_scene_delta_lights(self._h, None)
        out = (abi.DeltaLight * max(n, 1))()
        if n:
            self._L.gsph_scene_delta_lights(self._h, out)
        return list(out)[:n]

    @property
    def envmap_sampling(self):
        """Scene::envmapSampling as (enabled, extent); (False, 0.0) without sample_envmap / set_envmap_sampling."""
        extent = C.c_float(0.0)
        on = self._L.gsph_scene_envmap_sampling(self._h, C.byref(extent))
        return bool(on), float(extent.value)

    def set_envmap_sampling(self, enabled=True, extent=1.0):
        """Scene::envmapSampling (PathTracer sends the switch when its value changed; the tracer must run the textbook estimator)."""
        self._L.gsph_scene_set_envmap_sampling(self._h, 1 if enabled else 0, extent)

    def set_delta_lights(self, lights):
        """Scene::deltaLights = the abi.DeltaLight records of `lights` (PathTracer sends the table when its value changed)."""
        arr = abi.delta_light_array(lights)
        self._L.gsph_scene_set_delta_lights(self._h, arr, len(arr) if arr is not None else 0)

    def add_scattering_medium(self, sigma_a, sigma_s, g=0.0):
        """Scene::addMedium with scattering: the number of the (possibly shared) entry."""
        a, s = np.ascontiguousarray(sigma_a, np.float32), np.ascontiguousarray(sigma_s, np.float32)
        return int(self._L.gsph_scene_add_scattering_medium(self._h, a.ctypes.data, s.ctypes.data, float(g)))

    def object_medium(self, obj):
        """RenderObject::interiorMedium: 0 = none, k = media[k - 1]."""
        return int(self._L.gsph_scene_object_medium(self._h, obj))

    def add_medium(self, sigma_a):
        """Scene::addMedium: the number of the (possibly shared) entry."""
        s = np.ascontiguousarray(sigma_a, np.float32)
        return int(self._L.gsph_scene_add_medium(self._h, s.ctypes.data))

    def set_object_medium(self, obj, number):
        """Names entry `number` of the scene's media as the object's interior medium (0 = none) and flattens the scene again."""
        if self._L.gsph_scene_set_object_medium(self._h, obj, number) != 0:
            raise RuntimeError(self._L.gsph_last_error().decode())
        self._L.gsph_scene_reflatten(self._h)

    def set_lens(self, radius, focus_distance, blades=0, rotation=0.0):
        """Camera::setLens: the tracer sends it with the next pass (gsp_set_lens) when its value changed."""
        self._L.gsph_scene_set_lens(self._h, radius, focus_distance, blades, rotation)

    @property
    def num_materials(self):
        return self._L.gsph_scene_num_materials(self._h)

    # ---- edits between frames (a host application mutates its Scene; PathTracer::prepareScene compares by value) ----
    def _ok(self, rc, what):
        if rc != 0:
            raise GspError("%s: %s" % (what, _err(self._L)))

    @property
    def num_objects(self):
        return self._L.gsph_scene_num_objects(self._h)

    def set_camera(self, to_world, fov):
        m = np.ascontiguousarray(to_world, np.float32).reshape(16)
        self._ok(self._L.gsph_scene_set_camera(self._h, m.ctypes.data, float(fov)), "set_camera")

    def set_transform(self, obj, matrix16):
        m = np.ascontiguousarray(matrix16, np.float32).reshape(16)
        self._ok(self._L.gsph_scene_set_transform(self._h, obj, m.ctypes.data), "set_transform")

    def set_object_material(self, obj, emission=None, twofaced=None):
        e = np.ascontiguousarray(emission, np.float32).reshape(3) if emission is not None else None
        self._ok(self._L.gsph_scene_set_object_material(self._h, obj, e.ctypes.data if e is not None else None,
                                                        -1 if twofaced is None else int(bool(twofaced))), "set_object_material")

    def set_diffuse_reflectance(self, index, rgb):
        c = np.ascontiguousarray(rgb, np.float32).reshape(3)
        self._ok(self._L.gsph_scene_set_diffuse_reflectance(self._h, index, c.ctypes.data), "set_diffuse_reflectance")

    def make_object_rough_conductor(self, obj, eta, k, alpha):
        e, kk = np.ascontiguousarray(eta, np.float32).reshape(3), np.ascontiguousarray(k, np.float32).reshape(3)
        self._ok(self._L.gsph_scene_make_object_rough_conductor(self._h, obj, e.ctypes.data, kk.ctypes.data, float(alpha)),
                 "make_object_rough_conductor")

    def arrays(self):
        """Copy of the flattened scene AS IT IS NOW (what crosses the C ABI) as abi.SceneArrays."""
        self._ok(self._L.gsph_scene_reflatten(self._h), "flattenScene")
        d = self._L.gsph_scene_desc(self._h).contents
        sc = abi.SceneArrays()
        sc.instances = _view(d.instances, d.num_instances, abi.INSTANCE_DT)
        sc.positions = _view(d.positions, d.num_vertices * 3, np.float32).reshape(-1, 3)
        sc.normals = _view(d.normals, d.num_vertices * 3, np.float32).reshape(-1, 3)
        sc.bsdfs = [
            _view(getattr(d, name + "_bsdfs"), d.num_bsdfs[i], dt)
            for i, (name, dt) in enumerate(zip(abi.BSDF_NAMES, abi.BSDF_DTYPES))
        ]
        sc.lights = _view(d.lights, d.num_lights, abi.LIGHT_DT)
        sc.to_world = np.array(list(d.camera.to_world), np.float32)
        sc.fov = np.float32(d.camera.fov)
        if d.num_textures:
            sc.uvs = _view(d.uvs, d.num_vertices * 2, np.float32).reshape(-1, 2)
            sc.textures = _view(d.textures, d.num_textures, abi.TEXTURE_DT)
            sc.texels = _view(d.texels, d.num_texels, np.uint32)
            sc.texel_decode = _view(d.texel_decode, 256, np.float32) if d.texel_decode else None
        if d.envmap.texels:
            w, h = d.envmap.width, d.envmap.height
            sc.env_texels = _view(d.envmap.texels, w * h * 4, np.float32).reshape(h, w, 4)
            sc.env_to_local = np.array(list(d.envmap.to_local), np.float32)
        return sc


def load_bitmap(path):
    """Image.h loadBitmap: (H, W, 4) uint8, row 0 = bottom image row."""
    L = load()
    w, h = C.c_uint32(), C.c_uint32()
    if L.gsph_load_bitmap(path.encode(), C.byref(w), C.byref(h), None):
        raise GspError("loadBitmap(%s): %s" % (path, _err(L)))
    out = np.zeros((h.value, w.value), np.uint32)
    if L.gsph_load_bitmap(path.encode(), C.byref(w), C.byref(h), out.ctypes.data):
        raise GspError("loadBitmap(%s): %s" % (path, _err(L)))
    return out.view(np.uint8).reshape(h.value, w.value, 4)


def load_hdr_bitmap(path):
    """Image.h loadHdrBitmap: (H, W, 4) float32, row 0 = bottom image row."""
    L = load()
    w, h = C.c_uint32(), C.c_uint32()
    if L.gsph_load_hdr_bitmap(path.encode(), C.byref(w), C.byref(h), None):
        raise GspError("loadHdrBitmap(%s): %s" % (path, _err(L)))
    out = np.zeros((h.value, w.value, 4), np.float32)
    if L.gsph_load_hdr_bitmap(path.encode(), C.byref(w), C.byref(h), out.ctypes.data):
        raise GspError("loadHdrBitmap(%s): %s" % (path, _err(L)))
    return out


class PathTracer:
    """C++ GPUSpectral::PathTracer (drop-in for S/renderer/PathTracer.h:48-68)."""

    def __init__(self, width, height, device=0, pixel_ids=None):
        self._L = load()
        ids = np.ascontiguousarray(pixel_ids, np.uint32) if pixel_ids is not None else None
        self._h = self._L.gsph_pathtracer_create(width, height, device, ids.ctypes.data if ids is not None else None,
                                                 len(ids) if ids is not None else 0)
        if not self._h:
            raise GspError("PathTracer(): %s" % _err(self._L))
        self.width, self.height = width, height

    def _check(self, rc, what):
        if rc != 0:
            raise GspError("%s: %s" % (what, _err(self._L)))

    def close(self):
        if getattr(self, "_h", None):
            self._L.gsph_pathtracer_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def create_render_pass(self, scene):
        self._check(self._L.gsph_pathtracer_create_render_pass(self._h, scene._h), "createRenderPass")

    def render(self, scene, spp):
        self._check(self._L.gsph_pathtracer_render(self._h, scene._h, spp), "render")

    def render_files_same_slot(self, paths, spp, asset_dir=None):
        """Loads each file into a Scene in ONE stack slot (a C++ loop-local), renders `spp` samples from timestamp 0 and
        downloads: (images [n, H, W, 4], addresses of the n Scene objects)."""
        arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
        out = np.zeros((len(paths), self.height, self.width, 4), np.float32)
        addr = np.zeros(len(paths), np.uint64)
        self._check(self._L.gsph_pathtracer_render_files_same_slot(self._h, arr, asset_dir.encode() if asset_dir else None,
                                                                   len(paths), spp, out.ctypes.data, addr.ctypes.data),
                    "render_files_same_slot")
        return out, addr

    def set_params(self, params):
        self._check(self._L.gsph_pathtracer_set_params(self._h, C.byref(params)), "set_params")

    @property
    def timestamp(self):
        return self._L.gsph_pathtracer_timestamp(self._h)

    def reset(self):
        self._check(self._L.gsph_pathtracer_reset(self._h), "reset")

    def download(self):
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.gsph_pathtracer_download(self._h, out.ctypes.data, out.size), "download")
        return out

    def download_display(self, display=None):
        """PathTracer::downloadDisplay with PathTracer::display = `display` (abi.Display; None keeps the current one)."""
        if display is not None:
            self._check(self._L.gsph_pathtracer_set_display(self._h, C.byref(display)), "set_display")
        out = np.zeros((self.height, self.width), np.uint32)
        self._check(self._L.gsph_pathtracer_download_display(self._h, out.ctypes.data, out.size), "downloadDisplay")
        return out

    def render_features(self, scene, spp):
        """PathTracer::renderFeatures: spp feature samples per pixel under this tracer's filter and the scene's lens."""
        self._check(self._L.gsph_pathtracer_render_features(self._h, scene._h, spp), "renderFeatures")

    def download_features(self):
        """PathTracer::downloadFeatures: (albedo[h,w,4], geom[h,w,4]) float32."""
        a = np.zeros((self.height, self.width, 4), np.float32)
        g = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.gsph_pathtracer_download_features(self._h, a.ctypes.data, g.ctypes.data, a.size), "downloadFeatures")
        return a, g

    def download_denoised(self, denoise=None):
        """PathTracer::downloadDenoised (abi.Denoise; None = every default): (h, w, 4) float32."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.gsph_pathtracer_download_denoised(self._h, C.byref(denoise) if denoise is not None else None, out.ctypes.data, out.size),
                    "downloadDenoised")
        return out

    def download_denoised_display(self, denoise=None, display=None):
        """PathTracer::downloadDenoisedDisplay with PathTracer::display = `display` (None keeps the current one): (h, w) uint32."""
        if display is not None:
            self._check(self._L.gsph_pathtracer_set_display(self._h, C.byref(display)), "set_display")
        out = np.zeros((self.height, self.width), np.uint32)
        self._check(self._L.gsph_pathtracer_download_denoised_display(self._h, C.byref(denoise) if denoise is not None else None, out.ctypes.data,
                                                                      out.size), "downloadDenoisedDisplay")
        return out

    def next_frame(self):
        """PathTracer::nextFrame: a new frame whose samples continue the timestamp sequence."""
        self._check(self._L.gsph_pathtracer_next_frame(self._h), "nextFrame")

    def temporal_accumulate(self, temporal=None):
        """PathTracer::temporalAccumulate (abi.Temporal; None = every default)."""
        self._check(self._L.gsph_pathtracer_temporal_accumulate(self._h, C.byref(temporal) if temporal is not None else None), "temporalAccumulate")

    def temporal_reset(self):
        self._check(self._L.gsph_pathtracer_temporal_reset(self._h), "temporalReset")

    def download_temporal(self):
        """PathTracer::downloadTemporal: (h, w, 4) float32, .w = the history length."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.gsph_pathtracer_download_temporal(self._h, out.ctypes.data, out.size), "downloadTemporal")
        return out

    def download_temporal_denoised(self, denoise=None):
        """PathTracer::downloadTemporalDenoised (abi.Denoise; None = every default): (h, w, 4) float32."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.gsph_pathtracer_download_temporal_denoised(self._h, C.byref(denoise) if denoise is not None else None, out.ctypes.data,
                                                                       out.size), "downloadTemporalDenoised")
        return out

    def temporal_track_moments(self, on=True):
        """PathTracer::temporalTrackMoments: the history keeps its luminance moments (a change drops the history)."""
        self._check(self._L.gsph_pathtracer_temporal_track_moments(self._h, 1 if on else 0), "temporalTrackMoments")

    def download_temporal_moments(self):
        """PathTracer::downloadTemporalMoments: (h, w, 4) float32 {m1, m2, r, 0}."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.gsph_pathtracer_download_temporal_moments(self._h, out.ctypes.data, out.size), "downloadTemporalMoments")
        return out

    def download_temporal_svgf(self, denoise=None, svgf=None):
        """PathTracer::downloadTemporalSvgf (abi.Denoise, abi.Svgf; None = every default): (h, w, 4) float32."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.gsph_pathtracer_download_temporal_svgf(self._h, C.byref(denoise) if denoise is not None else None,
                                                                   C.byref(svgf) if svgf is not None else None, out.ctypes.data, out.size),
                    "downloadTemporalSvgf")
        return out

    def set_estimator(self, mode):
        """PathTracer::setEstimator: "reference" (the default) or "textbook" (gpuspectral_pt.h "Estimator")."""
        self._check(self._L.gsph_pathtracer_set_estimator(self._h, abi.estimator_mode(mode)), "setEstimator")

    def set_light_grid(self, enabled=True, resolution=None):
        """PathTracer::setLightGrid (gpuspectral_pt.h "Light grid"): resolution (nx, ny, nz), None = the library chooses.  Needs
        set_light_sampling("power") and set_estimator("textbook") first."""
        nx, ny, nz = (0, 0, 0) if resolution is None else resolution
        self._check(self._L.gsph_pathtracer_set_light_grid(self._h, 1 if enabled else 0, nx, ny, nz), "setLightGrid")

    def set_light_sampling(self, mode):
        """PathTracer::setLightSampling: "uniform" (the reference's pick) or "power" (gpuspectral_pt.h "Light selection")."""
        self._check(self._L.gsph_pathtracer_set_light_sampling(self._h, abi.light_sampling_mode(mode)), "setLightSampling")

    def download_light_pick(self):
        """PathTracer::downloadLightPick: the resident alias table as an abi.LIGHT_PICK_DT array."""
        n = C.c_uint32(0)
        self._L.gsph_pathtracer_download_light_pick(self._h, None, 0, C.byref(n))  # (the count)
        out = np.zeros(n.value, abi.LIGHT_PICK_DT)
        self._check(self._L.gsph_pathtracer_download_light_pick(self._h, out.ctypes.data if n.value else None, n.value, C.byref(n)), "downloadLightPick")
        return out

    def temporal_follow_instances(self, on=True):
        """PathTracer::temporalFollowInstances: the history follows moved objects (a change drops the history)."""
        self._check(self._L.gsph_pathtracer_temporal_follow_instances(self._h, 1 if on else 0), "temporalFollowInstances")

    def download_temporal_motion(self):
        """PathTracer::downloadTemporalMotion: (h, w, 4) float32 {dx, dy, kept weight, class}."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.gsph_pathtracer_download_temporal_motion(self._h, out.ctypes.data, out.size), "downloadTemporalMotion")
        return out

    def temporal_demodulate(self, on=True):
        """PathTracer::temporalDemodulate: the history accumulates colour / first-hit albedo (a change drops the history)."""
        self._check(self._L.gsph_pathtracer_temporal_demodulate(self._h, 1 if on else 0), "temporalDemodulate")

    def download_temporal_image(self):
        """PathTracer::downloadTemporalImage: (h, w, 4) float32, the history as a viewer shows it; .w = the history length."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.gsph_pathtracer_download_temporal_image(self._h, out.ctypes.data, out.size), "downloadTemporalImage")
        return out

    def temporal_image_to_device(self, dst, nbytes=None):
        """PathTracer::temporalImageToDevice: dst = a torch tensor on the device, or a device pointer with nbytes."""
        if hasattr(dst, "data_ptr"):
            ptr, nbytes = dst.data_ptr(), dst.numel() * dst.element_size()
        else:
            ptr = dst
        self._check(self._L.gsph_pathtracer_temporal_image_to_device(self._h, ptr, nbytes), "temporalImageToDevice")

    def temporal_svgf_feedback(self, denoise=None, svgf=None, levels=1, out=True):
        """PathTracer::temporalSvgfFeedback: download_temporal_svgf whose first `levels` levels go back into the history (once per
        temporal_accumulate).  out=False: no output, returns None."""
        res = np.zeros((self.height, self.width, 4), np.float32) if out else None
        self._check(self._L.gsph_pathtracer_temporal_svgf_feedback(self._h, C.byref(denoise) if denoise is not None else None,
                                                                   C.byref(svgf) if svgf is not None else None, levels,
                                                                   res.ctypes.data if out else None, res.size if out else 0), "temporalSvgfFeedback")
        return res

    def temporal_svgf_feedback_to_device(self, dst, nbytes=None, denoise=None, svgf=None, levels=1):
        """PathTracer::temporalSvgfFeedbackToDevice: dst = a torch tensor, a device pointer with nbytes, or None (no output)."""
        if dst is None:
            ptr, nbytes = None, 0
        elif hasattr(dst, "data_ptr"):
            ptr, nbytes = dst.data_ptr(), dst.numel() * dst.element_size()
        else:
            ptr = dst
        self._check(self._L.gsph_pathtracer_temporal_svgf_feedback_to_device(self._h, C.byref(denoise) if denoise is not None else None,
                                                                             C.byref(svgf) if svgf is not None else None, levels, ptr, nbytes),
                    "temporalSvgfFeedbackToDevice")

    def temporal_antilag(self, antilag=None):
        """PathTracer::temporalAntilag: the fast history of this frame's temporal_accumulate and the clamp of the long one into its
        box (once per temporal_accumulate, before any temporal_svgf_feedback).  antilag: an abi.Antilag, None = every default."""
        self._check(self._L.gsph_pathtracer_temporal_antilag(self._h, C.byref(antilag) if antilag is not None else None), "temporalAntilag")

    def download_temporal_fast(self):
        """PathTracer::downloadTemporalFast: (h, w, 4) float32, the fast history; .w = its length."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.gsph_pathtracer_download_temporal_fast(self._h, out.ctypes.data, out.size), "downloadTemporalFast")
        return out

    def temporal_fast_to_device(self, dst, nbytes=None):
        """PathTracer::temporalFastToDevice: dst = a torch tensor on the device, or a device pointer with nbytes."""
        if hasattr(dst, "data_ptr"):
            ptr, nbytes = dst.data_ptr(), dst.numel() * dst.element_size()
        else:
            ptr = dst
        self._check(self._L.gsph_pathtracer_temporal_fast_to_device(self._h, ptr, nbytes), "temporalFastToDevice")

    def temporal_taa(self, taa=None, display=None, src=None):
        """PathTracer::temporalTaa: resolves the tone-mapped frame over its own history (once per temporal_accumulate, with
        temporal_follow_instances on).  taa: an abi.Taa, None = every default; display: an abi.Display, None = the PathTracer's LDR
        film; src: (h, w, 4) float32, the HDR frame to resolve, None = the image of the newest history."""
        n = 0
        if src is not None:
            src = np.ascontiguousarray(src, np.float32)
            n = src.size
        self._check(self._L.gsph_pathtracer_temporal_taa(self._h, C.byref(taa) if taa is not None else None, C.byref(display) if display is not None else None,
                                                         src.ctypes.data if src is not None else None, n), "temporalTaa")

    def temporal_taa_from_device(self, src, nbytes=None, taa=None, display=None):
        """PathTracer::temporalTaaFromDevice: src = a torch tensor on the device, a device pointer with nbytes, or None."""
        if src is None:
            ptr, nbytes = None, 0
        elif hasattr(src, "data_ptr"):
            ptr, nbytes = src.data_ptr(), src.numel() * src.element_size()
        else:
            ptr = src
        self._check(self._L.gsph_pathtracer_temporal_taa_from_device(self._h, C.byref(taa) if taa is not None else None,
                                                                     C.byref(display) if display is not None else None, ptr, nbytes), "temporalTaaFromDevice")

    def download_taa(self):
        """PathTracer::downloadTaa: (h, w, 4) float32, the resolved display-linear frame; .w = 1 where the history was used."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.gsph_pathtracer_download_taa(self._h, out.ctypes.data, out.size), "downloadTaa")
        return out

    def download_taa_display(self):
        """PathTracer::downloadTaaDisplay: (h, w) uint32 RGBA8 words, the encode of the resolved frame."""
        out = np.zeros((self.height, self.width), np.uint32)
        self._check(self._L.gsph_pathtracer_download_taa_display(self._h, out.ctypes.data, out.size), "downloadTaaDisplay")
        return out

    def taa_display_to_device(self, dst, nbytes=None):
        """PathTracer::taaDisplayToDevice: dst = a torch tensor on the device, or a device pointer with nbytes."""
        if hasattr(dst, "data_ptr"):
            ptr, nbytes = dst.data_ptr(), dst.numel() * dst.element_size()
        else:
            ptr = dst
        self._check(self._L.gsph_pathtracer_taa_display_to_device(self._h, ptr, nbytes), "taaDisplayToDevice")

    def stats(self):
        s = abi.Stats()
        self._check(self._L.gsph_pathtracer_stats(self._h, C.byref(s)), "stats")
        return s.as_dict()


def write_pfm(path, rgba):
    rgba = np.ascontiguousarray(rgba, np.float32)
    h, w = rgba.shape[0], rgba.shape[1]
    L = load()
    if L.gsph_write_pfm(path.encode(), rgba.ctypes.data, w, h) != 0:
        raise GspError("write_pfm: %s" % _err(L))


def tone_map(rgba, aces=False):
    """uint8 RGB image: clamp (or ACESFilm, S/assets/shaders/common.glsl:74-82) then gamma 2.2."""
    rgba = np.ascontiguousarray(rgba, np.float32)
    h, w = rgba.shape[0], rgba.shape[1]
    out = np.zeros((h, w, 3), np.uint8)
    L = load()
    if L.gsph_tone_map(rgba.ctypes.data, w, h, 1 if aces else 0, out.ctypes.data) != 0:
        raise GspError("tone_map: %s" % _err(L))
    return out


def write_ppm(path, rgba, aces=False):
    rgba = np.ascontiguousarray(rgba, np.float32)
    L = load()
    if L.gsph_write_ppm(path.encode(), rgba.ctypes.data, rgba.shape[1], rgba.shape[0], 1 if aces else 0) != 0:
        raise GspError("write_ppm: %s" % _err(L))


def encode_png(rgba8, alpha=False):
    """Image.h encodePng: the PNG file (bytes) of an (H, W) uint32 RGBA8 image, row 0 = top."""
    rgba8 = np.ascontiguousarray(rgba8, np.uint32)
    L = load()
    size = C.c_uint64(0)
    if L.gsph_encode_png(rgba8.ctypes.data, rgba8.shape[1], rgba8.shape[0], 1 if alpha else 0, None, C.byref(size)) != 0:
        raise GspError("encode_png: %s" % _err(L))
    out = np.zeros(size.value, np.uint8)
    if L.gsph_encode_png(rgba8.ctypes.data, rgba8.shape[1], rgba8.shape[0], 1 if alpha else 0, out.ctypes.data, C.byref(size)) != 0:
        raise GspError("encode_png: %s" % _err(L))
    return out.tobytes()


def write_png(path, rgba8, alpha=False):
    rgba8 = np.ascontiguousarray(rgba8, np.uint32)
    L = load()
    if L.gsph_write_png(path.encode(), rgba8.ctypes.data, rgba8.shape[1], rgba8.shape[0], 1 if alpha else 0) != 0:
        raise GspError("write_png: %s" % _err(L))


def decode_png(data):
    """Image.h decodePng: (H, W) uint32 RGBA8 (A = 255), row 0 = BOTTOM image row."""
    buf = np.frombuffer(data, np.uint8)
    L = load()
    w, h = C.c_uint32(), C.c_uint32()
    if L.gsph_decode_png(buf.ctypes.data, len(buf), C.byref(w), C.byref(h), None) != 0:
        raise GspError("decode_png: %s" % _err(L))
    out = np.zeros((h.value, w.value), np.uint32)
    if L.gsph_decode_png(buf.ctypes.data, len(buf), C.byref(w), C.byref(h), out.ctypes.data) != 0:
        raise GspError("decode_png: %s" % _err(L))
    return out
