"""ctypes binding of libgpuspectral_pt.so (the C ABI, include/gpuspectral_pt.h).

No computation happens here and there is no fallback: if the HIP library is
not built, or no GPU is present, the calls raise.
"""
import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

# every symbol include/gpuspectral_pt.h declares
EXPORTS = (
    "gsp_default_render_params",
    "gsp_abi_version",
    "gsp_build_info",
    "gsp_device_count",
    "gsp_ctx_create",
    "gsp_default_ctx_options",
    "gsp_ctx_create_ex",
    "gsp_ctx_destroy",
    "gsp_upload_scene",
    "gsp_update_camera",
    "gsp_update_instances",
    "gsp_update_tables",
    "gsp_set_lens",
    "gsp_set_media",
    "gsp_set_media_scattering",
    "gsp_set_light_sampling",
    "gsp_download_light_pick",
    "gsp_set_estimator",
    "gsp_set_delta_lights",
    "gsp_set_envmap_sampling",
    "gsp_set_light_grid",
    "gsp_get_light_grid",
    "gsp_focus_distance",
    "gsp_frame_begin",
    "gsp_render",
    "gsp_download_pixel_stats",
    "gsp_sync",
    "gsp_download",
    "gsp_download_compact",
    "gsp_peek",
    "gsp_copy_accum_to_device",
    "gsp_peek_to_device",
    "gsp_upload_accum",
    "gsp_frame_luminance",
    "gsp_download_display",
    "gsp_peek_display",
    "gsp_peek_display_to_device",
    "gsp_render_features",
    "gsp_download_features",
    "gsp_copy_features_to_device",
    "gsp_download_denoised",
    "gsp_denoise_to_device",
    "gsp_download_denoised_display",
    "gsp_temporal_accumulate",
    "gsp_temporal_reset",
    "gsp_download_temporal",
    "gsp_temporal_to_device",
    "gsp_download_temporal_denoised",
    "gsp_download_temporal_denoised_display",
    "gsp_temporal_track_moments",
    "gsp_download_temporal_moments",
    "gsp_download_temporal_svgf",
    "gsp_temporal_svgf_to_device",
    "gsp_download_temporal_svgf_display",
    "gsp_temporal_follow_instances",
    "gsp_download_temporal_motion",
    "gsp_temporal_motion_to_device",
    "gsp_temporal_demodulate",
    "gsp_download_temporal_image",
    "gsp_temporal_image_to_device",
    "gsp_temporal_svgf_feedback",
    "gsp_temporal_svgf_feedback_to_device",
    "gsp_temporal_antilag",
    "gsp_download_temporal_fast",
    "gsp_temporal_fast_to_device",
    "gsp_temporal_taa",
    "gsp_temporal_taa_from_device",
    "gsp_download_taa",
    "gsp_download_taa_display",
    "gsp_taa_display_to_device",
    "gsp_frame_sample_base",
    "gsp_get_stats",
    "gsp_reset_stats",
    "gsp_trace",
    "gsp_debug_visit_histograms",
    "gsp_last_error",
    "gsp_tile_partition",
    "gsp_multi_create",
    "gsp_multi_create_ex",
    "gsp_multi_destroy",
    "gsp_multi_num_shares",
    "gsp_multi_upload_scene",
    "gsp_multi_update_camera",
    "gsp_multi_set_lens",
    "gsp_multi_set_media",
    "gsp_multi_set_media_scattering",
    "gsp_multi_set_light_sampling",
    "gsp_multi_set_estimator",
    "gsp_multi_set_delta_lights",
    "gsp_multi_set_envmap_sampling",
    "gsp_multi_set_light_grid",
    "gsp_multi_update_instances",
    "gsp_multi_update_tables",
    "gsp_multi_frame_begin",
    "gsp_multi_render",
    "gsp_multi_sync",
    "gsp_multi_gather",
    "gsp_multi_gather_route",
    "gsp_multi_download",
    "gsp_multi_download_display",
    "gsp_multi_render_features",
    "gsp_multi_download_features",
    "gsp_multi_download_denoised",
    "gsp_multi_get_stats",
    "gsp_multi_reset_stats",
    "gsp_multi_last_error",
)


class GspError(RuntimeError):
    pass


def lib_path():
    # GSP_LIB_PATH: developer override used to A/B kernel build variants (same ABI version only)
    return os.environ.get("GSP_LIB_PATH") or os.path.join(_HERE, "lib", "libgpuspectral_pt.so")


def load():
    """Load the HIP library; raises if it has not been built (no fallback)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise GspError(
            "HIP library %s not found: build it with `make -C gpuspectral_amd/csrc` "
            "(or python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback." % path
        )
    L = C.CDLL(path)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.gsp_default_render_params.argtypes = [C.POINTER(abi.RenderParams)]
    L.gsp_default_render_params.restype = None
    L.gsp_abi_version.restype = C.c_int
    L.gsp_build_info.restype = C.c_char_p
    L.gsp_device_count.restype = C.c_int
    L.gsp_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.gsp_default_ctx_options.argtypes = [C.POINTER(abi.CtxOptions)]
    L.gsp_default_ctx_options.restype = None
    L.gsp_ctx_create_ex.argtypes = [C.c_int, C.POINTER(abi.CtxOptions), C.POINTER(vp)]
    L.gsp_update_camera.argtypes = [vp, C.POINTER(abi.Camera)]
    L.gsp_set_lens.argtypes = [vp, C.POINTER(abi.Lens)]
    L.gsp_focus_distance.argtypes = [vp, u32, u32, C.c_float, C.c_float, C.POINTER(C.c_float)]
    L.gsp_multi_set_lens.argtypes = [vp, C.POINTER(abi.Lens)]
    L.gsp_set_media.argtypes = [vp, C.POINTER(abi.Medium), u32]
    L.gsp_multi_set_media.argtypes = [vp, C.POINTER(abi.Medium), u32]
    L.gsp_set_media_scattering.argtypes = [vp, C.POINTER(abi.MediumScatter), u32]
    L.gsp_multi_set_media_scattering.argtypes = [vp, C.POINTER(abi.MediumScatter), u32]
    L.gsp_set_light_sampling.argtypes = [vp, u32]
    L.gsp_download_light_pick.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.gsp_multi_set_light_sampling.argtypes = [vp, u32]
    L.gsp_set_estimator.argtypes = [vp, u32]
    L.gsp_multi_set_estimator.argtypes = [vp, u32]
    L.gsp_set_delta_lights.argtypes = [vp, C.POINTER(abi.DeltaLight), u32]
    L.gsp_multi_set_delta_lights.argtypes = [vp, C.POINTER(abi.DeltaLight), u32]
    L.gsp_set_envmap_sampling.argtypes = [vp, C.POINTER(abi.EnvmapSampling)]
    L.gsp_multi_set_envmap_sampling.argtypes = [vp, C.POINTER(abi.EnvmapSampling)]
    L.gsp_set_light_grid.argtypes = [vp, C.POINTER(abi.LightGrid)]
    L.gsp_get_light_grid.argtypes = [vp, C.POINTER(abi.LightGrid), C.POINTER(C.c_float)]
    L.gsp_multi_set_light_grid.argtypes = [vp, C.POINTER(abi.LightGrid)]
    L.gsp_update_instances.argtypes = [vp, vp, u32]
    L.gsp_update_tables.argtypes = [vp, C.POINTER(abi.SceneDesc)]
    L.gsp_ctx_destroy.argtypes = [vp]
    L.gsp_ctx_destroy.restype = None
    L.gsp_upload_scene.argtypes = [vp, C.POINTER(abi.SceneDesc)]
    L.gsp_frame_begin.argtypes = [vp, u32, u32, vp, u64]
    L.gsp_render.argtypes = [vp, C.POINTER(abi.RenderParams)]
    L.gsp_download_pixel_stats.argtypes = [vp, vp, vp]
    L.gsp_sync.argtypes = [vp]
    L.gsp_download.argtypes = [vp, vp]
    L.gsp_download_compact.argtypes = [vp, vp]
    L.gsp_peek.argtypes = [vp, vp, vp]
    L.gsp_copy_accum_to_device.argtypes = [vp, vp, u64]
    L.gsp_peek_to_device.argtypes = [vp, vp, u64, C.POINTER(C.c_uint32)]
    L.gsp_upload_accum.argtypes = [vp, vp, u64]
    L.gsp_frame_luminance.argtypes = [vp, C.c_int, C.POINTER(abi.Luminance)]
    L.gsp_download_display.argtypes = [vp, C.POINTER(abi.Display), vp]
    L.gsp_peek_display.argtypes = [vp, C.POINTER(abi.Display), vp, C.POINTER(C.c_uint32)]
    L.gsp_peek_display_to_device.argtypes = [vp, C.POINTER(abi.Display), vp, u64, C.POINTER(C.c_uint32)]
    L.gsp_multi_download_display.argtypes = [vp, C.POINTER(abi.Display), vp]
    L.gsp_render_features.argtypes = [vp, C.POINTER(abi.RenderParams)]
    L.gsp_download_features.argtypes = [vp, vp, vp, vp]
    L.gsp_copy_features_to_device.argtypes = [vp, vp, vp, vp, u64]
    L.gsp_multi_render_features.argtypes = [vp, C.POINTER(abi.RenderParams)]
    L.gsp_multi_download_features.argtypes = [vp, vp, vp, vp]
    L.gsp_download_denoised.argtypes = [vp, C.POINTER(abi.Denoise), vp]
    L.gsp_denoise_to_device.argtypes = [vp, C.POINTER(abi.Denoise), vp, u64]
    L.gsp_download_denoised_display.argtypes = [vp, C.POINTER(abi.Denoise), C.POINTER(abi.Display), vp]
    L.gsp_multi_download_denoised.argtypes = [vp, C.POINTER(abi.Denoise), vp]
    L.gsp_temporal_accumulate.argtypes = [vp, C.POINTER(abi.Temporal)]
    L.gsp_temporal_reset.argtypes = [vp]
    L.gsp_frame_sample_base.argtypes = [vp, C.c_uint32]
    L.gsp_download_temporal.argtypes = [vp, vp]
    L.gsp_temporal_to_device.argtypes = [vp, vp, u64]
    L.gsp_download_temporal_denoised.argtypes = [vp, C.POINTER(abi.Denoise), vp]
    L.gsp_download_temporal_denoised_display.argtypes = [vp, C.POINTER(abi.Denoise), C.POINTER(abi.Display), vp]
    L.gsp_temporal_track_moments.argtypes = [vp, C.c_int]
    L.gsp_download_temporal_moments.argtypes = [vp, vp]
    L.gsp_download_temporal_svgf.argtypes = [vp, C.POINTER(abi.Denoise), C.POINTER(abi.Svgf), vp]
    L.gsp_temporal_svgf_to_device.argtypes = [vp, C.POINTER(abi.Denoise), C.POINTER(abi.Svgf), vp, u64]
    L.gsp_download_temporal_svgf_display.argtypes = [vp, C.POINTER(abi.Denoise), C.POINTER(abi.Svgf), C.POINTER(abi.Display), vp]
    L.gsp_temporal_follow_instances.argtypes = [vp, C.c_int]
    L.gsp_download_temporal_motion.argtypes = [vp, vp]
    L.gsp_temporal_motion_to_device.argtypes = [vp, vp, u64]
    L.gsp_temporal_demodulate.argtypes = [vp, C.c_int]
    L.gsp_download_temporal_image.argtypes = [vp, vp]
    L.gsp_temporal_image_to_device.argtypes = [vp, vp, u64]
    L.gsp_temporal_svgf_feedback.argtypes = [vp, C.POINTER(abi.Denoise), C.POINTER(abi.Svgf), C.c_uint32, vp]
    L.gsp_temporal_svgf_feedback_to_device.argtypes = [vp, C.POINTER(abi.Denoise), C.POINTER(abi.Svgf), C.c_uint32, vp, u64]
    L.gsp_temporal_antilag.argtypes = [vp, C.POINTER(abi.Antilag)]
    L.gsp_download_temporal_fast.argtypes = [vp, vp]
    L.gsp_temporal_fast_to_device.argtypes = [vp, vp, u64]
    L.gsp_temporal_taa.argtypes = [vp, C.POINTER(abi.Taa), C.POINTER(abi.Display), vp]
    L.gsp_temporal_taa_from_device.argtypes = [vp, C.POINTER(abi.Taa), C.POINTER(abi.Display), vp, u64]
    L.gsp_download_taa.argtypes = [vp, vp]
    L.gsp_download_taa_display.argtypes = [vp, vp]
    L.gsp_taa_display_to_device.argtypes = [vp, vp, u64]
    L.gsp_get_stats.argtypes = [vp, C.POINTER(abi.Stats)]
    L.gsp_reset_stats.argtypes = [vp]
    L.gsp_trace.argtypes = [vp, vp, u64, C.c_int, vp]
    L.gsp_debug_visit_histograms.argtypes = [vp, vp, u64, vp, u64]
    L.gsp_last_error.argtypes = [vp]
    L.gsp_last_error.restype = C.c_char_p
    L.gsp_tile_partition.argtypes = [u32, u32, u32, u32, u32, vp]
    L.gsp_tile_partition.restype = u64
    L.gsp_multi_create.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
    L.gsp_multi_create_ex.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(abi.CtxOptions), C.POINTER(vp)]
    L.gsp_multi_update_camera.argtypes = [vp, C.POINTER(abi.Camera)]
    L.gsp_multi_update_instances.argtypes = [vp, vp, u32]
    L.gsp_multi_update_tables.argtypes = [vp, C.POINTER(abi.SceneDesc)]
    L.gsp_multi_destroy.argtypes = [vp]
    L.gsp_multi_destroy.restype = None
    L.gsp_multi_num_shares.argtypes = [vp]
    L.gsp_multi_upload_scene.argtypes = [vp, C.POINTER(abi.SceneDesc)]
    L.gsp_multi_frame_begin.argtypes = [vp, u32, u32]
    L.gsp_multi_render.argtypes = [vp, C.POINTER(abi.RenderParams)]
    L.gsp_multi_sync.argtypes = [vp]
    L.gsp_multi_gather.argtypes = [vp, C.POINTER(vp)]
    L.gsp_multi_download.argtypes = [vp, vp]
    L.gsp_multi_get_stats.argtypes = [vp, C.POINTER(abi.Stats), C.POINTER(abi.Stats)]
    L.gsp_multi_reset_stats.argtypes = [vp]
    L.gsp_multi_gather_route.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.gsp_multi_last_error.argtypes = [vp]
    L.gsp_multi_last_error.restype = C.c_char_p
    v = L.gsp_abi_version()
    # (exact match: an older library fills arrays of gsp_stats at ITS struct size and knows nothing of gsp_render_params.disable_nee)
    if v != abi.GSP_ABI_VERSION:
        raise GspError("ABI version mismatch: abi.py is %d, %s is %d" % (abi.GSP_ABI_VERSION, path, v))
    _LIB = L
    return L


def device_count():
    return load().gsp_device_count()


def build_info():
    """What the loaded library was built from (gsp_build_info): {'arch', 'digest', 'flags'}."""
    text = load().gsp_build_info().decode()
    head, _, flags = text.partition(" flags=")
    info = dict(kv.split("=", 1) for kv in head.split())
    info["flags"] = flags
    return info


# the files csrc/Makefile hashes into the digest, in its order
DIGEST_SOURCES = ("pt_render.hip", "pt_render_textbook.hip", "pt_render_scatter.hip", "pt_render_delta.hip", "pt_render_envlight.hip", "pt_render_lightgrid.hip", "pt_bvh.hip", "pt_multi.hip", "pt_render_kernels.inc", "pt_render_scene.inc", "pt_render_pipeline.inc", "pt_render_post.inc", "pt_wavetrace.h", "pt_versions.h", "pt_hostmath.h", "pt_lightpick.h", "pt_math.h", "pt_shading.h",
                  "pt_medium.h", "pt_deltalight.h", "pt_envlight.h", "pt_lightgrid.h", "pt_trace.h", "pt_stages.h", "pt_internal.h", "pt_display.h", "pt_features.h", "pt_denoise.h", "pt_temporal.h", "pt_svgf.h", "pt_motion.h", "pt_illum.h", "pt_antilag.h", "pt_taa.h", "../../include/gpuspectral_pt.h")


def source_digest():
    """The digest csrc/Makefile would stamp into a library built from the tree as it is now."""
    import hashlib

    h = hashlib.sha256()
    for f in DIGEST_SOURCES:
        with open(os.path.join(_HERE, "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


HIT_DT = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("prim", "<i4")])


def _options(options, kw):
    """abi.CtxOptions from an explicit struct, keyword fields, or -- test / A-B tooling only -- the GSP_* environment."""
    if options is None:
        options = abi.options_from_env()
    for k, v in kw.items():
        setattr(options, k, v)
    return options


class Context:
    """One HIP device + stream + scene + accumulate buffer (gsp_context).

    options: abi.CtxOptions (gsp_ctx_options); keyword arguments set single fields (pool_paths=..., primary_memo=2, ...).
    Without either, this TEST binding maps the GSP_* variables of the A/B scripts onto the struct (abi.options_from_env);
    the library itself never reads the environment."""

    def __init__(self, device=0, options=None, **option_fields):
        self._L = load()
        h = C.c_void_p()
        self.options = _options(options, option_fields)
        rc = self._L.gsp_ctx_create_ex(device, C.byref(self.options), C.byref(h))
        if rc != 0:
            raise GspError("gsp_ctx_create_ex: %s" % self._L.gsp_last_error(None).decode())
        self._h = h
        self._scene = None
        self.width = self.height = 0
        self.num_pixels = 0

    def _check(self, rc, what):
        if rc != 0:
            raise GspError("%s failed (%d): %s" % (what, rc, self._L.gsp_last_error(self._h).decode()))

    def close(self):
        if getattr(self, "_h", None):
            self._L.gsp_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def upload_scene(self, scene):
        """scene: abi.SceneArrays."""
        d = scene.desc()
        self._scene = scene
        self._check(self._L.gsp_upload_scene(self._h, C.byref(d)), "gsp_upload_scene")

    def update_camera(self, to_world, fov):
        """gsp_update_camera: to_world = 16 floats in glm memory order, fov in radians."""
        cam = abi.Camera()
        for i, v in enumerate(np.asarray(to_world, np.float32).reshape(16)):
            cam.to_world[i] = float(v)
        cam.fov = float(fov)
        self._check(self._L.gsp_update_camera(self._h, C.byref(cam)), "gsp_update_camera")

    def set_lens(self, radius=0.0, focus_distance=0.0, blades=0, rotation=0.0, lens=None):
        """gsp_set_lens: thin-lens depth of field (gpuspectral_pt.h "Thin lens").  Context state: holds until changed; radius 0
        (or no argument) = the pinhole.  lens: an abi.Lens to pass as it is (None with no other argument = NULL)."""
        if lens is None:
            lens = abi.lens(radius, focus_distance, blades, rotation)
        self._check(self._L.gsp_set_lens(self._h, C.byref(lens)), "gsp_set_lens")

    def set_media(self, sigmas=None):
        """gsp_set_media: the table of interior media (gpuspectral_pt.h "Interior media"), a list of (r, g, b) absorption
        coefficients; medium number k of abi.bsdf_handle(.., medium=k) is sigmas[k - 1].  None or empty = no media."""
        arr = abi.media_array(sigmas)
        self._check(self._L.gsp_set_media(self._h, arr, len(arr) if arr is not None else 0), "gsp_set_media")

    def set_media_scattering(self, scatter=None):
        """gsp_set_media_scattering: the table parallel to set_media's (gpuspectral_pt.h "Scattering media"), one entry per medium:
        (r, g, b) scattering coefficients, or ((r, g, b), g) with the Henyey-Greenstein asymmetry.  None or empty = no scattering."""
        arr = abi.media_scatter_array(scatter)
        self._check(self._L.gsp_set_media_scattering(self._h, arr, len(arr) if arr is not None else 0), "gsp_set_media_scattering")

    def set_delta_lights(self, lights=None):
        """gsp_set_delta_lights (gpuspectral_pt.h "Delta lights"): a list of abi.DeltaLight (abi.point_light, spot_light,
        directional_light).  None or empty = no delta lights."""
        arr = abi.delta_light_array(lights)
        self._check(self._L.gsp_set_delta_lights(self._h, arr, len(arr) if arr is not None else 0), "gsp_set_delta_lights")

    def set_envmap_sampling(self, enabled=True, extent=1.0):
        """gsp_set_envmap_sampling (gpuspectral_pt.h "Environment light"): sample the scene's environment map as a light (textbook
        estimator only).  extent: the radius of the scene as the power pick is to see it.  enabled=False drops the sampling."""
        s = abi.EnvmapSampling(1, extent, (C.c_uint32 * 2)(0, 0)) if enabled else None
        self._check(self._L.gsp_set_envmap_sampling(self._h, C.byref(s) if s is not None else None), "gsp_set_envmap_sampling")

    def set_light_grid(self, enabled=True, resolution=None):
        """gsp_set_light_grid (gpuspectral_pt.h "Light grid"): spatial light selection, one alias table per cell of a grid over the
        scene (needs set_light_sampling("power") and set_estimator("textbook") first).  resolution: (nx, ny, nz), None = auto.
        enabled=False drops the grid."""
        s = abi.light_grid(resolution) if enabled else None
        self._check(self._L.gsp_set_light_grid(self._h, C.byref(s) if s is not None else None), "gsp_set_light_grid")

    def light_grid(self):
        """gsp_get_light_grid: (enabled, (nx, ny, nz), (lo, hi)) of the grid the resident tables were built with."""
        s, b = abi.LightGrid(), (C.c_float * 6)()
        self._check(self._L.gsp_get_light_grid(self._h, C.byref(s), b), "gsp_get_light_grid")
        return bool(s.enabled), tuple(s.resolution), (tuple(b[:3]), tuple(b[3:]))

    def set_estimator(self, mode):
        """gsp_set_estimator (gpuspectral_pt.h "Estimator"): "reference" / "textbook" or abi.ESTIMATOR_REFERENCE / ESTIMATOR_TEXTBOOK."""
        self._check(self._L.gsp_set_estimator(self._h, abi.estimator_mode(mode)), "gsp_set_estimator")

    def set_light_sampling(self, mode):
        """gsp_set_light_sampling (gpuspectral_pt.h "Light selection"): "uniform" / "power" or abi.LIGHTS_UNIFORM / LIGHTS_POWER."""
        self._check(self._L.gsp_set_light_sampling(self._h, abi.light_sampling_mode(mode)), "gsp_set_light_sampling")

    def download_light_pick(self):
        """gsp_download_light_pick: the resident alias table as an abi.LIGHT_PICK_DT array, one entry per light triangle."""
        n = C.c_uint32(0)
        self._L.gsp_download_light_pick(self._h, None, 0, C.byref(n))  # (the count; the call itself may be refused)
        out = np.zeros(n.value, abi.LIGHT_PICK_DT)
        self._check(self._L.gsp_download_light_pick(self._h, out.ctypes.data if n.value else None, n.value, C.byref(n)), "gsp_download_light_pick")
        return out

    def focus_distance(self, width, height, fx, fy):
        """gsp_focus_distance: camera-space depth of what the pinhole ray through fragCoord (fx, fy) hits, 0.0 on a miss."""
        out = C.c_float(0.0)
        self._check(self._L.gsp_focus_distance(self._h, width, height, fx, fy, C.byref(out)), "gsp_focus_distance")
        return np.float32(out.value)

    def update_instances(self, instances):
        """gsp_update_instances: abi.INSTANCE_DT records (same count and vertex ranges as the uploaded scene)."""
        inst = np.ascontiguousarray(instances, abi.INSTANCE_DT)
        self._check(self._L.gsp_update_instances(self._h, inst.ctypes.data if len(inst) else None, len(inst)), "gsp_update_instances")

    def update_tables(self, scene):
        """gsp_update_tables: the BSDF arrays and lights of `scene` (abi.SceneArrays) replace the resident ones."""
        d = scene.desc()
        self._check(self._L.gsp_update_tables(self._h, C.byref(d)), "gsp_update_tables")

    def frame_begin(self, width, height, pixel_ids=None):
        if pixel_ids is not None:
            pixel_ids = np.ascontiguousarray(pixel_ids, np.uint32)
            rc = self._L.gsp_frame_begin(self._h, width, height, pixel_ids.ctypes.data, len(pixel_ids))
            self.num_pixels = len(pixel_ids)
        else:
            rc = self._L.gsp_frame_begin(self._h, width, height, None, 0)
            self.num_pixels = width * height
        self._check(rc, "gsp_frame_begin")
        self.width, self.height = width, height

    def render(self, spp=1, first_timestamp=0, params=None, **overrides):
        """gsp_render.  Keyword arguments set single fields of gsp_render_params: adaptive_threshold=..., pixel_filter=abi.FILTER_TENT,
        pixel_filter_param=1.5 (anti-aliasing, gpuspectral_pt.h "Pixel filter"), timestamps_in_flight=..., ..."""
        p = params or abi.default_render_params()
        p.spp, p.first_timestamp = spp, first_timestamp
        for k, v in overrides.items():
            setattr(p, k, v)
        self._check(self._L.gsp_render(self._h, C.byref(p)), "gsp_render")

    def sync(self):
        self._check(self._L.gsp_sync(self._h), "gsp_sync")

    def peek(self):
        """(compact RGBA32F frame as it stands, timestamps folded into every pixel) without draining the pipeline."""
        out = np.zeros((self.num_pixels, 4), np.float32)
        folded = C.c_uint32(0)
        self._check(self._L.gsp_peek(self._h, out.ctypes.data, C.byref(folded)), "gsp_peek")
        return out, int(folded.value)

    def download(self, out=None):
        """The frame as (height, width, 4) float32; `out`: the caller's own framebuffer (C-contiguous float32 of that size)."""
        if out is None:
            out = np.zeros((self.height, self.width, 4), np.float32)
        assert out.dtype == np.float32 and out.size == self.height * self.width * 4 and out.flags.c_contiguous
        self._check(self._L.gsp_download(self._h, out.ctypes.data), "gsp_download")
        return out

    def download_compact(self):
        out = np.zeros((self.num_pixels, 4), np.float32)
        self._check(self._L.gsp_download_compact(self._h, out.ctypes.data), "gsp_download_compact")
        return out

    def copy_accum_to_device(self, device_ptr, nbytes):
        self._check(self._L.gsp_copy_accum_to_device(self._h, device_ptr, nbytes), "gsp_copy_accum_to_device")

    def peek_to_device(self, device_ptr, nbytes):
        """gsp_peek into device memory (e.g. a torch tensor's data_ptr()); returns the timestamps folded into every pixel."""
        folded = C.c_uint32(0)
        self._check(self._L.gsp_peek_to_device(self._h, device_ptr, nbytes, C.byref(folded)), "gsp_peek_to_device")
        return int(folded.value)

    # ---- LDR film (gpuspectral_pt.h "LDR film"); display: an abi.Display (abi.display(...)), None = NULL = clamp + sRGB ----
    def download_display(self, display=None):
        """gsp_download_display: the frame tone-mapped and encoded on the GPU, (height, width) uint32 RGBA8 words (R in bits 0-7)."""
        out = np.zeros((self.height, self.width), np.uint32)
        self._check(self._L.gsp_download_display(self._h, C.byref(display) if display is not None else None, out.ctypes.data), "gsp_download_display")
        return out

    def peek_display(self, display=None):
        """gsp_peek_display: (compact RGBA8 words of the frame as it stands, timestamps folded), no drain."""
        out = np.zeros(self.num_pixels, np.uint32)
        folded = C.c_uint32(0)
        self._check(self._L.gsp_peek_display(self._h, C.byref(display) if display is not None else None, out.ctypes.data, C.byref(folded)),
                    "gsp_peek_display")
        return out, int(folded.value)

    def peek_display_to_device(self, device_ptr, nbytes, display=None):
        """gsp_peek_display into device memory (e.g. a torch tensor's data_ptr()); returns the timestamps folded."""
        folded = C.c_uint32(0)
        self._check(self._L.gsp_peek_display_to_device(self._h, C.byref(display) if display is not None else None, device_ptr, nbytes,
                                                       C.byref(folded)), "gsp_peek_display_to_device")
        return int(folded.value)

    def frame_luminance(self, drain=True):
        """gsp_frame_luminance: {log_sum_q20, pixels, log_avg, max} over the owned finite pixels."""
        out = abi.Luminance()
        self._check(self._L.gsp_frame_luminance(self._h, 1 if drain else 0, C.byref(out)), "gsp_frame_luminance")
        return out.as_dict()

    # ---- feature buffers (gpuspectral_pt.h "Feature buffers") ----
    def render_features(self, spp=1, first_timestamp=0, params=None, **overrides):
        """gsp_render_features: spp feature samples (first hit of the beauty sample's camera ray) for every owned pixel; of the
        keyword fields only pixel_filter / pixel_filter_param are read."""
        p = params or abi.default_render_params()
        p.spp, p.first_timestamp = spp, first_timestamp
        for k, v in overrides.items():
            setattr(p, k, v)
        self._check(self._L.gsp_render_features(self._h, C.byref(p)), "gsp_render_features")

    def download_features(self, albedo=True, geom=True, ids=True):
        """gsp_download_features: (albedo[h,w,4] float32 {r,g,b,coverage}, geom[h,w,4] float32 {nx,ny,nz,depth}, ids[h,w,4] uint32
        {triangle, bsdf, instance, samples folded}); a plane switched off is None (its pointer is NULL)."""
        a = np.zeros((self.height, self.width, 4), np.float32) if albedo else None
        g = np.zeros((self.height, self.width, 4), np.float32) if geom else None
        i = np.zeros((self.height, self.width, 4), np.uint32) if ids else None
        self._check(self._L.gsp_download_features(self._h, *(x.ctypes.data if x is not None else None for x in (a, g, i))), "gsp_download_features")
        return a, g, i

    def copy_features_to_device(self, albedo_ptr, geom_ptr, ids_ptr, nbytes_each):
        """gsp_copy_features_to_device: the compact planes into device memory (e.g. torch tensors' data_ptr()); a pointer may be None."""
        self._check(self._L.gsp_copy_features_to_device(self._h, albedo_ptr, geom_ptr, ids_ptr, nbytes_each), "gsp_copy_features_to_device")

    # ---- denoiser (gpuspectral_pt.h "Denoiser"); denoise: an abi.Denoise (abi.denoise(...)), None = NULL = every default ----
    def download_denoised(self, denoise=None):
        """gsp_download_denoised: the frame through the edge-avoiding a-trous filter, guided by the feature planes of a
        render_features call of this frame; (height, width, 4) float32.  The frame itself is not changed."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.gsp_download_denoised(self._h, C.byref(denoise) if denoise is not None else None, out.ctypes.data), "gsp_download_denoised")
        return out

    def denoise_to_device(self, device_ptr, nbytes, denoise=None):
        """gsp_denoise_to_device: the denoised frame into device memory (e.g. a torch tensor's data_ptr()), width*height*16 bytes."""
        self._check(self._L.gsp_denoise_to_device(self._h, C.byref(denoise) if denoise is not None else None, device_ptr, nbytes), "gsp_denoise_to_device")

    def download_denoised_display(self, denoise=None, display=None):
        """gsp_download_denoised_display: the LDR film of the denoised frame, (height, width) uint32 RGBA8 words."""
        out = np.zeros((self.height, self.width), np.uint32)
        self._check(self._L.gsp_download_denoised_display(self._h, C.byref(denoise) if denoise is not None else None,
                                                          C.byref(display) if display is not None else None, out.ctypes.data),
                    "gsp_download_denoised_display")
        return out

    # ---- temporal accumulation (gpuspectral_pt.h "Temporal accumulation"); temporal: an abi.Temporal, None = every default ----
    def temporal_accumulate(self, temporal=None):
        """gsp_temporal_accumulate: reprojects the history of earlier frames into this frame's camera and blends this frame in.
        Once per frame_begin, after render and render_features.  The frame itself is not changed."""
        self._check(self._L.gsp_temporal_accumulate(self._h, C.byref(temporal) if temporal is not None else None), "gsp_temporal_accumulate")

    def frame_sample_base(self, base):
        """gsp_frame_sample_base: between frame_begin and the frame's first render -- the frame's samples keep timestamps base,
        base + 1, ... for their seeds and are folded as samples 0, 1, ... of the fresh frame (its plain mean)."""
        self._check(self._L.gsp_frame_sample_base(self._h, base), "gsp_frame_sample_base")

    def temporal_reset(self):
        """gsp_temporal_reset: forgets the history."""
        self._check(self._L.gsp_temporal_reset(self._h), "gsp_temporal_reset")

    def download_temporal(self):
        """gsp_download_temporal: the newest history, (height, width, 4) float32; .w = the history length."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.gsp_download_temporal(self._h, out.ctypes.data), "gsp_download_temporal")
        return out

    def temporal_to_device(self, device_ptr, nbytes):
        """gsp_temporal_to_device: the newest history into device memory (e.g. a torch tensor's data_ptr()), width*height*16 bytes."""
        self._check(self._L.gsp_temporal_to_device(self._h, device_ptr, nbytes), "gsp_temporal_to_device")

    def download_temporal_denoised(self, denoise=None):
        """gsp_download_temporal_denoised: the a-trous filter of the history, guided by this frame's feature planes."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.gsp_download_temporal_denoised(self._h, C.byref(denoise) if denoise is not None else None, out.ctypes.data),
                    "gsp_download_temporal_denoised")
        return out

    def download_temporal_denoised_display(self, denoise=None, display=None):
        """gsp_download_temporal_denoised_display: the LDR film of the filtered history, (height, width) uint32 RGBA8 words."""
        out = np.zeros((self.height, self.width), np.uint32)
        self._check(self._L.gsp_download_temporal_denoised_display(self._h, C.byref(denoise) if denoise is not None else None,
                                                                   C.byref(display) if display is not None else None, out.ctypes.data),
                    "gsp_download_temporal_denoised_display")
        return out

    # ---- variance-guided filter (gpuspectral_pt.h "Variance-guided filter"); svgf: an abi.Svgf, None = every default ----
    def temporal_track_moments(self, on=True):
        """gsp_temporal_track_moments: temporal_accumulate also keeps the luminance moments; a change drops the history."""
        self._check(self._L.gsp_temporal_track_moments(self._h, 1 if on else 0), "gsp_temporal_track_moments")

    def download_temporal_moments(self):
        """gsp_download_temporal_moments: the newest M = {m1, m2, r, 0}, (height, width, 4) float32."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.gsp_download_temporal_moments(self._h, out.ctypes.data), "gsp_download_temporal_moments")
        return out

    def download_temporal_svgf(self, denoise=None, svgf=None):
        """gsp_download_temporal_svgf: the variance-guided a-trous filter of the history; .w = the history length."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.gsp_download_temporal_svgf(self._h, C.byref(denoise) if denoise is not None else None,
                                                       C.byref(svgf) if svgf is not None else None, out.ctypes.data), "gsp_download_temporal_svgf")
        return out

    def temporal_svgf_to_device(self, device_ptr, nbytes, denoise=None, svgf=None):
        """gsp_temporal_svgf_to_device: the same frame into device memory (e.g. a torch tensor's data_ptr()), width*height*16 bytes."""
        self._check(self._L.gsp_temporal_svgf_to_device(self._h, C.byref(denoise) if denoise is not None else None,
                                                        C.byref(svgf) if svgf is not None else None, device_ptr, nbytes), "gsp_temporal_svgf_to_device")

    def download_temporal_svgf_display(self, denoise=None, svgf=None, display=None):
        """gsp_download_temporal_svgf_display: the LDR film of the variance-guided filter, (height, width) uint32 RGBA8 words."""
        out = np.zeros((self.height, self.width), np.uint32)
        self._check(self._L.gsp_download_temporal_svgf_display(self._h, C.byref(denoise) if denoise is not None else None,
                                                               C.byref(svgf) if svgf is not None else None,
                                                               C.byref(display) if display is not None else None, out.ctypes.data),
                    "gsp_download_temporal_svgf_display")
        return out

    # ---- moved instances (gpuspectral_pt.h "Temporal accumulation: moved instances") ----
    def temporal_follow_instances(self, on=True):
        """gsp_temporal_follow_instances: temporal_accumulate takes a pixel of a moved instance back through the instance's motion
        and writes the motion plane; a change drops the history.  An update_instances belongs before the frame's render_features."""
        self._check(self._L.gsp_temporal_follow_instances(self._h, 1 if on else 0), "gsp_temporal_follow_instances")

    def download_temporal_motion(self):
        """gsp_download_temporal_motion: V = {dx, dy, kept weight, class} of the newest accumulate, (height, width, 4) float32."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.gsp_download_temporal_motion(self._h, out.ctypes.data), "gsp_download_temporal_motion")
        return out

    def temporal_motion_to_device(self, dst, nbytes=None):
        """gsp_temporal_motion_to_device: V into device memory, width*height*16 bytes.  dst: a torch tensor on the context's device
        (its bytes from its storage offset on), or a device pointer with nbytes."""
        if hasattr(dst, "data_ptr"):
            ptr, nbytes = dst.data_ptr(), dst.numel() * dst.element_size()
        else:
            ptr = dst
        self._check(self._L.gsp_temporal_motion_to_device(self._h, ptr, nbytes), "gsp_temporal_motion_to_device")

    # ---- illumination history (gpuspectral_pt.h "Illumination history") ----
    def temporal_demodulate(self, on=True):
        """gsp_temporal_demodulate: the history accumulates colour / first-hit albedo; a change drops the history."""
        self._check(self._L.gsp_temporal_demodulate(self._h, 1 if on else 0), "gsp_temporal_demodulate")

    def download_temporal_image(self):
        """gsp_download_temporal_image: what a viewer shows of the newest history -- re-modulated by this frame's albedo while
        demodulation is on, the history itself otherwise; (height, width, 4) float32, .w = the history length."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.gsp_download_temporal_image(self._h, out.ctypes.data), "gsp_download_temporal_image")
        return out

    def temporal_image_to_device(self, dst, nbytes=None):
        """gsp_temporal_image_to_device: the same into device memory, width*height*16 bytes.  dst: a torch tensor on the context's
        device (its bytes from its storage offset on), or a device pointer with nbytes."""
        if hasattr(dst, "data_ptr"):
            ptr, nbytes = dst.data_ptr(), dst.numel() * dst.element_size()
        else:
            ptr = dst
        self._check(self._L.gsp_temporal_image_to_device(self._h, ptr, nbytes), "gsp_temporal_image_to_device")

    def temporal_svgf_feedback(self, denoise=None, svgf=None, levels=1, out=True):
        """gsp_temporal_svgf_feedback: download_temporal_svgf, and the output of the first `levels` levels becomes the colour of
        the newest history (once per temporal_accumulate).  out=False passes NULL: no output, returns None."""
        res = np.zeros((self.height, self.width, 4), np.float32) if out else None
        self._check(self._L.gsp_temporal_svgf_feedback(self._h, C.byref(denoise) if denoise is not None else None,
                                                       C.byref(svgf) if svgf is not None else None, levels, res.ctypes.data if out else None),
                    "gsp_temporal_svgf_feedback")
        return res

    def temporal_svgf_feedback_to_device(self, dst, nbytes=None, denoise=None, svgf=None, levels=1):
        """gsp_temporal_svgf_feedback_to_device: the same with the output in device memory.  dst: a torch tensor, a device pointer
        with nbytes, or None (no output)."""
        if dst is None:
            ptr, nbytes = None, 0
        elif hasattr(dst, "data_ptr"):
            ptr, nbytes = dst.data_ptr(), dst.numel() * dst.element_size()
        else:
            ptr = dst
        self._check(self._L.gsp_temporal_svgf_feedback_to_device(self._h, C.byref(denoise) if denoise is not None else None,
                                                                 C.byref(svgf) if svgf is not None else None, levels, ptr, nbytes),
                    "gsp_temporal_svgf_feedback_to_device")

    # ---- temporal anti-lag (gpuspectral_pt.h "Temporal anti-lag") ----
    def temporal_antilag(self, antilag=None):
        """gsp_temporal_antilag: accumulates the fast history of the frame's temporal_accumulate and clamps the newest history into
        the box of its window statistics (once per temporal_accumulate, before any temporal_svgf_feedback).  antilag: an
        abi.Antilag, None = every default."""
        self._check(self._L.gsp_temporal_antilag(self._h, C.byref(antilag) if antilag is not None else None), "gsp_temporal_antilag")

    def download_temporal_fast(self):
        """gsp_download_temporal_fast: the newest fast history, (height, width, 4) float32, .w = its length."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.gsp_download_temporal_fast(self._h, out.ctypes.data), "gsp_download_temporal_fast")
        return out

    def temporal_fast_to_device(self, dst, nbytes=None):
        """gsp_temporal_fast_to_device: the same into device memory, width*height*16 bytes.  dst: a torch tensor on the context's
        device (its bytes from its storage offset on), or a device pointer with nbytes."""
        if hasattr(dst, "data_ptr"):
            ptr, nbytes = dst.data_ptr(), dst.numel() * dst.element_size()
        else:
            ptr = dst
        self._check(self._L.gsp_temporal_fast_to_device(self._h, ptr, nbytes), "gsp_temporal_fast_to_device")

    # ---- temporal anti-aliasing (gpuspectral_pt.h "Temporal anti-aliasing") ----
    def temporal_taa(self, taa=None, display=None, src=None):
        """gsp_temporal_taa: resolves the tone-mapped frame over its history D (once per temporal_accumulate, following on).  taa: an
        abi.Taa, display: an abi.Display, None = every default.  src: the HDR frame, (height, width, 4) float32 in host memory; None
        = the image of the newest history."""
        if src is not None:
            src = np.ascontiguousarray(src, np.float32)
            if src.size != self.height * self.width * 4:
                raise ValueError("temporal_taa: src must hold height*width*4 floats")
        self._check(self._L.gsp_temporal_taa(self._h, C.byref(taa) if taa is not None else None, C.byref(display) if display is not None else None,
                                             src.ctypes.data if src is not None else None), "gsp_temporal_taa")

    def temporal_taa_from_device(self, src, nbytes=None, taa=None, display=None):
        """gsp_temporal_taa_from_device: the same with the HDR frame in device memory, width*height*16 bytes of any alignment.  src:
        a torch tensor on the context's device (its bytes from its storage offset on), a device pointer with nbytes, or None (the
        image of the newest history)."""
        if src is None:
            ptr, nbytes = None, 0
        elif hasattr(src, "data_ptr"):
            ptr, nbytes = src.data_ptr(), src.numel() * src.element_size()
        else:
            ptr = src
        self._check(self._L.gsp_temporal_taa_from_device(self._h, C.byref(taa) if taa is not None else None,
                                                         C.byref(display) if display is not None else None, ptr, nbytes), "gsp_temporal_taa_from_device")

    def download_taa(self):
        """gsp_download_taa: the newest resolved frame D', (height, width, 4) float32 of display-linear colour, .w = 1 where the pixel
        was blended with its history."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.gsp_download_taa(self._h, out.ctypes.data), "gsp_download_taa")
        return out

    def download_taa_display(self):
        """gsp_download_taa_display: the encode of D' under the display of the last resolve, (height, width) uint32 RGBA8 words."""
        out = np.zeros((self.height, self.width), np.uint32)
        self._check(self._L.gsp_download_taa_display(self._h, out.ctypes.data), "gsp_download_taa_display")
        return out

    def taa_display_to_device(self, dst, nbytes=None):
        """gsp_taa_display_to_device: the same into device memory, width*height*4 bytes.  dst: a torch tensor on the context's device
        (its bytes from its storage offset on), or a device pointer with nbytes."""
        if hasattr(dst, "data_ptr"):
            ptr, nbytes = dst.data_ptr(), dst.numel() * dst.element_size()
        else:
            ptr = dst
        self._check(self._L.gsp_taa_display_to_device(self._h, ptr, nbytes), "gsp_taa_display_to_device")

    def pixel_stats(self):
        """Adaptive frame (ABI 9): (m2[n] float32, spp[n] uint32) of the owned pixels in pixel_ids order -- the running mean of
        Y^2 over each pixel's samples and the samples folded into it (gsp_download_pixel_stats)."""
        m2 = np.zeros(self.num_pixels, np.float32)
        spp = np.zeros(self.num_pixels, np.uint32)
        self._check(self._L.gsp_download_pixel_stats(self._h, m2.ctypes.data, spp.ctypes.data), "gsp_download_pixel_stats")
        return m2, spp

    def upload_accum(self, rgba):
        rgba = np.ascontiguousarray(rgba, np.float32).reshape(-1, 4)
        self._check(self._L.gsp_upload_accum(self._h, rgba.ctypes.data, len(rgba)), "gsp_upload_accum")

    def stats(self):
        s = abi.Stats()
        self._check(self._L.gsp_get_stats(self._h, C.byref(s)), "gsp_get_stats")
        return s.as_dict()

    def reset_stats(self):
        self._check(self._L.gsp_reset_stats(self._h), "gsp_reset_stats")

    def visit_histograms(self):
        """(visits per node index, tests per triangle slot) of the closest-hit rays traced with collect_traversal_stats=2."""
        st = self.stats()
        nodes = np.zeros(int(st["num_bvh_nodes"]), np.uint32)
        slots = np.zeros(int(st["num_triangles"]) + 8, np.uint32)
        self._check(self._L.gsp_debug_visit_histograms(self._h, nodes.ctypes.data, len(nodes), slots.ctypes.data, len(slots)),
                    "gsp_debug_visit_histograms")
        return nodes, slots

    def trace(self, rays, any_hit=False):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        hits = np.zeros(len(rays), HIT_DT)
        self._check(self._L.gsp_trace(self._h, rays.ctypes.data, len(rays), 1 if any_hit else 0, hits.ctypes.data),
                    "gsp_trace")
        return hits


def tile_partition(width, height, rank, world, tile=32):
    """Pixel ids of share `rank` of `world` (gsp_tile_partition: the C++ partition every multi-GPU path uses)."""
    L = load()
    n = L.gsp_tile_partition(width, height, rank, world, tile, None)
    ids = np.empty(n, np.uint32)
    if n:
        L.gsp_tile_partition(width, height, rank, world, tile, ids.ctypes.data)
    return ids


class MultiContext:
    """One frame over several GPUs of one node in ONE process (gsp_multi): tile partition, one host thread per share,
    device-to-device gather into the first device.  `devices` may repeat an index (several shares on one GPU)."""

    def __init__(self, devices, options=None, **option_fields):
        self._L = load()
        devs = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        self.options = _options(options, option_fields)
        rc = self._L.gsp_multi_create_ex(devs, len(devices), C.byref(self.options), C.byref(h))
        if rc != 0:
            raise GspError("gsp_multi_create_ex: %s" % self._L.gsp_multi_last_error(None).decode())
        self._h = h
        self._scene = None
        self.width = self.height = 0
        self.num_shares = len(devices)

    def _check(self, rc, what):
        if rc != 0:
            raise GspError("%s failed (%d): %s" % (what, rc, self._L.gsp_multi_last_error(self._h).decode()))

    def close(self):
        if getattr(self, "_h", None):
            self._L.gsp_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def upload_scene(self, scene):
        d = scene.desc()
        self._scene = scene
        self._check(self._L.gsp_multi_upload_scene(self._h, C.byref(d)), "gsp_multi_upload_scene")

    def update_camera(self, to_world, fov):
        cam = abi.Camera()
        for i, v in enumerate(np.asarray(to_world, np.float32).reshape(16)):
            cam.to_world[i] = float(v)
        cam.fov = float(fov)
        self._check(self._L.gsp_multi_update_camera(self._h, C.byref(cam)), "gsp_multi_update_camera")

    def set_lens(self, radius=0.0, focus_distance=0.0, blades=0, rotation=0.0, lens=None):
        """gsp_multi_set_lens: Context.set_lens on every share."""
        if lens is None:
            lens = abi.lens(radius, focus_distance, blades, rotation)
        self._check(self._L.gsp_multi_set_lens(self._h, C.byref(lens)), "gsp_multi_set_lens")

    def set_media(self, sigmas=None):
        """gsp_multi_set_media: Context.set_media on every share."""
        arr = abi.media_array(sigmas)
        self._check(self._L.gsp_multi_set_media(self._h, arr, len(arr) if arr is not None else 0), "gsp_multi_set_media")

    def set_delta_lights(self, lights=None):
        """gsp_multi_set_delta_lights: Context.set_delta_lights on every share."""
        arr = abi.delta_light_array(lights)
        self._check(self._L.gsp_multi_set_delta_lights(self._h, arr, len(arr) if arr is not None else 0), "gsp_multi_set_delta_lights")

    def set_envmap_sampling(self, enabled=True, extent=1.0):
        """gsp_multi_set_envmap_sampling: Context.set_envmap_sampling on every share."""
        s = abi.EnvmapSampling(1, extent, (C.c_uint32 * 2)(0, 0)) if enabled else None
        self._check(self._L.gsp_multi_set_envmap_sampling(self._h, C.byref(s) if s is not None else None), "gsp_multi_set_envmap_sampling")

    def set_light_grid(self, enabled=True, resolution=None):
        """gsp_multi_set_light_grid: Context.set_light_grid on every share."""
        s = abi.light_grid(resolution) if enabled else None
        self._check(self._L.gsp_multi_set_light_grid(self._h, C.byref(s) if s is not None else None), "gsp_multi_set_light_grid")

    def set_media_scattering(self, scatter=None):
        """gsp_multi_set_media_scattering: Context.set_media_scattering on every share."""
        arr = abi.media_scatter_array(scatter)
        self._check(self._L.gsp_multi_set_media_scattering(self._h, arr, len(arr) if arr is not None else 0), "gsp_multi_set_media_scattering")

    def set_estimator(self, mode):
        """gsp_multi_set_estimator: Context.set_estimator on every share."""
        self._check(self._L.gsp_multi_set_estimator(self._h, abi.estimator_mode(mode)), "gsp_multi_set_estimator")

    def set_light_sampling(self, mode):
        """gsp_multi_set_light_sampling: Context.set_light_sampling on every share."""
        self._check(self._L.gsp_multi_set_light_sampling(self._h, abi.light_sampling_mode(mode)), "gsp_multi_set_light_sampling")

    def update_instances(self, instances):
        inst = np.ascontiguousarray(instances, abi.INSTANCE_DT)
        self._check(self._L.gsp_multi_update_instances(self._h, inst.ctypes.data if len(inst) else None, len(inst)),
                    "gsp_multi_update_instances")

    def update_tables(self, scene):
        d = scene.desc()
        self._check(self._L.gsp_multi_update_tables(self._h, C.byref(d)), "gsp_multi_update_tables")

    def frame_begin(self, width, height):
        self._check(self._L.gsp_multi_frame_begin(self._h, width, height), "gsp_multi_frame_begin")
        self.width, self.height = width, height

    def render(self, spp=1, first_timestamp=0, params=None, **overrides):
        """gsp_multi_render: as Context.render (pixel_filter= / pixel_filter_param= included; adaptive sampling is refused)."""
        p = params or abi.default_render_params()
        p.spp, p.first_timestamp = spp, first_timestamp
        for k, v in overrides.items():
            setattr(p, k, v)
        self._check(self._L.gsp_multi_render(self._h, C.byref(p)), "gsp_multi_render")

    def sync(self):
        self._check(self._L.gsp_multi_sync(self._h), "gsp_multi_sync")

    def gather(self):
        """Assemble the frame on the first device; returns its device pointer (0 for a single share)."""
        p = C.c_void_p()
        self._check(self._L.gsp_multi_gather(self._h, C.byref(p)), "gsp_multi_gather")
        return p.value or 0

    def download(self):
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.gsp_multi_download(self._h, out.ctypes.data), "gsp_multi_download")
        return out

    def download_display(self, display=None):
        """gsp_multi_download_display: Context.download_display of the gathered frame."""
        out = np.zeros((self.height, self.width), np.uint32)
        self._check(self._L.gsp_multi_download_display(self._h, C.byref(display) if display is not None else None, out.ctypes.data),
                    "gsp_multi_download_display")
        return out

    def render_features(self, spp=1, first_timestamp=0, params=None, **overrides):
        """gsp_multi_render_features: Context.render_features on every share."""
        p = params or abi.default_render_params()
        p.spp, p.first_timestamp = spp, first_timestamp
        for k, v in overrides.items():
            setattr(p, k, v)
        self._check(self._L.gsp_multi_render_features(self._h, C.byref(p)), "gsp_multi_render_features")

    def download_features(self):
        """gsp_multi_download_features: Context.download_features of the gathered planes."""
        a = np.zeros((self.height, self.width, 4), np.float32)
        g = np.zeros((self.height, self.width, 4), np.float32)
        i = np.zeros((self.height, self.width, 4), np.uint32)
        self._check(self._L.gsp_multi_download_features(self._h, a.ctypes.data, g.ctypes.data, i.ctypes.data), "gsp_multi_download_features")
        return a, g, i

    def download_denoised(self, denoise=None):
        """gsp_multi_download_denoised: Context.download_denoised of the gathered frame and planes."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self._L.gsp_multi_download_denoised(self._h, C.byref(denoise) if denoise is not None else None, out.ctypes.data),
                    "gsp_multi_download_denoised")
        return out

    def stats(self, per_share=False):
        tot = abi.Stats()
        each = (abi.Stats * self.num_shares)()
        self._check(self._L.gsp_multi_get_stats(self._h, C.byref(tot), each), "gsp_multi_get_stats")
        return (tot.as_dict(), [e.as_dict() for e in each]) if per_share else tot.as_dict()

    def gather_route(self):
        """("rccl" | "copy", gathers carried by RCCL so far, gathers carried by peer copies so far)."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        r = self._L.gsp_multi_gather_route(self._h, C.byref(a), C.byref(b))
        return ("rccl" if r == 1 else "copy"), a.value, b.value

    def reset_stats(self):
        self._check(self._L.gsp_multi_reset_stats(self._h), "gsp_multi_reset_stats")
