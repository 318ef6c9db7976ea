"""ctypes / numpy mirror of ``include/gpuspectral_pt.h`` (the C-ABI boundary).

Nothing here computes anything: it only describes the POD layouts so that
Python callers (tests, bench.py) can hand arrays to the C ABI.  Layouts follow
the reference's scalar structs (S/renderer/Scene.h:29-109).
"""
import ctypes as C

import numpy as np

GSP_ABI_VERSION = 9
ADAPTIVE_LUMINANCE_FLOOR = 1e-3  # GSP_ADAPTIVE_LUMINANCE_FLOOR

BSDF_DIFFUSE = 0
BSDF_SMOOTH_DIELECTRIC = 1
BSDF_SMOOTH_CONDUCTOR = 2
BSDF_SMOOTH_PLASTIC = 3
BSDF_ROUGH_CONDUCTOR = 4
BSDF_SMOOTH_FLOOR = 5
BSDF_ROUGH_FLOOR = 6
BSDF_ROUGH_PLASTIC = 7
BSDF_TYPE_COUNT = 8

BSDF_NAMES = (
    "diffuse",
    "smooth_dielectric",
    "smooth_conductor",
    "smooth_plastic",
    "rough_conductor",
    "smooth_floor",
    "rough_floor",
    "rough_plastic",
)


MAX_MEDIA = 4095


def bsdf_handle(btype, index, medium=0):
    """(type << 16) | index -- S/renderer/Scene.h:83-97; medium: GSP_BSDF_HANDLE_MEDIUM, the interior medium's number in bits
    19..30 (0 = none, k = media[k - 1] of Context.set_media)."""
    return ((int(btype) & 0xFFFF) << 16) | (int(index) & 0xFFFF) | ((int(medium) & 0xFFF) << 19)


# numpy record layouts (all tightly packed, 4-byte scalars)
DIFFUSE_DT = np.dtype([("reflectance", "<f4", 3), ("has_texture", "<i4")])
SMOOTH_DIELECTRIC_DT = np.dtype([("ior_in", "<f4"), ("ior_out", "<f4")])
SMOOTH_CONDUCTOR_DT = np.dtype([("ior_in", "<f4"), ("ior_out", "<f4")])
SMOOTH_PLASTIC_DT = np.dtype([("diffuse", "<f4", 3), ("ior_in", "<f4"), ("ior_out", "<f4"), ("r0", "<f4")])
ROUGH_CONDUCTOR_DT = np.dtype(
    [("eta", "<f4", 3), ("k", "<f4", 3), ("reflectance", "<f4", 3), ("alpha", "<f4"), ("has_texture", "<i4")]
)
SMOOTH_FLOOR_DT = np.dtype([("diffuse", "<f4", 3), ("r0", "<f4")])
ROUGH_FLOOR_DT = np.dtype([("diffuse", "<f4", 3), ("r0", "<f4"), ("alpha", "<f4")])
ROUGH_PLASTIC_DT = np.dtype(
    [
        ("diffuse", "<f4", 3),
        ("ior_in", "<f4"),
        ("ior_out", "<f4"),
        ("r0", "<f4"),
        ("alpha", "<f4"),
        ("has_texture", "<i4"),
    ]
)
BSDF_DTYPES = (
    DIFFUSE_DT,
    SMOOTH_DIELECTRIC_DT,
    SMOOTH_CONDUCTOR_DT,
    SMOOTH_PLASTIC_DT,
    ROUGH_CONDUCTOR_DT,
    SMOOTH_FLOOR_DT,
    ROUGH_FLOOR_DT,
    ROUGH_PLASTIC_DT,
)
BSDF_SIZES = (16, 8, 8, 24, 44, 16, 20, 32)
assert tuple(d.itemsize for d in BSDF_DTYPES) == BSDF_SIZES

LIGHT_DT = np.dtype([("positions", "<f4", (3, 4)), ("radiance", "<f4", 4)])
assert LIGHT_DT.itemsize == 64

INSTANCE_DT = np.dtype(
    [
        ("transform", "<f4", 16),
        ("emission", "<f4", 3),
        ("bsdf", "<u4"),
        ("twofaced", "<u4"),
        ("first_vertex", "<u4"),
        ("vertex_count", "<u4"),
    ]
)
assert INSTANCE_DT.itemsize == 92


class Camera(C.Structure):
    _fields_ = [("to_world", C.c_float * 16), ("fov", C.c_float)]


TEXTURE_DT = np.dtype([("width", "<u4"), ("height", "<u4"), ("first_texel", "<u8")])  # gsp_texture, 16 B


class Envmap(C.Structure):  # gsp_envmap
    _fields_ = [("texels", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("to_local", C.c_float * 16)]


class SceneDesc(C.Structure):
    _fields_ = [
        ("instances", C.c_void_p),
        ("num_instances", C.c_uint32),
        ("positions", C.c_void_p),
        ("normals", C.c_void_p),
        ("num_vertices", C.c_uint64),
        ("diffuse_bsdfs", C.c_void_p),
        ("smooth_dielectric_bsdfs", C.c_void_p),
        ("smooth_conductor_bsdfs", C.c_void_p),
        ("smooth_plastic_bsdfs", C.c_void_p),
        ("rough_conductor_bsdfs", C.c_void_p),
        ("smooth_floor_bsdfs", C.c_void_p),
        ("rough_floor_bsdfs", C.c_void_p),
        ("rough_plastic_bsdfs", C.c_void_p),
        ("num_bsdfs", C.c_uint32 * BSDF_TYPE_COUNT),
        ("lights", C.c_void_p),
        ("num_lights", C.c_uint32),
        ("camera", Camera),
        # dormant-feature extension (textures / environment map); all zero = the reference's behaviour
        ("uvs", C.c_void_p),
        ("textures", C.c_void_p),
        ("num_textures", C.c_uint32),
        ("texels", C.c_void_p),
        ("num_texels", C.c_uint64),
        ("texel_decode", C.c_void_p),
        ("envmap", Envmap),
    ]


class RenderParams(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),  # (ABI 8) sizeof the host's struct; 0 = the ABI-8 layout
        ("spp", C.c_uint32),
        ("first_timestamp", C.c_uint32),
        ("max_depth", C.c_uint32),
        ("rr_start_depth", C.c_uint32),
        ("clamp", C.c_float),
        ("timestamps_in_flight", C.c_uint32),
        ("collect_traversal_stats", C.c_uint32),
        ("collect_kernel_times", C.c_uint32),
        ("disable_nee", C.c_uint32),  # (ABI 7) RenderParams.nee inverted, PathTracer.h:36-41; 0 = the shipped shader (`#define NEE true`)
        # (ABI 9) adaptive sampling: 0 = off; > 0 = stop a pixel once its relative standard error is at most this (gpuspectral_pt.h)
        ("adaptive_threshold", C.c_float),
        ("adaptive_min_spp", C.c_uint32),  # first checkpoint, 0 = 16
        ("adaptive_step", C.c_uint32),  # samples between checkpoints, 0 = 16
        # pixel filter (added at the end under the struct_size rule, ABI still 9): FILTER_*; 0 = the reference as shipped
        ("pixel_filter", C.c_uint32),
        ("pixel_filter_param", C.c_float),  # tent radius (0 = 1.0) / Gaussian standard deviation (0 = 0.5), in pixels
    ]


class Lens(C.Structure):
    """gsp_lens (include/gpuspectral_pt.h "Thin lens"): context state set with gsp_set_lens; radius 0 = the pinhole."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("radius", C.c_float),
        ("focus_distance", C.c_float),
        ("blades", C.c_uint32),  # 0 = circle, 3..16 = polygon
        ("rotation", C.c_float),  # radians
    ]


def lens(radius=0.0, focus_distance=0.0, blades=0, rotation=0.0):
    return Lens(C.sizeof(Lens), radius, focus_distance, blades, rotation)


class Medium(C.Structure):
    """gsp_medium (include/gpuspectral_pt.h "Interior media"): a pure absorber, sigma_a per channel in 1 / length."""

    _fields_ = [("sigma_a", C.c_float * 3), ("reserved", C.c_float)]


def media_array(sigmas):
    """[(r, g, b), ...] -> (Medium * n), or None for an empty list."""
    sigmas = [tuple(float(x) for x in s) for s in (sigmas if sigmas is not None else [])]
    if not sigmas:
        return None
    return (Medium * len(sigmas))(*[Medium((C.c_float * 3)(*s), 0.0) for s in sigmas])


class MediumScatter(C.Structure):
    """gsp_medium_scatter (include/gpuspectral_pt.h "Scattering media"): sigma_s per channel in 1 / length, Henyey-Greenstein g."""

    _fields_ = [("sigma_s", C.c_float * 3), ("g", C.c_float)]


def media_scatter_array(scatter):
    """[(r, g, b) or ((r, g, b), g_hg), ...] -> (MediumScatter * n), or None for an empty list."""
    out = []
    for e in (scatter if scatter is not None else []):
        e = tuple(e)
        sig, g = (e[0], e[1]) if len(e) == 2 and hasattr(e[0], "__len__") else (e, 0.0)
        out.append(MediumScatter((C.c_float * 3)(*[float(x) for x in sig]), float(g)))
    return (MediumScatter * len(out))(*out) if out else None


# Delta lights (include/gpuspectral_pt.h "Delta lights")
LIGHT_POINT, LIGHT_SPOT, LIGHT_DIRECTIONAL = 1, 2, 3


class DeltaLight(C.Structure):
    """gsp_delta_light, 64 B: a point, spot or directional emitter."""

    _fields_ = [("position", C.c_float * 3), ("kind", C.c_uint32), ("direction", C.c_float * 3), ("cos_cutoff", C.c_float),
                ("intensity", C.c_float * 3), ("cos_beam", C.c_float), ("extent", C.c_float), ("reserved", C.c_float * 3)]


def point_light(position, intensity):
    return DeltaLight((C.c_float * 3)(*position), LIGHT_POINT, (C.c_float * 3)(0, 0, 0), 0.0, (C.c_float * 3)(*intensity), 0.0, 0.0, (C.c_float * 3)(0, 0, 0))


def spot_light(position, direction, intensity, cos_cutoff, cos_beam):
    """direction: unit, the spot's axis (the way the light travels); the cosines of the cutoff angle and of the beam width."""
    return DeltaLight((C.c_float * 3)(*position), LIGHT_SPOT, (C.c_float * 3)(*direction), cos_cutoff, (C.c_float * 3)(*intensity), cos_beam, 0.0,
                      (C.c_float * 3)(0, 0, 0))


def directional_light(direction, irradiance, extent):
    """direction: unit, the way the light travels; extent: the radius of the scene as the power pick is to see it."""
    return DeltaLight((C.c_float * 3)(0, 0, 0), LIGHT_DIRECTIONAL, (C.c_float * 3)(*direction), 0.0, (C.c_float * 3)(*irradiance), 0.0, extent,
                      (C.c_float * 3)(0, 0, 0))


def delta_light_array(lights):
    """[DeltaLight, ...] -> (DeltaLight * n), or None for an empty list."""
    lights = list(lights) if lights is not None else []
    return (DeltaLight * len(lights))(*lights) if lights else None


# Environment light (include/gpuspectral_pt.h "Environment light")
LIGHT_ENVIRONMENT = 4  # internal: the kind word of the environment record


class EnvmapSampling(C.Structure):
    """gsp_envmap_sampling, 16 B"""

    _fields_ = [("enabled", C.c_uint32), ("extent", C.c_float), ("reserved", C.c_uint32 * 2)]


# Light grid (include/gpuspectral_pt.h "Light grid")
class LightGrid(C.Structure):
    """gsp_light_grid, 32 B"""

    _fields_ = [("enabled", C.c_uint32), ("resolution", C.c_uint32 * 3), ("reserved", C.c_uint32 * 4)]


def light_grid(resolution=None):
    """An enabled gsp_light_grid: resolution (nx, ny, nz), or None = auto"""
    nx, ny, nz = (0, 0, 0) if resolution is None else resolution
    return LightGrid(1, (C.c_uint32 * 3)(nx, ny, nz), (C.c_uint32 * 4)(0, 0, 0, 0))


# Light selection (include/gpuspectral_pt.h "Light selection")
LIGHTS_UNIFORM, LIGHTS_POWER = 0, 1
LIGHT_SAMPLING_NAMES = {"uniform": LIGHTS_UNIFORM, "power": LIGHTS_POWER}
LIGHT_PICK_DT = np.dtype([("threshold", "<u4"), ("alias", "<u4"), ("pmf_self", "<f4"), ("pmf_alias", "<f4")])  # gsp_light_pick, 16 B


def light_sampling_mode(mode):
    """A mode name or number -> the number gsp_set_light_sampling takes (an unknown number goes through: the library refuses it)."""
    if isinstance(mode, str):
        if mode not in LIGHT_SAMPLING_NAMES:
            raise ValueError("light sampling mode %r: one of %s" % (mode, ", ".join(sorted(LIGHT_SAMPLING_NAMES))))
        return LIGHT_SAMPLING_NAMES[mode]
    return int(mode)


# Estimator (include/gpuspectral_pt.h "Estimator")
ESTIMATOR_REFERENCE, ESTIMATOR_TEXTBOOK = 0, 1
ESTIMATOR_NAMES = {"reference": ESTIMATOR_REFERENCE, "textbook": ESTIMATOR_TEXTBOOK}


def estimator_mode(mode):
    """A mode name or number -> the number gsp_set_estimator takes (an unknown number goes through: the library refuses it)."""
    if isinstance(mode, str):
        if mode not in ESTIMATOR_NAMES:
            raise ValueError("estimator %r: one of %s" % (mode, ", ".join(sorted(ESTIMATOR_NAMES))))
        return ESTIMATOR_NAMES[mode]
    return int(mode)


# LDR film (include/gpuspectral_pt.h "LDR film")
TONEMAP_CLAMP, TONEMAP_REINHARD, TONEMAP_ACES = 0, 1, 2
TONEMAP_NAMES = {"clamp": TONEMAP_CLAMP, "reinhard": TONEMAP_REINHARD, "aces": TONEMAP_ACES}


class Display(C.Structure):
    """gsp_display: how gsp_download_display / gsp_peek_display turn the accumulate buffer into RGBA8; all zero = clamp + sRGB."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("tonemap", C.c_uint32),  # TONEMAP_*
        ("exposure", C.c_float),  # f-stops
        ("gamma", C.c_float),  # > 0: v^(1/gamma); 0 = the sRGB curve
        ("key", C.c_float),  # Reinhard; 0 = 0.18
        ("burn", C.c_float),
        ("log_avg_luminance", C.c_float),  # Reinhard: > 0 = use this value, 0 = measure the frame
        ("max_luminance", C.c_float),
    ]


def display(tonemap=TONEMAP_CLAMP, exposure=0.0, gamma=0.0, key=0.0, burn=0.0, log_avg_luminance=0.0, max_luminance=0.0):
    return Display(C.sizeof(Display), tonemap, exposure, gamma, key, burn, log_avg_luminance, max_luminance)


class Denoise(C.Structure):
    """gsp_denoise: the edge-avoiding a-trous denoiser's parameters (gsp_download_denoised); all zero = every default."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("iterations", C.c_uint32),  # 0 = 5; otherwise 1..8
        ("sigma_color", C.c_float),  # 0 = default, +inf = the term is off
        ("sigma_normal", C.c_float),
        ("sigma_depth", C.c_float),
        ("sigma_albedo", C.c_float),
    ]


def denoise(iterations=0, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0):
    return Denoise(C.sizeof(Denoise), iterations, sigma_color, sigma_normal, sigma_depth, sigma_albedo)


class Temporal(C.Structure):
    """gsp_temporal: the parameters of temporal accumulation (gsp_temporal_accumulate); all zero = every default."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("max_history", C.c_uint32),  # 0 = 32; otherwise 1..65536
        ("alpha", C.c_float),  # 0 = 0.2; otherwise (0, 1]; FLT_MIN = the pure running mean
        ("depth_tolerance", C.c_float),  # 0 = 0.02
        ("normal_min", C.c_float),  # 0 = 0.9; otherwise [-1, 1]
    ]


def temporal(max_history=0, alpha=0.0, depth_tolerance=0.0, normal_min=0.0):
    return Temporal(C.sizeof(Temporal), max_history, alpha, depth_tolerance, normal_min)


class Svgf(C.Structure):
    """gsp_svgf: the parameters of the variance-guided filter (gsp_download_temporal_svgf); all zero = every default."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("min_history", C.c_uint32),  # 0 = 4; otherwise 2..65536
        ("sigma_variance", C.c_float),  # 0 = 4.0; +inf = the term is off
    ]


def svgf(min_history=0, sigma_variance=0.0):
    return Svgf(C.sizeof(Svgf), min_history, sigma_variance)


class Antilag(C.Structure):
    """gsp_antilag: the parameters of the temporal anti-lag (gsp_temporal_antilag); all zero = every default."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("fast_history", C.c_uint32),  # 0 = 4; otherwise 1..64
        ("radius", C.c_uint32),  # 0 = 2 (5 x 5); otherwise 1..3
        ("sigma_scale", C.c_float),  # 0 = 2.0; otherwise > 0 and finite
    ]


def antilag(fast_history=0, radius=0, sigma_scale=0.0):
    return Antilag(C.sizeof(Antilag), fast_history, radius, sigma_scale)


class Taa(C.Structure):
    """gsp_taa: the parameters of temporal anti-aliasing (gsp_temporal_taa); all zero = every default."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("alpha", C.c_float),  # weight of the new frame; 0 = 0.1; otherwise (0, 1]
        ("sigma_clip", C.c_float),  # half-width of the neighbourhood box in standard deviations; 0 = 1.0; otherwise > 0 and finite
    ]


def taa(alpha=0.0, sigma_clip=0.0):
    return Taa(C.sizeof(Taa), alpha, sigma_clip)


class Luminance(C.Structure):
    """gsp_luminance: the frame statistics of the Reinhard operator (gsp_frame_luminance)."""

    _fields_ = [("log_sum_q20", C.c_int64), ("pixels", C.c_uint64), ("log_avg", C.c_float), ("max", C.c_float)]

    def as_dict(self):
        return dict(log_sum_q20=int(self.log_sum_q20), pixels=int(self.pixels), log_avg=float(self.log_avg), max=float(self.max))


# gsp_render_params.pixel_filter (GSP_FILTER_*, include/gpuspectral_pt.h "Pixel filter")
FILTER_NONE, FILTER_BOX, FILTER_TENT, FILTER_GAUSSIAN = 0, 1, 2, 3
FILTER_NAMES = {"none": FILTER_NONE, "box": FILTER_BOX, "tent": FILTER_TENT, "gaussian": FILTER_GAUSSIAN}


def default_render_params(spp=1, first_timestamp=0):
    """The reference's shader literals: raygen.rgen:27,60,66; rayhit.rchit:656."""
    return RenderParams(C.sizeof(RenderParams), spp, first_timestamp, 50, 10, 20.0, 0, 0, 0, 0)


GATHER_AUTO, GATHER_RCCL, GATHER_COPY = 0, 1, 2


class CtxOptions(C.Structure):
    """gsp_ctx_options (ABI 5, refit_growth: 6); a field left 0 means "default"."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("lanes", C.c_uint32),
        ("pool_paths", C.c_uint64),
        ("ring_bytes", C.c_uint64),
        ("memory_share", C.c_double),
        ("primary_memo", C.c_uint32),
        ("finish_paths", C.c_uint32),
        ("reinsert_rounds", C.c_uint32),
        ("gather_route", C.c_uint32),
        ("refit_growth", C.c_double),  # (ABI 6) 0 default (1.25); <= 1: gsp_update_instances always rebuilds
        ("geometry_versions", C.c_uint32),  # (r05) slots of the geometry ring: 0 default (as many as fit, <= 64), 1 = none
        ("reserved_", C.c_uint32),
    ]

    def __init__(self, **kw):
        super().__init__(**kw)
        self.struct_size = C.sizeof(CtxOptions)


def options_from_env(env=None):
    """TEST / A-B TOOLING: the GSP_* variables the probe scripts of earlier rounds set, mapped onto gsp_ctx_options (the
    library itself never reads the environment).  GSP_POOL_PATHS, GSP_RING_BYTES, GSP_MEMORY_SHARE, GSP_PRIMARY_MEMO=0|1,
    GSP_FINISH_PATHS (0 = never), GSP_LANES, GSP_BVH_REINSERT=rounds, GSP_MULTI_GATHER=rccl|copy."""
    import os

    e = os.environ if env is None else env
    o = CtxOptions()
    if "GSP_POOL_PATHS" in e:
        o.pool_paths = int(e["GSP_POOL_PATHS"])
    if "GSP_RING_BYTES" in e:
        o.ring_bytes = int(e["GSP_RING_BYTES"])
    if "GSP_MEMORY_SHARE" in e:
        o.memory_share = float(e["GSP_MEMORY_SHARE"])
    if "GSP_PRIMARY_MEMO" in e:
        o.primary_memo = 1 if int(e["GSP_PRIMARY_MEMO"]) else 2
    if "GSP_FINISH_PATHS" in e:
        o.finish_paths = int(e["GSP_FINISH_PATHS"]) or 0xFFFFFFFF
    if "GSP_LANES" in e:
        o.lanes = int(e["GSP_LANES"])
    if "GSP_BVH_REINSERT" in e:
        o.reinsert_rounds = int(e["GSP_BVH_REINSERT"]) + 1
    if "GSP_MULTI_GATHER" in e:
        o.gather_route = {"rccl": GATHER_RCCL, "copy": GATHER_COPY}.get(e["GSP_MULTI_GATHER"], GATHER_AUTO)
    return o


class Stats(C.Structure):
    _fields_ = [
        ("extension_rays", C.c_uint64),
        ("shadow_rays", C.c_uint64),
        ("shaded_vertices", C.c_uint64),
        ("samples", C.c_uint64),
        ("nodes_visited", C.c_uint64),
        ("tris_tested", C.c_uint64),
        ("stat_rays", C.c_uint64),
        ("shadow_nodes_visited", C.c_uint64),
        ("shadow_tris_tested", C.c_uint64),
        ("shadow_stat_rays", C.c_uint64),
        ("render_seconds", C.c_double),
        ("extend_kernel_ms", C.c_double),
        ("extend_launches", C.c_uint64),
        ("shade_kernel_ms", C.c_double),
        ("connect_kernel_ms", C.c_double),
        ("bvh_build_ms", C.c_double),
        ("num_triangles", C.c_uint64),
        ("num_bvh_nodes", C.c_uint64),
        ("device_bytes", C.c_uint64),
        ("algorithmic_bytes", C.c_uint64),
        ("memoised_rays", C.c_uint64),
        ("memo_build_rays", C.c_uint64),
        ("bvh_depth", C.c_uint64),
        ("nodes_from_lds", C.c_uint64),
        ("shadow_nodes_from_lds", C.c_uint64),
        ("shadow_stat_occluded", C.c_uint64),
        ("shadow_stat_occluded_nodes", C.c_uint64),
        ("scene_updates", C.c_uint64),
        ("scene_refits", C.c_uint64),  # (ABI 6)
        ("shadow_stat_no_triangle", C.c_uint64),  # (ABI 7)
        ("scene_drains", C.c_uint64),  # (ABI 7)
        ("scene_splits", C.c_uint64),  # (ABI 7)
        ("adaptive_rounds", C.c_uint64),  # (ABI 9)
        ("adaptive_active_pixels", C.c_uint64),  # (ABI 9) 0 = the adaptive frame has converged
    ]

    def as_dict(self):
        d = {name: getattr(self, name) for name, _ in self._fields_}
        # rays that were actually traced: path segments answered from the primary-hit memo are not
        d["traced_rays"] = d["extension_rays"] - d["memoised_rays"] + d["memo_build_rays"] + d["shadow_rays"]
        return d


class SceneArrays:
    """A flattened scene held in numpy arrays, convertible to ``SceneDesc``.

    This is the POD form of the reference's ``Scene`` (S/renderer/Scene.h:140-186)
    that crosses the C ABI.
    """

    def __init__(self):
        self.instances = np.zeros(0, INSTANCE_DT)
        self.positions = np.zeros((0, 3), np.float32)
        self.normals = np.zeros((0, 3), np.float32)
        self.bsdfs = [np.zeros(0, dt) for dt in BSDF_DTYPES]
        self.lights = np.zeros(0, LIGHT_DT)
        self.to_world = np.eye(4, dtype=np.float32).T.reshape(16).copy()  # glm memory order
        self.fov = np.float32(0.5)
        # dormant-feature extension (include/gpuspectral_pt.h): absent by default
        self.uvs = None            # (num_vertices, 2) float32
        self.textures = np.zeros(0, TEXTURE_DT)
        self.texels = np.zeros(0, np.uint32)     # RGBA8, all textures back to back
        self.texel_decode = None   # 256 float32, None = byte / 255
        self.env_texels = None     # (height, width, 4) float32, rows bottom-up
        self.env_to_local = np.eye(4, dtype=np.float32).reshape(16).copy()

    def add_texture(self, rgba8):
        """Append an (H, W, 4) uint8 image whose row 0 is the BOTTOM row; returns the has_texture value (index + 1)."""
        img = np.ascontiguousarray(rgba8, np.uint8)
        h, w = img.shape[:2]
        t = np.zeros(1, TEXTURE_DT)
        t["width"], t["height"], t["first_texel"] = w, h, len(self.texels)
        self.textures = np.concatenate([self.textures, t])
        self.texels = np.concatenate([self.texels, img.reshape(-1, 4).view("<u4").reshape(-1)])
        return len(self.textures)

    @property
    def num_triangles(self):
        return int(self.instances["vertex_count"].sum() // 3) if len(self.instances) else 0

    def desc(self):
        """Build a ``SceneDesc`` pointing at this object's arrays (keep `self` alive)."""
        self.instances = np.ascontiguousarray(self.instances, INSTANCE_DT)
        self.positions = np.ascontiguousarray(self.positions, np.float32).reshape(-1, 3)
        self.normals = np.ascontiguousarray(self.normals, np.float32).reshape(-1, 3)
        self.bsdfs = [np.ascontiguousarray(b, dt) for b, dt in zip(self.bsdfs, BSDF_DTYPES)]
        self.lights = np.ascontiguousarray(self.lights, LIGHT_DT)
        d = SceneDesc()
        d.instances = self.instances.ctypes.data
        d.num_instances = len(self.instances)
        d.positions = self.positions.ctypes.data
        d.normals = self.normals.ctypes.data
        d.num_vertices = len(self.positions)
        for name, arr in zip(BSDF_NAMES, self.bsdfs):
            setattr(d, name + "_bsdfs", arr.ctypes.data if len(arr) else None)
        for i, arr in enumerate(self.bsdfs):
            d.num_bsdfs[i] = len(arr)
        d.lights = self.lights.ctypes.data if len(self.lights) else None
        d.num_lights = len(self.lights)
        for i in range(16):
            d.camera.to_world[i] = float(self.to_world[i])
        d.camera.fov = float(self.fov)
        if len(self.textures):
            if self.uvs is None:
                self.uvs = np.zeros((len(self.positions), 2), np.float32)
            self.uvs = np.ascontiguousarray(self.uvs, np.float32).reshape(-1, 2)
            assert len(self.uvs) == len(self.positions)
            self.textures = np.ascontiguousarray(self.textures, TEXTURE_DT)
            self.texels = np.ascontiguousarray(self.texels, np.uint32)
            d.uvs = self.uvs.ctypes.data
            d.textures = self.textures.ctypes.data
            d.num_textures = len(self.textures)
            d.texels = self.texels.ctypes.data
            d.num_texels = len(self.texels)
            if self.texel_decode is not None:
                self.texel_decode = np.ascontiguousarray(self.texel_decode, np.float32)
                assert self.texel_decode.shape == (256,)
                d.texel_decode = self.texel_decode.ctypes.data
        if self.env_texels is not None:
            self.env_texels = np.ascontiguousarray(self.env_texels, np.float32)
            h, w = self.env_texels.shape[:2]
            d.envmap.texels = self.env_texels.ctypes.data
            d.envmap.width, d.envmap.height = w, h
            for i in range(16):
                d.envmap.to_local[i] = float(self.env_to_local[i])
        return d

    def save(self, path):
        """Write the flattened scene as one .npz (the POD arrays that cross the C ABI)."""
        np.savez_compressed(
            path, instances=self.instances, positions=self.positions, normals=self.normals, lights=self.lights,
            to_world=np.asarray(self.to_world, np.float32), fov=np.float32(self.fov),
            **{"bsdf_" + n: b for n, b in zip(BSDF_NAMES, self.bsdfs)}, **self._extension_arrays())

    def _extension_arrays(self):
        ext = {}
        if len(self.textures):
            ext.update(uvs=self.uvs, textures=self.textures, texels=self.texels)
            if self.texel_decode is not None:
                ext["texel_decode"] = self.texel_decode
        if self.env_texels is not None:
            ext.update(env_texels=self.env_texels, env_to_local=self.env_to_local)
        return ext

    @classmethod
    def load(cls, path):
        z = np.load(path)
        s = cls()
        s.instances = z["instances"].astype(INSTANCE_DT)
        s.positions, s.normals, s.lights = z["positions"], z["normals"], z["lights"].astype(LIGHT_DT)
        s.bsdfs = [z["bsdf_" + n].astype(dt) for n, dt in zip(BSDF_NAMES, BSDF_DTYPES)]
        s.to_world, s.fov = z["to_world"].copy(), np.float32(z["fov"])
        if "textures" in z:
            s.uvs, s.textures, s.texels = z["uvs"], z["textures"].astype(TEXTURE_DT), z["texels"]
            s.texel_decode = z["texel_decode"] if "texel_decode" in z else None
        if "env_texels" in z:
            s.env_texels, s.env_to_local = z["env_texels"], z["env_to_local"]
        return s
