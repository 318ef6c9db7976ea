/*
 * gpuspectral_pt.h -- C ABI of the MI355X-native path-tracing integrator.
 *
 * This is the drop-in boundary for the reference's PathTracer render pass
 * (sunho/GPUSpectral).  Everything a reference maintainer needs in order to
 * replace `PathTracer::createRenderPass` + the Vulkan ray-tracing pipeline
 * with the HIP wavefront tracer is declared here: plain pointers and sizes,
 * `extern "C"`, no C++/torch types.
 *
 * Reference interfaces each entry point replaces (S/ = src/GPUSpectral/):
 *   gsp_ctx_create / gsp_ctx_destroy
 *        PathTracer::PathTracer(Renderer&) + setup()           S/renderer/PathTracer.h:50-53, PathTracer.cpp:5-7
 *        (the Vulkan device/driver objects it borrows)         S/renderer/Renderer.cpp:19-45
 *   gsp_upload_scene
 *        PathTracer::prepareScene (instance table, 8 BSDF
 *        arrays, light array)                                  S/renderer/PathTracer.cpp:58-93
 *        Renderer::getOrCreateBLAS / HwDriver::createTLAS      S/renderer/Renderer.cpp:122-131, PathTracer.cpp:10-19
 *        (vkCmdBuildAccelerationStructuresKHR)                 S/backend/vulkan/VulkanRays.cpp:6-86,91-181
 *   gsp_update_camera / gsp_update_instances / gsp_update_tables   (ABI 5)
 *        what the reference re-reads on EVERY createRenderPass while the BLAS of a mesh stays cached by mesh id:
 *        renderState.camera                                     S/renderer/PathTracer.cpp:88-90
 *        the TLAS over obj.transform + the per-object Instance
 *        records (transformInvT, emission, bsdf, twofaced)     S/renderer/PathTracer.cpp:10-19,58-70
 *        the eight BSDF tables and the triangle lights          S/renderer/PathTracer.cpp:74-87
 *   gsp_ctx_create_ex / gsp_ctx_options
 *        the knobs of the device objects PathTracer borrows     S/renderer/Renderer.cpp:19-45 (none are per-pass there;
 *        here: path-pool size, result ring, memory share, ...)
 *   gsp_frame_begin
 *        accumulateBuffer = createTexture(RGBA32F, W, H)       S/renderer/PathTracer.cpp:5-7
 *   gsp_render
 *        driver.traceRays(pipeline, W, H) once per sample      S/renderer/PathTracer.cpp:24-39,
 *        (raygen.rgen + rayhit.rchit + miss shaders)           S/backend/vulkan/VulkanDriver.cpp:319-347
 *   gsp_download / gsp_download_compact / gsp_peek / gsp_peek_to_device / gsp_copy_accum_to_device
 *        the RGBA32F accumulateBuffer the blit pass samples    S/renderer/PathTracer.cpp:41-55, raygen.rgen:84-108
 *   gsp_last_error
 *        std::runtime_error thrown by the driver               e.g. S/backend/vulkan/VulkanDevice.cpp:31,58,66
 *   gsp_multi_* (one frame over the N GPUs of a node; the reference has one VkDevice: Renderer.cpp:19-45)
 *        the same calls as above, applied to every GPU's share of the frame: the image is cut into interleaved
 *        32x32 tiles (gsp_tile_partition), the scene is replicated, and gsp_multi_download gathers the HDR tiles
 *        into GPU 0 over xGMI before the one copy to the host                                SURVEY.md 8(e)
 *
 * All structs are POD with the reference's scalar layouts
 * (S/renderer/Scene.h:29-109) so the reference's std::vectors can be passed
 * by pointer without repacking.
 *
 * Threading: one host thread per context.  All device work is queued on the
 * context's own HIP stream; gsp_render is asynchronous, the download calls and
 * gsp_sync block.
 */
#ifndef GPUSPECTRAL_PT_H
#define GPUSPECTRAL_PT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSP_ABI_VERSION 9 /* 8: gsp_render_params.struct_size (first field); 2: gsp_multi_*, gsp_tile_partition, gsp_stats.algorithmic_bytes; 4: gsp_stats.memoised_rays, memo_build_rays, bvh_depth;
                             5: gsp_update_camera / _instances / _tables (+ gsp_multi_*), gsp_ctx_options + gsp_ctx_create_ex /
                                gsp_multi_create_ex, gsp_render_params.nee, gsp_stats.scene_updates;
                             6: gsp_update_instances refits the tree (gsp_ctx_options.refit_growth, gsp_stats.scene_refits);
                             7: gsp_render_params.nee -> disable_nee (a zeroed struct is the reference as shipped),
                                gsp_stats.shadow_stat_no_triangle;
                             9: adaptive sampling: gsp_render_params.adaptive_threshold / _min_spp / _step,
                                gsp_download_pixel_stats, gsp_stats.adaptive_rounds / adaptive_active_pixels;
                                additions within version 9 (new exports only, no struct changed): gsp_set_lens,
                                gsp_multi_set_lens, gsp_focus_distance (see "Thin lens"); gsp_frame_luminance, gsp_download_display,
                                gsp_peek_display, gsp_peek_display_to_device, gsp_multi_download_display (see "LDR film");
                                gsp_render_features, gsp_download_features, gsp_copy_features_to_device,
                                gsp_multi_render_features, gsp_multi_download_features (see "Feature buffers");
                                gsp_download_denoised, gsp_denoise_to_device, gsp_download_denoised_display,
                                gsp_multi_download_denoised (see "Denoiser"); gsp_temporal_accumulate, gsp_temporal_reset,
                                gsp_download_temporal, gsp_temporal_to_device, gsp_download_temporal_denoised,
                                gsp_download_temporal_denoised_display, gsp_frame_sample_base (see "Temporal accumulation");
                                gsp_temporal_track_moments, gsp_download_temporal_moments, gsp_download_temporal_svgf,
                                gsp_temporal_svgf_to_device, gsp_download_temporal_svgf_display (see "Variance-guided filter");
                                gsp_temporal_follow_instances, gsp_download_temporal_motion, gsp_temporal_motion_to_device
                                (see "Temporal accumulation: moved instances");
                                gsp_temporal_demodulate, gsp_download_temporal_image, gsp_temporal_image_to_device,
                                gsp_temporal_svgf_feedback, gsp_temporal_svgf_feedback_to_device (see "Illumination history");
                                gsp_temporal_antilag, gsp_download_temporal_fast, gsp_temporal_fast_to_device (see "Temporal
                                anti-lag"); gsp_temporal_taa, gsp_temporal_taa_from_device, gsp_download_taa,
                                gsp_download_taa_display, gsp_taa_display_to_device (see "Temporal anti-aliasing");
                                gsp_set_media, gsp_multi_set_media (see "Interior media");
                                gsp_set_light_sampling, gsp_download_light_pick, gsp_multi_set_light_sampling (see "Light
                                selection"); gsp_set_estimator, gsp_multi_set_estimator (see "Estimator");
                                gsp_set_media_scattering, gsp_multi_set_media_scattering (see "Scattering media");
                                gsp_set_delta_lights, gsp_multi_set_delta_lights (see "Delta lights");
                                gsp_set_envmap_sampling, gsp_multi_set_envmap_sampling (see "Environment light");
                                gsp_set_light_grid, gsp_get_light_grid, gsp_multi_set_light_grid (see "Light grid") */

/* ---- status codes (0 = ok); the message is at gsp_last_error(ctx) ---- */
#define GSP_OK 0
#define GSP_ERR_INVALID 1 /* bad argument / call order            */
#define GSP_ERR_DEVICE 2  /* HIP runtime error                    */
#define GSP_ERR_NOMEM 3   /* device or host allocation failed     */
#define GSP_ERR_SCENE 4   /* scene description is inconsistent    */

/* ---- BSDF type ids: S/assets/shaders/BSDF.inc:1-8, rayhit.rchit:332-339 ---- */
#define GSP_BSDF_DIFFUSE 0
#define GSP_BSDF_SMOOTH_DIELECTRIC 1
#define GSP_BSDF_SMOOTH_CONDUCTOR 2
#define GSP_BSDF_SMOOTH_PLASTIC 3
#define GSP_BSDF_ROUGH_CONDUCTOR 4
#define GSP_BSDF_SMOOTH_FLOOR 5
#define GSP_BSDF_ROUGH_FLOOR 6
#define GSP_BSDF_ROUGH_PLASTIC 7
#define GSP_BSDF_TYPE_COUNT 8

/* handle = (type << 16) | index        S/renderer/Scene.h:83-97, pt_common.glsl:30-42 */
#define GSP_BSDF_HANDLE(type, index) ((((uint32_t)(type)) << 16) | ((uint32_t)(index) & 0xFFFFu))
/* ... with an interior medium (see "Interior media"): bits 19..30 = medium number, 0 = none, k = media[k - 1] of gsp_set_media */
#define GSP_MAX_MEDIA 4095u
#define GSP_BSDF_HANDLE_MEDIUM(type, index, medium) (GSP_BSDF_HANDLE(type, index) | ((((uint32_t)(medium)) & 0xFFFu) << 19))

/* ---- BSDF parameter records, scalar layout = S/renderer/Scene.h:29-81 ---- */
typedef struct gsp_diffuse_bsdf {
  float reflectance[3];
  int32_t has_texture; /* never set by the reference loader.  0 = none; k > 0 = gsp_scene_desc.textures[k - 1] replaces
                          `reflectance` (dormant-feature extension below); the same in the two other records with this field */
} gsp_diffuse_bsdf; /* 16 B */

typedef struct gsp_smooth_dielectric_bsdf {
  float ior_in;
  float ior_out;
} gsp_smooth_dielectric_bsdf; /* 8 B */

typedef struct gsp_smooth_conductor_bsdf {
  float ior_in;
  float ior_out;
} gsp_smooth_conductor_bsdf; /* 8 B */

typedef struct gsp_smooth_plastic_bsdf {
  float diffuse[3];
  float ior_in;
  float ior_out;
  float r0;
} gsp_smooth_plastic_bsdf; /* 24 B */

typedef struct gsp_rough_conductor_bsdf {
  float eta[3];
  float k[3];
  float reflectance[3];
  float alpha;
  int32_t has_texture;
} gsp_rough_conductor_bsdf; /* 44 B */

typedef struct gsp_smooth_floor_bsdf {
  float diffuse[3];
  float r0;
} gsp_smooth_floor_bsdf; /* 16 B */

typedef struct gsp_rough_floor_bsdf {
  float diffuse[3];
  float r0;
  float alpha;
} gsp_rough_floor_bsdf; /* 20 B */

typedef struct gsp_rough_plastic_bsdf {
  float diffuse[3];
  float ior_in;
  float ior_out;
  float r0;
  float alpha;
  int32_t has_texture;
} gsp_rough_plastic_bsdf; /* 32 B */

/* S/renderer/Scene.h:106-109; rayhit.rchit:17-20 (world space, built on the host) */
typedef struct gsp_triangle_light {
  float positions[3][4];
  float radiance[4];
} gsp_triangle_light; /* 64 B */

/*
 * One render object = one TLAS instance (S/renderer/PathTracer.cpp:12-17,60-70).
 * `transform` is the glm::mat4 object-to-world matrix in glm's memory order
 * (column-major: transform[4*c + r]).  Vertices [first_vertex, first_vertex +
 * vertex_count) of the shared position/normal arrays are the instance's
 * de-indexed mesh: three consecutive vertices form one triangle
 * (S/renderer/Mesh.cpp:7-51, rayhit.rchit:670).
 */
typedef struct gsp_instance {
  float transform[16];
  float emission[3];
  uint32_t bsdf;     /* GSP_BSDF_HANDLE */
  uint32_t twofaced; /* Material::twofaced */
  uint32_t first_vertex;
  uint32_t vertex_count; /* multiple of 3 */
} gsp_instance; /* 92 B */

/* S/renderer/PathTracer.h:10-15: eye = to_world column 3, fov in radians */
typedef struct gsp_camera {
  float to_world[16]; /* glm memory order (column-major) */
  float fov;
} gsp_camera;

/*
 * ---- Dormant features of the reference, SURVEY 8(f).3: bitmap / checkerboard textures and an environment map ----
 * The reference declares them -- `hasTexture` in DiffuseBSDF / RoughConductorBSDF / RoughPlasticBSDF
 * (S/renderer/Scene.h:31,66,75; rayhit.rchit:24,54,63), `Scene::envMap` + `Envmap` (Scene.h:116-119,182), the loaders
 * loadTexture / loadHdrTexture (S/engine/Loader.cpp:66-116), the texture and emitter branches (:122-143,338-346) --
 * but the branches are commented out, no shader samples a texture and the closest-hit shader passes uv = vec2(0)
 * (rayhit.rchit:716,729).  A scene loaded the reference's way therefore never sets any field below, and all-zero
 * (absent) reproduces the reference exactly.  When a caller does set them, the semantics are the ones the declarations
 * imply, fixed here because no running reference code defines them:
 *   texture    RGBA8 texels, rows bottom-up as loadTexture writes them (Loader.cpp:74-81: image row height-1 first), so
 *              v = 0 is the bottom of the image; channel value = texel_decode[byte] (NULL: byte / 255); repeat wrap,
 *              bilinear filter, texel centres at (i + 0.5) / width; A ignored
 *   uv         per-vertex (Mesh Vertex::uv, Loader.cpp:50-52), interpolated with the hit's barycentrics like the normal
 *   where      a record with has_texture = k > 0 takes its kD (Diffuse::reflectance, RoughConductor::reflectance,
 *              RoughPlastic::diffuse: the `vec3 kD = bsdf.reflectance` lines, rayhit.rchit:342,352,512,526,552,574) from
 *              textures[k - 1] at the hit's uv
 *   envmap     RGBA32F lat-long image, rows bottom-up as loadHdrTexture writes them (Loader.cpp:103-110); a path that
 *              escapes the scene (miss.rmiss) adds weight * texel(direction) behind the firefly test like any emitted term;
 *              light sampling does not see it (sampleLight draws triangle lights only, rayhit.rchit:123-153).  Direction d
 *              (world) -> e = to_local * d; u = atan2(e.x, -e.z) / 2pi + 0.5, v = 1 - atan2(|e.xz|, e.y) / pi; wrap in u,
 *              clamp in v, bilinear.
 */
typedef struct gsp_texture {
  uint32_t width, height;
  uint64_t first_texel; /* index of texel (0, 0) in gsp_scene_desc.texels */
} gsp_texture;          /* 16 B */

typedef struct gsp_envmap {
  const float* texels; /* width * height RGBA32F, NULL = no environment map */
  uint32_t width, height;
  float to_local[16];  /* world -> envmap frame, glm memory order (the inverse of Envmap::transform, Scene.h:118; the
                          host inverts it so that no matrix inversion sits on the parity path) */
} gsp_envmap;

typedef struct gsp_scene_desc {
  const gsp_instance* instances;
  uint32_t num_instances;
  const float* positions; /* tight float3, object space */
  const float* normals;   /* tight float3, object space */
  uint64_t num_vertices;

  const gsp_diffuse_bsdf* diffuse_bsdfs;
  const gsp_smooth_dielectric_bsdf* smooth_dielectric_bsdfs;
  const gsp_smooth_conductor_bsdf* smooth_conductor_bsdfs;
  const gsp_smooth_plastic_bsdf* smooth_plastic_bsdfs;
  const gsp_rough_conductor_bsdf* rough_conductor_bsdfs;
  const gsp_smooth_floor_bsdf* smooth_floor_bsdfs;
  const gsp_rough_floor_bsdf* rough_floor_bsdfs;
  const gsp_rough_plastic_bsdf* rough_plastic_bsdfs;
  uint32_t num_bsdfs[GSP_BSDF_TYPE_COUNT]; /* indexed by GSP_BSDF_* */

  const gsp_triangle_light* lights;
  uint32_t num_lights;

  gsp_camera camera;

  /* dormant-feature extension (see above); all zero = the reference's behaviour */
  const float* uvs;             /* tight float2 per vertex (same indexing as positions), or NULL */
  const gsp_texture* textures;
  uint32_t num_textures;
  const uint32_t* texels;       /* RGBA8, R in bits 0-7 */
  uint64_t num_texels;
  const float* texel_decode;    /* 256 floats (e.g. an sRGB -> linear table), or NULL = byte / 255 */
  gsp_envmap envmap;
} gsp_scene_desc;

/*
 * Integrator constants.  Defaults (gsp_default_render_params) are the
 * reference's shader literals: MAX_DEPTH 50 (raygen.rgen:27), Russian
 * roulette when depth > 10 (raygen.rgen:66), firefly cutoff 20 (raygen.rgen:60).
 */
typedef struct gsp_render_params {
  uint32_t struct_size;     /* (ABI 8) sizeof(gsp_render_params) of the host's header; gsp_default_render_params sets it.  The library
                               reads min(struct_size, its own size) bytes and takes the fields beyond as 0 (= the reference's
                               behaviour, for every field added so far and from here on), so a host built against an older
                               header of ABI >= 8 keeps working.  0 (a zero-initialised struct) = the ABI-8 layout */
  uint32_t spp;             /* samples per pixel to add in this call      */
  uint32_t first_timestamp; /* RenderParams.timestamp of the first sample */
  uint32_t max_depth;
  uint32_t rr_start_depth;
  float clamp;
  uint32_t timestamps_in_flight; /* samples traced concurrently; 0 = auto */
  uint32_t collect_traversal_stats; /* 1: count BVH nodes / triangles per ray (slower); 2: and per-record visit counts of the
                                       closest-hit rays (gsp_debug_visit_histograms) */
  uint32_t collect_kernel_times;    /* 1: HIP-event time every extend/shade/connect launch (2: and print one line per iteration to stderr) */
  uint32_t disable_nee;     /* (ABI 7; ABI 5-6: `nee` with the opposite sense) RenderParams.nee (S/renderer/PathTracer.h:36-41),
                               which the shipped shader replaces by `#define NEE true` (rayhit.rchit:656).  0 (default, and what a
                               zero-initialised struct says) = the reference as shipped.  1 = the other side of its `if (NEE)`
                               branches (rayhit.rchit:733,763-768): no shadow ray, every emitter met counts with full weight,
                               directWeight stays 1; the light sample is still DRAWN (rayhit.rchit:720 is outside the branch),
                               so the random streams of the two settings coincide */
  /* (ABI 9) Adaptive sampling.  0 (default, and what a zero-initialised struct or an older host says) = off: every owned pixel
     gets spp samples per call, exactly as before.  > 0: a pixel stops being sampled once its relative standard error is at
     most this value; see "Adaptive sampling" at gsp_render. */
  float adaptive_threshold;
  uint32_t adaptive_min_spp; /* first checkpoint; 0 = 16 */
  uint32_t adaptive_step;    /* samples between checkpoints; 0 = 16 */
  /* Pixel filter (see "Pixel filter" below).  Added at the end under the struct_size rule of ABI 8, WITHOUT a new ABI version: a
     host built against the earlier ABI-9 header passes a shorter struct_size, the library takes both fields as 0, and 0 =
     GSP_FILTER_NONE = the reference as shipped. */
  uint32_t pixel_filter;     /* GSP_FILTER_* */
  float pixel_filter_param;  /* tent: radius in pixels, 0 = 1.0; Gaussian: standard deviation in pixels, 0 = 0.5; else ignored */
} gsp_render_params;

/*
 * Pixel filter: opt-in anti-aliasing by filter importance sampling.
 *
 * The reference shoots every sample of a pixel through the integer pixel coordinate; its sub-pixel jitter is the dormant line
 * raygen.rgen:38 and the <rfilter> of its scenes is ignored.  With pixel_filter != GSP_FILTER_NONE each sample's camera ray goes
 * through fragCoord = vec2(pixel) + offset, the offset drawn from the filter's own density, and the sample is accumulated into
 * its own pixel with weight 1, exactly as without a filter.  Samples are never splatted across pixels, so pixels stay
 * independent: tile shares, adaptive sampling and progressive accumulation mean what they meant.
 *
 *   u1 = randUniform(), then u2 = randUniform(), drawn from rngState directly after pcgHash(tea(W*y + x, timestamp)) (the
 *   position of raygen.rgen:38); prd.seed is the state AFTER the two draws.  Every filter other than NONE draws exactly two
 *   variates, so the random streams of all filtered modes coincide from the first bounce on.  NONE draws nothing.
 *
 *   NONE      offset = (0, 0), no draw: the reference as shipped, bit for bit.  The parameter is ignored.
 *   BOX       offset = (u1, u2): the reference's dormant line.
 *   TENT      r = param, 0 = 1.0 (Mitsuba's default).  Per axis offset = 0.5 + r * t(u),
 *             t(u) = u < 0.5 ? sqrt(2u) - 1 : 1 - sqrt(2 - 2u).
 *   GAUSSIAN  sigma = param, 0 = 0.5 (Mitsuba's default).  rho = min(sigma * sqrt(-2 log(max(1 - u1, 2^-32))), 4 sigma),
 *             offset = 0.5 + rho * (cos 2 pi u2, sin 2 pi u2).
 *
 * All arithmetic is float32 in the order written; log, sin and cos are the library's deterministic functions, sqrt is correctly
 * rounded.  fragCoord enters rayDir unchanged, so a pixel's footprint is [p, p + 1): BOX, TENT and GAUSSIAN are centred on
 * p + 0.5 while NONE samples the corner p, i.e. a filtered image is moved by half a pixel against the unfiltered one.
 *
 * A filtered call traces every camera ray (the primary-hit memo answers only the unjittered ray): gsp_stats.memoised_rays does
 * not grow.  The filter may change from call to call; it composes with adaptive sampling and with gsp_multi_render.  An unknown
 * filter id, or a negative or non-finite parameter: GSP_ERR_INVALID.  gsp_trace is not affected.
 */
#define GSP_FILTER_NONE 0u
#define GSP_FILTER_BOX 1u
#define GSP_FILTER_TENT 2u
#define GSP_FILTER_GAUSSIAN 3u

/* (ABI 9) Luminance below which the stopping rule measures the error against this floor instead of the pixel's own luminance. */
#define GSP_ADAPTIVE_LUMINANCE_FLOOR 1e-3

typedef struct gsp_stats {
  uint64_t extension_rays;
  uint64_t shadow_rays;
  uint64_t shaded_vertices;
  uint64_t samples;          /* pixels * spp completed                           */
  uint64_t nodes_visited;    /* extension rays: BVH node records read (stats mode) */
  uint64_t tris_tested;      /* extension rays: triangle packets read (stats mode) */
  uint64_t stat_rays;        /* extension rays the two counters above cover        */
  uint64_t shadow_nodes_visited; /* same three for shadow rays                     */
  uint64_t shadow_tris_tested;
  uint64_t shadow_stat_rays;
  double render_seconds;     /* host wall time inside gsp_render.. sync          */
  double extend_kernel_ms;   /* sum of HIP-event durations of the extend kernel  */
  uint64_t extend_launches;
  double shade_kernel_ms;
  double connect_kernel_ms;
  double bvh_build_ms;       /* last gsp_upload_scene / gsp_update_instances (build or refit) */
  uint64_t num_triangles;
  uint64_t num_bvh_nodes;
  uint64_t device_bytes;     /* device memory currently held by the context      */
  uint64_t algorithmic_bytes; /* SURVEY 8(d) bytes of the rays the stats mode covered: per extension ray 32 (ray)
                                 + 16 (hit) + 64 per node + 48 per triangle record read, per shadow ray 32 (+ 36 when it is
                                 occluded: the commit) + the same node / triangle terms.  What the traversal ASKS of the memory hierarchy; the
                                 bytes that reach HBM are a quarter of it (rocprofv3 FETCH_SIZE) */
  /* (ABI 4) primary-hit memo: every sample of a pixel shoots the same camera ray (raygen.rgen:31-38, no jitter), so the
     camera rays of a frame are traced once (memo_build_rays) and later samples copy the hit.  extension_rays keeps
     counting PATH SEGMENTS (what the reference traces: it equals the oracle's count); memoised_rays of them were
     answered from the memo.  Rays actually traced = extension_rays - memoised_rays + memo_build_rays + shadow_rays.
     gsp_ctx_options.primary_memo = 2 turns the memo off. */
  uint64_t memoised_rays;
  uint64_t memo_build_rays;
  uint64_t bvh_depth;        /* (ABI 4) levels of the wide BVH: a traversal stacks at most one entry per level; beyond the 20
                                levels a lane keeps in LDS the stack continues in HBM, beyond 34 the tail of a drain is left
                                to the wavefront kernels */
  uint64_t nodes_from_lds;             /* (ABI 5, stats mode) of nodes_visited / shadow_nodes_visited: node records the traversal read ... */
  uint64_t shadow_nodes_from_lds;      /* ... from its LDS copy of the top of the tree (no request on the vector-memory path)         */
  uint64_t shadow_stat_occluded;       /* (ABI 5, stats mode) shadow rays of shadow_stat_rays that were occluded ...          */
  uint64_t shadow_stat_occluded_nodes; /* ... and the node records those read (the rest of shadow_nodes_visited: unoccluded) */
  uint64_t scene_updates;    /* (ABI 5) gsp_update_camera / _instances / _tables calls that changed something since the last
                                gsp_upload_scene (a test hook: which path did the host layer take?) */
  uint64_t scene_refits;     /* (ABI 6) of those, gsp_update_instances calls that kept the tree's topology (refit) */
  uint64_t shadow_stat_no_triangle; /* (ABI 7, stats mode) shadow rays of shadow_stat_rays that ended without ONE triangle test
                                       (the ray's shear constants Sx, Sy were computed for nothing: VERDICT r04 item 7) */
  uint64_t scene_drains;     /* (ABI 7) of scene_updates: calls that first let the samples in flight finish (a test hook: an edited
                                BSDF record / light / transform does not, once the version rings exist: INTEGRATION.md) */
  uint64_t scene_splits;     /* (ABI 7) of scene_updates: gsp_update_instances calls that built the scene as TWO trees -- the instances
                                edited so far and the rest (the first edit that arrives while samples are in flight, and every later
                                one that touches an instance not edited before); edits of those instances then refit the small tree */
  uint64_t adaptive_rounds;        /* (ABI 9) rounds run by adaptive gsp_render calls (each ends at a checkpoint or at the end of a call) */
  uint64_t adaptive_active_pixels; /* (ABI 9) owned pixels the adaptive frame still samples (0 = converged: a viewer is done; 0 on a
                                      uniform frame).  `samples` keeps its meaning: samples folded, the sum over pixels of N_p */
} gsp_stats;

typedef struct gsp_context gsp_context;

/* Fill `p` with the reference's literals.  */
void gsp_default_render_params(gsp_render_params* p);

/* ABI version of the loaded library (== GSP_ABI_VERSION of this header).  gsp_stats carries no struct_size (the library FILLS it
 * at its own size): a C host MUST check gsp_abi_version() == GSP_ABI_VERSION once after loading the library;
 * gpuspectral_amd/pt.py and host/PathTracer.cpp do.  gsp_render_params and gsp_ctx_options are sized by their first field. */
int gsp_abi_version(void);

/* What the loaded library was built from: "arch=gfx950 digest=<sha256[:16] of csrc/{pt_render,pt_bvh,pt_multi}.hip + the
 * headers, in the Makefile's order> flags=<compiler flags>".  A deployment (and tests/test_abi_and_host.py) compares the
 * digest with the tree to tell a stale prebuilt .so from a fresh build.  Static storage, never NULL. */
const char* gsp_build_info(void);

/* Number of HIP devices visible (0 if none / runtime unavailable). */
int gsp_device_count(void);

/* Create a context on HIP device `device`.  Fails (GSP_ERR_DEVICE) when no
 * gfx950-capable device is present: there is no CPU fallback. */
int gsp_ctx_create(int device, gsp_context** out);
void gsp_ctx_destroy(gsp_context* ctx);

/*
 * (ABI 5) Per-context resources and scheduling choices.  None of them changes a result: images, ray counts and sample
 * order are the same for every setting (the GPU suite runs the non-default ones).  gsp_default_ctx_options fills in the
 * defaults; a field left 0 also means "default", so a zero-initialised struct with struct_size set is valid.
 * The library never reads the environment: a host application sets these per context.  (The Python test binding,
 * gpuspectral_amd/pt.py, maps the GSP_* variables the A/B scripts of earlier rounds used onto this struct.)
 */
#define GSP_GATHER_AUTO 0 /* RCCL when the shares sit on distinct devices and the communicator comes up, else copies */
#define GSP_GATHER_RCCL 1 /* ncclSend / ncclRecv group; creation fails if RCCL cannot be initialised               */
#define GSP_GATHER_COPY 2 /* hipMemcpyPeerAsync into the gathering device                                         */
typedef struct gsp_ctx_options {
  uint32_t struct_size;      /* sizeof(gsp_ctx_options) of the caller's header                                        */
  uint32_t lanes;            /* independent pipelines per context, 1 (default) or 2                                   */
  uint64_t pool_paths;       /* paths in flight the pool aims at (default 96 Mi; at most 192 per owned pixel)         */
  uint64_t ring_bytes;       /* upper bound of the sample-result ring (default 16 GiB)                                */
  double memory_share;       /* share of the device's TOTAL memory which path pool + ring may take (r05; until r04: of the
                                memory FREE when a render starts, so contexts sized themselves by creation order), never
                                more than 90 % of what is free; 0.01 .. 0.9 (default 0.4): lower it when contexts share a GPU */
  uint32_t primary_memo;     /* 0 default (on), 1 on, 2 off: trace the camera ray of a pixel once per frame           */
  uint32_t finish_paths;     /* k_finish takes over a drain below this many live paths; 0 default (262144),
                                0xffffffff = never                                                                    */
  uint32_t reinsert_rounds;  /* BVH build: parallel-reinsertion rounds + 1 (0 default = 6 rounds, 1 = none, ...)      */
  uint32_t gather_route;     /* gsp_multi_create_ex only: GSP_GATHER_*                                                */
  double refit_growth;       /* (ABI 6) gsp_update_instances keeps the tree's topology and only recomputes its boxes while
                                their summed surface area stays below this multiple of what it was after the last full
                                build; beyond it the tree is rebuilt.  0 default (1.25); <= 1 = always rebuild             */
  uint32_t geometry_versions; /* (r05) slots of the geometry ring that lets gsp_update_instances go on while samples are in
                                flight (176 B of device memory per triangle and slot): 0 default = as many as fit a quarter of
                                the free memory, at most 64; 1 = no ring: a transform edit first completes the samples queued;
                                other values are rounded down to a power of two (2 and 3: no ring)                        */
  uint32_t reserved_;
} gsp_ctx_options;
void gsp_default_ctx_options(gsp_ctx_options* o);
int gsp_ctx_create_ex(int device, const gsp_ctx_options* options, gsp_context** out);

/* Copy the scene to the device, bake world-space triangles and build the BVH
 * on the device.  The caller keeps ownership of every array in `scene`.  Limit: fewer than 2^25 (33.5 M) triangles -- the
 * traversal's packed stack entry holds node indices below 2^25 and a tree has fewer nodes than triangles -- checked here,
 * before any device work (GSP_ERR_SCENE). */
int gsp_upload_scene(gsp_context* ctx, const gsp_scene_desc* scene);

/*
 * (ABI 5) Per-frame scene edits.  The reference re-reads camera, object transforms, materials, BSDF tables and lights on
 * every createRenderPass (S/renderer/PathTracer.cpp:10-19,58-93) and only keeps the BLAS of a mesh (Renderer.cpp:122-131);
 * a host that mirrors it calls these between gsp_render calls instead of uploading the whole scene again.  The samples
 * already queued belong to the scene as it was and finish as such; accumulate buffer and timestamps are left alone -- like the
 * reference, where an edit simply shows up in the next frame's sample; call gsp_frame_begin to restart the running mean -- and
 * the primary-hit memo is invalidated.  All need a prior gsp_upload_scene.  Every call COMPARES first and returns at once,
 * before any wait, when its input equals what the device holds: a host that mirrors the reference makes all three every frame.
 *   gsp_update_camera     new camera; no geometry work and NO WAIT: paths in flight have left the camera behind (only ray
 *                         generation reads it), so a viewer that moves its camera every frame keeps the path pool full.
 *                         The two calls below do not wait either in the usual case (r05): the tables and the geometry
 *                         live in rings of versions, a sample carries the versions it was generated under and finishes on
 *                         them (gsp_stats.scene_drains counts the calls that did have to wait).
 *   gsp_update_instances  new transform / emission / bsdf / twofaced per instance.  `num_instances` and every
 *                         first_vertex / vertex_count must equal the uploaded ones (the meshes stay: they are resident on
 *                         the device); BSDF handles are checked against the resident tables.  Re-bakes the world-space
 *                         packets into their slots and REFITS the tree -- same topology, every node box and child order
 *                         recomputed bottom-up (0.35 ms for a million triangles) -- as the reference rebuilds only its
 *                         TLAS; when the boxes have grown past gsp_ctx_options.refit_growth (an object has moved far
 *                         from where the tree was built for) the BVH is rebuilt instead (16 ms).  Images do not
 *                         depend on which of the two happened: the closest-hit rule is independent of the tree.
 *                         An edit that arrives while samples are in flight (a viewer) builds the scene as TWO trees once --
 *                         the instances edited so far and the rest (gsp_stats.scene_splits; no wait the first time) -- and later
 *                         edits of those instances refit only their small tree (0.08 ms) into the next slot of a ring of
 *                         up to 64 versions while the samples in flight finish in theirs.  Scenes that do not split (more
 *                         than a quarter of the triangles edited, textures, a host that has touched new objects 16 times since the upload --
 *                         kMaxSceneSplits = 16, gpuspectral_amd/csrc/pt_versions.h) keep a ring of whole refitted
 *                         trees instead (176 B per triangle and version, at most a quarter of the free device memory).
 *                         A rebuild, a ring without a free slot or a scene above 8 M triangles first complete the samples
 *                         already queued; an edit that arrives with nothing in flight refits in place.
 *   gsp_update_tables     the eight BSDF arrays + num_bsdfs and the lights + num_lights of `scene` replace the resident
 *                         ones (all other fields of `scene` are ignored); every resident instance's handle must stay in
 *                         range.  No geometry work.  Textured scenes (dormant-feature extension): has_texture values are
 *                         checked against the resident textures.  Same record counts as the resident tables: the next slot
 *                         of a ring of versions, no wait; other counts first complete the samples already queued.  The ring
 *                         is made by the first such edit that arrives with samples in flight (gsp_upload_scene holds ONE
 *                         copy of the tables): up to 64 versions, at most a sixteenth of the free device memory and 1 GiB
 *                         (a 64-MB light table gets 16); where not even two fit, edits wait as they did before the ring.
 */
int gsp_update_camera(gsp_context* ctx, const gsp_camera* camera);
int gsp_update_instances(gsp_context* ctx, const gsp_instance* instances, uint32_t num_instances);
int gsp_update_tables(gsp_context* ctx, const gsp_scene_desc* scene);

/*
 * Allocate (and zero) the accumulate buffer for a width x height frame.
 * `pixel_ids` optionally restricts this context to `num_pixels` pixels of the
 * frame (global index = width*y + x, strictly increasing); NULL = the whole
 * frame.  Seeds depend only on the global pixel index (raygen.rgen:37), so any
 * partition of the frame over contexts/GPUs reproduces the same image.
 */
int gsp_frame_begin(gsp_context* ctx, uint32_t width, uint32_t height,
                    const uint32_t* pixel_ids, uint64_t num_pixels);

/* Trace params->spp more samples for every owned pixel and fold them into the
 * accumulate buffer with the reference's running mean (raygen.rgen:84-108).
 * Returns once every sample has been injected into the path pool; the last
 * paths may still be in flight (they share launches with the next call's
 * samples) and samples are always folded in call / timestamp order.  gsp_sync,
 * the download / copy / upload_accum calls, gsp_get_stats, gsp_reset_stats,
 * gsp_frame_begin, gsp_upload_scene and gsp_ctx_destroy complete them first. */
int gsp_render(gsp_context* ctx, const gsp_render_params* params);
/*
 * (ABI 9) Adaptive sampling: params->adaptive_threshold > 0.
 *   Checkpoints are at n = min_spp + j * step samples (j >= 0).  At a checkpoint every pixel still sampled is tested and stops
 *   when err <= threshold * max(Ybar, GSP_ADAPTIVE_LUMINANCE_FLOOR).  The rule is evaluated in double from the float32 buffers:
 *     Y    = 0.2126 r + 0.7152 g + 0.0722 b
 *     Ybar = Y of the pixel's accumulate-buffer mean
 *     m2   = running mean of Y^2 over the pixel's folded samples, with the colour's recurrence: sample t enters with weight
 *            1 / (t + 1) (Y and Y^2 of a sample formed in float32); a sample whose colour mix is NaN leaves m2 alone, as it
 *            leaves the colour
 *     var  = max(m2 - Ybar^2, 0) * n / (n - 1),   err = sqrt(var / n)      (n = 1: the pixel does not stop)
 *   It is an estimator: whether a pixel stops depends on the noise it measures, so the adaptive image carries a small stopping
 *   bias that the uniform renderer does not have.  A pixel that stops after N_p samples holds exactly the uniform image of that
 *   pixel at N_p samples, bit for bit.
 * Frame rules.  The first gsp_render after gsp_frame_begin decides whether the frame is adaptive; later calls of the frame must
 *   agree (threshold > 0 or not), else GSP_ERR_INVALID.  first_timestamp must equal the samples the still-sampled pixels hold
 *   (0 for the first call; not checked once no pixel is left).  A call adds up to spp samples to every pixel still sampled, in
 *   ROUNDS that end at the checkpoints and at the end of the call.  A stop is decided only at a checkpoint, so the result does
 *   not depend on how the samples are split over calls, on timestamps_in_flight or on gsp_ctx_options.lanes.  Stopped pixels
 *   stay stopped until the next gsp_frame_begin; scene edits leave them (and the accumulate buffer) alone.  An adaptive
 *   gsp_render returns DRAINED: every sample it added has been folded.  gsp_peek's samples_folded is the count of the pixels
 *   still sampled (the largest per-pixel count).  gsp_multi_render and gsp_upload_accum refuse adaptive frames
 *   (GSP_ERR_INVALID).  The per-pixel state: gsp_download_pixel_stats.
 */

/* (ABI 9) The owned pixels' m2 (see above) and folded sample counts after adaptive gsp_render calls, compact (pixel_ids
 * order), num_pixels entries each; either pointer may be NULL.  GSP_ERR_INVALID on a frame that is not adaptive. */
int gsp_download_pixel_stats(gsp_context* ctx, float* second_moment, uint32_t* spp);

/*
 * Thin lens: opt-in depth of field.
 *
 * The reference's camera is a pinhole (raygen.rgen has no lens code) and its loader ignores a `thinlens` sensor's parameters.
 * The lens is CONTEXT STATE, like the camera: it holds until changed, survives gsp_update_camera, gsp_frame_begin and
 * gsp_upload_scene, needs no drain (paths in flight have left the camera behind) and may change between the gsp_render calls of
 * one frame; a change takes effect with the next gsp_render.  gsp_set_lens(ctx, NULL) and radius == 0 are the pinhole: the
 * reference, bit for bit, whatever the other fields hold.  struct_size follows the rule of gsp_render_params: fields beyond it are
 * taken as 0.  GSP_ERR_INVALID (text at gsp_last_error) for: a non-finite or negative radius; radius > 0 with a focus distance
 * that is not finite and positive; blades outside {0, 3..16}; a non-finite rotation.
 *
 * Camera ray.  The pinhole ray of fragCoord (fx, fy) is v = (-(fx - W/2), fy - H/2, zplane), dir = flipY(M * normalize(v)),
 * origin = eye (M = the upper 3x3 of to_world, flipY negates y).  With a lens point l = (lx, ly, 0) in camera space and
 * s = focus_distance / zplane (formed once on the host, like zplane):
 *     pf     = (v.x * s, v.y * s, focus_distance)       the pinhole ray's point on the plane of focus
 *     dir    = flipY(M * normalize(pf - l))
 *     origin = eye + flipY(M * l)
 * Offset and direction go through the same linear map, so all lens rays of one fragCoord meet on the plane of focus where the
 * pinhole ray crosses it.  All arithmetic is float32 in the order written.
 *
 * Draws.  u3 = randUniform(), then u4 = randUniform(), from rngState directly after the pixel filter's two draws (directly after
 * pcgHash(tea(..)) when the filter is NONE); prd.seed is the state AFTER them.  Radius 0 draws nothing.
 *   blades == 0  circle: Shirley's concentric map of (u3, u4) (the one of rayhit.rchit:89-111), times radius.
 *   blades == n  regular polygon inscribed in the circle, vertices v_j = radius * (cos, sin)(rotation + (2 pi j) / n), j = 0..n-1,
 *                v_n = v_0:  t = u3 * n, k = min((uint)t, n - 1), a = sqrt(t - k), b = u4,
 *                l = a * ((1 - b) * v_k + b * v_{k+1}).
 * Both are uniform over the aperture.  sin and cos are the library's deterministic functions, sqrt is correctly rounded.
 *
 * A call with radius > 0 traces every camera ray, exactly as a filtered call does: the primary-hit memo is neither read nor
 * touched, gsp_stats.memoised_rays does not grow, and a later pinhole call of the same frame reuses the memo.  The lens composes
 * with pixel filters, adaptive sampling, pixel_ids shares and gsp_multi_render (gsp_multi_set_lens sets it on every share).
 */
typedef struct gsp_lens {
  uint32_t struct_size;   /* sizeof(gsp_lens) of the host's header; same rule as gsp_render_params */
  float radius;           /* aperture radius in camera-space units; 0 = pinhole = the reference, bit for bit */
  float focus_distance;   /* distance of the plane of focus along the camera's local z; > 0 when radius > 0 */
  uint32_t blades;        /* 0 = circular aperture; 3..16 = regular polygon inscribed in the circle */
  float rotation;         /* radians, angle of polygon vertex 0 */
} gsp_lens;
int gsp_set_lens(gsp_context* ctx, const gsp_lens* lens); /* NULL = pinhole */
/* Autofocus: traces the pinhole ray through fragCoord (fx, fy) of a width x height frame against the uploaded scene (the
 * closest-hit path of gsp_trace) and writes the hit's camera-space depth t * normalize(v).z -- the value to put into
 * gsp_lens.focus_distance -- or 0 on a miss.  Not affected by the current lens or pixel filter; needs no gsp_frame_begin.
 * Completes the samples already queued first, like gsp_sync. */
int gsp_focus_distance(gsp_context* ctx, uint32_t width, uint32_t height, float fx, float fy, float* out);

/*
 * Interior media: opt-in Beer-Lambert absorption inside closed shapes (coloured glass).
 *
 * The reference's scenes declare <medium type="homogeneous" name="interior"> children on glass shapes and its loader never
 * looks at them; every one has sigmaS = 0.  A medium here is a pure absorber: it draws no random number and bends no ray, it
 * scales the path weight over the segment that ran inside the object.  sigma_a is in units of 1 / world-space length, finite
 * and >= 0.
 *
 * The media are CONTEXT STATE: gsp_set_media(ctx, media, n) replaces the table (NULL or n == 0 = none; at most GSP_MAX_MEDIA
 * entries), holds until changed and survives gsp_upload_scene.  The samples in flight finish first (the wait of every scene
 * edit), so it may be called between the gsp_render calls of one frame.  GSP_ERR_INVALID for a non-finite or negative
 * coefficient, a count above GSP_MAX_MEDIA, and when the resident scene names a medium number above the new count (the
 * table is then unchanged and the scene still renders).
 *
 * Assignment: bits 19..30 of gsp_instance.bsdf (GSP_BSDF_HANDLE_MEDIUM) hold the medium number k, 0 = none, k = media[k - 1].
 * A number above the context's count -- any nonzero number while no media are set -- is GSP_ERR_SCENE, "BSDF handle out of
 * range", at gsp_upload_scene and gsp_update_instances.
 *
 * The attenuation, in the shading vertex straight after the material word and the geometric normal N are read (the test of
 * rayhit.rchit:698 on N, BEFORE the two-sided flip), float32 in this order:
 *     k = (material >> 19) & 0xfff;  bsdf = material & 0x0007ffff
 *     if (k != 0 && dot(N, -rayDir) < 0)   a_c = exp(-(sigma_a[k-1].c * t)), c = r, g, b;   w = weight * a   (component-wise)
 *     else                                 w = weight
 * and every later use of the path weight in that vertex reads w: the NEE term, both emission terms, the next vertex's weight
 * and through it Russian roulette.  t is the hit's parametric distance along the unit direction as traced; exp is the library's
 * deterministic one, exp(-0) = 1 exactly, so sigma_a = 0 leaves every bit of the frame in place.
 *
 * The entry piece.  A segment that runs inside an object starts 1e-4 below its surface along the normal (rayhit.rchit:793), so
 * the traced ray meets the surface's plane 1e-4 / |dot(N, wi)| behind its origin and the next vertex's t is short by that much
 * (sigma_a = 1000 would turn it into 10 % of the weight).  The vertex that sends the path inside absorbs it: when the path
 * continues, k != 0 and wi points against the geometric normal (c = dot(wi, N) < 0; > 0 where N is the two-sided flip of it),
 *     s = min(1e-4 / |c|, 1e30);   weight' = weight' * exp(-(sigma_a[k-1].c * s))     behind weight' = w * f * NoW / pdf (:795)
 * float32 in this order.  A slab of thickness d crossed at angle theta then absorbs over d / cos(theta) to float32 rounding.
 *
 * The rule is stateless: the object whose back face is hit is the one the segment ran inside.  That is exact for closed shapes
 * that do not overlap.  Overlapping or open shapes, and a camera inside a shape, get exactly this rule and nothing cleverer.
 * Shadow rays are untouched: a shadow ray through a glass object is occluded by its surface as before.  The feature buffers
 * report the handle without the medium bits.  A context without media runs the kernels it ran before media existed.
 */
typedef struct gsp_medium {
  float sigma_a[3]; /* absorption coefficient per channel, 1 / length; finite, >= 0 */
  float reserved;   /* 0 */
} gsp_medium;
int gsp_set_media(gsp_context* ctx, const gsp_medium* media, uint32_t num_media); /* NULL or 0 = none */

/*
 * Scattering media: opt-in volumetric scattering inside the closed shapes that carry an interior medium (milk, wax, jade, smoke
 * in a glass box).  Free-path sampling and a Henyey-Greenstein phase function, in the shading vertex.
 *
 * gsp_set_media_scattering(ctx, scatter, n) gives the context a table PARALLEL to the one of gsp_set_media: entry k - 1 belongs
 * to medium k.  n is 0 (or scatter NULL: no scattering) or equal to the context's media count.  sigma_s is in units of 1 /
 * world-space length, finite and >= 0; g is the Henyey-Greenstein asymmetry, finite, |g| < 1 (> 0 scatters forward).
 * GSP_ERR_INVALID for a coefficient or g outside that and for a count that is neither 0 nor the media count; the table is then
 * unchanged.  Context state like the media: the samples in flight finish first, it holds until changed and survives
 * gsp_upload_scene.  gsp_set_media with a DIFFERENT count drops the scattering table (the same count keeps it).  A context
 * whose table is absent or all sigma_s == 0 runs the kernels and computes the bits it did before this call existed.
 *
 * Where: a vertex whose medium k != 0, on a back face (dot(N, -rayDir) < 0 on the geometric normal, before the two-sided flip),
 * and sigma_s[k-1] has a nonzero channel.  The line w = weight * exp(-(sigma_a * t)) of "Interior media" is replaced by the
 * following, float32 in this order, sigma_t = sigma_a + sigma_s per channel, log / exp / sin / cos the library's deterministic ones:
 *   1. two draws from the path's stream, BEFORE any other draw of the vertex: u_c, then u_d.
 *        c* = min((uint)(u_c * 3), 2);   s = -log(1 - u_d) / sigma_t[c*]     (sigma_t[c*] == 0: s = +inf, the surface)
 *   2. surface event, !(s < t):   Tr_c = exp(-(sigma_t_c * t));   p = ((Tr_r + Tr_g) + Tr_b) / 3;   w = (weight * Tr) / p
 *      and the ordinary vertex goes on with w and the stream as it stands.
 *   3. medium event, s < t:   Tr_c = exp(-(sigma_t_c * s));   p = ((sigma_t_r * Tr_r + sigma_t_g * Tr_g) + sigma_t_b * Tr_b) / 3;
 *        w = ((weight * sigma_s) * Tr) / p
 *      two more draws u1, u2 sample Henyey-Greenstein about rayDir:
 *        |g| < 1e-3:  cos = 1 - 2 * u1;   pdf_hg = 1 / (4 * pi)
 *        else:        sq = (1 - g * g) / ((1 - g) + (2 * g) * u1);   cos = clamp(((1 + g * g) - sq * sq) / (2 * g), -1, 1)
 *                     d = (1 + g * g) - (2 * g) * cos;   pdf_hg = (1 - g * g) / ((4 * pi) * (d * sqrt(d)))
 *        sin = sqrt(max(0, 1 - cos * cos));   phi = (2 * pi) * u2;   dir = frame(rayDir) * (sin * cos(phi), sin * sin(phi), cos)
 *      with the frame of the shading vertex's make_frame.  The phase value equals its pdf and cancels.  The vertex emits nothing
 *      and traces NO shadow ray.  Its next state: o = in.o + rayDir * s (no offset), d = dir, weight = w, depth + 1, wasDelta = 0,
 *      countEmitted = 0, the version stamps as a surface vertex carries them, directWeight = pdf_hg under GSP_ESTIMATOR_TEXTBOOK
 *      and 1 otherwise.  Russian roulette (on w, peeking the next draw) and the max_depth test run as for a surface vertex.
 *   4. p == 0 or not finite (every channel's transmittance underflowed): the path ends and adds nothing.
 *   5. The entry piece of "Interior media" keeps its line, with sigma_a: absorption over the 1e-4 offset is kept, scattering
 *      inside it is neglected -- the path is merely not scattered over 1e-4 / |c|, which loses no energy.
 *   6. A medium whose sigma_s is all 0 takes the deterministic line of "Interior media" and draws nothing, also in a context
 *      where other media scatter.
 *
 * Limits.  No next-event estimation from inside a medium: a shadow ray would be stopped by the object's own surface, so nothing
 * is lost for closed shapes; an index-matched boundary stays opaque to shadow rays as it is without scattering.  No emitters
 * inside a medium.  A scatter event counts as a bounce and max_depth is at most 250: dense, high-albedo media are truncated
 * (the mean number of events grows like the square of the optical thickness).  The stateless rule of "Interior media" carries
 * over: a path that scatters inside a closed shape meets a back face of the same shape next.
 */
typedef struct gsp_medium_scatter {
  float sigma_s[3]; /* scattering coefficient per channel, 1 / length; finite, >= 0 */
  float g;          /* Henyey-Greenstein asymmetry, |g| < 1; 0 = isotropic */
} gsp_medium_scatter;
int gsp_set_media_scattering(gsp_context* ctx, const gsp_medium_scatter* scatter, uint32_t num_media); /* NULL or 0 = none */

/*
 * Light selection: opt-in choice of the light for next-event estimation in proportion to its emitted power.
 *
 * The reference picks the light triangle as r % num_lights (rayhit.rchit:148): every triangle is equally likely whatever it
 * emits.  GSP_LIGHTS_UNIFORM is that pick, bit for bit, with the kernels a context ran before this section existed.
 * GSP_LIGHTS_POWER picks light i with a probability proportional to w_i = Y(radiance_i) * area_i through an alias table.  The
 * rest of the vertex is the reference's: the point on the light, the solid-angle pdf, the power heuristic, the emitter-hit weight
 * formed from the NEE sample's pdf (directWeight, rchit:786).
 *
 * The mode is CONTEXT STATE, like the lens and the media: gsp_set_light_sampling(ctx, mode) holds until changed and survives
 * gsp_upload_scene.  It may be called with a scene resident: the samples in flight finish first (the wait of every scene edit),
 * then the tables are packed again from the context's host copy and uploaded, with or without the pick table.  An unknown mode
 * is GSP_ERR_INVALID and leaves the state unchanged.
 *
 * The table.  One gsp_light_pick per light triangle, straight behind the light records of the resident table image (so it is
 * staged into LDS with them when the image is at most 8192 bytes, and every table version of gsp_update_tables has its own).
 * Built on the host, in double, from the caller's records as they came:
 *     w_i = max(0.2126 R + 0.7152 G + 0.0722 B, 0) * 0.5 |cross(v2 - v0, v1 - v0)|;  a non-finite or negative w_i counts as 0;
 *     if every w_i is 0, every w_i becomes 1
 *     s_i = w_i * n / sum(w)
 * Vose's alias construction on s, in a fixed order: the lists "small" (s_i < 1) and "large" (s_i >= 1) are filled in ascending
 * index; while both hold an entry, the FRONT small entry a is finished against the FRONT large entry g: s'_a = s_a, alias_a = g,
 * s_g = (s_g + s_a) - 1; if s_g < 1 now, g leaves the front of "large" and is appended at the BACK of "small".  What is left
 * on either list has s' = 1.  The same records therefore always give the same table bytes.  Entry j:
 *     threshold = round(s'_j * 2^32) as an integer, saturated to 0xffffffff; 0xffffffff means "always self" (2^32)
 *     alias     = the donor g; j itself where the threshold is saturated
 *     pmf_self  = float32(p_j),  pmf_alias = float32(p_alias),  with the probability the INTEGER table implies, in double:
 *     p_i = (T_i + sum over j != i with alias_j = i of (2^32 - T_j)) / (n * 2^32),   T = 2^32 for a saturated entry
 * so the pdf the estimator divides by is the pdf it samples with, to float32 rounding; |p_i - w_i / sum(w)| is at most
 * (1 + d_i) / (n * 2^32), d_i = the entries aliased to i.  A light of weight 0 has threshold 0 and is nobody's alias: p = 0,
 * never picked.  So is a VERY WEAK light: one whose share of sum(w) is below about 2^-33 / n rounds to threshold 0 and is
 * dropped.
 *
 * The pick, in the shading vertex where the reference draws its light (the same three draws, so the random streams of the two
 * modes coincide from the light sample on); uint32 / uint64 integer operations and float32 in this order:
 *     r = pcg_next(rng);  e1 = rand_uniform(rng);  e2 = rand_uniform(rng)
 *     m = (uint64)r * num_lights;   j = (uint32)(m >> 32);   lo = (uint32)m
 *     E = pick[j];   self = lo < E.threshold || E.threshold == 0xffffffff
 *     k = self ? j : E.alias;        pmf = self ? E.pmf_self : E.pmf_alias
 *     the point on light k, c and A exactly as the uniform pick forms them;   pdf = ((ldist * ldist) / (|c| * A)) * pmf
 * The high word of the product is the slot, the low word an independent 32-bit coin.  num_lights == 0: no light, pdf 0, as before.
 *
 * What changes and what does not.  The path's continuation (BSDF sample, weight, Russian roulette) does not read the light
 * sample: extension rays and shaded vertices are those of the uniform mode, only the shadow rays differ; with disable_nee the
 * two modes give the same frame, and so they do with one light triangle (pmf = 1.0f = 1 / num_lights, j = 0).  THE EXPECTED
 * IMAGE SHIFTS SLIGHTLY between the modes: the reference's emitter-hit weight is formed from the pdf of the vertex's own NEE
 * sample, not from the pdf of the light that was hit (its documented departure from textbook multiple importance sampling,
 * rchit:763-790), and that pdf depends on the selection density.  Where BSDF-sampled emitter hits matter, the two modes
 * therefore converge to slightly different images.  Both are the reference's estimator with a selection density; neither is
 * the textbook estimator.
 *
 * gsp_download_light_pick reads the resident table of the current table version: count receives the number of light
 * triangles; GSP_ERR_INVALID in uniform mode, without a scene, or when capacity < that number.
 */
#define GSP_LIGHTS_UNIFORM 0u /* r % num_lights, rayhit.rchit:148: the reference */
#define GSP_LIGHTS_POWER 1u   /* proportional to Y(radiance) * area, through an alias table */
typedef struct gsp_light_pick {
  uint32_t threshold, alias;
  float pmf_self, pmf_alias;
} gsp_light_pick; /* 16 B */
int gsp_set_light_sampling(gsp_context* ctx, uint32_t mode);
int gsp_download_light_pick(gsp_context* ctx, gsp_light_pick* out, uint32_t capacity, uint32_t* count);

/*
 * Estimator: opt-in textbook multiple importance sampling in place of the reference's weights.
 *
 * The reference's estimator departs from an unbiased path tracer with next-event estimation (NEE) in three places of the shading
 * vertex: the NEE weight takes the BSDF's pdf of the SAMPLED direction, not of the direction L to the light (rayhit.rchit:751);
 * an emitter that a BSDF-sampled ray hits is weighted with the pdf of the light the previous vertex sampled, or 1 when that
 * shadow ray was occluded, not with the pdf of reaching the emitter that is hit (:763-765, :785-790); and rough plastic's eval
 * pdf carries a one-sided floor max(D cos, 0.01) that its sample pdf does not (:577 against :541).  GSP_ESTIMATOR_REFERENCE (the
 * default) is the reference, bit for bit, with the kernels a context ran before this section existed.  GSP_ESTIMATOR_TEXTBOOK
 * replaces the three by the textbook forms below; its frames converge to what plain path tracing (disable_nee) converges to,
 * under either light selection mode.  The firefly cut-off stays gsp_render_params.clamp in both modes.
 *
 * The mode is CONTEXT STATE, like the lens, the media and the light selection: gsp_set_estimator(ctx, mode) holds until changed
 * and survives gsp_upload_scene.  It may be called with a scene resident: the samples in flight finish first (the wait of every
 * scene edit); under GSP_LIGHTS_POWER the tables are then packed again and uploaded, as gsp_set_light_sampling does.  An unknown
 * mode is GSP_ERR_INVALID and leaves the state unchanged.
 *
 * The rule, float32 in this order, with the vertex's quantities as rayhit.rchit names them (bs = the BSDF's sample, lb = the
 * BSDF's value and pdf for L, power_heuristic(f, g) = (f * f) / (f * f + g * g)):
 *   1. NEE weight:      w = power_heuristic(lightPdf, lb.pdf)                       (the reference: bs.pdf)
 *   2. rough plastic:   the eval pdf is ((0.5 * D(wh)) * |wh.z|) / (4 * |dot(wo, wh)|) + 0.5 * cosine_pdf(wi), the form its
 *                       sample reports, without the max(.., 0.01)
 *   3. emitter hit, with NEE on, countEmitted == 0 and wasDelta == 0:
 *          isLight = emission.r != 0 || emission.g != 0 || emission.b != 0
 *          A       = 0.5 * |length(cross(v2 - v0, v1 - v0))|        v0, v1, v2: the hit triangle's world-space vertices
 *          hitPdf  = ((t * t) / (|dot(-rayDir, N)| * A)) * p_sel    t: the hit distance, N: the geometric normal
 *          weight  = isLight ? power_heuristic(lastPdf, hitPdf) : 1
 *      lastPdf = bs.pdf of the vertex that sent the ray.  The triangle's vertices are read only when isLight.
 *   4. p_sel, the probability with which light selection picks the triangle that was hit:
 *          GSP_LIGHTS_UNIFORM:   p_sel = 1.0f / (float)num_lights
 *          GSP_LIGHTS_POWER:     w_hit = max((0.2126f * r + 0.7152f * g) + 0.0722f * b, 0) * A   of the hit's emission and A above;
 *                                a non-finite or negative w_hit counts as 0
 *                                p_sel = w_hit * inv_sum_w
 *      inv_sum_w = the float32 rounding of 1 / sum(w), the sum of "Light selection" (in double, ascending index, from the caller's
 *      light records).  When every w was 0 the table fell back to uniform: inv_sum_w is then stored as 0 (as it is when the sum
 *      or its reciprocal leaves the format) and p_sel = 1.0f / (float)num_lights.  inv_sum_w travels in ONE trailing 16-byte
 *      record {inv_sum_w, 0, 0, 0} behind the alias table, present only when BOTH GSP_LIGHTS_POWER and GSP_ESTIMATOR_TEXTBOOK are
 *      on: every other context keeps the table image it had, and gsp_download_light_pick its count.
 *      p_sel is the pmf of the weights, not of the integer table: it equals the probability the table samples with only to
 *      within (1 + d_i) / (n * 2^32) ("Light selection"), far below float32 rounding of the weights for any table that fits memory.
 *      Like the reference's 1 / num_lights, it assumes that EVERY EMISSIVE TRIANGLE IS ONE LIGHT RECORD of the same radiance and
 *      vertices: an emissive triangle without a record is weighted as if NEE could reach it.
 *
 * Path state does not grow: the path's directWeight field is dead in this mode and carries lastPdf; a shadow ray carries the same
 * value for both of its verdicts, and the occluded commit leaves the field alone.
 *
 * What changes and what does not.  Extension rays, shaded vertices and shadow rays are those of the reference mode under the
 * same light selection (the weights do not steer the path), and with disable_nee the two modes give the same frame bit for bit.
 */
#define GSP_ESTIMATOR_REFERENCE 0u /* the reference's weights, rayhit.rchit:751,763-765,785-790,577 */
#define GSP_ESTIMATOR_TEXTBOOK 1u  /* power heuristic over the pdfs of the direction taken; unbiased */
int gsp_set_estimator(gsp_context* ctx, uint32_t mode);

/*
 * Delta lights: opt-in point, spot and directional emitters beside the emissive triangles.
 *
 * Every light of the reference is an emissive triangle.  gsp_set_delta_lights(ctx, lights, count) gives the context a table of
 * emitters WITHOUT AREA: a point light (a bulb), a spot light (a bulb behind a smooth-edged cone) and a directional light (the
 * sun).  Only next-event estimation reaches them: no ray ever hits one, and a BSDF sample never finds one.
 *
 * The table is CONTEXT STATE like the media table: it holds until changed and survives gsp_upload_scene and gsp_update_tables.
 * It may be set with a scene resident: the samples in flight finish first (the wait of every scene edit), then the tables are
 * packed again from the context's host copy and uploaded, as gsp_set_light_sampling does.  count == 0 (or lights NULL) drops the
 * table.  A context without delta lights runs the kernels, holds the table bytes and returns the frame it did before this section
 * existed, bit for bit.
 *
 * Validation.  GSP_ERR_INVALID, and the state unchanged, when: kind is not one of the three; any field is not finite; a channel
 * of intensity is negative; the direction of a spot or directional light is not unit within 1e-3 (|length - 1| <= 1e-3 in double;
 * an accepted direction is renormalised in double and rounded to float32, and that is what the device reads); a spot has
 * cos_beam <= cos_cutoff; a directional light has extent <= 0; a word of reserved is not 0.  The direction of a point light and
 * the position of a directional light are finite and otherwise ignored.
 *
 * Where the records live.  The delta records (64 bytes, the size of gsp_triangle_light) sit in the light table straight behind
 * the triangle lights, in every table version.  num_lights and 1.0f / (float)num_lights of the shading vertex count BOTH kinds,
 * so under GSP_LIGHTS_POWER the alias table still starts at (lights + num_lights), and the records ride into LDS with the lights
 * when the image is at most 8192 bytes.  gsp_download_light_pick reports triangles + delta records, in that order.
 *
 * The pick.  The shading vertex makes the three draws of the reference (r, e1, e2) and the same pick: r % num_lights, or the
 * alias table.  An index >= the number of TRIANGLE lights names delta record (index - triangles).  e1 and e2 are then drawn and
 * unused: the random stream of a path does not depend on the kind of light it picked.  pmf = 1.0f / (float)num_lights, or the
 * stored pmf of the alias table.
 *
 * The sample, float32 in this order (p = the shading point, dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z, sqrt and the
 * divisions IEEE):
 *   point:        toL = position - p;   d2 = dot(toL, toL);   Ldist = sqrt(d2);   L = toL / Ldist  (per component)
 *                 emission = intensity;   lightPdf = d2 * pmf
 *                 d2 == 0: lightPdf = 0 (no shadow ray), L = (0, 0, 1), Ldist = 0
 *   spot:         as point, then   c = dot(direction, -L);   t = clamp((c - cos_cutoff) / (cos_beam - cos_cutoff), 0, 1)
 *                 s = (t * t) * (3 - 2 * t);   emission = intensity * s
 *                 The smoothstep of the COSINE between the cutoff and the beam: no inverse trigonometric function runs on the
 *                 device.  This is NOT Mitsuba's ramp, which is linear in the angle; inside the beam and outside the cutoff the two agree.
 *   directional:  L = -direction;   Ldist = 1e30f;   emission = intensity (the irradiance on a plane facing the light);   lightPdf = pmf
 * (toL points from the shading point to the light; with it the NEE term below is intensity * cos / d2.)
 *
 * NEE for a delta sample.  The gate is the reference's: NEE on, the BSDF sample not delta, the side tests on the geometric
 * normal (or a transmitting BSDF), lightPdf != 0.  NoL = |dot(SN, L)|, lb = the BSDF's value for L.  The weight is 1 -- no BSDF
 * sample can reach a delta light, so there is no second strategy to weigh against:
 *     nee = (((NoL * lb.f) * weight) * emission) / lightPdf            (weight = the path weight of the vertex)
 * The shadow ray runs from p along L with tmin 0.01 and tmax = Ldist - 0.01f (1e30f for a directional light: float32 absorbs the
 * 0.01).  The directWeight that the continuing path carries to its next emitter hit when the shadow ray is unoccluded is
 * 1.0f (GSP_ESTIMATOR_TEXTBOOK: bs.pdf, as always): what a vertex without a shadow ray hands on.  A pick that lands on a
 * TRIANGLE light in a context with delta lights computes, operation for operation, what the vertex computed before.
 *
 * Emitter hits.  Delta lights are never hit.  Under GSP_ESTIMATOR_TEXTBOOK the weight of a TRIANGLE emitter that is hit uses the
 * p_sel of the table that includes the delta records: 1.0f / (float)num_lights over both kinds, or w_hit * inv_sum_w with the sum
 * over both kinds.
 *
 * Power pick weights ("Light selection"), in double, from the accepted records, BEHIND the triangle weights in the same
 * ascending sum; Y(c) = max(0.2126 R + 0.7152 G + 0.0722 B, 0):
 *     point:        4 pi Y(intensity)
 *     spot:         2 pi (1 - (cos_beam + cos_cutoff) / 2) Y(intensity)
 *     directional:  pi extent^2 Y(intensity)          extent = the radius of the scene as the power pick is to see it
 *
 * Media.  A medium event of "Scattering media" still takes no light sample.  A context that holds delta lights and media runs
 * the kernels of scattering media whatever its sigma_s: a medium whose sigma_s is 0 takes the deterministic line there and draws
 * nothing, so the frame is that of the absorbing kernels.
 *
 * disable_nee.  Delta lights are DARK under it: nothing but next-event estimation reaches them.  The sentence of "Estimator"
 * that textbook frames converge to what plain path tracing converges to therefore holds for the triangle lights only.
 *
 * Limits.  A delta light behind a refracting or index-matched boundary stays hidden (shadow rays stop at every surface); no
 * light sample from a medium event; no textured or goniometric emitters.
 */
#define GSP_LIGHT_POINT 1u
#define GSP_LIGHT_SPOT 2u
#define GSP_LIGHT_DIRECTIONAL 3u
typedef struct gsp_delta_light { /* 64 B, the size of gsp_triangle_light */
  float position[3];  /* point, spot: world position */
  uint32_t kind;      /* GSP_LIGHT_* */
  float direction[3]; /* spot, directional: unit, the way the light TRAVELS (the spot's axis) */
  float cos_cutoff;   /* spot: cosine of the cutoff angle (no light outside it) */
  float intensity[3]; /* point, spot: radiant intensity per channel; directional: irradiance on a plane facing the light */
  float cos_beam;     /* spot: cosine of the beam width (full intensity inside it); > cos_cutoff */
  float extent;       /* directional: radius R of the scene as the power pick sees it; > 0 */
  float reserved[3];  /* 0 */
} gsp_delta_light;
int gsp_set_delta_lights(gsp_context* ctx, const gsp_delta_light* lights, uint32_t count); /* NULL or 0 = none */

/*
 * Environment light: opt-in next-event estimation towards the environment map, with MIS.
 *
 * gsp_scene_desc.envmap lights only the paths that leave the scene by chance ("light sampling does not see it", above).
 * gsp_set_envmap_sampling(ctx, &{enabled = 1, extent}) makes the map ONE MORE RECORD of the light table: the light pick may land on
 * it, the vertex then samples a direction from a piecewise-constant density over the map and traces a shadow ray of length 1e30f,
 * and a path that escapes along a BSDF sample weighs the map's radiance against that density.  Path state, queues and the traversal
 * kernel are what they were.
 *
 * The switch is CONTEXT STATE like the delta-light table: it survives gsp_upload_scene and gsp_update_tables and may be set with a
 * scene resident (the samples in flight finish first, then the tables are packed again and uploaded, as gsp_set_delta_lights
 * does).  NULL or enabled == 0 drops the sampling.  It takes effect only while the resident scene has an envmap; without one it is
 * inert.  A context that never enables it, or has disabled it again, runs the kernels, holds the table bytes and returns the frame
 * of before, bit for bit.
 *
 * Validation (the state stays unchanged on every failure).  GSP_ERR_INVALID when enabled != 0 and: extent is not finite or not > 0;
 * a word of reserved is not 0; the context runs GSP_ESTIMATOR_REFERENCE -- the environment light exists under
 * GSP_ESTIMATOR_TEXTBOOK only (the reference has no environment sampling to restate), so gsp_set_estimator(.., TEXTBOOK) comes
 * first, and gsp_set_estimator(.., REFERENCE) with the switch on is GSP_ERR_INVALID as well.  ROTATION: sampling needs the inverse
 * of envmap.to_local, and the density below has no Jacobian term, so the upper 3x3 A of to_local must be orthonormal: every entry
 * of A^T A - I at most 1e-4 in magnitude, in double.  gsp_set_envmap_sampling on a resident scene that fails this is
 * GSP_ERR_INVALID; gsp_upload_scene of such a scene with the switch on is GSP_ERR_SCENE.  The library forms local -> world = A^-1
 * (cofactors over the determinant, in double, rounded to float32 once) when it packs the record.
 *
 * The sampling distribution: piecewise constant over a grid of Cw x Ch cells in the map's own (u, v), Cw = min(width, 512),
 * Ch = min(height, 256) (at most 131 072 entries of 16 B = 2 MiB: resident in one L2, where a table per texel of a 2k x 1k map
 * would be 32 MiB of random access).  Cell (i, j), i < Cw, j < Ch, has number j * Cw + i and covers u in [i / Cw, (i + 1) / Cw),
 * v in [j / Ch, (j + 1) / Ch).  Its weight, in double on the host at upload:
 *     w = sin(pi * (j + 0.5) / Ch) * max Y(texel)            Y(c) = max(0.2126 R + 0.7152 G + 0.0722 B, 0), not finite: 0
 * the maximum over EVERY texel the bilinear lookup above can read for a (u, v) inside the cell: columns floor(i * width / Cw - 0.5
 * - eps) .. floor((i + 1) * width / Cw - 0.5 + eps) + 1, wrapped; rows likewise with height and Ch, clamped; eps = width (height)
 * * 2^-21 covers the float32 rounding of the lookup's coordinate.  Taking the maximum over the filter's footprint makes the density
 * positive wherever the looked-up radiance is not 0: the condition for an unbiased estimator.  The weights go through the alias
 * construction of "Light selection" as they stand; pmf(cell) is the mass the integer table implies (pmf_self of the cell's entry).
 * The table is scene state, made by gsp_upload_scene (or, when the switch is first set under a resident scene, from the resident
 * texels), one copy beside the table versions: gsp_update_tables does not touch it.
 *
 * The light record: ONE 64-byte record behind the delta records in every table version, counted by num_lights and
 * 1.0f / (float)num_lights and reported LAST by gsp_download_light_pick.  Its kind is GSP_LIGHT_ENVIRONMENT, for internal use:
 * gsp_set_delta_lights keeps rejecting it.  Under GSP_LIGHTS_POWER its weight is, in double, behind the delta weights in the same
 * ascending sum,
 *     pi * extent^2 * sum over texels of Y(texel) * (2 pi / width) * (pi / height) * sin(pi * (row + 0.5) / height)
 * (rows in ascending order, columns ascending inside a row) -- extent = the radius of the scene as the power pick is to see it,
 * as gsp_delta_light.extent.  The record carries p_sel, the selection probability the table of the context's mode implies for
 * it: 1.0f / (float)num_lights, or pmf_self of its entry of the alias table.  Both sides below read THIS word.
 *
 * radiance and density of a world direction d -- ONE function, called by both sides (float32 in this order):
 *     e = to_local * d;   s = sqrt(e.x * e.x + e.z * e.z);   u = atan2(e.x, -e.z) * (1 / 2pi) + 0.5;   v = 1 - atan2(s, e.y) * (1 / pi)
 *     radiance = the bilinear lookup at (u, v), operation for operation the one of the escape above
 *     ci = (uint32)clamp(u * (float)Cw, 0, Cw - 1) with NaN -> 0;   cj likewise from v and Ch
 *     density = s > 0 ? ((pmf(cj * Cw + ci) * (float)Cw) * (float)Ch) / ((2 pi^2) * s) : 0        (2 pi^2 = 19.739208802178716f)
 * (s is sin(theta) of a unit direction: taken from the direction, not from v.)
 *
 * Pick and sample.  The vertex makes the same three draws (r, e1, e2) and the same pick.  A pick that lands on the environment
 * record draws ONE FURTHER 32-bit word r2 and picks the cell c through the cell table as "Light selection" picks a light.  This
 * is the one kind of light whose pick lengthens the path's random stream by one draw.  (Under disable_nee no light sample is
 * used: the word is not drawn, lightPdf = 0, and the stream is that of a context without the switch.)  Then
 *     u = ((float)(c % Cw) + e1) / (float)Cw;   v = ((float)(c / Cw) + e2) / (float)Ch
 *     theta = (1 - v) * pi;   phi = (u - 0.5) * (2 pi);   (st, ct) = sincos(theta);   (sp, cp) = sincos(phi)
 *     e = (st * sp, ct, -(st * cp));   L = local_to_world * e   (row r: (m[r][0] * e.x + m[r][1] * e.y) + m[r][2] * e.z)
 * and the function above is called on L: emission = its radiance, lightPdf = its density * p_sel, Ldist = 1e30f.
 *
 * NEE.  The gate is the existing one (lightPdf != 0 included).  weight = power_heuristic(lightPdf, lb.pdf), the triangle's
 * textbook form;  nee = ((((w * NoL) * lb.f) * weight) * emission) / lightPdf, behind the firefly test like every emitted term.
 *
 * Escapes.  With NEE on, countEmitted == 0 and wasDelta == 0 an escaping path adds
 *     (radiance * power_heuristic(lastPdf, density * p_sel)) * weight
 * and otherwise radiance * weight as before: camera rays, rays after a delta bounce, disable_nee.  With disable_nee the frame is
 * therefore that of a context without the switch.  A medium event of "Scattering media" still takes no light sample (the ray it
 * sends meets a back face of its own closed shape next, not the environment).
 *
 * Media: as "Delta lights" -- a context with the switch on and an envmap resident runs the kernels of scattering media whatever
 * its media.
 *
 * Limits.  Shadow rays stop at every surface, so the sky behind a window pane is still found by BSDF sampling only.  The density
 * is per cell, not per texel, above 512 x 256.
 */
#define GSP_LIGHT_ENVIRONMENT 4u /* internal: the kind word of the environment record; gsp_set_delta_lights rejects it */
typedef struct gsp_envmap_sampling {
  uint32_t enabled;     /* 0 = off */
  float extent;         /* radius of the scene as the power pick is to see it; > 0 and finite when enabled */
  uint32_t reserved[2]; /* 0 */
} gsp_envmap_sampling;  /* 16 B */
int gsp_set_envmap_sampling(gsp_context* ctx, const gsp_envmap_sampling* sampling); /* NULL = off */

/*
 * Light grid: opt-in SPATIAL light selection -- one alias table per cell of a regular grid over the scene.
 *
 * GSP_LIGHTS_POWER stores one selection probability per light for the whole scene: a wall point next to a small lamp sends that
 * lamp one shadow ray in a thousand when a large panel elsewhere holds the power.  gsp_set_light_grid(ctx, &{enabled = 1,
 * resolution}) makes the table a function of position: a grid over the bounding box of the scene's geometry, one alias table per
 * cell, each light weighted by power / distance^2 to that cell.  The pick makes the same three draws and reads ONE 16-byte entry,
 * of the table of the shading point's cell; traversal, the queues and the path state are what they were.
 *
 * A switch of its own, CONTEXT STATE beside the light mode and the estimator: it survives gsp_upload_scene and gsp_update_tables
 * and may be set with a scene resident (the samples in flight finish first, then the tables are packed again from the context's
 * host copy and uploaded, as gsp_set_light_sampling does).  NULL or enabled == 0 drops the grid.  A context that never enables it,
 * or has disabled it again, runs the kernels, holds the table bytes and returns the frame of before, bit for bit.
 *
 * Prerequisites and validation (the state stays unchanged on every failure).  GSP_ERR_INVALID when enabled != 0 and: a word of
 * reserved is not 0; a component of resolution is above 64; resolution mixes zero and non-zero components (0, 0, 0 = auto); the
 * context does not run GSP_LIGHTS_POWER together with GSP_ESTIMATOR_TEXTBOOK -- the reference estimator's weights read the pdf of
 * ANOTHER light, which a position-dependent pick would only compound, so gsp_set_light_sampling(.., POWER) and
 * gsp_set_estimator(.., TEXTBOOK) come first, and leaving either mode with the grid on is GSP_ERR_INVALID as well; the context
 * samples its environment map as a light (gsp_set_envmap_sampling) -- and gsp_set_envmap_sampling(enabled) with the grid on is
 * GSP_ERR_INVALID in turn.  The environment record stores one p_sel per table; a p_sel per cell is a follow-up.  Delta lights are
 * in scope.
 *
 * Bounds.  The box [lo, hi] of every vertex of every instance as gsp_upload_scene received it (object -> world as the BVH forms
 * it, float32).  gsp_update_instances does not move it.  A scene without lights, or without a vertex, has no grid.
 *
 * Resolution.  Explicit: nx, ny, nz as given.  Auto: the largest m <= 32 with n_axis = clamp(round(extent_axis / (longest / m)),
 * 1, m) (cells as near cubic as the rounding allows) whose cells * num_lights is at most 2^20 entries (a 16 MB image).  An axis
 * without extent has 1 cell either way.  An explicit resolution beyond that cap -- or a light table beyond it at 1 x 1 x 1 -- is
 * GSP_ERR_NOMEM from the call that would build the grid (the setter under a resident scene, else gsp_upload_scene).
 * gsp_get_light_grid reports what the RESIDENT tables were built with: enabled (0 when there is no grid resident), the resolved
 * resolution, and bounds = {lo.x, lo.y, lo.z, hi.x, hi.y, hi.z}; either pointer may be NULL.
 *
 * Cell of a point p, float32 per axis:  cell = (hi - lo) / (float)n;  inv_cell = (float)n / (hi - lo)  (both 0 on an axis without
 * extent);  f = floor((p - lo) * inv_cell);  the axis index is f when 0 <= f < n.  A point that fails the test on any axis -- outside
 * the box, on its upper face when the product reaches n, or not finite -- takes the FALLBACK: the power alias table of "Light
 * selection" with its trailing inv_sum_w, which stays in front of the grid.  Moved instances and escaped positions are therefore
 * always defined and unbiased.  Cell number = (iz * ny + iy) * nx + ix.
 *
 * The weight of light i for the cell of centre c = lo + (index + 0.5f) * cell -- ONE function (csrc/pt_lightgrid.h), float32, called by
 * the builder and by the emitter-hit pdf below.  Rcell = 0.5f * sqrt((cell.x^2 + cell.y^2) + cell.z^2);  Y as in "Light selection":
 *     triangle:     cen = ((v0 + v1) + v2) * (1 / 3.f);  Rtri = sqrt(max over vertices of |v - cen|^2);  n = cross(v1 - v0, v2 - v0)
 *                   d = c - cen;  R = Rcell + Rtri;   w = (Y(radiance) * A) / max(dot(d, d), R * R)
 *                   w = 0 when EVERY corner of the cell lies behind the emitting side by more than a margin:
 *                       smax = dot(n, d) + ((|n.x| * (0.5f * cell.x) + |n.y| * (0.5f * cell.y)) + |n.z| * (0.5f * cell.z))
 *                       S = ((|c.x| + |c.y|) + |c.z|) + ((|cen.x| + |cen.y|) + |cen.z|)) + (Rcell + Rtri);   smax < -((1e-4f * S) * |n|)
 *                   (the margin is fifty times the float32 error of smax, so a cell never loses a light that a point in it sees
 *                   from the front; a cell the light's plane cuts has smax >= 0)
 *     point, spot:  d = position - c;   w = Y(intensity) / max(dot(d, d), Rcell * Rcell)
 *     directional:  w = Y(intensity)
 * All three are luminous-irradiance scales, so the kinds stay comparable inside a cell.  A weight that is not finite or not
 * positive counts as 0.  The weights of a cell go, widened to double, through the alias construction of "Light selection" as
 * they stand (sums in double, ascending index) and give the cell's table of num_lights entries and one 16-byte tail
 * {inv_sum_w, 0, 0, 0}, inv_sum_w = float32(1 / sum).  A cell whose weights are ALL 0 holds a copy of the fallback table and tail
 * 0: its picks and its hit pdf are the fallback's.  It never becomes a uniform table, which the hit pdf could not restate.
 *
 * Layout.  Behind the power pick table and its trailing record in EVERY table version (gsp_update_tables rebuilds it with the
 * tables; nothing new to call):  a 64-byte header {lo, nx | inv_cell, ny | cell, nz | hi, Rcell}, then the cells in number order,
 * (num_lights + 1) * 16 bytes each.  The LDS staging decision and the staged copy see only the bytes IN FRONT of the grid: a small
 * scene keeps its BSDF tables, lights and fallback table in LDS, the grid is read from L2 / HBM.
 *
 * The pick.  r, e1, e2 as always; the table is that of the cell of q (below), the slot and coin the r * num_lights split of "Light
 * selection"; no further draw, so the random streams of all modes coincide behind the light sample.  The point on the light and
 * the solid-angle pdf are formed at the shading point p as before.
 *
 * The emitter-hit pdf (rule 4 of "Estimator", made positional):  p_sel = weight(cell of the ray's origin o, the hit triangle's
 * vertices from the intersection packet, the hit's emission, A) * inv_sum_w[cell];  a cell with tail 0 or an origin without a
 * cell:  the rule of GSP_LIGHTS_POWER on the fallback's tail.
 *
 * WHICH POINT NAMES THE CELL.  The two ends of MIS must name the same cell, and the ray's origin is not the shading point: it is
 * q = p + 0.0001f * faceforward(N, -wi, N), the origin the vertex gives its continuation ray (rayhit.rchit:793).  So the PICK
 * uses the cell of q -- formed before the light sample from the BSDF sample's direction, the very expression the continuation
 * stores -- and the hit end reads the origin its path record carries, the same three floats.  (A vertex whose BSDF sample is
 * invalid forms q from that sample all the same; a NaN takes the fallback, and such a path ends there.)  Camera rays and rays
 * behind a delta bounce take the full weight as before and read no cell.
 */
typedef struct gsp_light_grid {
  uint32_t enabled;       /* 0 = off */
  uint32_t resolution[3]; /* cells along x, y, z: each 1..64, or 0, 0, 0 = auto */
  uint32_t reserved[4];   /* 0 */
} gsp_light_grid;         /* 32 B */
int gsp_set_light_grid(gsp_context* ctx, const gsp_light_grid* grid); /* NULL or enabled == 0: off */
int gsp_get_light_grid(gsp_context* ctx, gsp_light_grid* resolved, float bounds[6]); /* what the resident tables were built with */

/* Block until all queued work of the context has finished. */
int gsp_sync(gsp_context* ctx);

/* Full frame, RGBA32F row-major, width*height*4 floats; pixels this context
 * does not own are written as 0. */
int gsp_download(gsp_context* ctx, float* out_rgba);
/* Only the owned pixels, in pixel_ids order: num_pixels*4 floats. */
int gsp_download_compact(gsp_context* ctx, float* out_rgba);
/* The accumulate buffer as it stands, WITHOUT waiting for the paths still in
 * flight (compact layout, num_pixels*4 floats): every pixel holds the running
 * mean of its first *samples_folded timestamps.  This is what the reference's
 * presentation pass shows each frame (DrawTexture blit of accumulateBuffer,
 * S/renderer/PathTracer.cpp:41-55) while the next frames are already tracing;
 * a viewer calls it once per displayed frame and gsp_download only at the end. */
int gsp_peek(gsp_context* ctx, float* out_rgba, uint32_t* samples_folded);
/* Device-to-device copy of the compact accumulate buffer into caller-owned
 * device memory (e.g. a tensor handed to an RCCL gather). */
int gsp_copy_accum_to_device(gsp_context* ctx, void* device_dst, uint64_t bytes);
/* (r05) gsp_peek into caller-owned DEVICE memory: the compact accumulate buffer as it stands, no wait for the paths in flight,
 * no trip through host memory -- the reference's blit samples accumulateBuffer on the GPU (S/renderer/PathTracer.cpp:41-55); a
 * viewer that presents from device memory (an interop texture, a tensor) calls this once per displayed frame.  The copy is
 * complete when the call returns.  `bytes` >= num_pixels * 16. */
int gsp_peek_to_device(gsp_context* ctx, void* device_dst, uint64_t bytes, uint32_t* samples_folded);
/* Overwrite the compact accumulate buffer from host memory (checkpoint/resume:
 * buffer + next timestamp are the whole integrator state). */
int gsp_upload_accum(gsp_context* ctx, const float* rgba, uint64_t num_pixels);

/*
 * LDR film: tone mapping on the GPU and an 8-bit read-back.
 *
 * The reference's scenes declare <film type="ldrfilm"> (PNG, gamma 2.2) and its presentation pass tone-maps in a shader
 * (ACESFilm, common.glsl:74-82); no running reference code defines an 8-bit frame, so this header does.  The calls below read
 * the accumulate buffer and write RGBA8 (R in bits 0-7, the convention of gsp_texture); they change no state of the frame.  A
 * display needs 4 bytes per pixel over PCIe instead of 16.
 *
 * Per pixel.  Arithmetic is float32 in the order written; log and exp are the library's deterministic functions.  The constants
 * derived from the struct are formed once on the host in double and rounded to float: 2^exposure, 1/gamma, scale, invWp2.
 *   1. rgb from the accumulate buffer; a NaN channel becomes 0 and a negative channel (-Inf included) becomes 0.
 *   2. c *= 2^exposure.
 *   3. the tone curve:
 *        CLAMP     nothing.
 *        ACES      per channel (x * (2.51 x + 0.03)) / (x * (2.43 x + 0.59) + 0.14).
 *        REINHARD  Y = (0.2126 r + 0.7152 g) + 0.0722 b  (the weights of the adaptive rule), Lp = Y * scale,
 *                  Y' = (Lp * (1 + Lp * invWp2)) / (1 + Lp), c *= Y' / Y; Y == 0: the pixel is black.
 *                  scale = key / Lavg (key 0 = 0.18), invWp2 = 1 / ((Lmax * scale)^2 * b^4), b = clamp(1 - burn, 1e-8, 1).
 *   4. clamp to [0, 1].  A NaN at this point can only be an overflowed curve (Inf / Inf: a saturated pixel) and becomes 1.
 *   5. encode: gamma > 0: v == 0 ? 0 : exp(log(v) * (1 / gamma));
 *              gamma == 0 (sRGB): v <= 0.0031308 ? 12.92 v : 1.055 * exp(log(v) * (1 / 2.4f)) - 0.055.
 *   6. byte = (uint32)(v * 255 + 0.5); A = 255.
 *
 * Frame statistics (REINHARD with log_avg_luminance or max_luminance left 0, and gsp_frame_luminance).  Over the owned pixels
 * whose three channels are finite and whose Y is, on the buffer as it is (exposure does not enter), channels after step 1:
 *     q = (int64) rintf(log(Y + 1e-3f) * 1048576.0f),  S = sum of q,  n = their number,  Lmax = max Y,
 *     Lavg = (float) exp((double) S / (1048576.0 * n)).
 * S is an INTEGER sum and Lmax a max over non-negative float bit patterns: neither depends on the order of summation, so any
 * launch shape, any partition of the frame over shares or GPUs and a plain host loop give the same bits.  A frame with n == 0,
 * Lavg <= 0 or Lmax <= 0 tone-maps with scale = 1 and invWp2 = 0.
 *
 * struct_size follows the rule of gsp_render_params (fields beyond it are 0); a NULL gsp_display and struct_size 0 are the zeroed
 * struct = CLAMP + sRGB.  GSP_ERR_INVALID (text at gsp_last_error) for: an unknown tonemap id; an exposure that is not finite or
 * lies outside -64 .. 64; a negative or non-finite gamma; key or burn outside 0 .. 1; negative or non-finite supplied luminances.
 */
#define GSP_TONEMAP_CLAMP 0u    /* ldrfilm tonemapMethod "gamma": scale, clamp, encode */
#define GSP_TONEMAP_REINHARD 1u /* ldrfilm tonemapMethod "reinhard" (global photographic operator) */
#define GSP_TONEMAP_ACES 2u     /* the reference's ACESFilm, common.glsl:74-82 */
typedef struct gsp_display {
  uint32_t struct_size;    /* sizeof(gsp_display) of the host's header; same rule as gsp_render_params / gsp_lens */
  uint32_t tonemap;        /* GSP_TONEMAP_* */
  float exposure;          /* f-stops; colour is multiplied by 2^exposure first */
  float gamma;             /* > 0: v^(1/gamma); 0 = the sRGB curve */
  float key, burn;         /* Reinhard: key 0 = 0.18; burn in [0, 1] */
  float log_avg_luminance; /* Reinhard: > 0 = use this value; 0 = measure the frame */
  float max_luminance;     /* same */
} gsp_display;             /* all zero = clamp + sRGB */
typedef struct gsp_luminance {
  int64_t log_sum_q20; /* S */
  uint64_t pixels;     /* n */
  float log_avg, max;  /* Lavg (0 when n == 0), Lmax */
} gsp_luminance;
/* The frame statistics above.  drain != 0 completes the queued samples first (like gsp_download); 0 measures the buffer as it
 * stands (like gsp_peek). */
int gsp_frame_luminance(gsp_context* ctx, int drain, gsp_luminance* out);
/* gsp_download's 8-bit counterpart: completes the queued samples; full frame, width*height words, unowned pixels = 0. */
int gsp_download_display(gsp_context* ctx, const gsp_display* display, uint32_t* out_rgba8);
/* gsp_peek's: compact (num_pixels words), no wait for the paths in flight, same meaning of samples_folded. */
int gsp_peek_display(gsp_context* ctx, const gsp_display* display, uint32_t* out_rgba8, uint32_t* samples_folded);
/* gsp_peek_to_device's: `bytes` >= num_pixels * 4; complete when the call returns.  The kernel writes a 16-byte aligned
 * destination directly; any other one receives a device-to-device copy of the context's own RGBA8 buffer. */
int gsp_peek_display_to_device(gsp_context* ctx, const gsp_display* display, void* device_dst, uint64_t bytes, uint32_t* samples_folded);

/*
 * Feature buffers: first-hit albedo, shading normal, depth and object identity per pixel.
 *
 * What a denoiser, a compositor or a debugger needs beside the beauty image.  No reference code defines them, so this header does.
 *
 * A FEATURE SAMPLE of (pixel, timestamp) is the primary ray generate_path yields for that pixel and timestamp under the context's
 * lens (gsp_set_lens) and the pixel_filter / pixel_filter_param of the call: the camera ray of the beauty sample with the same
 * timestamp, bit for bit.  With no filter and no lens every feature sample of a pixel is the same ray and the mean equals one
 * sample, bit for bit; with a filter or a lens the planes are anti-aliased / defocused exactly as the beauty image is.
 *
 * The closest hit follows the library's rule (min t, then min triangle id).  At the hit, with shade_vertex's expressions:
 *   normal    SN as shade_vertex forms it: the interpolated transformInvT * n, normalised, after the two-faced flip
 *             (rayhit.rchit:690-707); world space.
 *   depth     the hit's t: the distance along the ray -- not camera z (with a lens there is no single camera axis).
 *   albedo    DIFFUSE: reflectance.  SMOOTH_PLASTIC, ROUGH_PLASTIC, SMOOTH_FLOOR, ROUGH_FLOOR: diffuse.  ROUGH_CONDUCTOR:
 *             reflectance.  SMOOTH_CONDUCTOR, SMOOTH_DIELECTRIC: (1, 1, 1).  A record whose has_texture resolves in a textured
 *             scene: the texture value shade_vertex takes as kD.  A hit on a triangle with non-zero emission: min(emission, 1)
 *             per channel instead.  The resident diffuse record holds reflectance / pi (float32, formed at upload): the albedo of
 *             DIFFUSE is DEFINED as that float32 value times float32 pi, which may differ from the uploaded reflectance in the
 *             last bit.
 *   coverage  1 on a hit.  A miss contributes 0 to every channel of both float planes, with or without an environment map.
 *   ids       uint32 x 4, not averaged: {scene-wide triangle index as gsp_trace reports it, BSDF handle, instance index, feature
 *             samples folded}.  The first three are those of the FIRST feature sample folded into the pixel in this frame, and
 *             0xffffffff when that sample missed.
 *
 * Three planes per owned pixel, 16 bytes each: albedo = {r, g, b, coverage} and geom = {nx, ny, nz, depth} (RGBA32F running means)
 * and ids.  The mean: with n = the pixel's folded count and a = 1.0f / (float)(n + 1), every channel becomes
 *     mean + (sample - mean) * a            (float32, in this order: mix(mean, sample, a))
 * -- the form that returns the sample exactly for n == 0 and the mean exactly when sample == mean.  Samples are folded in
 * increasing timestamp order, so one call of 5 samples and calls of 2 + 3 give the same bits.  The mean normal is not
 * re-normalised.  gsp_frame_begin clears the planes; they are allocated by the first call of a context that asks for them
 * (48 bytes per owned pixel), a context that never does holds nothing.
 *
 * gsp_render_features reads struct_size, spp, first_timestamp, pixel_filter and pixel_filter_param of `params` and ignores the
 * rest, the adaptive fields included: EVERY owned pixel gets spp feature samples.  It does not touch the accumulate buffer, the
 * primary-hit memo, the pixel statistics or the beauty timestamps, and adds nothing to gsp_stats.  It does NOT wait for the
 * samples gsp_render has left in flight: they stay queued and finish with the next gsp_render / gsp_download exactly as they would
 * have without this call, so a frame's image and counters do not depend on feature calls between its render calls.  The pass sees
 * the newest version of the scene (tables and geometry, whatever versions the samples in flight still carry); on a scene that
 * gsp_update_instances has split into two trees it walks BOTH trees per ray and keeps the closer hit, as the tail of a drain does
 * -- the scene is not rebuilt.
 * The pass is complete when the call returns.  GSP_ERR_INVALID (text at gsp_last_error): no scene or no frame, spp == 0, an
 * unknown filter id, a negative or non-finite filter parameter, or a BVH deeper than the 34 levels a lane's stack holds.
 */
int gsp_render_features(gsp_context* ctx, const gsp_render_params* params);
/* Full-frame layout like gsp_download: width*height records of 4 floats / 4 floats / 4 words, unowned pixels 0.  Any pointer may
 * be NULL.  Staged through the pinned buffers of the frame read-back. */
int gsp_download_features(gsp_context* ctx, float* albedo, float* geom, uint32_t* ids);
/* The same planes, COMPACT (num_pixels records each, pixel_ids order, as gsp_copy_accum_to_device), into caller-owned device
 * memory of bytes_each >= num_pixels * 16 bytes per destination; any pointer may be NULL.  Complete when the call returns. */
int gsp_copy_features_to_device(gsp_context* ctx, void* albedo, void* geom, void* ids, uint64_t bytes_each);

/*
 * Denoiser: an edge-avoiding a-trous wavelet filter of the frame, guided by the feature buffers.
 *
 * For a frame stopped at a few samples per pixel.  No reference code defines one, so this header does, down to the order of the
 * float32 operations.  The calls complete the queued samples first (as gsp_download does), read the accumulate buffer c (RGBA) and
 * the feature planes albedo = {a.rgb, cov} and geom = {n.xyz, z}, and change no state of the frame: the image, the feature planes,
 * the pixel statistics, the memo and gsp_stats stay as they were.  Scratch buffers of 16 bytes per pixel each (four of them) are
 * allocated by the first denoise call of a context; a context that never denoises holds none.
 *
 * Arithmetic is float32 in the order written (no contraction); exp is the library's deterministic exp (0 below -87.34).
 *
 * Prepare, per pixel p:
 *     valid = every one of c.r, c.g, c.b is finite
 *     a'_k  = a_k + (1 - cov)                 (a miss counts as albedo 1: the background passes through)
 *     A_k   = a'_k < 0.01f ? 0.01f : a'_k
 *     e_k   = c_k / A_k
 *     L     = (0.2126 e.r + 0.7152 e.g) + 0.0722 e.b
 * Level i = 0 .. iterations-1, step s = 2^i.  For a valid centre p the taps are q = p + s * (dx, dy), dy = -2..2 in the outer loop,
 * dx = -2..2 in the inner loop: this is the order of summation.  A tap outside the frame is skipped, a tap whose pixel is not
 * valid is skipped.  For every other tap, with k = {0.0625, 0.25, 0.375, 0.25, 0.0625}:
 *     h   = k[dx+2] * k[dy+2]
 *     dn  = ((n_p-n_q).x^2 + (n_p-n_q).y^2) + (n_p-n_q).z^2
 *     rz  = z_p == z_q ? 0 : (z_p - z_q) / (z_p + z_q)
 *     da  = ((a'_p-a'_q).r^2 + (a'_p-a'_q).g^2) + (a'_p-a'_q).b^2
 *     rl  = (L_p - L_q) / ((L_p + L_q) + 1e-3f)                  (L of THIS level's input)
 *     x   = ((dn * inv_sn2 + rz*rz * inv_sz2) + da * inv_sa2) + (rl*rl) * (inv_sc2 * 4^i)
 *     w   = h * exp(-x);   sum_w += w;   sum_k += w * e_q.k
 * then e'_p.k = sum_k / sum_w and L' is recomputed from e'.  The centre tap has x = 0 exactly, so sum_w >= 9/64.  inv_* are
 * 1 / sigma^2, formed once on the host in double and rounded to float (at most FLT_MAX); a sigma of +Inf gives 0: that term is
 * off.  4^i is an exact float.  A pixel that is not valid keeps its e, is never a neighbour, and leaves the filter as c, unchanged
 * bit for bit.
 * Output: out.k = e_final.k * A_k for a valid pixel, out.w = c.w.
 *
 * Defaults (a field left 0): iterations 5, sigma_color 0.5, sigma_normal 0.3, sigma_depth 0.05, sigma_albedo 0.1.
 *
 * struct_size follows the rule of gsp_render_params (fields beyond it are 0); a NULL gsp_denoise and struct_size 0 are the zeroed
 * struct = every default.  GSP_ERR_INVALID (text at gsp_last_error) for: no frame; a frame begun with pixel_ids (a share has no
 * neighbours: use gsp_multi_*); no gsp_render_features call since gsp_frame_begin; iterations > 8; a negative or NaN sigma; a NULL
 * output pointer; `bytes` too small.
 */
typedef struct gsp_denoise {
  uint32_t struct_size; /* sizeof(gsp_denoise) of the host's header; same rule as gsp_render_params / gsp_display */
  uint32_t iterations;  /* a-trous levels, step 2^i for level i; 0 = 5; otherwise 1..8 */
  float sigma_color, sigma_normal, sigma_depth, sigma_albedo; /* 0 = default; +Inf = that term off */
} gsp_denoise;
/* Full frame like gsp_download: width*height*4 floats, through the staged read-back. */
int gsp_download_denoised(gsp_context* ctx, const gsp_denoise* denoise, float* out_rgba);
/* The same frame into caller-owned device memory of `bytes` >= width*height*16 (any alignment); complete when the call returns. */
int gsp_denoise_to_device(gsp_context* ctx, const gsp_denoise* denoise, void* device_dst, uint64_t bytes);
/* The LDR film (see "LDR film") of the DENOISED frame: the tone map, the encode and -- where the display asks for them -- the frame
 * statistics are those of the denoised buffer, not of the accumulate buffer.  width*height RGBA8 words. */
int gsp_download_denoised_display(gsp_context* ctx, const gsp_denoise* denoise, const gsp_display* display, uint32_t* out_rgba8);

/*
 * Temporal accumulation: the history of earlier frames reprojected into the new camera and blended with the new frame.
 *
 * For a viewer that renders a sample or a few per frame under a moving camera: gsp_frame_begin clears the accumulate buffer, this
 * keeps what earlier frames collected.  It is the temporal half of SVGF; the "Denoiser" above is the spatial half and runs on the
 * result (gsp_download_temporal_denoised).  No reference code defines it, so this header does, down to the order of the float32
 * operations.  Arithmetic is float32 in the order written (no contraction).
 *
 * State, allocated by the first temporal call of a context (a context that never makes one holds none): two ping-pong sets of
 * history planes over the full frame, H = {r, g, b, len} (16 bytes; len = the history length as a float), G = {n.x, n.y, n.z, z}
 * (16 bytes) and I = the instance index (4 bytes, 0xffffffff = background) -- 72 bytes per pixel in all --, the camera and the
 * frame size the history belongs to, and a flag history_valid.  history_valid is cleared by gsp_temporal_reset, by
 * gsp_upload_scene and by a gsp_frame_begin whose width or height differs from the history's.
 *
 * The pixel's own data come from the feature planes of THIS frame (gsp_render_features): cov = albedo.w, inst = ids.z, geom.
 *     surface pixel      inst != 0xffffffff && cov >= 0.5f:   n = geom.xyz / cov (three divisions), z = geom.w / cov, I = inst
 *                        (exact for the unfiltered pinhole, where cov == 1)
 *     background pixel   otherwise:  n = 0, z = 0, I = 0xffffffff
 *     c = the pixel's accumulate record; c is finite when c.r, c.g and c.b are.
 *
 * Reprojection of pixel (px, py), W x H the frame, M / eye / zplane the CURRENT camera's (see "Thin lens": Camera ray):
 *  1. d = flipY(M * normalize((-((float)px - W/2), (float)py - H/2, zplane))) -- the PINHOLE ray through the integer pixel
 *     coordinate, whatever lens or pixel filter the frame was rendered with.
 *  2. surface:     P.k = eye.k + d.k * z;   v.k = P.k - eye_prev.k;   ze = sqrt((v.x*v.x + v.y*v.y) + v.z*v.z)
 *     background:  v = d  (a point at infinity: the camera's translation does not move it)
 *  3. l = Minv_prev * (v.x, -v.y, v.z), each component summed as (m_r0 * a + m_r1 * b) + m_r2 * c.  Minv_prev is the inverse of
 *     the upper-left 3x3 of the previous to_world, formed once on the host in double (adjugate / determinant) and rounded to
 *     float.  A determinant that is 0 or not finite, or an entry that is not finite as a float: GSP_ERR_INVALID at the call.
 *  4. not (l.z > 0): no history.
 *  5. t = zplane_prev / l.z;   fx = W/2 - l.x * t;   fy = H/2 + l.y * t.   zplane_prev = (max(W, H) / 2) / tanf(fov_prev / 2),
 *     formed on the host in float as gsp_focus_distance forms zplane; W/2 is (float)W / 2.0f.
 *  6. Snap: r = rint(fx); if |fx - r| < 1e-3f then fx = r; the same for fy.  An unmoved camera then reads exactly its own pixel
 *     with weight 1.  The constant, a thousandth of a pixel, is part of the definition.
 *  7. not (fx > -1 && fx < W && fy > -1 && fy < H): no tap can lie inside the frame: no history.  Otherwise x0 = floor(fx),
 *     wx = fx - x0, y0 = floor(fy), wy = fy - y0; the taps are (x0,y0), (x0+1,y0), (x0,y0+1), (x0+1,y0+1) in this order with
 *     weights (1-wx)*(1-wy), wx*(1-wy), (1-wx)*wy, wx*wy.
 * A tap q is skipped when its weight is 0; when it lies outside the frame; when not (H_q.len > 0) or one of H_q.r, .g, .b is not
 * finite; when I_q != I (for a background pixel: I_q != 0xffffffff); and, for a surface pixel, when
 * |ze - z_q| > depth_tolerance * ze, or when (n.x*n_q.x + n.y*n_q.y) + n.z*n_q.z < normal_min.  ze is the distance of P from the
 * previous eye: the sense in which the feature depth of the previous frame is a depth.  Over the kept taps, in tap order:
 *     sw += w;   s.k += w * H_q.k;   sl += w * H_q.len
 * Blend.  There is history when history_valid and sw >= 0.01f.
 *     with history:     prev.k = s.k / sw;   len = sl / sw
 *         c finite:     N = min(len + 1, max_history);  a = max(alpha, 1 / N);  H'.k = prev.k + (c.k - prev.k) * a;  H'.len = N
 *         c not finite: H'.k = prev.k;  H'.len = min(len, max_history)
 *     without history:  H' = {c.r, c.g, c.b, 1} when c is finite, {c.r, c.g, c.b, 0} when not: the pixel is nobody's history
 * G' = {n, z} and I' = I of this frame in both cases.
 *
 * Defaults (a field left 0): max_history 32, alpha 0.2, depth_tolerance 0.02, normal_min 0.9 (the last three formed in double
 * and rounded to float).  Because 0 means the default, alpha is any value in (0, 1]; the pure running mean is alpha = FLT_MIN
 * (a = 1 / N until max_history caps N).  Likewise a tolerance or normal_min of exactly 0 is written as a tiny value.
 *
 * Frames of a viewer.  Each frame is gsp_frame_begin, gsp_frame_sample_base(first timestamp of the frame), gsp_render,
 * gsp_render_features, gsp_temporal_accumulate: with the base the frame's record c is the plain mean of its own samples and every
 * frame draws new random numbers (see gsp_frame_sample_base below); without it a frame rendered at first_timestamp T > 0 on the
 * cleared buffer is darker by n / (T + n), and frames that all start at timestamp 0 repeat one noise pattern.
 *
 * Out of scope.  By default the world is taken as static between two frames: an instance that moved is handled only by rejection
 * (the instance-index, depth and normal tests); "Temporal accumulation: moved instances" below follows it.  There are no gsp_multi_* variants: a
 * share has no neighbours, and gathering the ids plane is a change of its own -- a frame begun with pixel_ids is refused.  The
 * filtered output is not fed back into the history by the calls of this section ("Illumination history" below adds that).
 */
typedef struct gsp_temporal {
  uint32_t struct_size; /* sizeof(gsp_temporal) of the host's header; same rule as gsp_denoise (fields beyond it are 0; NULL and
                           struct_size 0 = the zeroed struct = every default) */
  uint32_t max_history; /* cap of the history length; 0 = 32; otherwise 1..65536 */
  float alpha;           /* floor of the blend weight of the new frame; 0 = 0.2; otherwise (0, 1] */
  float depth_tolerance; /* relative; 0 = 0.02; otherwise > 0 */
  float normal_min;      /* smallest dot product of the two normals; 0 = 0.9; otherwise [-1, 1] */
} gsp_temporal;
/* The frame's samples are numbered from `base`.  gsp_frame_begin clears the accumulate buffer, and the fold of sample `timestamp`
 * weighs it 1 / (timestamp + 1) (raygen.rgen:84-108): a fresh frame rendered at first_timestamp T > 0 holds its mean times
 * n / (T + n), not its mean.  A viewer that wants a NEW random sequence in every frame (the seed is tea(pixel, timestamp)) and the
 * plain mean of the frame's own samples calls this between gsp_frame_begin and the frame's first gsp_render: the samples keep
 * their timestamps for the seeds, bit for bit, and sample base + k is folded as the frame's k-th sample, so the frame equals,
 * bit for bit, what a frame would hold whose timestamps 0 .. n-1 drew the random numbers of base .. base + n-1.  The frame's
 * gsp_render calls then take first_timestamp >= base; gsp_peek's *samples_folded counts from base.  gsp_frame_begin sets the
 * base back to 0.  GSP_ERR_INVALID: no frame; after the frame's first gsp_render; with base != 0 an adaptive gsp_render or a
 * first_timestamp below base (at that gsp_render).  gsp_render_features is not concerned: its planes fold by their own count. */
int gsp_frame_sample_base(gsp_context* ctx, uint32_t base);
/* Completes the queued samples (as gsp_download does), runs the reprojection from the old history set into the other one and
 * swaps them, records the current camera and size and sets history_valid.  Changes nothing of the frame: the accumulate buffer,
 * the feature planes, the pixel statistics, the memo and gsp_stats stay as they were.  GSP_ERR_INVALID (text at gsp_last_error):
 * no frame; a frame begun with pixel_ids; no gsp_render_features call since gsp_frame_begin; a second accumulate in the same
 * frame; max_history > 65536; alpha outside [0, 1] or NaN; a negative or NaN depth_tolerance; normal_min outside [-1, 1] or NaN;
 * a singular previous camera (step 3). */
int gsp_temporal_accumulate(gsp_context* ctx, const gsp_temporal* temporal);
/* Forgets the history: the next gsp_temporal_accumulate starts from its frame alone.  Frees nothing. */
int gsp_temporal_reset(gsp_context* ctx);
/* The four read-outs below return GSP_ERR_INVALID when no gsp_temporal_accumulate has succeeded since the history was last
 * invalidated (or since the context was made). */
/* H of the newest set as stored: width*height*4 floats, .w = the history length.  Through the staged read-back.  With
 * gsp_temporal_demodulate on, H.rgb is illumination (see "Illumination history"; gsp_download_temporal_image is the image). */
int gsp_download_temporal(gsp_context* ctx, float* out_rgba);
/* The same into caller-owned device memory of `bytes` >= width*height*16 (any alignment); complete when the call returns. */
int gsp_temporal_to_device(gsp_context* ctx, void* device_dst, uint64_t bytes);
/* The "Denoiser" with H as its colour source c instead of the accumulate buffer, guided by THIS frame's feature planes (so it
 * needs a frame and its gsp_render_features, like gsp_download_denoised); out.w = the history length. */
int gsp_download_temporal_denoised(gsp_context* ctx, const gsp_denoise* denoise, float* out_rgba);
/* ... and the LDR film of that (as gsp_download_denoised_display): width*height RGBA8 words. */
int gsp_download_temporal_denoised_display(gsp_context* ctx, const gsp_denoise* denoise, const gsp_display* display, uint32_t* out_rgba8);

/*
 * Variance-guided filter: luminance moments beside the history, and the a-trous filter with SVGF's variance-scaled edge-stop.
 *
 * The "Denoiser" tolerates a fixed relative luminance difference, whatever the pixel's noise.  This section adds the part that
 * gives SVGF its name: the temporal pass keeps the first and second luminance moments of the history, they become a per-pixel
 * variance (a spatial estimate where the history is too short), and the luminance edge-stop of every level is scaled by the local
 * standard deviation, with the variance carried through the levels.  No reference code defines it, so this header does, down to
 * the order of the float32 operations.  Arithmetic is float32 in the order written (no contraction); exp is the library's
 * deterministic exp (0 below -87.34); sqrt and / are correctly rounded; max(x, 0) is x > 0 ? x : 0, so a NaN gives 0.
 *
 * 1. Moments.  gsp_temporal_track_moments(ctx, on) is context state, off by default.  A CHANGE of the value clears history_valid,
 * so moments and history always have the same age; a call with the current value does nothing.  While it is on,
 * gsp_temporal_accumulate also keeps two ping-pong planes M = {m1, m2, r, 0} (16 bytes per pixel each, allocated by the first
 * accumulate with tracking on: 104 bytes per pixel of temporal state in all), and H, G and I are, bit for bit, what the call
 * produces with tracking off.  Per pixel, with l = L of "Denoiser: Prepare" applied to this frame's c and albedo record:
 *     over the kept taps of H, in tap order, with the same weights w:   sm.k += w * M_q.k   (k = m1, m2, r)
 *     with history:      prev.k = sm.k / sw
 *         c finite:      a = the blend weight of H;   m1' = prev.m1 + (l - prev.m1) * a;   m2' = prev.m2 + (l*l - prev.m2) * a;
 *                        r' = ((1 - a) * (1 - a)) * prev.r + a * a
 *         c not finite:  M' = prev
 *     without history:   M' = {l, l*l, 1, 0} when c is finite, {0, 0, 1, 0} when not
 * r is the sum of the squared frame weights inside the history: 1 / N for a running mean of N frames.  It is exact for an unmoved
 * camera; under reprojection it is mixed bilinearly like everything else, which makes it an approximation (the frames of four
 * neighbours are not the same frames).  Luminances whose square overflows float32 are outside the filter's domain.
 *
 * 2. The filter of the history.  gsp_denoise supplies iterations, sigma_normal, sigma_depth and sigma_albedo; sigma_color is
 * validated as always and not used: the variance term replaces it.
 * Prepare: "Denoiser: Prepare" with H as c.  It yields e, L, a', valid; n and z are this frame's geom plane.
 * Initial variance V of a valid pixel p (an invalid pixel has V = 0 and is nobody's neighbour):
 *     H.len >= min_history && M.r < 1:    V = max(M.m2 - M.m1 * M.m1, 0) * (M.r / (1 - M.r))
 *         (the unbiased variance of the blended history; s^2 / (N - 1) for a running mean)
 *     otherwise, over q = p + (dx, dy), dy = -3..3 in the outer loop, dx = -3..3 in the inner loop, taps outside the frame or not
 *     valid skipped, with dn and rz as in the "Denoiser":
 *         g = exp(-(dn * inv_sn2 + rz*rz * inv_sz2));   sg += g;   s1 += g * L_q;   s2 += g * (L_q * L_q)
 *         m = s1 / sg;   V = max(s2 / sg - m * m, 0)
 * Level i = 0 .. iterations-1, step s = 2^i, for a valid centre p (a pixel that is not valid keeps its e and its V):
 *     Vg: over q = p + (dx, dy), dy = -1..1 outer, dx = -1..1 inner (step 1 at every level), in-frame valid taps only, with
 *         t = {0.25, 0.5, 0.25}[dx+1] * {0.25, 0.5, 0.25}[dy+1]:   st += t;   sv += t * V_q;   Vg = sv / st
 *     inv_l = 1 / (sigma_variance * sqrt(Vg) + 1e-4f), once per centre; 0 (and Vg not formed) when sigma_variance is +Inf
 *     per tap q = p + s * (dx, dy) in the "Denoiser"'s order, with its h, dn, rz, da and its skips:
 *         x = ((dn * inv_sn2 + rz*rz * inv_sz2) + da * inv_sa2) + |L_p - L_q| * inv_l
 *         w = h * exp(-x);   sum_w += w;   sum_k += w * e_q.k;   sum_v += (w * w) * V_q
 *     e'.k = sum_k / sum_w, L' recomputed from e';   V' = sum_v / (sum_w * sum_w).  There is no 4^i factor.
 * Output: as the "Denoiser"'s (out.k = e_final.k * A_k; an invalid pixel leaves as H's record, bit for bit); out.w = H.len.
 *
 * Defaults (a field left 0): min_history 4, sigma_variance 4.  Scratch: the denoiser's four planes and two V planes of 4 bytes
 * per pixel, allocated by the first call.  The calls change no state of the frame or of the history.  GSP_ERR_INVALID: what
 * gsp_download_temporal_denoised refuses; tracking off; min_history 1 or above 65536; a negative or NaN sigma_variance.
 *
 * Out of scope.  These calls do not feed the filtered frame back into the history (gsp_temporal_svgf_feedback, "Illumination
 * history" below, does); there are no gsp_multi_* variants.
 */
typedef struct gsp_svgf {
  uint32_t struct_size; /* sizeof(gsp_svgf) of the host's header; same rule as gsp_denoise (NULL and struct_size 0 = every default) */
  uint32_t min_history; /* shortest history whose moments are trusted; 0 = 4; otherwise 2..65536 */
  float sigma_variance; /* luminance tolerance in standard deviations; 0 = 4.0; +Inf = the term off */
} gsp_svgf;
/* on != 0: gsp_temporal_accumulate keeps M.  Never fails on a context; frees nothing. */
int gsp_temporal_track_moments(gsp_context* ctx, int on);
/* M of the newest set: width*height*4 floats.  GSP_ERR_INVALID when tracking is off or there is no valid history. */
int gsp_download_temporal_moments(gsp_context* ctx, float* out_rgba);
/* The variance-guided filter of H: full frame like gsp_download_temporal_denoised. */
int gsp_download_temporal_svgf(gsp_context* ctx, const gsp_denoise* denoise, const gsp_svgf* svgf, float* out_rgba);
/* The same frame into caller-owned device memory of `bytes` >= width*height*16 (any alignment); complete when the call returns. */
int gsp_temporal_svgf_to_device(gsp_context* ctx, const gsp_denoise* denoise, const gsp_svgf* svgf, void* device_dst, uint64_t bytes);
/* ... and the LDR film of it (as gsp_download_denoised_display): width*height RGBA8 words. */
int gsp_download_temporal_svgf_display(gsp_context* ctx, const gsp_denoise* denoise, const gsp_svgf* svgf, const gsp_display* display,
                                       uint32_t* out_rgba8);

/*
 * Temporal accumulation: moved instances.  The history follows an instance whose transform gsp_update_instances changed, and the
 * screen-space motion vector of every pixel is exported.
 *
 * "Temporal accumulation" reprojects a pixel as if only the camera had moved.  With gsp_temporal_follow_instances(ctx, 1) -- context
 * state, off by default; a CHANGE of the value clears history_valid; a call with the current value does nothing -- a surface pixel
 * of an instance that moved is taken back through the instance's motion first.  With following off every call runs the
 * instructions and returns the bits it returns without this section, and nothing below is allocated, copied or launched.
 * Arithmetic is float32 in the order written (no contraction); sqrt and / are correctly rounded.
 *
 * Snapshot.  While following is on, every successful gsp_temporal_accumulate records the 16 transform floats of every instance
 * beside the camera it already records.  gsp_upload_scene drops the snapshot with the history.
 *
 * Which transforms a frame belongs to.  The context counts instance edits: a gsp_update_instances call that changes something
 * (the call compares first; one that changes nothing does not count).  The frame's first gsp_render_features records the
 * counter.  With following on, a gsp_temporal_accumulate whose counter differs from the recorded one returns GSP_ERR_INVALID: the
 * feature planes would show other transforms than the ones the call would record.  An edit belongs BEFORE the frame's
 * gsp_render_features.  With following off nothing is checked.
 *
 * Per-instance record, formed on the host in double at the accumulate and rounded to float once; T_prev = the snapshot's
 * transform, T_cur = the current one, both taken as affine (3x3 A, translation t = column 3; the fourth row is not read).  6 quads
 * = 96 bytes:
 *     B = T_prev * T_cur^-1 as three rows of four floats: B3 = A_prev * A_cur^-1, b_r3 = t_prev.r - (B3 * t_cur).r.  A_cur^-1 is
 *         adjugate / determinant, as step 3 of "Temporal accumulation" forms Minv_prev.
 *     N = transpose(B3^-1) = transpose(A_cur * A_prev^-1) as three rows, computed from the two transforms (A_prev^-1 again
 *         adjugate / determinant), not by inverting the rounded B.
 *     a class word: 0 static, 1 moved, 2 no history.
 *         static: the 16 floats of T_prev and T_cur are equal as bits (tested first).
 *         no history: A_prev or A_cur has a determinant that is 0 or not finite, or an entry of B or N is not finite as a float.
 *         This is not an error: a host may scale an object to nothing to hide it.
 *     B and N of a record of class 0 or 2 are zero.  An instance index >= num_instances is of class 2.
 *
 * Pixel.  A background pixel and a surface pixel of a class-0 instance run steps 1-7 and the tap tests of "Temporal
 * accumulation" as they stand: H', G', I' (and M') are bit for bit what they are with following off.  Class 2: no history.
 * Class 1, after step 2's P:
 *     P'.r = ((b_r0 * P.x + b_r1 * P.y) + b_r2 * P.z) + b_r3          (r = x, y, z)
 *     v.k = P'.k - eye_prev.k;   ze = sqrt((v.x*v.x + v.y*v.y) + v.z*v.z)
 *     m.r = (n_r0 * n.x + n_r1 * n.y) + n_r2 * n.z;   s = (m.x*m.x + m.y*m.y) + m.z*m.z
 *     not (s > 0): no history;  otherwise q = sqrt(s), n' = (m.x / q, m.y / q, m.z / q)
 * Steps 3-7 run on this v.  The tap test uses n' in its normal term; the instance test and the depth test (on this ze) are
 * unchanged.  G' and I' hold this frame's own n, z and I, as always.
 *
 * Motion plane.  V, 16 bytes per pixel, one plane over the full frame (nothing reads it back), made by the first followed
 * accumulate together with the table (96 bytes per instance) and counted in the context's bytes:
 *     V = {fx - (float)px, fy - (float)py, sw, cls}     fx, fy after the snap of step 6; sw = the summed weight of the kept taps
 *     cls = 0.0 where there is no reprojection (history_valid is 0, step 4 or 7 fails, class 2, s fails): the record is all zero
 *     cls = 1.0 for the static path, 2.0 for a followed pixel
 * V.xy is the screen-space motion vector an external TAA or denoiser asks for: this frame's pixel centre plus V.xy is where the
 * surface point was in the previous frame.
 *
 * Limits.  The lighting of a moved object and the shadows it casts on others lag by the history: only alpha bounds that.
 * Deforming meshes are not covered: a transform per instance is all gsp_update_instances knows.  There are no gsp_multi_* variants.
 */
/* on != 0: gsp_temporal_accumulate follows moved instances and writes V.  Never fails on a context; frees nothing. */
int gsp_temporal_follow_instances(gsp_context* ctx, int on);
/* V of the newest accumulate: width*height*4 floats.  GSP_ERR_INVALID when following is off or there is no valid history. */
int gsp_download_temporal_motion(gsp_context* ctx, float* out_rgba);
/* The same into caller-owned device memory of `bytes` >= width*height*16 (any alignment); complete when the call returns. */
int gsp_temporal_motion_to_device(gsp_context* ctx, void* device_dst, uint64_t bytes);

/*
 * Illumination history.  The two parts of SVGF that decide what a 1-spp viewer shows after a few frames: the history accumulates
 * the frame's colour divided by its first-hit albedo (illumination is smooth where textures are not, so the four bilinear taps
 * stop low-passing every texel edge once per frame), and the output of the filter's first level(s) is written back into the
 * history, so that the next frame starts from a filtered estimate.  Both are opt-in; without them every call of the sections
 * above runs the kernels it runs without this section and returns the same bits.  Arithmetic is float32 in the order written
 * (no contraction); / is correctly rounded.
 *
 * Demodulation.  gsp_temporal_demodulate(ctx, on) -- context state, off by default; a CHANGE of the value clears history_valid; a
 * call with the current value does nothing.  It allocates no plane: H then holds illumination in the same 16 bytes.  With it on,
 * gsp_temporal_accumulate forms per pixel (e, A) = "Denoiser: Prepare" of this frame's accumulate record c and albedo record:
 *     a'_k = albedo.k + (1 - cov);   A_k = max(a'_k, 0.01f);   e.k = c.k / A_k;   L = the luminance of e
 *     u = c.r, c.g, c.b finite and e.r, e.g, e.b finite        (the second half guards a quotient that overflows)
 * and "Temporal accumulation: Blend", "Variance-guided filter: 1. Moments" and "Temporal accumulation: moved instances" apply as
 * written with u for "c finite" and e.k for c.k:
 *     with history, u:         H'.k = prev.k + (e.k - prev.k) * a,  H'.len = N
 *     with history, not u:     H' = prev, the length capped as there
 *     without history, u:      H' = {e.r, e.g, e.b, 1}
 *     without history, not u:  H' = {c.r, c.g, c.b, 0}            (the raw record: nobody's history)
 * l of the moments already is L, the luminance of e, so M's formulas do not change (their "c finite" is u).  Steps 1-7, the
 * taps, their weights and tests, len, G', I' and the motion plane V are untouched: demodulation composes with
 * gsp_temporal_track_moments and gsp_temporal_follow_instances in every combination.
 *
 * Read-outs.  gsp_download_temporal and gsp_temporal_to_device return H as stored: illumination while demodulation is on.
 * gsp_download_temporal_image / gsp_temporal_image_to_device return what a viewer shows.  With demodulation on,
 *     out.k = H.k * A_k  where H.len > 0;   out = H as stored  where H.len == 0;   out.w = H.len
 * with A from THIS frame's albedo record; through a scratch plane of 16 bytes per pixel (the denoiser's output plane) where the
 * result is not written straight into an aligned destination.  With demodulation off they return H bit for bit, so one viewer
 * loop serves both settings.  Both need a gsp_temporal_accumulate in the current frame -- otherwise the albedo plane belongs to
 * another frame -- and return GSP_ERR_INVALID without one; null pointer and size are refused as by gsp_download_temporal /
 * gsp_temporal_to_device.
 *
 * Filters on a demodulated history (gsp_download_temporal_denoised*, gsp_*_temporal_svgf*, the feedback calls below).  Prepare
 * takes e = H.rgb as it is, valid = H's three channels finite, A and a' from the albedo record as always, L from e.  Everything
 * after Prepare is unchanged: the output is e_final.k * A_k for a valid pixel and H's record bit for bit for an invalid one,
 * out.w = H.len.
 *
 * Feedback.  gsp_temporal_svgf_feedback / _to_device run the variance-guided filter exactly as gsp_download_temporal_svgf /
 * gsp_temporal_svgf_to_device do (validation, defaults, scratch; tracking must be on) and, in addition, overwrite the colour
 * of the NEWEST history set with the output of the first `levels` levels, e_after = E of level levels - 1:
 *     valid pixel, demodulation on:    H.k = e_after.k
 *     valid pixel, demodulation off:   H.k = e_after.k * A_k
 * H.len, G, I, M, V, every invalid pixel and the older set keep their bits.  levels must be within 1 .. iterations, the
 * iterations being those the call resolves (5 for gsp_denoise.iterations = 0).  The call's output -- out_rgba / device_dst may
 * be NULL: then there is none, and the levels after the fed-back one are not run -- is the full filter of the history as it was
 * before the write: bit for bit what gsp_download_temporal_svgf would have returned in its place.  At most one feedback per
 * accumulate: it needs a gsp_temporal_accumulate in the current frame, and a second call before the next one is
 * GSP_ERR_INVALID ("... fed back already"): a history filtered twice is not what anyone means.
 *
 * Limits.  After a feedback every read-out of H, and the next accumulate, sees the fed-back history.  M is not filtered: the
 * variance it gives then describes the unfiltered history and is an upper bound of the fed-back one's.  Out of scope:
 * gsp_multi_* variants, separate direct and indirect histories, temporal gradients (A-SVGF).
 */
/* on != 0: the history holds illumination.  Never fails on a context; frees nothing. */
int gsp_temporal_demodulate(gsp_context* ctx, int on);
/* The image of the newest history (see "Read-outs"): width*height*4 floats, .w = the history length. */
int gsp_download_temporal_image(gsp_context* ctx, float* out_rgba);
/* The same into caller-owned device memory of `bytes` >= width*height*16 (any alignment); complete when the call returns. */
int gsp_temporal_image_to_device(gsp_context* ctx, void* device_dst, uint64_t bytes);
/* gsp_download_temporal_svgf plus the feedback of its first `levels` levels into the newest history. */
int gsp_temporal_svgf_feedback(gsp_context* ctx, const gsp_denoise* denoise, const gsp_svgf* svgf, uint32_t levels, float* out_rgba /* may be NULL */);
/* gsp_temporal_svgf_to_device plus the feedback; `bytes` is checked when device_dst is not NULL. */
int gsp_temporal_svgf_feedback_to_device(gsp_context* ctx, const gsp_denoise* denoise, const gsp_svgf* svgf, uint32_t levels,
                                         void* device_dst /* may be NULL */, uint64_t bytes);

/*
 * Temporal anti-lag.  A tap of the history is rejected by geometry alone (instance index, depth, normal), so when the LIGHTING
 * changes -- gsp_update_tables dims a light, a moved object drags its shadow across a wall -- every tap passes and the stale
 * illumination decays only as (1 - alpha)^frames.  gsp_temporal_antilag keeps a second, short history F beside the long one
 * (the responsive history of ReLAX-style denoisers), takes the mean and the standard deviation of F over a small window and
 * clamps the long history into that box; a clamped pixel's history length is cut to the short one's.  It is a call of its own
 * after gsp_temporal_accumulate: a context that never makes it runs the kernels it ran before, holds no plane of this section
 * and returns the same bits.  Arithmetic is float32 in the order written (no contraction); / and sqrt are correctly rounded.
 *
 * State.  Two ping-pong planes F = {r, g, b, len}, 16 bytes per pixel each, made by the first gsp_temporal_antilag of the
 * context and counted in its bytes.  fast_valid is true exactly when the accumulate BEFORE the current one was followed by a
 * gsp_temporal_antilag and history_valid has not been cleared since; everything that clears history_valid clears fast_valid.
 *
 * Call order.  The call needs a gsp_temporal_accumulate in the current frame, at most one call per accumulate, and it comes
 * before the gsp_temporal_svgf_feedback* of that accumulate; otherwise GSP_ERR_INVALID.
 *
 * Step A, the fast history.  Per pixel F' is what the frame's gsp_temporal_accumulate computed for H' -- the same context state,
 * the same resolved gsp_temporal, the same cameras and motion records: steps 1-7, taps, weights and tests, following and
 * demodulation -- with
 *     F_q of the OLDER fast plane for H_q, in the "len > 0, rgb finite" test of a tap and in the sums;
 *     G_q and I_q of the OLDER history set, which the accumulate left as it was;
 *     min(fast_history, max_history) for max_history;
 *     history_valid && fast_valid for history_valid.
 * Without a fast history F' = {x.r, x.g, x.b, 1} for a finite x and {c.r, c.g, c.b, 0} otherwise, x = c, or e under
 * demodulation: what "Blend" says.  The frame's records are read as they are at the call.
 *
 * Step B, the clamp, in place on H of the NEWEST set; G and I below are the newest set's.  A pixel p is processed when
 * H_p.len > 0, F'_p.len > 0 and both have finite rgb.  The window is q = p + (dx, dy), dy = -radius .. radius outer and dx
 * inner; a q counts when it is inside the frame, F'_q.len > 0 with rgb finite, I_q == I_p and, for a surface pixel (I_p is not
 * the background's 0xffffffff), (n_p.x * n_q.x + n_p.y * n_q.y) + n_p.z * n_q.z >= normal_min -- the accumulate's normal_min:
 *     n += 1.0f;  s1.k += F'_q.k;  s2.k += F'_q.k * F'_q.k                                   (k = r, g, b)
 *     n < 2 radius + 1:  the pixel is left alone
 *     m.k = s1.k / n;  v.k = max(s2.k / n - m.k * m.k, 0);  sd.k = sqrt(v.k)
 *     lo.k = m.k - sigma_scale * sd.k;  hi.k = m.k + sigma_scale * sd.k
 *     H.k = H.k < lo.k ? lo.k : (H.k > hi.k ? hi.k : H.k)
 *     if any channel changed:  H.len = min(H.len, F'_p.len)
 * G, I, M, V, the older set, every pixel that is not processed and every pixel that already lies inside its box keep their bits.
 *
 * Read-outs.  gsp_download_temporal_fast / gsp_temporal_fast_to_device return F' of the newest fast plane, .w = its length;
 * they need a gsp_temporal_antilag since the history was last invalidated and after the newest accumulate.
 *
 * Limits.  M is not clamped: with fast_history < gsp_svgf.min_history a clamped pixel falls back to the variance-guided
 * filter's spatial variance estimate.  Values whose square overflows float32 are outside the domain.  Out of scope:
 * gsp_multi_* variants, separate direct and indirect histories, temporal gradients (A-SVGF).
 */
typedef struct gsp_antilag {
  uint32_t struct_size;  /* sizeof(gsp_antilag) of the host's header; same rule as gsp_denoise / gsp_temporal (NULL and struct_size 0 = every default) */
  uint32_t fast_history; /* cap of the fast history's length; 0 = 4; otherwise 1 .. 64 */
  uint32_t radius;       /* half-width of the window; 0 = 2 (5 x 5); otherwise 1 .. 3 */
  float sigma_scale;     /* half-width of the box in standard deviations; 0 = 2.0; otherwise > 0 and finite */
} gsp_antilag;
/* Steps A and B on the frame's accumulate; complete when the call returns. */
int gsp_temporal_antilag(gsp_context* ctx, const gsp_antilag* antilag);
/* F' of the newest fast plane: width*height*4 floats, .w = its length. */
int gsp_download_temporal_fast(gsp_context* ctx, float* out_rgba);
/* The same into caller-owned device memory of `bytes` >= width*height*16 (any alignment); complete when the call returns. */
int gsp_temporal_fast_to_device(gsp_context* ctx, void* device_dst, uint64_t bytes);

/*
 * Temporal anti-aliasing.  The last stage of SVGF: the tone-mapped frame resolved over its own history.  The edge stops of the
 * filters are steered by one-sample feature planes, so under a pixel filter a silhouette pixel keeps or drops its neighbours
 * differently each frame and object edges shimmer.  The histories H cannot settle that: they are HDR, they sit in front of the
 * filter and the tone curve, and a tone curve applied to an average is not the average of tone-mapped samples.
 * gsp_temporal_taa keeps a history D of DISPLAY-LINEAR colour -- after the tone curve and the clamp to [0, 1], before the encode
 * -- fetches it through the motion plane V of the frame's accumulate, clamps it into the box of the frame's 3 x 3 neighbourhood
 * in YCoCg and blends the frame in.  It is a call of its own after gsp_temporal_accumulate: a context that never makes it runs the
 * kernels it ran before, holds no plane of this section and returns the same bits.  Arithmetic is float32 in the order written
 * (no contraction); / and sqrt are correctly rounded.
 *
 * Source.  The frame to resolve is an HDR frame of width*height*4 floats: what gsp_download_temporal_svgf,
 * gsp_temporal_svgf_feedback, gsp_download_temporal_denoised or gsp_download_temporal_image wrote, in host memory
 * (gsp_temporal_taa) or in caller-owned device memory of any alignment (gsp_temporal_taa_from_device: what the *_to_device calls
 * wrote).  A NULL source is the image of the newest history as it is at the call: what gsp_download_temporal_image would
 * return.  src.w is not read.
 *
 * State.  Two ping-pong planes D = {r, g, b, used}, 16 bytes per pixel each over the full frame, made by the first resolve of the
 * context and counted in gsp_stats.device_bytes.  (A source in host memory, a device source that is not 16-byte aligned and the
 * NULL source of a demodulated history pass through the filters' 16-byte output plane, made on first use like every plane.)
 * taa_valid is true exactly when the accumulate BEFORE the current one was followed by a resolve and history_valid has not been
 * cleared since; everything that clears history_valid clears taa_valid.  The context keeps the resolved gsp_display of the last
 * resolve for the two display read-outs.
 *
 * Call order.  A resolve needs a successful gsp_temporal_accumulate in the current frame with gsp_temporal_follow_instances on
 * (V is made only then: it holds, for every pixel, where the surface point was in the frame D belongs to, and the reprojection
 * is not derived a second time), at most one resolve per accumulate; otherwise GSP_ERR_INVALID.  Where the resolve sits
 * relative to gsp_temporal_antilag and the feedback calls matters only for the NULL source.  The call completes before it
 * returns and changes nothing else: the accumulate buffer, the feature planes, H, G, I, M, V, F, the primary-hit memo and
 * gsp_stats keep their bits (device_bytes grows at the first call).
 *
 * Per pixel p = (px, py):
 *  1. Tone.  T_q = steps 1-4 of "LDR film" on source pixel q with the resolved display: NaN and negative channels to 0,
 *     exposure, the tone curve, the clamp to [0, 1] with a NaN becoming 1.  Every T is finite in [0, 1].  REINHARD with a
 *     statistic left 0 measures "Frame statistics" over all width*height source pixels; a viewer should pass fixed
 *     log_avg_luminance / max_luminance, otherwise the exposure itself flickers from frame to frame.
 *  2. YCoCg.  X.y = (0.25f*r + 0.5f*g) + 0.25f*b;  X.co = 0.5f*r - 0.5f*b;  X.cg = (-0.25f*r + 0.5f*g) - 0.25f*b  of T.
 *     Back: t = y - cg;  r = t + co;  g = y + cg;  b = t - co.
 *  3. Neighbourhood box.  q = p + (dx, dy), dy = -1..1 outer and dx inner, for q inside the frame (k = y, co, cg):
 *         n += 1.0f;  s1.k += X_q.k;  s2.k += X_q.k * X_q.k
 *         m.k = s1.k / n;  v.k = max(s2.k / n - m.k * m.k, 0);  sd.k = sqrt(v.k)
 *         lo.k = m.k - sigma_clip * sd.k;  hi.k = m.k + sigma_clip * sd.k
 *  4. History.  V_p = {mx, my, sw, cls}, the motion record of this frame's accumulate.  No history when !taa_valid, cls == 0 or
 *     sw < 0.01f.  Otherwise fx = (float)px + mx;  fy = (float)py + my;  x0 = floor(fx);  wx = fx - x0, likewise for y; the
 *     four taps, their order and their weights are those of "Temporal accumulation" step 7, read from the OLDER D plane.  A
 *     tap is skipped when its weight is 0 or it lies outside the frame (no tap lies inside it unless fx is within (-1, W) and
 *     fy within (-1, H)).  Over the kept taps, in tap order:  sw2 += w;  s.k += w * D_q.k  (k = r, g, b).  sw2 < 0.01f: no
 *     history.  Otherwise h.k = s.k / sw2 and Hc = YCoCg of h.
 *  5. Without history:  D' = {rgb(X_p) clamped to [0, 1] per channel, 0}.
 *  6. With history:  c.k = Hc.k < lo.k ? lo.k : (Hc.k > hi.k ? hi.k : Hc.k);  o.k = c.k + (X_p.k - c.k) * alpha -- and, for
 *     alpha == 1, o.k = X_p.k itself: c.k + (X_p.k - c.k) may round away from X_p.k, and a frame of full weight keeps no trace
 *     of the history.  D' = {rgb(o) clamped to [0, 1] per channel (the clamp of "LDR film" step 4), 1}.
 *  7. Read-out.  The RGBA8 word is steps 5-6 of "LDR film" on D'.rgb under the stored display, A = 255.
 *
 * GSP_ERR_INVALID (text at gsp_last_error) for: no frame, or a frame begun with pixel_ids; no gsp_temporal_accumulate in this
 * frame; following off; a second resolve for the same accumulate; alpha outside [0, 1] or NaN; a negative, NaN or infinite
 * sigma_clip; whatever the gsp_display of "LDR film" is refused for; device_src non-NULL with `bytes` < width*height*16; a
 * read-out before any resolve since the history was last invalidated; NULL destinations and short sizes as in
 * gsp_download_temporal / gsp_temporal_to_device.
 *
 * Limits.  The history is fetched bilinearly, so it softens under sub-pixel motion; a sharper (Catmull-Rom) fetch is out of
 * scope.  Disocclusion is handled by V.z (the summed weight of the accumulate's kept taps) and the clamp alone.  Out of scope:
 * deforming meshes and gsp_multi_* variants, as in the rest of the temporal family.
 */
typedef struct gsp_taa {
  uint32_t struct_size; /* sizeof(gsp_taa) of the host's header; same rule as gsp_antilag (NULL and struct_size 0 = every default) */
  float alpha;          /* weight of the new frame; 0 = 0.1; otherwise (0, 1] */
  float sigma_clip;     /* half-width of the neighbourhood box in standard deviations; 0 = 1.0; otherwise > 0 and finite */
} gsp_taa;
/* The resolve of src_rgba (host memory, width*height*4 floats; NULL = the image of the newest history); complete when it returns. */
int gsp_temporal_taa(gsp_context* ctx, const gsp_taa* taa, const gsp_display* display, const float* src_rgba);
/* The same with the source in caller-owned device memory of `bytes` >= width*height*16 (any alignment); device_src NULL = the same
 * default, `bytes` then not read. */
int gsp_temporal_taa_from_device(gsp_context* ctx, const gsp_taa* taa, const gsp_display* display, const void* device_src, uint64_t bytes);
/* D' as stored: width*height*4 floats, .w = used. */
int gsp_download_taa(gsp_context* ctx, float* out_rgba);
/* The encode of D' under the display of the last resolve: width*height RGBA8 words. */
int gsp_download_taa_display(gsp_context* ctx, uint32_t* out_rgba8);
/* The same into caller-owned device memory of `bytes` >= width*height*4 (any alignment); complete when the call returns. */
int gsp_taa_display_to_device(gsp_context* ctx, void* device_dst, uint64_t bytes);

int gsp_get_stats(gsp_context* ctx, gsp_stats* out);
int gsp_reset_stats(gsp_context* ctx);

/*
 * Test hook: closest-hit / any-hit queries against the uploaded BVH.
 * rays = n * 8 floats {ox,oy,oz,tmin, dx,dy,dz,tmax}; hits = n * 4 words
 * {t (f32), u (f32), v (f32), prim (i32, -1 = miss)}.  any_hit != 0 runs the
 * shadow-ray kernel (prim = 0 when occluded, -1 when not).
 */
int gsp_trace(gsp_context* ctx, const float* rays, uint64_t n, int any_hit, void* hits);

/* Measurement hook: after renders with collect_traversal_stats = 2, how often the closest-hit rays read each node record
 * (index = position in the level-ordered node array) and tested each triangle slot.  Copies min(count, available) words,
 * then drops the counters.  It answers "which records would an LDS copy have to hold?" (DESIGN.md 4). */
int gsp_debug_visit_histograms(gsp_context* ctx, uint32_t* node_counts, uint64_t num_nodes, uint32_t* slot_counts, uint64_t num_slots);

/* Last error message of this context (or of the failed gsp_ctx_create when
 * ctx == NULL).  Never NULL. */
const char* gsp_last_error(const gsp_context* ctx);

/* ---- several GPUs of one node --------------------------------------------------------------------------------
 * Pixels are independent (the seed depends on the global pixel index and the timestamp only, raygen.rgen:37), so a
 * frame is partitioned by image tile: tile (tx, ty) of the tile x tile grid belongs to share
 * (ty * tiles_x + tx + ty) % world.  gsp_tile_partition writes the pixel ids of one share in increasing order
 * (out_ids may be NULL) and returns their number; it needs no GPU.  bench.py's one-process-per-GPU path hands these
 * lists to gsp_frame_begin; a C++ host uses the gsp_multi_* calls below, which do the same inside one process. */
uint64_t gsp_tile_partition(uint32_t width, uint32_t height, uint32_t rank, uint32_t world, uint32_t tile,
                            uint32_t* out_ids);

typedef struct gsp_multi gsp_multi;

/* One context per entry of `devices` (HIP device indices; an index may repeat: several shares on one GPU).  The
 * first device gathers.  Same error convention as gsp_ctx_create (gsp_multi_last_error(NULL) after a failure). */
int gsp_multi_create(const int* devices, int n, gsp_multi** out);
/* (ABI 5) the same with options: every share's context is created with `options` (memory_share is divided among the shares
 * of one device), options->gather_route picks the gather (GSP_GATHER_*). */
int gsp_multi_create_ex(const int* devices, int n, const gsp_ctx_options* options, gsp_multi** out);
void gsp_multi_destroy(gsp_multi* m);
int gsp_multi_num_shares(const gsp_multi* m);
/* gsp_upload_scene / gsp_frame_begin (32x32 tiles) / gsp_render / gsp_sync on every share, one host thread each. */
int gsp_multi_upload_scene(gsp_multi* m, const gsp_scene_desc* scene);
/* (ABI 5) gsp_update_camera / _instances / _tables on every share */
int gsp_multi_update_camera(gsp_multi* m, const gsp_camera* camera);
int gsp_multi_set_lens(gsp_multi* m, const gsp_lens* lens); /* gsp_set_lens on every share */
int gsp_multi_set_media(gsp_multi* m, const gsp_medium* media, uint32_t num_media); /* gsp_set_media on every share */
int gsp_multi_set_media_scattering(gsp_multi* m, const gsp_medium_scatter* scatter, uint32_t num_media); /* gsp_set_media_scattering on every share */
int gsp_multi_set_delta_lights(gsp_multi* m, const gsp_delta_light* lights, uint32_t count); /* gsp_set_delta_lights on every share */
int gsp_multi_set_envmap_sampling(gsp_multi* m, const gsp_envmap_sampling* sampling); /* gsp_set_envmap_sampling on every share */
int gsp_multi_set_light_grid(gsp_multi* m, const gsp_light_grid* grid); /* gsp_set_light_grid on every share */
int gsp_multi_set_light_sampling(gsp_multi* m, uint32_t mode); /* gsp_set_light_sampling on every share */
int gsp_multi_set_estimator(gsp_multi* m, uint32_t mode);      /* gsp_set_estimator on every share */
int gsp_multi_update_instances(gsp_multi* m, const gsp_instance* instances, uint32_t num_instances);
int gsp_multi_update_tables(gsp_multi* m, const gsp_scene_desc* scene);
int gsp_multi_frame_begin(gsp_multi* m, uint32_t width, uint32_t height);
int gsp_multi_render(gsp_multi* m, const gsp_render_params* params);
int gsp_multi_sync(gsp_multi* m);
/* The one exchange of a render: completes the queued samples, brings every share's HDR tiles into devices[0] and
 * assembles the frame there.  With one share per device the gather is ONE RCCL group over xGMI (every share
 * ncclSend()s its tiles, devices[0] ncclRecv()s them); a device list with repeats (several shares on one GPU, for
 * tests) uses peer copies instead -- RCCL wants one rank per device -- and so does a node on which librccl cannot be
 * loaded or the communicator does not come up (GSP_GATHER_AUTO; the reason is kept in gsp_multi_last_error).
 * gsp_ctx_options.gather_route forces a route (GSP_GATHER_RCCL with ONE share performs a self send / recv: the RCCL smoke
 * test of a one-GPU box).
 * *device_frame (optional) = the RGBA32F frame on devices[0] (NULL for a single share without RCCL, whose frame is its
 * context's accumulate buffer). */
int gsp_multi_gather(gsp_multi* m, void** device_frame);
/* 1: the gathers of `m` go through RCCL, 0: through peer copies (-1: m is NULL).  The optional outputs receive the
 * number of gathers each route has carried so far. */
int gsp_multi_gather_route(const gsp_multi* m, uint64_t* rccl_gathers, uint64_t* copy_gathers);
/* gsp_multi_gather + one copy to the host: width*height*4 floats, identical to a single-GPU gsp_download. */
int gsp_multi_download(gsp_multi* m, float* out_rgba);
/* gsp_multi_gather + the LDR film on the gathered frame (statistics over the whole frame) + one copy to the host: width*height
 * words, identical to a single-GPU gsp_download_display. */
int gsp_multi_download_display(gsp_multi* m, const gsp_display* display, uint32_t* out_rgba8);
/* Feature buffers over the shares: gsp_render_features on every share (its gsp_tile_partition pixels); the download gathers the
 * three planes into devices[0] with peer copies (also where the beauty gather goes through RCCL), assembles them there and
 * copies them to the host: identical to a single-GPU gsp_download_features.  Any pointer may be NULL. */
int gsp_multi_render_features(gsp_multi* m, const gsp_render_params* params);
int gsp_multi_download_features(gsp_multi* m, float* albedo, float* geom, uint32_t* ids);
/* The denoiser on the gathered frame: gsp_multi_gather, the albedo and geom planes of every share brought to devices[0] (into two
 * frame buffers of the denoiser's own, made on first use), the same kernels there, one copy to the host: identical to a single-GPU
 * gsp_download_denoised.  Every share must have had gsp_multi_render_features since gsp_multi_frame_begin. */
int gsp_multi_download_denoised(gsp_multi* m, const gsp_denoise* denoise, float* out_rgba);
/* total (optional): counters summed over the shares, times of the slowest share (they run concurrently);
 * per_share (optional): gsp_multi_num_shares() records. */
int gsp_multi_get_stats(gsp_multi* m, gsp_stats* total, gsp_stats* per_share);
int gsp_multi_reset_stats(gsp_multi* m);
const char* gsp_multi_last_error(const gsp_multi* m);

#ifdef __cplusplus
}
#endif
#endif /* GPUSPECTRAL_PT_H */
