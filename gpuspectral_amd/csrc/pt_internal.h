// pt_internal.h -- declarations shared by the HIP translation units of
// libgpuspectral_pt.so (not part of the public ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/gpuspectral_pt.h"
#include "pt_antilag.h"
#include "pt_denoise.h"
#include "pt_display.h"
#include "pt_illum.h"
#include "pt_stages.h"
#include "pt_motion.h"
#include "pt_svgf.h"
#include "pt_taa.h"
#include "pt_temporal.h"

namespace gsp {

// GSP_ESTIMATOR_TEXTBOOK: the <EST = true> instantiations of k_shade / k_finish are compiled in a translation unit of their own
// (pt_render_textbook.hip; the library's two large units then build side by side) and launched through these two entries.  The
// queues travel as plain pointers: the queue records of pt_render_kernels.inc are types of an unnamed namespace.  TEX / VER / LSEL
// and media != nullptr (MED) pick the instantiation as tex_ver_med_kernel (pt_render_pipeline.inc) does for the reference mode.
struct TextbookLaunch {
  bool tex, ver, lsel;
  const gsp_medium* media;  // nullptr: the context holds no media
  const SceneView* view;    // the view the reference-mode launch would take (the versioned one when ver)
  const RenderConstsBase* rc;
  hipStream_t stream;
  uint32_t blocks;
  const uint32_t* n_ptr;  // k_shade: the queue's size on the device;  k_finish: n
  uint32_t n;
  q4* cur[4];
  const q4* hits;  // k_shade
  q4* next[4];     // k_shade
  q4* shadow[3];   // k_shade
  q4* result;
  uint32_t* tails;
  uint32_t* live;
  uint32_t slot_paths, chunk;  // (chunk: k_shade)
  void* stats;                 // DevStats*
};
void launch_shade_textbook(const TextbookLaunch& a);
void launch_finish_textbook(const TextbookLaunch& a);
// Scattering media: the <MED = true, SCT = true> instantiations of both kernels, over TEX x VER x LSEL x EST, live in
// pt_render_scatter.hip and take the same record + the scattering table and the estimator flag.  media and scatter are never null here.
struct ScatterLaunch : TextbookLaunch {
  const gsp_medium_scatter* scatter;
  bool est;
};
void launch_shade_scatter(const ScatterLaunch& a);
void launch_finish_scatter(const ScatterLaunch& a);
// Delta lights: the <DLT = true> instantiations, over TEX x VER x LSEL x EST with MED = SCT = true, live in pt_render_delta.hip.  A
// context without media hands null tables (no handle carries a medium number then: the media lines never run), one whose media
// only absorb a scattering table of zeros (such a medium takes the deterministic line).  The view's num_lights counts both kinds.
struct DeltaLaunch : ScatterLaunch {
  uint32_t num_tri_lights;
};
void launch_shade_delta(const DeltaLaunch& a);
void launch_finish_delta(const DeltaLaunch& a);
// Environment light: the <ENV = true> instantiations, over VER x LSEL with TEX = MED = EST = SCT = DLT = true, live in
// pt_render_envlight.hip.  The delta record as it stands (a context without textures still holds an envmap: TEX; no delta lights:
// num_tri_lights == the records in front of the environment record) + the cell table
struct EnvLaunch : DeltaLaunch {
  const gsp_light_pick* env_cells;
};
void launch_shade_envlight(const EnvLaunch& a);
void launch_finish_envlight(const EnvLaunch& a);
// Light grid: the <GRD = true> instantiations, over VER with TEX = MED = LSEL = EST = SCT = DLT = true and ENV = false, live in
// pt_render_lightgrid.hip.  The delta record as it stands (no textures: an empty texture view; no delta lights: num_tri_lights ==
// num_lights) + where the grid sits inside a table version.  The view's tables_bytes ends in front of the grid
struct GridLaunch : DeltaLaunch {
  uint32_t grid_off;
};
void launch_shade_lightgrid(const GridLaunch& a);
void launch_finish_lightgrid(const GridLaunch& a);

#define GSP_HIP_TRY(expr)                                                                     \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      err = std::string(#expr) + ": " + hipGetErrorString(e_) + " (" __FILE__ ":" + std::to_string(__LINE__) + ")"; \
      return e_ == hipErrorOutOfMemory ? GSP_ERR_NOMEM : GSP_ERR_DEVICE;                      \
    }                                                                                         \
  } while (0)

// 16-byte quads per triangle slot of the intersection and the shading array (a node record: kNodeQuads, pt_trace.h)
constexpr uint32_t kIsectQuads = 3u, kShadeQuads = 4u;

// scratch of refit_bvh, allocated by the first refit of a tree and kept with it (a per-frame call: seven hipMalloc / hipFree
// pairs cost more than the kernels): padded triangle boxes by slot, node boxes, per-node areas, reduction space
struct RefitScratch {
  q4 *leaf_lo = nullptr, *leaf_hi = nullptr, *box_lo = nullptr, *box_hi = nullptr;
  double *area = nullptr, *total = nullptr;
  void* tmp = nullptr;
  size_t tmp_bytes = 0;
  uint32_t* bounds = nullptr;  // allocated last: non-null marks the set complete
  void release() {
    for (void* p : {(void*)leaf_lo, (void*)leaf_hi, (void*)box_lo, (void*)box_hi, (void*)area, (void*)total, tmp, (void*)bounds}) (void)hipFree(p);
    *this = RefitScratch{};
  }
};

// Result of the device BVH build; all pointers are device memory owned by the caller's context.
struct DeviceBvh {
  q4* nodes = nullptr;      // wide BVH, kNodeQuads quads per node (pt_trace.h); node 0 is the root
  q4* tri_isect = nullptr;  // kIsectQuads quads per slot
  q4* tri_shade = nullptr;  // kShadeQuads quads per slot
  uint32_t* slot_to_global = nullptr;
  bool arrays_external = false;  // nodes / tri_isect / tri_shade are a slot of the context's geometry ring (pt_render.hip): not free_bvh's
  int32_t root = 0;
  uint32_t num_tris = 0;   // real triangles (0 allowed)
  uint32_t first_slot = 0; // triangle slots in use: [first_slot, first_slot + num_tris); the leading ones are all-zero triangles
  uint32_t num_nodes = 0;
  uint32_t depth = 0;      // levels of the wide tree (bounds the traversal stack: <= 1 node group per level)
  size_t bytes = 0;
  // refit (refit_bvh): the tree is stored level by level -- level l = nodes [level_first[l], level_first[l + 1]) -- so the
  // boxes can be recomputed bottom-up, one launch per level, without parent links
  std::vector<uint32_t> level_first;
  double area_built = 0.0;  // sum of the child-box surface areas right after the last full build (0 = not measured yet)
  uint32_t refits = 0;      // refits since that build
  RefitScratch rf;
  // the three arrays a tree owns go (free_bvh; pt_render_scene.inc when they move into the geometry ring): not for arrays_external
  void free_tree_arrays() {
    (void)hipFree(nodes);
    (void)hipFree(tri_isect);
    (void)hipFree(tri_shade);
    nodes = tri_isect = tri_shade = nullptr;
  }
};
// triangle slots a tree's intersection / shading arrays hold: first_slot leading all-zero slots (build_bvh), the triangles, and
// the kWide - 1 all-zero slots behind them that a wide leaf may read
inline uint64_t tree_slots(uint64_t num_tris, uint32_t first_slot) { return num_tris + first_slot + (kWide - 1); }
inline uint64_t tree_slots(const DeviceBvh& t) { return tree_slots(t.num_tris, t.first_slot); }

struct BuildInput {
  const gsp_instance* instances;  // device
  const float* inv_t;             // device, 16 floats per instance: inverse(transpose(M))
  const uint32_t* tri_first;      // device, num_instances + 1 prefix of triangle counts
  uint32_t num_instances;
  const float* positions;  // device, object space
  const float* normals;    // device
  uint32_t num_tris;
  const uint32_t* tri_id_first = nullptr;  // device, per instance: the scene-wide index of its first triangle when `instances` is a
                                           // SUBSET of the scene's (the closest-hit tie-break key must order like the scene's
                                           // triangle list across both trees of a split scene); nullptr = tri_first
  int reinsert_rounds = -1;  // parallel-reinsertion rounds of the build, < 0 = the default (gsp_ctx_options.reinsert_rounds - 1)
};

// ---- internal entry points of a context for pt_multi.hip (same library, not exported) ------------------------------
// Completes everything queued and returns the context's compact RGBA32F accumulate buffer (device memory on the
// context's device, num_pixels records) and the stream its copies are ordered on.
__attribute__((visibility("hidden"))) int gsp_internal_accum(gsp_context* ctx, void** accum, uint64_t* num_pixels, hipStream_t* stream);
// ... and its three compact feature planes (gsp_render_features), 16 bytes per owned pixel each
__attribute__((visibility("hidden"))) int gsp_internal_features(gsp_context* ctx, void** albedo, void** geom, void** ids, uint64_t* num_pixels);
// ... and whether gsp_render_features has run on it since its gsp_frame_begin (1 / 0; the denoiser refuses planes nobody rendered)
__attribute__((visibility("hidden"))) int gsp_internal_features_rendered(const gsp_context* ctx);
// The options a context was created with, defaults filled in (pt_multi.hip divides memory_share among the shares of a device).
__attribute__((visibility("hidden"))) void gsp_internal_resolve_options(const gsp_ctx_options* in, gsp_ctx_options* out);

// ---- LDR film (pt_display.h) on `n` RGBA32F records at `src`, device memory of the current device; both queue on `stream` ----
// display_measure: the frame statistics through the 24-byte device record `d_rec` and its pinned host mirror `h_rec`;
// synchronises the stream.  display_map: `n` RGBA8 words into `dst` (device, 16-byte aligned); does not synchronise.
__attribute__((visibility("hidden"))) hipError_t display_measure(hipStream_t stream, uint32_t num_cus, const void* src, uint64_t n, DisplayStatsRec* d_rec,
                                                                 DisplayStatsRec* h_rec, gsp_luminance* out);
__attribute__((visibility("hidden"))) hipError_t display_map(hipStream_t stream, uint32_t num_cus, const void* src, uint64_t n, const DisplayConsts& k, uint32_t* dst);

// ---- denoiser (pt_denoise.h) on a full frame of width x height: `accum`, `albedo`, `geom` are its RGBA32F planes, `e0`, `e1`, `a`
// scratch planes and `out` the result, all 16 bytes per pixel, 16-byte aligned device memory of the current device.  Queues
// k_denoise_prepare and k.iterations launches of k_denoise_atrous on `stream`; does not synchronise.  illum: `accum` is a
// demodulated history (pt_illum.h) and k_illum_prepare stands for k_denoise_prepare.
__attribute__((visibility("hidden"))) hipError_t denoise_run(hipStream_t stream, uint32_t num_cus, const void* accum, const void* albedo, const void* geom,
                                                             uint32_t width, uint32_t height, const DenoiseConsts& k, void* e0, void* e1, void* a, void* out,
                                                             bool illum = false);

// Bakes the instances' triangles to world space and builds the wide BVH (PLOC + reinsertion + collapse) on `stream`.
// Returns GSP_OK or an error code with `err` set.
int build_bvh(hipStream_t stream, const BuildInput& in, DeviceBvh& out, std::string& err);
// The instances of `in` have changed (transforms, materials, emission) but not the triangle list: re-bakes every triangle
// packet into its slot and recomputes all node boxes, child orders included, bottom-up in the existing topology.  Results of a
// trace do not depend on the topology (closest-hit rule, pt_trace.h), its speed does: *growth = summed child-box area after /
// right after the last full build; the caller rebuilds when that exceeds its bound.  Synchronises the stream.
int refit_bvh(hipStream_t stream, const BuildInput& in, DeviceBvh& bvh, double* growth, std::string& err);
void free_bvh(DeviceBvh& b);

}  // namespace gsp
