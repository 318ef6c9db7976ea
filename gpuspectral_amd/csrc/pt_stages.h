// pt_stages.h -- per-path bodies of the wavefront stages.
//
//   generate : raygen.rgen:29-48          camera ray + RNG seed + payload init
//   shade    : rayhit.rchit:666-797       one shading vertex (closest-hit shader)
//              raygen.rgen:59-80          firefly clamp, Russian roulette, depth logic
//   connect  : rayhit.rchit:737-757       shadow-ray verdict -> NEE contribution, MIS weight
//   resolve  : raygen.rgen:84-108         running-mean accumulate
//
// The reference runs these as one recursive shader invocation per pixel; here
// they are separate passes over ray queues in HBM.  The state a path carries
// between passes is the reference's HitPayload (pt_common.glsl:4-14).
//
// Sample sum order: the reference adds `prd.emitted` (NEE term first, emission
// term second, rayhit.rchit:752,763-768) to `result` once per bounce behind the
// firefly test (raygen.rgen:60-63).  The NEE term needs the shadow ray, so the
// shade pass hands both terms to the connect pass, which forms the same sum.
#pragma once
#include "pt_deltalight.h"
#include "pt_envlight.h"
#include "pt_lightgrid.h"
#include "pt_medium.h"
#include "pt_shading.h"
#include "pt_trace.h"

namespace gsp {

// The per-instance shading data of RenderState::Instance (emission, bsdf, twofaced; PathTracer.h:27-34) is baked
// into the w components of every triangle's shading packet: one dependent fetch less per shaded vertex.
GSP_HD uint32_t pack_material(uint32_t bsdf, uint32_t twofaced) {
  return (bsdf & 0x7fffffffu) | (twofaced == 1u ? 0x80000000u : 0u);
}

// What every stage reads.  k_shade, k_finish and the unfiltered k_generate take this struct: its size is part of their kernel
// argument layout, and so of their instruction streams (the committed counter files belong to those, profiles/pmc_bench_*.json).
struct RenderConstsBase {
  uint32_t width, height;
  uint32_t max_depth, rr_start_depth;
  float clamp;
  uint32_t nee;        // RenderParams.nee (PathTracer.h:36-41); the shipped shader hard-wires 1 (`#define NEE true`, rchit:656)
  float zplane;        // (max(W,H)/2) / tan(fov/2), raygen.rgen:22 (tan evaluated on the host)
  float cam_origin[3]; // camera.eye = toWorld[3]
  float cam_to_world[16];
};

// ... plus what only the generation of a FILTERED sample reads (k_generate_filtered, k_generate_active_filtered, generate_path):
// the pixel filter (include/gpuspectral_pt.h, "Pixel filter"): GSP_FILTER_* and the RESOLVED parameter (tent radius / Gaussian
// standard deviation, never 0 for those two).  0 = the reference as shipped: the ray through the integer pixel coordinate
struct RenderConsts : RenderConstsBase {
  uint32_t pixel_filter = 0;
  float pixel_filter_param = 0.0f;
};

// ... plus what only the generation of a sample through a THIN LENS reads (k_generate_lens, k_generate_active_lens): the lens
// of include/gpuspectral_pt.h, "Thin lens", resolved on the host.  lens_radius == 0 = the pinhole: never handed to those kernels
struct RenderConstsLens : RenderConsts {
  float lens_radius = 0.0f;
  float lens_focus = 0.0f;     // gsp_lens.focus_distance
  float lens_s = 0.0f;         // focus_distance / zplane, formed once on the host like zplane
  uint32_t lens_blades = 0;    // 0 = circle, 3..16 = polygon
  float lens_rotation = 0.0f;  // radians
};

// (host) the lens of a context into the constants; zplane must be set.  s is formed here, once, like zplane
inline void set_lens_consts(RenderConstsLens& rc, const gsp_lens& lens) {
  if (!(lens.radius > 0.0f)) return;  // pinhole: the fields stay 0 whatever the lens holds
  rc.lens_radius = lens.radius;
  rc.lens_focus = lens.focus_distance;
  rc.lens_s = lens.focus_distance / rc.zplane;
  rc.lens_blades = lens.blades;
  rc.lens_rotation = lens.rotation;
}

struct SceneView {
  const q4* nodes;
  const q4* tri_isect;  // 3 quads per slot
  const q4* tri_shade;  // 4 quads per slot: {N, bits(bsdf | twofaced << 31)}, {n0, emission.r}, {n1, .g}, {n2, .b}
  BsdfTables bsdf;
  const gsp_triangle_light* lights;  // baked records (pt_shading.h bake_light), as is the diffuse table (bake_diffuse)
  uint32_t num_lights;
  float inv_num_lights = 0.0f;       // 1.0f / (float)num_lights (rayhit.rchit:151), formed once on the host
  uint32_t static_slots = 0;        // <VER = true>, split scene: triangle slots (and 64-B node records) of the STATIC tree that sits in front
                                    // of the geometry ring -- slots below it are the same in every version; 0 = the ring holds whole trees
  uint32_t geo = 0;                 // <VER = true>: geometry ring (below): phys slot that stamp 0 stands for << 29 | triangle slots per version
  const uint8_t* tables = nullptr;  // the BSDF tables + lights back to back (device: one allocation), for LDS staging
  uint32_t tables_bytes = 0;
  uint32_t ver_stride = 0;          // <VER = true> instantiations: bytes between two versions of the tables (slot 0 is what the pointers name)
  TextureView tex;                  // dormant-feature extension; read only by the <TEX = true> instantiations
};
// ... and what the <MED = true> instantiations of k_shade / k_finish take in its place: the view + the table of interior media
// (gsp_set_media).  A struct of its own, not a field of SceneView: the size of SceneView is part of the kernel argument layout of
// every kernel that takes it, and so of the instruction streams the committed counter files belong to (profiles/pmc_bench_*.json)
struct SceneViewMed : SceneView {
  const gsp_medium* media = nullptr;
};
// ... and the <MED = true, SCT = true> ones: + the table of scattering coefficients parallel to it (gsp_set_media_scattering)
struct SceneViewSct : SceneViewMed {
  const gsp_medium_scatter* scatter = nullptr;
};
// ... and the <DLT = true> ones (gsp_set_delta_lights): + the number of TRIANGLE lights in front of the delta records of the light
// table (num_lights counts both).  They are built for MED = SCT = false and MED = SCT = true only and take this one view
struct SceneViewDlt : SceneViewSct {
  uint32_t num_tri_lights = 0;
};
// ... and the <ENV = true> ones (gsp_set_envmap_sampling with an envmap resident): + the cell table of the environment light
// (pt_envlight.h), scene state beside the table versions.  The record that names its size is the LAST of the light table
struct SceneViewEnv : SceneViewDlt {
  const gsp_light_pick* env_cells = nullptr;
};
// ... and the <GRD = true> ones (gsp_set_light_grid with a grid resident): + the byte offset of the light grid (pt_lightgrid.h)
// inside a table version, counted from SceneView::tables.  The grid is read from there, NEVER from the LDS copy: tables_bytes of
// such a view names only the bytes in front of the grid
struct SceneViewGrd : SceneViewDlt {
  uint32_t grid_off = 0;
};
template <bool MED, bool SCT = false, bool DLT = false, bool ENV = false, bool GRD = false>
struct ShadeViewOf {
  using type = SceneView;
};
template <bool MED, bool SCT>
struct ShadeViewOf<MED, SCT, true, false, false> {
  using type = SceneViewDlt;
};
template <bool MED, bool SCT>
struct ShadeViewOf<MED, SCT, true, true, false> {
  using type = SceneViewEnv;
};
template <bool MED, bool SCT>
struct ShadeViewOf<MED, SCT, true, false, true> {
  using type = SceneViewGrd;
};
template <>
struct ShadeViewOf<true, false, false, false, false> {
  using type = SceneViewMed;
};
template <>
struct ShadeViewOf<true, true, false, false, false> {
  using type = SceneViewSct;
};
GSP_HD const gsp_medium* view_media(const SceneView&) { return nullptr; }
GSP_HD const gsp_medium* view_media(const SceneViewMed& v) { return v.media; }
GSP_HD const gsp_medium_scatter* view_scatter(const SceneView&) { return nullptr; }
GSP_HD const gsp_medium_scatter* view_scatter(const SceneViewSct& v) { return v.scatter; }
GSP_HD uint32_t view_tri_lights(const SceneView&) { return 0u; }
GSP_HD uint32_t view_tri_lights(const SceneViewDlt& v) { return v.num_tri_lights; }
GSP_HD const gsp_light_pick* view_env_cells(const SceneView&) { return nullptr; }
GSP_HD const gsp_light_pick* view_env_cells(const SceneViewEnv& v) { return v.env_cells; }
GSP_HD uint32_t view_grid_off(const SceneView&) { return 0u; }
GSP_HD uint32_t view_grid_off(const SceneViewGrd& v) { return v.grid_off; }

// path flags word: depth [0,7] | wasDelta << 8 | countEmitted << 9 | table version << 10 [10,15] | geometry version << 16 [16,21]
GSP_HD uint32_t pack_flags(uint32_t depth, uint32_t wasDelta, uint32_t countEmitted) {
  return depth | (wasDelta << 8) | (countEmitted << 9);
}
// r05: a path carries the VERSION of the BSDF / light tables it was generated under (gsp_update_tables without a drain: the
// samples in flight finish on the tables they started with, new samples read the new ones; the versions live in a ring of
// kTableVersions slots, SceneView::ver_stride bytes apart).  Stamped by k_generate, handed on by shade_vertex<VER = true>.
// While every sample in flight belongs to ONE version -- always, for a scene that is not being edited -- that version sits in
// slot 0, the field is 0 and the <VER = false> kernels neither read nor write it: their code is what it was before versions existed.
constexpr uint32_t kVerShift = 10, kTableVersions = 64, kVerMask = (kTableVersions - 1u) << kVerShift;
// ... and the version of the GEOMETRY (gsp_update_instances without a drain: bits [16,21]): the node records, intersection
// triangles and shading packets of up to kGeoVersions edits live in a ring of G = 2^g slots -- version slot p at nodes + p * stride
// * 64 B (a tree of n triangles has fewer than n nodes), tri_isect + 3 * p * stride, tri_shade + 4 * p * stride quads, stride =
// triangle slots per version -- and a path's stamp s names slot (s + base) % G, base = the slot of the one live version the last
// time only one was (then the field is 0, as for the tables).  A path of 52 bounces lives 52 iterations -- 52 frames of a viewer
// that renders one sample per frame -- so the ring is as long as the tables' when memory and the 32-bit node offsets allow
// (G * stride * 64 B < 4 GB: 64 versions up to a million triangles, 8 up to eight million).  g, base and stride travel in one
// word (SceneView::geo / GeoRing).
constexpr uint32_t kGeoShift = 16, kGeoVersions = 64, kGeoMask = (kGeoVersions - 1u) << kGeoShift;
constexpr uint32_t kStampMask = kVerMask | kGeoMask;
constexpr uint32_t kGeoStrideBits = 23, kGeoStrideMask = (1u << kGeoStrideBits) - 1u;  // stride | base << 23 | g << 29
constexpr uint32_t kGeoMaxStride = kGeoStrideMask;
GSP_HD uint32_t pack_geo(uint32_t base, uint32_t stride, uint32_t log2_versions) {
  return stride | (base << kGeoStrideBits) | (log2_versions << 29);
}
// slot offset (in triangle slots) of the geometry version a stamp names
GSP_HD uint32_t geo_slot_offset(uint32_t geo, uint32_t stamp) {
  const uint32_t mask = (1u << (geo >> 29)) - 1u;
  return ((stamp + ((geo >> kGeoStrideBits) & (kGeoVersions - 1u))) & mask) * (geo & kGeoStrideMask);
}
GSP_HD uint32_t geo_stamp(uint32_t flags) { return (flags & kGeoMask) >> kGeoShift; }

struct PathState {
  f3 o, d;
  f3 weight;
  float directWeight;
  uint32_t seed;
  uint32_t flags;
  uint32_t sid;  // sample slot: k * num_pixels + local pixel
};

struct ShadowRay {
  f3 o, d;
  float tmax;     // Ldist - 0.01 (tmin is the literal 0.01)
  f3 nee;         // contribution if unoccluded
  f3 emis;        // emission term of the same vertex
  float dw_nee;   // directWeight of the continuing path if NEE happens
  uint32_t sid;
  int32_t next;   // index of the continuing path in the next queue, -1 if the path ended here
};

// Sub-pixel offset of one sample, drawn from the pixel filter's own density (filter importance sampling: the sample then counts
// with weight 1 in its own pixel).  The formulas are fixed in include/gpuspectral_pt.h; log / sin / cos are the deterministic
// ones of pt_math.h, so host and device agree bit for bit.  Always two draws: the streams of all filters coincide afterwards.
GSP_HD void filter_offset(uint32_t filter, float param, uint32_t& rng, float& ox, float& oy) {
  const float u1 = rand_uniform(rng);
  const float u2 = rand_uniform(rng);
  if (filter == 2u) {  // GSP_FILTER_TENT: inverse CDF of the tent on [-1, 1], scaled by the radius
    const float t1 = u1 < 0.5f ? gsqrt(2.0f * u1) - 1.0f : 1.0f - gsqrt(2.0f - 2.0f * u1);
    const float t2 = u2 < 0.5f ? gsqrt(2.0f * u2) - 1.0f : 1.0f - gsqrt(2.0f - 2.0f * u2);
    ox = 0.5f + param * t1;
    oy = 0.5f + param * t2;
  } else if (filter == 3u) {  // GSP_FILTER_GAUSSIAN: Box-Muller, radius cut at 4 sigma
    const float rho = gmin(param * gsqrt(-2.0f * det_logf(gmax(1.0f - u1, 2.3283064365386962890625e-10f))), 4.0f * param);
    float sn, cs;
    det_sincosf((2.0f * kPi) * u2, sn, cs);
    ox = 0.5f + rho * cs;
    oy = 0.5f + rho * sn;
  } else {  // GSP_FILTER_BOX: the reference's dormant line, raygen.rgen:38
    ox = u1;
    oy = u2;
  }
}

// rayDir(size, fragCoord, fov) + the camera transform + the y flip, raygen.rgen:20-25,41-45
GSP_HD f3 camera_dir(const RenderConstsBase& rc, float fx, float fy) {
  const float x = fx - (float)rc.width / 2.0f;
  const float y = fy - (float)rc.height / 2.0f;
  f3 dl = normalize(mk3(-x, y, rc.zplane));
  f3 dir = xform_dir(rc.cam_to_world, dl);
  dir.y = dir.y * -1.0f;
  return dir;
}

// Point on the aperture, uniform over it, in camera space (include/gpuspectral_pt.h, "Thin lens").  Always two draws.
// Circle: the concentric map of sample_cosine_hemisphere (pt_shading.h, rayhit.rchit:89-111), operation for operation, times the
// radius.  Polygon: u3 picks the triangle (centre, v_k, v_k+1) and, stretched, the square-root coordinate inside it.
GSP_HD void lens_vertex(float radius, uint32_t blades, float rotation, uint32_t j, float& vx, float& vy) {
  float sn, cs;
  det_sincosf(rotation + ((2.0f * kPi) * (float)j) / (float)blades, sn, cs);
  vx = radius * cs;
  vy = radius * sn;
}
GSP_HD void lens_point(float radius, uint32_t blades, float rotation, uint32_t& rng, float& lx, float& ly) {
  const float u3 = rand_uniform(rng);
  const float u4 = rand_uniform(rng);
  if (blades == 0u) {
    const float ux = 2.0f * u3 - 1.0f;
    const float uy = 2.0f * u4 - 1.0f;
    float dx = 0.0f, dy = 0.0f;
    if (!(ux == 0.0f && uy == 0.0f)) {
      float r, th;
      if (gabs(ux) > gabs(uy)) {
        r = ux;
        th = (kPi / 4.0f) * (uy / ux);
      } else {
        r = uy;
        th = kPi / 2.0f - (kPi / 4.0f) * (ux / uy);
      }
      float s, c;
      det_sincosf(th, s, c);
      dx = r * c;
      dy = r * s;
    }
    lx = dx * radius;
    ly = dy * radius;
  } else {
    const float t = u3 * (float)blades;
    const uint32_t k = (uint32_t)t < blades - 1u ? (uint32_t)t : blades - 1u;
    const float a = gsqrt(t - (float)k);
    const float b = u4;
    float x0, y0, x1, y1;
    lens_vertex(radius, blades, rotation, k, x0, y0);
    lens_vertex(radius, blades, rotation, k + 1u == blades ? 0u : k + 1u, x1, y1);  // (vertex n is vertex 0: the polygon closes exactly)
    lx = a * ((1.0f - b) * x0 + b * x1);
    ly = a * ((1.0f - b) * y0 + b * y1);
  }
}

// The camera ray of fragCoord (fx, fy) through the lens point l = (lx, ly, 0): towards the point where the pinhole ray of that
// fragCoord crosses the plane of focus.  Offset and direction go through the same linear map (xform_dir, then the y flip)
GSP_HD void camera_ray_lens(const RenderConstsLens& rc, float fx, float fy, float lx, float ly, f3& o, f3& d) {
  const float x = fx - (float)rc.width / 2.0f;
  const float y = fy - (float)rc.height / 2.0f;
  const f3 pf = mk3(-x * rc.lens_s, y * rc.lens_s, rc.lens_focus);
  const f3 l = mk3(lx, ly, 0.0f);
  f3 dir = xform_dir(rc.cam_to_world, normalize(pf - l));
  dir.y = dir.y * -1.0f;
  f3 off = xform_dir(rc.cam_to_world, l);
  off.y = off.y * -1.0f;
  o = mk3(rc.cam_origin[0], rc.cam_origin[1], rc.cam_origin[2]) + off;
  d = dir;
}

// raygen.rgen:31-48.  FILTER = false is the reference as shipped (the jitter of raygen.rgen:38 commented out), instruction
// for instruction what it was before pixel filters existed; FILTER = true draws the offset at the position of that line.
// LENS = true (RC = RenderConstsLens, radius > 0): the lens point is drawn right behind the filter's two variates and the ray
// leaves from it; LENS = false is the pinhole, instruction for instruction what it was before the lens existed.
template <bool FILTER, bool LENS = false, class RC>
GSP_HD void generate_path_t(const RC& rc, uint32_t gid, uint32_t timestamp, uint32_t sid, PathState& p) {
  const uint32_t px = gid % rc.width, py = gid / rc.width;
  uint32_t rng = pcg_hash(tea(rc.width * py + px, timestamp));
  float fx = (float)px, fy = (float)py;  // fragCoord
  if constexpr (FILTER) {
    float ox, oy;
    filter_offset(rc.pixel_filter, rc.pixel_filter_param, rng, ox, oy);
    fx = fx + ox;
    fy = fy + oy;
  }
  if constexpr (LENS) {
    float lx, ly;
    lens_point(rc.lens_radius, rc.lens_blades, rc.lens_rotation, rng, lx, ly);
    camera_ray_lens(rc, fx, fy, lx, ly, p.o, p.d);
  } else {
    p.o = mk3(rc.cam_origin[0], rc.cam_origin[1], rc.cam_origin[2]);
    p.d = camera_dir(rc, fx, fy);
  }
  p.weight = splat(1.0f);
  p.directWeight = 1.0f;
  p.seed = rng;
  p.flags = pack_flags(0, 0, 1);
  p.sid = sid;
}
GSP_HD void generate_path(const RenderConsts& rc, uint32_t gid, uint32_t timestamp, uint32_t sid, PathState& p) {
  if (rc.pixel_filter != 0u) generate_path_t<true>(rc, gid, timestamp, sid, p);
  else generate_path_t<false>(rc, gid, timestamp, sid, p);
}
// ... through a lens of radius > 0 (the filter by the same runtime branch), and the entry that takes either camera
GSP_HD void generate_path_lens(const RenderConstsLens& rc, uint32_t gid, uint32_t timestamp, uint32_t sid, PathState& p) {
  if (rc.pixel_filter != 0u) generate_path_t<true, true>(rc, gid, timestamp, sid, p);
  else generate_path_t<false, true>(rc, gid, timestamp, sid, p);
}
GSP_HD void generate_path(const RenderConstsLens& rc, uint32_t gid, uint32_t timestamp, uint32_t sid, PathState& p) {
  if (rc.lens_radius > 0.0f) generate_path_lens(rc, gid, timestamp, sid, p);
  else generate_path(static_cast<const RenderConsts&>(rc), gid, timestamp, sid, p);
}

// firefly test + add, raygen.rgen:60-63
GSP_HD void add_emitted(float clampv, f3 e, q4& result) {
  if (e.x < clampv && e.y < clampv && e.z < clampv) {
    result.x = result.x + e.x;
    result.y = result.y + e.y;
    result.z = result.z + e.z;
  }
}

struct ShadeOut {
  bool alive;        // path continues: `next` is valid
  PathState next;
  bool has_shadow;   // a shadow ray must be traced: `shadow` is valid (sid/next filled by the caller)
  ShadowRay shadow;
  f3 emitted;        // when !has_shadow: prd.emitted of this bounce (emission term only)
};

// TEX: the scene carries textures (include/gpuspectral_pt.h, dormant-feature extension).  The reference's shader
// passes uv = vec2(0) and never reads a texture (rayhit.rchit:716,729): TEX = false is that code, instruction for
// instruction; TEX = true interpolates the hit's uv and, for a record with has_texture, takes kD from the texture.
// VER: tables of several versions are live (an edit through gsp_update_tables while samples were in flight): the vertex reads
// the version its path carries.  VER = false is the code of a scene that is not being edited, instruction for instruction.
// MED: the context holds interior media (include/gpuspectral_pt.h, "Interior media"): bits 19..30 of the material word name the
// medium of the hit object, and a vertex on a BACK face scales the path weight by exp(-sigma_a * t) of the segment that ran inside
// it.  MED = false is the code of a context without media, instruction for instruction (no handle carries those bits then);
// `media` (MED only) = the table, view_media() of the view the kernel was handed.
// LSEL: the context picks its light by emitted power (include/gpuspectral_pt.h, "Light selection"): sample_light_power reads the
// alias table that sits straight behind the light records of this vertex's version of the tables (LDS or global, wherever the
// lights are).  LSEL = false is the reference's uniform pick, instruction for instruction.
// EST: the context runs the textbook estimator (include/gpuspectral_pt.h, "Estimator"): the NEE weight takes the BSDF's pdf of L
// itself, rough plastic's eval pdf loses its floor, and an emitter met with NEE on, countEmitted == 0 and wasDelta == 0 is weighted
// with power_heuristic(lastPdf, hitPdf), hitPdf = light sampling's pdf of reaching THIS point of THIS emitter.  The path's
// directWeight field is dead in this mode and carries lastPdf, the bs.pdf of the vertex that sent the ray (the same for both
// verdicts of its shadow ray).  EST = false is the reference's estimator, instruction for instruction.
// SCT (only with MED): some medium of the context scatters (include/gpuspectral_pt.h, "Scattering media"; `scatter` = the table
// parallel to `media`).  A back-face vertex of a medium with any sigma_s != 0 draws the free path first: a medium event leaves
// through the early return below -- no BSDF, no light sample, no shadow ray --, a surface event goes on as the ordinary vertex with
// the weight of the decision.  A medium whose sigma_s is 0 takes the MED line and draws nothing.  SCT = false is the code of a
// context whose media only absorb, instruction for instruction.
// DLT: the context holds delta lights (include/gpuspectral_pt.h, "Delta lights"): the light table has S.num_lights records, the first
// num_tri_lights of them triangles, the rest gsp_delta_light (never empty here: num_lights != 0).  The same three draws and the same
// pick; an index >= num_tri_lights takes sample_delta_light (pt_deltalight.h) and an NEE term without the power heuristic, a
// smaller one the triangle's operations as they stand.  DLT = false is the code of a context without delta lights, instruction for
// instruction.
// ENV (only with TEX, EST and DLT): the context samples its environment map as a light (include/gpuspectral_pt.h, "Environment
// light"): the LAST record of the light table is the EnvLightRecord, `env_cells` its cell table.  The same three draws and the same
// pick; a pick that lands on the record draws one further word, picks a cell and takes sample_env_light (pt_envlight.h) and the
// triangle's textbook NEE term with Ldist = 1e30f.  ENV = false is the code of a context without the switch, instruction for
// instruction.
// GRD (only with LSEL, EST and DLT, never with ENV): the context selects its light through the light grid (include/gpuspectral_pt.h,
// "Light grid"): `grid_off` = the byte offset of the grid inside this vertex's version of the tables, from S.tables (global memory
// also where the tables in front of it were staged into LDS).  The same three draws; the pick reads the alias table of the cell of
// q = the origin this vertex gives its continuation ray, and an emitter that is hit takes p_sel from the cell of in.o -- the q of
// the vertex that sent the ray, the same three floats (nx.o below).  GRD = false is the code of a context without the grid,
// instruction for instruction.
template <bool TEX = false, bool VER = false, bool MED = false, bool LSEL = false, bool EST = false, bool SCT = false, bool DLT = false, bool ENV = false,
          bool GRD = false>
GSP_HD void shade_vertex(const SceneView& S, const RenderConstsBase& rc, const PathState& in, const HitRec& hit,
                         ShadeOut& out, const gsp_medium* media = nullptr, const gsp_medium_scatter* scatter = nullptr,
                         uint32_t num_tri_lights = 0u, const gsp_light_pick* env_cells = nullptr, uint32_t grid_off = 0u) {
  static_assert(MED || !SCT, "the scattering table is parallel to the media table");
  static_assert(!ENV || (TEX && EST && DLT), "the environment light lives in the textbook estimator, behind the delta records");
  static_assert(!GRD || (LSEL && EST && DLT && !ENV), "the light grid lives under the power pick and the textbook estimator, without the environment record");
  uint32_t rng = in.seed;                                                 // rchit:668
  BsdfTables Tv;  // (VER only: this lane's version of the tables)
  const gsp_triangle_light* lights_v = nullptr;
  if (VER) {
    const size_t voff = (size_t)((in.flags & kVerMask) >> kVerShift) * S.ver_stride;
    Tv.diffuse = (const gsp_diffuse_bsdf*)((const char*)S.bsdf.diffuse + voff);
    Tv.smooth_dielectric = (const gsp_smooth_dielectric_bsdf*)((const char*)S.bsdf.smooth_dielectric + voff);
    Tv.smooth_conductor = (const gsp_smooth_conductor_bsdf*)((const char*)S.bsdf.smooth_conductor + voff);
    Tv.smooth_plastic = (const gsp_smooth_plastic_bsdf*)((const char*)S.bsdf.smooth_plastic + voff);
    Tv.rough_conductor = (const gsp_rough_conductor_bsdf*)((const char*)S.bsdf.rough_conductor + voff);
    Tv.smooth_floor = (const gsp_smooth_floor_bsdf*)((const char*)S.bsdf.smooth_floor + voff);
    Tv.rough_floor = (const gsp_rough_floor_bsdf*)((const char*)S.bsdf.rough_floor + voff);
    Tv.rough_plastic = (const gsp_rough_plastic_bsdf*)((const char*)S.bsdf.rough_plastic + voff);
    lights_v = (const gsp_triangle_light*)((const char*)S.lights + voff);
  }
  const BsdfTables& T = VER ? Tv : S.bsdf;
  const gsp_triangle_light* lights = VER ? lights_v : S.lights;
  // (GRD only) the grid of this vertex's version of the tables, in global memory
  const uint8_t* grid = GRD ? S.tables + ((VER ? (size_t)((in.flags & kVerMask) >> kVerShift) * S.ver_stride : (size_t)0) + grid_off) : nullptr;
  GSP_PROF_BEGIN(PR_PACKET);
  const long long slot_v = (long long)hit.slot + (VER && (uint32_t)hit.slot >= S.static_slots ? (long long)geo_slot_offset(S.geo, geo_stamp(in.flags)) : 0ll);
  const q4* sp = S.tri_shade + 4ll * slot_v;
  const q4 s0 = sp[0], s1 = sp[1], s2 = sp[2], s3 = sp[3];
  const uint32_t material = f2u(s0.w);                                    // :672 (instance record, baked per triangle)
  const uint32_t bsdf = material & (MED ? 0x0007ffffu : 0x7fffffffu);
  const bool twofaced = (material >> 31) != 0u;
  const f3 emission = mk3(s1.w, s2.w, s3.w);
  const f3 rayDir = in.d;                                                 // :696
  const f3 position = in.o + rayDir * hit.t;                              // :692
  const float b0 = (1.0f - hit.u) - hit.v;                                // :690
  f3 SN = normalize((b0 * mk3(s1.x, s1.y, s1.z) + hit.u * mk3(s2.x, s2.y, s2.z)) + hit.v * mk3(s3.x, s3.y, s3.z));
  f3 N = mk3(s0.x, s0.y, s0.z);                                           // :694 (precomputed at bake)
  // MED: the path weight this vertex works with.  Formed here, on the geometric normal before the two-sided flip and before the
  // BSDF's inputs are live (the three exponentials then need no register the rest of the vertex does not)
  f3 weight = in.weight;
  const uint32_t medium = MED ? (material >> 19) & 0xfffu : 0u;
  bool flipped = false;  // (MED only) N below is the geometric normal turned round
  if (MED) {
    if (medium != 0u && dot(N, -rayDir) < 0.0f) {
      const gsp_medium* m = media + (medium - 1u);
      bool scatters = false;
      if constexpr (SCT) {
        const gsp_medium_scatter* sc = scatter + (medium - 1u);
        const f3 sigma_s = mk3(sc->sigma_s[0], sc->sigma_s[1], sc->sigma_s[2]);
        scatters = sigma_s.x != 0.0f || sigma_s.y != 0.0f || sigma_s.z != 0.0f;
        if (scatters) {
          const float u_c = rand_uniform(rng);
          const float u_d = rand_uniform(rng);
          const MediumEvent ev = medium_event(mk3(m->sigma_a[0], m->sigma_a[1], m->sigma_a[2]), sigma_s, hit.t, u_c, u_d, in.weight);
          if (ev.scatter || !ev.valid) {
            // a medium event (or an invalid density: the path ends): the vertex is a point inside the object.  It emits nothing,
            // traces no shadow ray and continues along the phase function's sample; roulette and the depth test as at a surface
            const uint32_t depth = in.flags & 0xffu;
            PathState nx = in;
            bool alive = ev.valid;
            if (ev.valid) {
              const float u1 = rand_uniform(rng);
              const float u2 = rand_uniform(rng);
              float pdf;
              nx.d = sample_hg(rayDir, sc->g, u1, u2, pdf);
              nx.o = in.o + rayDir * ev.s;
              nx.weight = ev.w;
              nx.directWeight = EST ? pdf : 1.0f;
            }
            nx.seed = rng;
            if (depth > rc.rr_start_depth) {
              const float q = gclamp(gmax(gmax(nx.weight.x, nx.weight.y), nx.weight.z), 0.05f, 1.0f);
              uint32_t peek = nx.seed;
              if (rand_uniform(peek) > q) alive = false;
              nx.weight = nx.weight / q;
            }
            if (depth > rc.max_depth) alive = false;
            nx.flags = pack_flags(depth + 1u, 0u, 0u) | (VER ? (in.flags & kStampMask) : 0u);
            out.alive = alive;
            out.next = nx;
            out.has_shadow = false;
            out.emitted = splat(0.0f);
            return;
          }
          weight = ev.w;
        }
      }
      if (!scatters) weight = in.weight * mk3(det_expf(-(m->sigma_a[0] * hit.t)), det_expf(-(m->sigma_a[1] * hit.t)), det_expf(-(m->sigma_a[2] * hit.t)));
    }
  }
  if (dot(N, -rayDir) < 0.0f) {                                           // :698-707
    if (twofaced && emission.x == 0.0f && emission.y == 0.0f && emission.z == 0.0f) {
      N = N * -1.0f;
      SN = SN * -1.0f;
      if (MED) flipped = true;
    }
  }
  const Frame onb = make_frame(SN);                                       // :712
  const f3 wo = normalize(to_local(onb, -rayDir));                        // :713
  bool kd_on = false;
  f3 kd = splat(0.0f);
  if (TEX) {
    const uint32_t tid = bsdf_texture(T, bsdf);
    if (tid != 0u && tid <= S.tex.num_textures && S.tex.tri_uv != nullptr) {
      const q4* uv = (const q4*)S.tex.tri_uv + 2ll * hit.slot;  // {u0 v0 u1 v1}, {u2 v2 - -}
      const q4 ua = uv[0], ub2 = uv[1];
      const float tu = (b0 * ua.x + hit.u * ua.z) + hit.v * ub2.x;
      const float tv = (b0 * ua.y + hit.u * ua.w) + hit.v * ub2.y;
      kd = sample_texture(S.tex, tid - 1u, tu, tv);
      kd_on = true;
    }
  }
  BsdfResult bs;
  f3 wi_l;
  GSP_PROF_END(PR_PACKET);
  GSP_PROF_BEGIN(PR_SAMPLE);
  BsdfCarry cy;
  bsdf_sample(T, bsdf, rng, wo, wi_l, bs, cy, kd_on, kd);            // :716
  GSP_PROF_END(PR_SAMPLE);
  GSP_PROF_BEGIN(PR_LIGHT);
  const float NoW = gabs(wi_l.z);                                         // :717
  const f3 wi = to_world(onb, wi_l);                                      // :718

  LightSample ls;
  f3 L;
  float Ldist;
  bool delta_light = false;  // (DLT only) the pick landed on a delta record
  if constexpr (DLT) {
    const uint32_t r = pcg_next(rng);
    const float e1 = rand_uniform(rng);
    const float e2 = rand_uniform(rng);
    float pmf = S.inv_num_lights;
    uint32_t k;
    if constexpr (GRD) {  // the table of the cell of q, the origin of the continuation ray (nx.o below: the same expression)
      k = lightgrid_pick(grid, (const gsp_light_pick*)(lights + S.num_lights), S.num_lights, position + 0.0001f * faceforward(N, -wi, N), r, pmf);
    } else {
      k = LSEL ? light_pick_index((const gsp_light_pick*)(lights + S.num_lights), S.num_lights, r, pmf) : r % S.num_lights;
    }
    const bool env_light = ENV && k == S.num_lights - 1u;  // (ENV only) the pick landed on the environment record, the last one
    delta_light = !env_light && k >= num_tri_lights;
    if constexpr (ENV) {
      if (env_light && rc.nee != 0u) {  // one further draw picks the cell; (e1, e2) place the direction inside it
        const uint32_t r2 = pcg_next(rng);
        const EnvSample es = sample_env_light(S.tex, env_cells, *(const EnvLightRecord*)(lights + k), r2, e1, e2);
        L = es.L;
        Ldist = 1e30f;
        ls.emission = es.emission;
        ls.pdf = es.pdf;
      } else if (env_light) {  // disable_nee: no light sample is used, so none is made and the random stream is that of the switch off
        L = mk3(0.0f, 0.0f, 1.0f);
        Ldist = 1e30f;
        ls.emission = splat(0.0f);
        ls.pdf = 0.0f;
      }
    }
    if (env_light) {
    } else if (delta_light) {  // (e1, e2: drawn and unused)
      const DeltaSample ds = sample_delta_light(*(const gsp_delta_light*)(lights + k), position, pmf);
      L = ds.L;
      Ldist = ds.Ldist;
      ls.emission = ds.emission;
      ls.pdf = ds.pdf;
    } else {
      ls = sample_light_triangle(lights + k, e1, e2, position, pmf);
      const f3 toL = ls.position - position;
      L = normalize(toL);
      Ldist = length(toL);
    }
  } else {
    ls = LSEL ? sample_light_power(lights, (const gsp_light_pick*)(lights + S.num_lights), S.num_lights, rng, position)
              : sample_light(lights, S.num_lights, S.inv_num_lights, rng, position);  // :720
    const f3 toL = ls.position - position;
    L = normalize(toL);                                                   // :722
    Ldist = length(toL);                                                  // :724
  }
  const f3 wL = to_local(onb, L);                                         // :723
  const float NoL = gabs(dot(SN, L));                                     // :725
  const float lightPdf = ls.pdf;
  BsdfResult lb;
  GSP_PROF_END(PR_LIGHT);
  GSP_PROF_BEGIN(PR_EVAL);
  bsdf_eval<EST>(T, bsdf, wo, wL, lb, cy, kd_on, kd);                // :729
  GSP_PROF_END(PR_EVAL);
  GSP_PROF_BEGIN(PR_TAIL);

  const bool transmits = bsdf_transmits(bsdf);
  const float NdotV = dot(N, -rayDir);
  // :733-736 gate (`if (NEE)` first); `lightPdf != 0` (:750) is known before tracing
  const bool nee_on = rc.nee != 0u;
  const bool want_shadow = nee_on && !bs.delta && ((NdotV > 0.0f && dot(N, L) > 0.0f) || transmits) && (lightPdf != 0.0f);
  f3 nee = splat(0.0f);
  if (want_shadow) {
    if (DLT && delta_light) {  // no BSDF sample reaches a delta light: weight 1
      nee = (((NoL * lb.f) * weight) * ls.emission) / lightPdf;
    } else {
      const float w = power_heuristic(lightPdf, EST ? lb.pdf : bs.pdf);   // :751 (EST: the pdf of L itself)
      nee = ((((w * NoL) * lb.f) * weight) * ls.emission) / lightPdf;     // :752
    }
  }
  const uint32_t depth = in.flags & 0xffu;
  const uint32_t wasDelta = (in.flags >> 8) & 1u;
  const uint32_t countEmitted = (in.flags >> 9) & 1u;
  const float lightFlag = NdotV > 0.0f ? 1.0f : 0.0f;                     // :760
  f3 emis = splat(0.0f);
  float directWeight = in.directWeight;
  if constexpr (EST) {
    // the textbook weight: in.directWeight is lastPdf.  The hit triangle's world-space vertices (the intersection packet, at the
    // slot the shading packet was read from) are fetched only for an emitter
    directWeight = 1.0f;
    if (nee_on && countEmitted == 0 && wasDelta == 0 && (emission.x != 0.0f || emission.y != 0.0f || emission.z != 0.0f)) {
      const q4* ip = S.tri_isect + 3ll * slot_v;
      const q4 i0 = ip[0], i1 = ip[1], i2 = ip[2];
      const f3 v0 = mk3(i0.x, i0.y, i0.z), v1 = mk3(i1.x, i1.y, i1.z), v2 = mk3(i2.x, i2.y, i2.z);
      const float A = light_hit_area(v0, v1, v2);
      float p_sel = S.inv_num_lights;
      // LSEL: the selection probability of the light that was HIT, through the trailing record behind the alias table (no lights: no table)
      if constexpr (GRD) {  // ... positional: the cell of the ray's origin, the weight from the hit's own data (pt_lightgrid.h)
        p_sel = lightgrid_hit_select_pmf(grid, (const gsp_light_pick*)(lights + S.num_lights), S.num_lights, S.inv_num_lights, in.o, v0, v1, v2, emission, A);
      } else
      if (LSEL && S.num_lights != 0u) p_sel = light_hit_select_pmf(emission, A, *(const float*)((const gsp_light_pick*)(lights + S.num_lights) + S.num_lights), S.inv_num_lights);
      directWeight = power_heuristic(in.directWeight, light_hit_pdf(hit.t, rayDir, N, A, p_sel));
    }
  }
  if (nee_on && countEmitted == 0 && wasDelta == 0) emis = emis + ((directWeight * emission) * lightFlag) * weight;  // :763-765
  if (!nee_on || countEmitted == 1 || wasDelta == 1) emis = emis + (emission * lightFlag) * weight;                      // :766-768

  bool done = false;
  if (dot(wi, N) <= 0.0f && !transmits) done = true;                      // :770-773
  if (NdotV <= 0.0f && !transmits) done = true;                           // :776-779
  if (!gisvalid(bs.pdf) || !gisvalid(bs.f.x) || !gisvalid(bs.f.y) || !gisvalid(bs.f.z) || bs.pdf == 0.0f)
    done = true;                                                          // :781-784

  PathState nx = in;
  nx.seed = rng;                                                          // :759
  if (MED) nx.weight = weight;
  if (!done) {
    nx.directWeight = EST ? bs.pdf : 1.0f;                                // :785-790 (connect overwrites when NEE happens); EST: lastPdf
    nx.o = position + 0.0001f * faceforward(N, -wi, N);                   // :793
    nx.d = wi;                                                            // :794
    nx.weight = weight * ((bs.f * NoW) / bs.pdf);                         // :795
    if (MED) {
      // the segment that starts here runs INSIDE the object (wi points against the geometric normal): its origin sits 1e-4 below the
      // surface along the normal (:793), so the traced ray meets the surface's plane 1e-4 / |dot(N, wi)| behind its origin and the
      // next vertex's t is short by that much.  The missing piece is absorbed here, where the normal is known
      const float c = dot(wi, N);
      if (medium != 0u && (flipped ? c > 0.0f : c < 0.0f)) {
        const gsp_medium* m = media + (medium - 1u);
        const float s = gmin(0.0001f / gabs(c), 1e30f);
        nx.weight = nx.weight * mk3(det_expf(-(m->sigma_a[0] * s)), det_expf(-(m->sigma_a[1] * s)), det_expf(-(m->sigma_a[2] * s)));
      }
    }
  }
  // back in raygen: Russian roulette reads the NEXT vertex's first variate (rgen:59,66-71)
  bool alive = true;
  if (depth > rc.rr_start_depth) {
    const float q = gclamp(gmax(gmax(nx.weight.x, nx.weight.y), nx.weight.z), 0.05f, 1.0f);
    uint32_t peek = nx.seed;
    if (rand_uniform(peek) > q) alive = false;
    nx.weight = nx.weight / q;
  }
  if (depth > rc.max_depth) alive = false;                                // rgen:73-75
  if (done) alive = false;                                                // rgen:77-78
  nx.flags = pack_flags(depth + 1u, bs.delta ? 1u : 0u, 0u) | (VER ? (in.flags & kStampMask) : 0u);  // rgen:80, rchit:792,796; VER: the versions ride along

  out.alive = alive;
  out.next = nx;
  out.has_shadow = want_shadow;
  out.emitted = emis;                                                     // (0 + nee) + emis with nee absent
  if (want_shadow) {
    out.shadow.o = position;                                              // :744 (un-offset origin, tmin 0.01)
    out.shadow.d = L;
    out.shadow.tmax = Ldist - 0.01f;                                      // :747
    out.shadow.nee = nee;
    out.shadow.emis = emis;
    out.shadow.dw_nee = EST ? bs.pdf : power_heuristic(bs.pdf, lightPdf); // :786; EST: lastPdf, whatever the verdict
    if (DLT && !EST && delta_light) out.shadow.dw_nee = 1.0f;              // what a vertex without a shadow ray hands on
    out.shadow.sid = in.sid;
    out.shadow.next = -1;
  }
  GSP_PROF_END(PR_TAIL);
}

// dormant-feature extension: a path that leaves the scene (miss.rmiss:15-18 ends it) first picks up the environment
// map along its direction.  MIS: sampleLight never draws the environment, so the weight is the one an emitter met after a
// delta bounce gets (rayhit.rchit:766-768): the full path weight.
GSP_HD f3 miss_emitted(const SceneView& S, const PathState& in) { return sample_envmap(S.tex, in.d) * in.weight; }
// ... in a context that samples the environment as a light (include/gpuspectral_pt.h, "Environment light"; `in` complete: flags and
// directWeight = lastPdf too): an escape that next-event estimation could have produced -- NEE on, countEmitted == 0, wasDelta == 0
// -- is weighted against the density of its own direction, from the function the sampling side called; every other escape adds the
// full weight as above.  The record is read from the path's version of the tables
template <bool VER>
GSP_HD f3 miss_emitted_env(const SceneView& S, const RenderConstsBase& rc, const PathState& in, const gsp_light_pick* env_cells) {
  const gsp_triangle_light* lights = VER ? (const gsp_triangle_light*)((const char*)S.lights + (size_t)((in.flags & kVerMask) >> kVerShift) * S.ver_stride) : S.lights;
  const EnvLightRecord& rec = *(const EnvLightRecord*)(lights + (S.num_lights - 1u));
  const EnvEval ev = env_eval(S.tex, env_cells, rec.cw, rec.ch, in.d);
  const uint32_t wasDelta = (in.flags >> 8) & 1u;
  const uint32_t countEmitted = (in.flags >> 9) & 1u;
  if (rc.nee != 0u && countEmitted == 0u && wasDelta == 0u) return (ev.radiance * power_heuristic(in.directWeight, ev.density * rec.p_sel)) * in.weight;
  return ev.radiance * in.weight;
}

// rayhit.rchit:750-754 + raygen.rgen:60-63 for a vertex that traced a shadow ray
GSP_HD void connect_vertex(float clampv, const ShadowRay& s, bool occluded, q4& result, bool& nee_done) {
  f3 e = splat(0.0f);
  if (!occluded) e = e + s.nee;
  e = e + s.emis;
  add_emitted(clampv, e, result);
  nee_done = !occluded;
}

// raygen.rgen:84-108: fold one finished sample into the running mean
GSP_HD void resolve_sample(uint32_t timestamp, q4 sample, q4& accum) {
  f3 c = mk3(sample.x, sample.y, sample.z);
  if (timestamp > 0) {
    const float a = 1.0f / (float)(timestamp + 1u);
    const f3 prev = mk3(accum.x, accum.y, accum.z);
    c = prev * (1.0f - a) + c * a;  // mix(prev, c, a)
  }
  if (!(gisnan(c.x) || gisnan(c.y) || gisnan(c.z))) {
    accum.x = c.x;
    accum.y = c.y;
    accum.z = c.z;
    accum.w = 1.0f;
  }
}

}  // namespace gsp
