// pt_lightgrid.h -- spatial light selection (include/gpuspectral_pt.h, "Light grid"): a regular grid over the scene's bounding box,
// one alias table per cell, every light weighted by power / distance^2 to the cell.  ONE weight function, float32 in the order the
// header states: the host builder at the end of this file, the emitter-hit pdf of shade_vertex<.., GRD = true> (pt_stages.h) and
// the tests' host emulation (tests/emu/lightgrid_emu.cpp) all call it.  Small GSP_HD functions, each callable on its own
// (tests/devfn).  The grid sits BEHIND the power pick table and its trailing record inside the table image:
//     [LightGridHeader, 64 B] [cell 0: num_lights gsp_light_pick, one 16-byte tail {inv_sum_w, 0, 0, 0}] [cell 1 ...] ...
// cell (ix, iy, iz) has number (iz * ny + iy) * nx + ix.
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/gpuspectral_pt.h"
#include "pt_lightpick.h"
#include "pt_math.h"
#include "pt_shading.h"

namespace gsp {

struct alignas(16) LightGridHeader {
  float lo[3];        // the box: the bounds of the scene's geometry as uploaded
  uint32_t nx;
  float inv_cell[3];  // (float)n / (hi - lo) per axis; 0 on an axis without extent (its one cell spans the axis)
  uint32_t ny;
  float cell[3];      // (hi - lo) / (float)n per axis: the cell's edges
  uint32_t nz;
  float hi[3];
  float half_diag;    // 0.5f * sqrt((cell.x * cell.x + cell.y * cell.y) + cell.z * cell.z): Rcell
};
static_assert(sizeof(LightGridHeader) == 64, "the cells start 64 bytes behind the header, on a 16-byte boundary");
constexpr uint32_t kLightGridNoCell = 0xffffffffu;  // a point outside the box, or not finite: the fallback table
constexpr uint32_t kLightGridMaxAxis = 64u, kLightGridAutoAxis = 32u;
constexpr uint64_t kLightGridMaxEntries = 1ull << 20;  // cells * num_lights: a 16 MB image

// bytes of one cell (table + tail) and of the whole grid behind the power pick table's trailing record
GSP_HD size_t lightgrid_cell_bytes(uint32_t num_lights) { return sizeof(gsp_light_pick) * ((size_t)num_lights + 1u); }
GSP_HD size_t lightgrid_bytes(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t num_lights) {
  return sizeof(LightGridHeader) + (((size_t)nx * ny) * nz) * lightgrid_cell_bytes(num_lights);
}

// The cell of a point: per axis f = floor((x - lo) * inv_cell); 0 <= f < n or the point takes the fallback (NaN fails both tests).
// The box is half open: a point on a cell's lower face belongs to that cell, a point on the box's upper face is outside whenever
// the product reaches n.
GSP_HD uint32_t lightgrid_axis(float x, float lo, float inv_cell, uint32_t n) {
  const float f = __builtin_floorf((x - lo) * inv_cell);
  return (f >= 0.0f && f < (float)n) ? (uint32_t)f : kLightGridNoCell;
}
GSP_HD uint32_t lightgrid_cell(const LightGridHeader& g, f3 p, uint32_t& ix, uint32_t& iy, uint32_t& iz) {
  ix = lightgrid_axis(p.x, g.lo[0], g.inv_cell[0], g.nx);
  iy = lightgrid_axis(p.y, g.lo[1], g.inv_cell[1], g.ny);
  iz = lightgrid_axis(p.z, g.lo[2], g.inv_cell[2], g.nz);
  if (ix == kLightGridNoCell || iy == kLightGridNoCell || iz == kLightGridNoCell) return kLightGridNoCell;
  return (iz * g.ny + iy) * g.nx + ix;
}
GSP_HD f3 lightgrid_cell_centre(const LightGridHeader& g, uint32_t ix, uint32_t iy, uint32_t iz) {
  return mk3(g.lo[0] + ((float)ix + 0.5f) * g.cell[0], g.lo[1] + ((float)iy + 0.5f) * g.cell[1], g.lo[2] + ((float)iz + 0.5f) * g.cell[2]);
}

GSP_HD float lightgrid_luminance(f3 c) { return gmax((0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z, 0.0f); }
GSP_HD float lightgrid_valid(float w) { return (gisvalid(w) && w > 0.0f) ? w : 0.0f; }

// The weight of a TRIANGLE light for the cell of centre c: Y * A / max(D^2, R^2), D = |centroid - c|, R = Rcell + the largest
// centroid-to-vertex distance (so no point of the cell sees a weight that understates 1 / distance^2 to the centroid by more than
// the factor 4 of D <= 2 R).  The emitting side is that of n = cross(v1 - v0, v2 - v0) (bake_light's normal, sample_light_triangle's c).
//
// BACK-FACE CULL.  The largest signed distance of a point of the cell to the light's plane, times |n|, is
//     smax = dot(n, c - centroid) + (|n.x| half.x + |n.y| half.y) + |n.z| half.z            (half = cell / 2, the support of a box)
// and the weight is 0 only when smax < -margin * |n|, margin = 1e-4f * S, S = |c|_1 + |centroid|_1 + Rcell + Rtri.  Why this can
// never zero a light that a point x of the cell sees from the front: such an x has dot(n, x - centroid) > 0, and x lies in the cell
// up to the rounding of lightgrid_axis (a few ulp of its coordinates, <= 2^-22 |x|), so the exact smax is > -2^-22 S |n|.  The
// float32 evaluation of smax is a sum of nine products whose magnitudes are bounded by |n| S: its absolute error is below
// 16 * 2^-24 * |n| S, the vertices' and the centre's own rounding (2^-24 of their magnitudes, again <= |n| S 2^-23 after the dot
// product) included.  Together < 2e-6 |n| S, a fiftieth of the margin.  The margin in turn is small against the cell: a cell cut
// by the plane has smax >= 0.  A degenerate triangle (|n| = 0) is never culled; its area makes the weight 0.
GSP_HD float lightgrid_tri_weight(const LightGridHeader& g, f3 c, f3 v0, f3 v1, f3 v2, f3 radiance, float A) {
  const f3 cen = ((v0 + v1) + v2) * (1.0f / 3.0f);
  const f3 a0 = v0 - cen, a1 = v1 - cen, a2 = v2 - cen;
  const float rt = gsqrt(gmax(gmax(dot(a0, a0), dot(a1, a1)), dot(a2, a2)));
  const f3 n = cross(v1 - v0, v2 - v0);
  const f3 d = c - cen;
  const float smax = dot(n, d) + ((gabs(n.x) * (0.5f * g.cell[0]) + gabs(n.y) * (0.5f * g.cell[1])) + gabs(n.z) * (0.5f * g.cell[2]));
  const float S = (((gabs(c.x) + gabs(c.y)) + gabs(c.z)) + ((gabs(cen.x) + gabs(cen.y)) + gabs(cen.z))) + (g.half_diag + rt);
  if (smax < -((1e-4f * S) * length(n))) return 0.0f;
  const float R = g.half_diag + rt;
  return lightgrid_valid((lightgrid_luminance(radiance) * A) / gmax(dot(d, d), R * R));
}
// ... of a delta record: point and spot Y(intensity) / max(D^2, Rcell^2), directional Y(intensity): luminous-irradiance scales all
GSP_HD float lightgrid_delta_weight(const LightGridHeader& g, f3 c, const gsp_delta_light& L) {
  const float Y = lightgrid_luminance(mk3(L.intensity[0], L.intensity[1], L.intensity[2]));
  if (L.kind == GSP_LIGHT_DIRECTIONAL) return lightgrid_valid(Y);
  const f3 d = mk3(L.position[0], L.position[1], L.position[2]) - c;
  return lightgrid_valid(Y / gmax(dot(d, d), g.half_diag * g.half_diag));
}

// The table a vertex at p picks from: its cell's, or `fallback` (the power pick table in front of the grid).  `grid` = the header
GSP_HD const gsp_light_pick* lightgrid_table(const uint8_t* grid, const gsp_light_pick* fallback, uint32_t num_lights, f3 p) {
  const LightGridHeader g = *(const LightGridHeader*)grid;
  uint32_t ix, iy, iz;
  const uint32_t cell = lightgrid_cell(g, p, ix, iy, iz);
  if (cell == kLightGridNoCell) return fallback;
  return (const gsp_light_pick*)(grid + sizeof(LightGridHeader) + (size_t)cell * lightgrid_cell_bytes(num_lights));
}
// The pick: the draw r of sample_light_power on the table of p's cell -- light_pick_index, one 16-byte load of the entry
GSP_HD uint32_t lightgrid_pick(const uint8_t* grid, const gsp_light_pick* fallback, uint32_t num_lights, f3 p, uint32_t r, float& pmf) {
  return light_pick_index(lightgrid_table(grid, fallback, num_lights, p), num_lights, r, pmf);
}
// The selection probability of a triangle emitter that a ray from `origin` HIT: weight(cell of origin, the hit's own vertices,
// emission and area) * inv_sum_w[cell].  A cell whose tail holds 0 (every weight of the cell was 0: its table is the fallback's)
// and a point without a cell take light_hit_select_pmf on the fallback's tail, the rule of a context without the grid.
GSP_HD float lightgrid_hit_select_pmf(const uint8_t* grid, const gsp_light_pick* fallback, uint32_t num_lights, float inv_num_lights, f3 origin, f3 v0, f3 v1,
                                      f3 v2, f3 emission, float A) {
  const LightGridHeader g = *(const LightGridHeader*)grid;
  uint32_t ix, iy, iz;
  const uint32_t cell = lightgrid_cell(g, origin, ix, iy, iz);
  if (cell != kLightGridNoCell) {
    const float inv_sum_w = *(const float*)(grid + sizeof(LightGridHeader) + (size_t)cell * lightgrid_cell_bytes(num_lights) + sizeof(gsp_light_pick) * (size_t)num_lights);
    if (inv_sum_w != 0.0f) return lightgrid_tri_weight(g, lightgrid_cell_centre(g, ix, iy, iz), v0, v1, v2, emission, A) * inv_sum_w;
  }
  return light_hit_select_pmf(emission, A, *(const float*)(fallback + num_lights), inv_num_lights);
}
}  // namespace gsp

// ---- host side: validation, bounds, resolution, the builder -------------------------------------------------------------------
namespace gsp {

// nullptr = acceptable; else what is wrong
inline const char* check_light_grid(const gsp_light_grid* s) {
  if (!s || s->enabled == 0u) return nullptr;
  for (uint32_t r : s->reserved)
    if (r != 0u) return "gsp_light_grid.reserved must be 0";
  const uint32_t* n = s->resolution;
  if (n[0] > kLightGridMaxAxis || n[1] > kLightGridMaxAxis || n[2] > kLightGridMaxAxis) return "gsp_light_grid.resolution: at most 64 cells along an axis";
  const int zeros = (n[0] == 0u) + (n[1] == 0u) + (n[2] == 0u);
  if (zeros != 0 && zeros != 3) return "gsp_light_grid.resolution: either 0, 0, 0 (auto) or three counts >= 1";
  return nullptr;
}

// The bounding box of the scene's geometry as uploaded: every vertex of every instance through xform_point, as the BVH's bake
// forms it.  false (and a zero box) for a scene without a vertex
inline bool lightgrid_scene_bounds(const gsp_scene_desc* sc, float lo[3], float hi[3]) {
  bool any = false;
  for (int c = 0; c < 3; ++c) lo[c] = hi[c] = 0.0f;
  for (uint32_t a = 0; a < sc->num_instances; ++a) {
    const gsp_instance& I = sc->instances[a];
    for (uint32_t k = 0; k + 3 <= I.vertex_count; k += 3)
      for (uint32_t v = 0; v < 3; ++v) {
        const float* P = sc->positions + 3ull * (I.first_vertex + k + v);
        const f3 p = xform_point(I.transform, mk3(P[0], P[1], P[2]));
        const float q[3] = {p.x, p.y, p.z};
        for (int c = 0; c < 3; ++c) {
          if (!any || q[c] < lo[c]) lo[c] = q[c];
          if (!any || q[c] > hi[c]) hi[c] = q[c];
        }
        any = true;
      }
  }
  return any;
}

// Auto resolution: the largest m <= 32 cells along the longest axis with cells as near cubic as the rounding allows --
// n_axis = clamp(round(extent_axis / (longest / m)), 1, m), in double -- whose cells * num_lights stays within 2^20 entries.
// An axis without extent gets 1 cell.  false when even 1 x 1 x 1 is beyond the cap
inline bool lightgrid_auto_resolution(const float lo[3], const float hi[3], uint32_t num_lights, uint32_t res[3]) {
  double ext[3], longest = 0.0;
  for (int c = 0; c < 3; ++c) {
    ext[c] = (double)hi[c] - (double)lo[c];
    if (!(ext[c] > 0.0) || !std::isfinite(ext[c])) ext[c] = 0.0;
    longest = ext[c] > longest ? ext[c] : longest;
  }
  for (uint32_t m = kLightGridAutoAxis; m >= 1u; --m) {
    uint64_t cells = 1;
    for (int c = 0; c < 3; ++c) {
      double n = longest > 0.0 ? std::floor(ext[c] / (longest / (double)m) + 0.5) : 1.0;
      n = n < 1.0 ? 1.0 : (n > (double)m ? (double)m : n);
      res[c] = (uint32_t)n;
      cells *= res[c];
    }
    if (cells * (uint64_t)num_lights <= kLightGridMaxEntries) return true;
  }
  return false;
}
// the resolution a grid is built with: the caller's, or auto; an axis without extent always has 1 cell.  0 = fine, 1 = beyond the cap
inline int lightgrid_resolve(const gsp_light_grid& want, const float lo[3], const float hi[3], uint32_t num_lights, uint32_t res[3]) {
  if (want.resolution[0] == 0u) return lightgrid_auto_resolution(lo, hi, num_lights, res) ? 0 : 1;
  for (int c = 0; c < 3; ++c) res[c] = (hi[c] > lo[c]) ? want.resolution[c] : 1u;
  return (((uint64_t)res[0] * res[1]) * res[2]) * (uint64_t)num_lights <= kLightGridMaxEntries ? 0 : 1;
}

inline LightGridHeader make_lightgrid_header(const float lo[3], const float hi[3], const uint32_t res[3]) {
  LightGridHeader g{};
  for (int c = 0; c < 3; ++c) {
    const float ext = hi[c] - lo[c];
    const bool flat = !(ext > 0.0f) || !gisvalid(ext);
    g.lo[c] = lo[c];
    g.hi[c] = hi[c];
    g.inv_cell[c] = flat ? 0.0f : (float)res[c] / ext;
    g.cell[c] = flat ? 0.0f : ext / (float)res[c];
  }
  g.nx = res[0], g.ny = res[1], g.nz = res[2];
  g.half_diag = 0.5f * gsqrt((g.cell[0] * g.cell[0] + g.cell[1] * g.cell[1]) + g.cell[2] * g.cell[2]);
  return g;
}

// the weights of one cell, float32 from the one function, widened: triangles (the caller's UNBAKED records), then delta records
inline void lightgrid_cell_weights(const LightGridHeader& g, f3 c, const gsp_triangle_light* lights, uint32_t n, const gsp_delta_light* delta, uint32_t nd, double* w) {
  for (uint32_t i = 0; i < n; ++i) {
    const f3 v0 = ld3(lights[i].positions[0]), v1 = ld3(lights[i].positions[1]), v2 = ld3(lights[i].positions[2]);
    w[i] = (double)lightgrid_tri_weight(g, c, v0, v1, v2, ld3(lights[i].radiance), light_hit_area(v0, v1, v2));
  }
  for (uint32_t i = 0; i < nd; ++i) w[(size_t)n + i] = (double)lightgrid_delta_weight(g, c, delta[i]);
}

// The grid image at `out` (lightgrid_bytes(...) bytes, zeroed by the caller).  `fallback` = the power pick table of the same lights:
// a cell whose weights are all 0 copies it and stores tail 0 -- never a uniform table, which the hit pdf could not restate.
// weights_out (optional): cells * (n + nd) doubles, the weights as the tables were built from
inline void build_light_grid(const LightGridHeader& g, const gsp_triangle_light* lights, uint32_t n, const gsp_delta_light* delta, uint32_t nd,
                             const gsp_light_pick* fallback, uint8_t* out, double* weights_out = nullptr) {
  const uint32_t all = n + nd;
  std::memcpy(out, &g, sizeof(g));
  std::vector<double> w(all);
  uint8_t* cellp = out + sizeof(LightGridHeader);
  for (uint32_t iz = 0; iz < g.nz; ++iz)
    for (uint32_t iy = 0; iy < g.ny; ++iy)
      for (uint32_t ix = 0; ix < g.nx; ++ix, cellp += lightgrid_cell_bytes(all)) {
        lightgrid_cell_weights(g, lightgrid_cell_centre(g, ix, iy, iz), lights, n, delta, nd, w.data());
        if (weights_out) std::memcpy(weights_out + (size_t)((iz * g.ny + iy) * g.nx + ix) * all, w.data(), sizeof(double) * all);
        const float inv_sum_w = light_pick_inv_sum_from_weights(w.data(), all);
        if (inv_sum_w != 0.0f) build_light_pick_from_weights(w.data(), all, (gsp_light_pick*)cellp);
        else std::memcpy(cellp, fallback, sizeof(gsp_light_pick) * (size_t)all);
        std::memcpy(cellp + sizeof(gsp_light_pick) * (size_t)all, &inv_sum_w, sizeof(float));
      }
}
}  // namespace gsp
