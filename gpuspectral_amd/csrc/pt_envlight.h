// pt_envlight.h -- the environment map as a light (include/gpuspectral_pt.h, "Environment light"): the record behind the delta
// records of the light table, the ONE function that gives radiance and solid-angle density of a world direction, and the sampler
// that inverts sample_envmap's mapping.  Small GSP_HD functions, each callable on its own (tests/devfn); shade_vertex<.., ENV = true>
// and miss_emitted_env (pt_stages.h) are their callers in the product.  Every expression is written in the order the header states,
// so the host compile (tests/emu/envlight_emu.cpp) and the device agree bit for bit.  The host side (validation, the cell weights,
// the record) is plain C++ at the end of the file: the library (pt_render_scene.inc) and the emulation build the same bytes.
#pragma once
#include <cmath>
#include <vector>

#include "../../include/gpuspectral_pt.h"
#include "pt_math.h"
#include "pt_shading.h"

namespace gsp {

// the record of kind GSP_LIGHT_ENVIRONMENT: 64 B like every light record, the kind word where gsp_delta_light has it
struct EnvLightRecord {
  float row0[3];   // local -> world, row by row (the inverse of the upper 3x3 of envmap.to_local)
  uint32_t kind;   // GSP_LIGHT_ENVIRONMENT
  float row1[3];
  float p_sel;     // the selection probability the light table of the context's mode implies for this record
  float row2[3];
  uint32_t cw;     // cells in u: min(width, 512)
  uint32_t ch;     // cells in v: min(height, 256)
  float reserved[3];
};
static_assert(sizeof(EnvLightRecord) == sizeof(gsp_triangle_light), "the environment record sits behind the delta records, in the same array");
constexpr uint32_t kEnvCellsU = 512u, kEnvCellsV = 256u;

struct EnvEval {
  f3 radiance;
  float density;  // solid angle, of the cell table alone (the caller multiplies by p_sel); 0 at the poles
  uint32_t cell;
};

// cell coordinate of a map coordinate t in [0, 1]: (uint32)clamp(t * n, 0, n - 1), NaN -> 0
GSP_HD uint32_t env_cell_coord(float t, uint32_t n) {
  float f = t * (float)n;
  if (!(f >= 0.0f)) f = 0.0f;
  if (f > (float)(n - 1u)) f = (float)(n - 1u);
  return (uint32_t)f;
}

// radiance and density of world direction d.  `cells` = the cell table (cw * ch entries; pmf(cell) = pmf_self of its entry)
GSP_HD EnvEval env_eval(const TextureView& T, const gsp_light_pick* cells, uint32_t cw, uint32_t ch, f3 d) {
  EnvEval r;
  const f3 e = xform_dir(T.env_to_local, d);
  const float kInv2Pi = 0.15915494309189533577f, kInvPi = 0.31830988618379067154f;
  const float s = gsqrt(e.x * e.x + e.z * e.z);
  const float u = det_atan2f(e.x, -e.z) * kInv2Pi + 0.5f;
  const float v = 1.0f - det_atan2f(s, e.y) * kInvPi;
  // the cell first: its entry is the one fetch of this function that depends on nothing but (u, v)
  r.cell = env_cell_coord(v, ch) * cw + env_cell_coord(u, cw);
  const float pmf = ((const LightPickQuad*)cells)[r.cell].pmf_self;
  const int32_t w = (int32_t)T.env_width, h = (int32_t)T.env_height;
  const float x = texel_coord(u, T.env_width), y = texel_coord(v, T.env_height);
  const float fx = __builtin_floorf(x), fy = __builtin_floorf(y);
  const int32_t x0 = wrap_index((int32_t)fx, w);
  const int32_t x1 = x0 + 1 == w ? 0 : x0 + 1;
  int32_t y0 = (int32_t)fy, y1 = y0 + 1;
  y0 = y0 < 0 ? 0 : (y0 > h - 1 ? h - 1 : y0);
  y1 = y1 < 0 ? 0 : (y1 > h - 1 ? h - 1 : y1);
  const float* p = T.env_texels;
  const f3 c00 = ld3(p + 4 * ((int64_t)y0 * w + x0)), c10 = ld3(p + 4 * ((int64_t)y0 * w + x1));
  const f3 c01 = ld3(p + 4 * ((int64_t)y1 * w + x0)), c11 = ld3(p + 4 * ((int64_t)y1 * w + x1));
  r.radiance = lerp4(c00, c10, c01, c11, x - fx, y - fy);
  r.density = s > 0.0f ? ((pmf * (float)cw) * (float)ch) / (19.739208802178716f * s) : 0.0f;
  return r;
}

// the world direction of cell c and the variates (e1, e2) inside it
GSP_HD f3 env_cell_direction(const EnvLightRecord& rec, uint32_t c, float e1, float e2) {
  const float u = ((float)(c % rec.cw) + e1) / (float)rec.cw;
  const float v = ((float)(c / rec.cw) + e2) / (float)rec.ch;
  const float theta = (1.0f - v) * kPi;
  const float phi = (u - 0.5f) * (2.0f * kPi);
  float st, ct, sp, cp;
  det_sincosf(theta, st, ct);
  det_sincosf(phi, sp, cp);
  const f3 e = mk3(st * sp, ct, -(st * cp));
  return mk3((rec.row0[0] * e.x + rec.row0[1] * e.y) + rec.row0[2] * e.z, (rec.row1[0] * e.x + rec.row1[1] * e.y) + rec.row1[2] * e.z,
             (rec.row2[0] * e.x + rec.row2[1] * e.y) + rec.row2[2] * e.z);
}

struct EnvSample {
  f3 L;         // world, from the shading point towards the sky
  f3 emission;  // the map's radiance along L
  float pdf;    // density * p_sel; 0: no shadow ray
  uint32_t cell_picked, cell_of_L;
};
// r2 = the one further draw of an environment pick; (e1, e2) the vertex's two variates
GSP_HD EnvSample sample_env_light(const TextureView& T, const gsp_light_pick* cells, const EnvLightRecord& rec, uint32_t r2, float e1, float e2) {
  EnvSample es;
  float pmf_unused;
  es.cell_picked = light_pick_index(cells, rec.cw * rec.ch, r2, pmf_unused);
  es.L = env_cell_direction(rec, es.cell_picked, e1, e2);
  const EnvEval ev = env_eval(T, cells, rec.cw, rec.ch, es.L);  // the density of the direction as BUILT: what the escape side computes for it
  es.emission = ev.radiance;
  es.pdf = ev.density * rec.p_sel;
  es.cell_of_L = ev.cell;
  return es;
}
}  // namespace gsp

// ---- host side: validation, the cell weights, the power weight, the record ---------------------------------------------------
namespace gsp {

// nullptr = acceptable; else what is wrong
inline const char* check_envmap_sampling(const gsp_envmap_sampling* s) {
  if (!s || s->enabled == 0u) return nullptr;
  if (!(s->extent > 0.0f) || !std::isfinite(s->extent)) return "gsp_envmap_sampling.extent must be finite and > 0";
  if (s->reserved[0] != 0u || s->reserved[1] != 0u) return "gsp_envmap_sampling.reserved must be 0";
  return nullptr;
}

// the upper 3x3 A of to_local (glm memory order: A[r][c] = m[4 c + r]) is a rotation: every entry of A^T A - I within 1e-4, in double
inline bool env_frame_is_rotation(const float* m) {
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      double dotp = 0.0;
      for (int r = 0; r < 3; ++r) dotp += (double)m[4 * a + r] * (double)m[4 * b + r];
      if (!(std::fabs(dotp - (a == b ? 1.0 : 0.0)) <= 1e-4)) return false;
    }
  return true;
}
// A^-1, cofactors over the determinant in double, rounded to float32 once; out[r][c]
inline void env_local_to_world(const float* m, float out[3][3]) {
  double A[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) A[r][c] = (double)m[4 * c + r];
  const double det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
                     A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;  // cofactor of A[c][r]
      out[r][c] = (float)((A[r1][c1] * A[r2][c2] - A[r1][c2] * A[r2][c1]) / det);
    }
}

inline double env_texel_y(const float* texels, uint32_t width, uint32_t x, uint32_t y) {
  const float* t = texels + 4 * ((size_t)y * width + x);
  const double Y = 0.2126 * (double)t[0] + 0.7152 * (double)t[1] + 0.0722 * (double)t[2];
  return (std::isfinite(Y) && Y > 0.0) ? Y : 0.0;
}

// The weights of the cw * ch cells: sin(theta of the cell's centre row) * max Y over every texel the bilinear lookup can read for a
// (u, v) inside the cell (wrap in u, clamp in v).  The column maxima are formed first (one pass over the map per cell column range).
inline std::vector<double> env_cell_weights(const float* texels, uint32_t width, uint32_t height, uint32_t& cw, uint32_t& ch) {
  const double pi = 3.14159265358979323846;
  cw = width < kEnvCellsU ? width : kEnvCellsU;
  ch = height < kEnvCellsV ? height : kEnvCellsV;
  const double eps_u = (double)width / 2097152.0, eps_v = (double)height / 2097152.0;
  // rowmax[y * cw + i] = max Y over the columns cell column i can read, in row y
  std::vector<double> rowmax((size_t)height * cw, 0.0);
  for (uint32_t i = 0; i < cw; ++i) {
    const long long lo = (long long)std::floor((double)i * width / cw - 0.5 - eps_u);
    const long long hi = (long long)std::floor((double)(i + 1u) * width / cw - 0.5 + eps_u) + 1;
    for (uint32_t y = 0; y < height; ++y) {
      double m = 0.0;
      for (long long x = lo; x <= hi && x < lo + (long long)width; ++x) {
        const uint32_t xw = (uint32_t)(((x % (long long)width) + (long long)width) % (long long)width);
        const double Y = env_texel_y(texels, width, xw, y);
        m = Y > m ? Y : m;
      }
      rowmax[(size_t)y * cw + i] = m;
    }
  }
  std::vector<double> w((size_t)cw * ch, 0.0);
  for (uint32_t j = 0; j < ch; ++j) {
    long long lo = (long long)std::floor((double)j * height / ch - 0.5 - eps_v);
    long long hi = (long long)std::floor((double)(j + 1u) * height / ch - 0.5 + eps_v) + 1;
    lo = lo < 0 ? 0 : lo;
    hi = hi > (long long)height - 1 ? (long long)height - 1 : hi;
    const double sn = std::sin(pi * ((double)j + 0.5) / (double)ch);
    for (uint32_t i = 0; i < cw; ++i) {
      double m = 0.0;
      for (long long y = lo; y <= hi; ++y) m = rowmax[(size_t)y * cw + i] > m ? rowmax[(size_t)y * cw + i] : m;
      w[(size_t)j * cw + i] = sn * m;
    }
  }
  return w;
}

// the weight of the record under GSP_LIGHTS_POWER: pi extent^2 * sum over texels of Y * solid angle, rows and columns ascending
inline double env_radiant_sum(const float* texels, uint32_t width, uint32_t height) {
  const double pi = 3.14159265358979323846;
  double sum = 0.0;
  for (uint32_t y = 0; y < height; ++y) {
    const double sa = (2.0 * pi / (double)width) * (pi / (double)height) * std::sin(pi * ((double)y + 0.5) / (double)height);
    for (uint32_t x = 0; x < width; ++x) sum += env_texel_y(texels, width, x, y) * sa;
  }
  return sum;
}
inline double env_power_weight(double radiant_sum, float extent) {
  const double w = 3.14159265358979323846 * ((double)extent * (double)extent) * radiant_sum;
  return std::isfinite(w) ? w : 0.0;
}

inline EnvLightRecord make_env_record(const float* to_local, uint32_t cw, uint32_t ch, float p_sel) {
  EnvLightRecord r{};
  float R[3][3];
  env_local_to_world(to_local, R);
  for (int c = 0; c < 3; ++c) r.row0[c] = R[0][c], r.row1[c] = R[1][c], r.row2[c] = R[2][c];
  r.kind = GSP_LIGHT_ENVIRONMENT;
  r.p_sel = p_sel;
  r.cw = cw;
  r.ch = ch;
  return r;
}
}  // namespace gsp
