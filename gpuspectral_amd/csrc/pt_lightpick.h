// Light selection by emitted power (include/gpuspectral_pt.h, "Light selection"): the HOST builder of the alias table that sits
// behind the light records of a GSP_LIGHTS_POWER context.  Plain C++, no HIP: the library (pt_render_scene.inc pack_tables) and
// the tests' host emulation (tests/emu/lights_emu.cpp) include this one file, so both hold the same bytes for the same records.
// The pick that reads the table is device code: sample_light_power, pt_shading.h.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/gpuspectral_pt.h"
#include "pt_deltalight.h"

namespace gsp {

// w_i = max(Y(radiance), 0) * area, in double, from the caller's (unbaked) record; a non-finite weight counts as 0
inline double light_pick_weight(const gsp_triangle_light& L) {
  const double y = 0.2126 * (double)L.radiance[0] + 0.7152 * (double)L.radiance[1] + 0.0722 * (double)L.radiance[2];
  double a[3], b[3];
  for (int c = 0; c < 3; ++c) {
    a[c] = (double)L.positions[2][c] - (double)L.positions[0][c];  // v2 - v0
    b[c] = (double)L.positions[1][c] - (double)L.positions[0][c];  // v1 - v0
  }
  const double cx = a[1] * b[2] - a[2] * b[1], cy = a[2] * b[0] - a[0] * b[2], cz = a[0] * b[1] - a[1] * b[0];
  const double w = (y > 0.0 ? y : 0.0) * (0.5 * std::sqrt(cx * cx + cy * cy + cz * cz));
  return std::isfinite(w) ? w : 0.0;
}

// ... and of an accepted delta record: the power it emits into the scene, with Y of its intensity (a directional light: through the
// disc of radius `extent` that faces it)
inline double light_pick_weight(const gsp_delta_light& L) {
  const double pi = 3.14159265358979323846;
  const double y0 = 0.2126 * (double)L.intensity[0] + 0.7152 * (double)L.intensity[1] + 0.0722 * (double)L.intensity[2];
  const double y = y0 > 0.0 ? y0 : 0.0;
  double w = 0.0;
  if (L.kind == GSP_LIGHT_POINT) w = 4.0 * pi * y;
  else if (L.kind == GSP_LIGHT_SPOT) w = 2.0 * pi * (1.0 - ((double)L.cos_beam + (double)L.cos_cutoff) / 2.0) * y;
  else if (L.kind == GSP_LIGHT_DIRECTIONAL) w = pi * ((double)L.extent * (double)L.extent) * y;
  return std::isfinite(w) ? w : 0.0;
}

// Vose's alias construction over weights w[0..n) -> out[0..n).  Deterministic: both work lists are filled in ascending index
// and consumed from the front; an entry that turns from large to small or stays large is appended at the back of its list.
// Weights that are not finite or not positive count as 0; if every weight is 0, every weight becomes 1.
inline void build_light_pick_from_weights(const double* w_in, uint32_t n, gsp_light_pick* out) {
  if (n == 0) return;
  std::vector<double> s(n);
  double sum = 0.0;
  for (uint32_t i = 0; i < n; ++i) {
    s[i] = (std::isfinite(w_in[i]) && w_in[i] > 0.0) ? w_in[i] : 0.0;
    sum += s[i];
  }
  if (!(sum > 0.0) || !std::isfinite(sum)) {
    // (all zero -- or a sum beyond double: scaled down first, and all ones if that does not help)
    double big = 0.0;
    for (uint32_t i = 0; i < n; ++i) big = s[i] > big ? s[i] : big;
    sum = 0.0;
    for (uint32_t i = 0; i < n; ++i) {
      s[i] = big > 0.0 ? s[i] / big : 1.0;
      sum += s[i];
    }
  }
  for (uint32_t i = 0; i < n; ++i) s[i] = s[i] * (double)n / sum;
  std::vector<uint32_t> small, large, alias(n);
  small.reserve(n);
  large.reserve(n);
  for (uint32_t i = 0; i < n; ++i) {
    alias[i] = i;
    (s[i] < 1.0 ? small : large).push_back(i);
  }
  std::vector<double> self(n, 1.0);  // s'_j: the share of slot j that stays with j
  size_t si = 0, li = 0;
  while (si < small.size() && li < large.size()) {
    const uint32_t a = small[si++], g = large[li];
    self[a] = s[a];
    alias[a] = g;
    s[g] = (s[g] + s[a]) - 1.0;
    if (s[g] < 1.0) {
      ++li;
      small.push_back(g);
    }
  }
  // (what is left on either list is 1 up to rounding: always self)
  const double two32 = 4294967296.0;
  std::vector<double> T(n);
  for (uint32_t j = 0; j < n; ++j) {
    double t = std::floor(self[j] * two32 + 0.5);  // round(s'_j * 2^32)
    if (!(t >= 0.0)) t = 0.0;
    if (t >= 4294967295.0 || alias[j] == j) {  // saturated: always self
      out[j].threshold = 0xffffffffu;
      out[j].alias = j;
      T[j] = two32;
    } else {
      out[j].threshold = (uint32_t)t;
      out[j].alias = alias[j];
      T[j] = t;
    }
  }
  // the probability the integer table implies: p_i = (T_i + sum over j aliased to i of (2^32 - T_j)) / (n * 2^32)
  std::vector<double> mass(T);
  for (uint32_t j = 0; j < n; ++j)
    if (out[j].alias != j) mass[out[j].alias] += two32 - T[j];
  for (uint32_t j = 0; j < n; ++j) {
    out[j].pmf_self = (float)(mass[j] / ((double)n * two32));
    out[j].pmf_alias = (float)(mass[out[j].alias] / ((double)n * two32));
  }
}

// What follows the light records in the table image: the alias table (GSP_LIGHTS_POWER with at least one light), and behind it the
// one trailing record {inv_sum_w, 0, 0, 0} when the context ALSO runs GSP_ESTIMATOR_TEXTBOOK.  Every other combination of the two
// modes keeps the image it had before the estimator mode existed.
inline size_t light_pick_table_bytes(uint32_t n, uint32_t light_mode) { return light_mode == GSP_LIGHTS_POWER ? sizeof(gsp_light_pick) * (size_t)n : 0; }
inline size_t light_pick_tail_bytes(uint32_t n, uint32_t light_mode, uint32_t estimator) {
  return light_pick_table_bytes(n, light_mode) != 0 && estimator == GSP_ESTIMATOR_TEXTBOOK ? 16 : 0;
}

// GSP_ESTIMATOR_TEXTBOOK under GSP_LIGHTS_POWER (include/gpuspectral_pt.h, "Estimator"): the float32 rounding of 1 / sum(w), the sum
// formed as above (the same weights, in double, in ascending index).  0 when every weight was 0 (the table fell back to uniform:
// the selection probability of a light that is hit is then 1 / n), and when the sum or its reciprocal is beyond the format
inline float light_pick_inv_sum_from_weights(const double* w_in, uint32_t n) {
  double sum = 0.0;
  for (uint32_t i = 0; i < n; ++i) sum += (std::isfinite(w_in[i]) && w_in[i] > 0.0) ? w_in[i] : 0.0;
  if (!(sum > 0.0) || !std::isfinite(sum)) return 0.0f;
  const float r = (float)(1.0 / sum);
  return std::isfinite(r) ? r : 0.0f;
}
// the weights of a light table: the n triangle lights, then the nd delta lights behind them (include/gpuspectral_pt.h, "Delta lights"),
// then the environment record's (env_w, "Environment light"; null = the table has none)
inline std::vector<double> light_pick_weights(const gsp_triangle_light* lights, uint32_t n, const gsp_delta_light* delta, uint32_t nd, const double* env_w = nullptr) {
  std::vector<double> w((size_t)n + nd + (env_w ? 1u : 0u));
  for (uint32_t i = 0; i < n; ++i) w[i] = light_pick_weight(lights[i]);
  for (uint32_t i = 0; i < nd; ++i) w[(size_t)n + i] = light_pick_weight(delta[i]);
  if (env_w) w[(size_t)n + nd] = *env_w;
  return w;
}
inline float light_pick_inv_sum(const gsp_triangle_light* lights, uint32_t n, const gsp_delta_light* delta = nullptr, uint32_t nd = 0, const double* env_w = nullptr) {
  const std::vector<double> w = light_pick_weights(lights, n, delta, nd, env_w);
  return light_pick_inv_sum_from_weights(w.data(), (uint32_t)w.size());
}

inline void build_light_pick(const gsp_triangle_light* lights, uint32_t n, const gsp_delta_light* delta, uint32_t nd, gsp_light_pick* out, const double* env_w = nullptr) {
  const std::vector<double> w = light_pick_weights(lights, n, delta, nd, env_w);
  build_light_pick_from_weights(w.data(), (uint32_t)w.size(), out);
}
inline void build_light_pick(const gsp_triangle_light* lights, uint32_t n, gsp_light_pick* out) { build_light_pick(lights, n, nullptr, 0, out); }

}  // namespace gsp
