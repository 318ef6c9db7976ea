// pt_deltalight.h -- point, spot and directional emitters (include/gpuspectral_pt.h, "Delta lights"): the light sample of a record
// of the delta-light table.  Small GSP_HD functions, each callable on its own (tests/devfn); shade_vertex<.., DLT = true>
// (pt_stages.h) is their one caller in the product.  Every expression is written in the order the header states, so the host
// compile (tests/emu/delta_emu.cpp) and the device agree bit for bit.
#pragma once
#include "../../include/gpuspectral_pt.h"
#include "pt_math.h"

namespace gsp {

static_assert(sizeof(gsp_delta_light) == sizeof(gsp_triangle_light), "delta records sit behind the triangle lights, in the same array");

// the smoothstep of the cosine c between the cutoff (0) and the beam (1); cos_beam > cos_cutoff (gsp_set_delta_lights)
GSP_HD float spot_falloff(float c, float cos_cutoff, float cos_beam) {
  const float t = gclamp((c - cos_cutoff) / (cos_beam - cos_cutoff), 0.0f, 1.0f);
  return (t * t) * (3.0f - 2.0f * t);
}

struct DeltaSample {
  f3 L;          // unit, from the shading point to the light
  float Ldist;   // 1e30f for a directional light
  f3 emission;
  float pdf;     // 0: no shadow ray
};

// `rec` = a record as gsp_set_delta_lights accepted it (direction unit), pos = the shading point, pmf = the probability of the pick
GSP_HD DeltaSample sample_delta_light(const gsp_delta_light& rec, f3 pos, float pmf) {
  DeltaSample ds;
  const f3 intensity = mk3(rec.intensity[0], rec.intensity[1], rec.intensity[2]);
  const f3 direction = mk3(rec.direction[0], rec.direction[1], rec.direction[2]);
  if (rec.kind == GSP_LIGHT_DIRECTIONAL) {
    ds.L = -direction;
    ds.Ldist = 1e30f;
    ds.emission = intensity;
    ds.pdf = pmf;
    return ds;
  }
  const f3 toL = mk3(rec.position[0], rec.position[1], rec.position[2]) - pos;
  const float d2 = dot(toL, toL);
  if (d2 == 0.0f) {
    ds.L = mk3(0.0f, 0.0f, 1.0f);
    ds.Ldist = 0.0f;
    ds.emission = intensity;
    ds.pdf = 0.0f;
    return ds;
  }
  ds.Ldist = gsqrt(d2);
  ds.L = toL / ds.Ldist;
  ds.emission = intensity;
  if (rec.kind == GSP_LIGHT_SPOT) ds.emission = intensity * spot_falloff(dot(direction, -ds.L), rec.cos_cutoff, rec.cos_beam);
  ds.pdf = d2 * pmf;
  return ds;
}

// ---- host side of gsp_set_delta_lights: validation and the accepted record -------------------------------------------------
// nullptr = acceptable; else what is wrong (the first finding)
inline const char* check_delta_lights(const gsp_delta_light* lights, uint32_t n) {
  if (!lights || n == 0u) return nullptr;
  for (uint32_t k = 0; k < n; ++k) {
    const gsp_delta_light& l = lights[k];
    if (l.kind != GSP_LIGHT_POINT && l.kind != GSP_LIGHT_SPOT && l.kind != GSP_LIGHT_DIRECTIONAL) return "gsp_delta_light.kind must be GSP_LIGHT_POINT, _SPOT or _DIRECTIONAL";
    const float all[] = {l.position[0], l.position[1], l.position[2], l.direction[0], l.direction[1], l.direction[2], l.cos_cutoff,
                         l.intensity[0], l.intensity[1], l.intensity[2], l.cos_beam, l.extent, l.reserved[0], l.reserved[1], l.reserved[2]};
    for (float v : all)
      if (!gisvalid(v)) return "gsp_delta_light: every field must be finite";
    for (int c = 0; c < 3; ++c)
      if (l.intensity[c] < 0.0f) return "gsp_delta_light.intensity must be >= 0";
    for (int c = 0; c < 3; ++c)
      if (f2u(l.reserved[c]) != 0u) return "gsp_delta_light.reserved must be 0";
    if (l.kind != GSP_LIGHT_POINT) {
      const double x = l.direction[0], y = l.direction[1], z = l.direction[2];
      const double len = __builtin_sqrt(x * x + y * y + z * z);
      if (!(__builtin_fabs(len - 1.0) <= 1e-3)) return "gsp_delta_light.direction must be a unit vector (within 1e-3)";
    }
    if (l.kind == GSP_LIGHT_SPOT && !(l.cos_beam > l.cos_cutoff)) return "gsp_delta_light: a spot needs cos_beam > cos_cutoff";
    if (l.kind == GSP_LIGHT_DIRECTIONAL && !(l.extent > 0.0f)) return "gsp_delta_light: a directional light needs extent > 0";
  }
  return nullptr;
}
// the record the library keeps and the device reads: the direction of a spot / directional light renormalised in double
inline gsp_delta_light accept_delta_light(gsp_delta_light l) {
  if (l.kind != GSP_LIGHT_POINT) {
    const double x = l.direction[0], y = l.direction[1], z = l.direction[2];
    const double len = __builtin_sqrt(x * x + y * y + z * z);
    l.direction[0] = (float)(x / len);
    l.direction[1] = (float)(y / len);
    l.direction[2] = (float)(z / len);
  }
  return l;
}
}  // namespace gsp
