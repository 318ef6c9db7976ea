// pt_medium.h -- scattering interior media (include/gpuspectral_pt.h, "Scattering media"): the Henyey-Greenstein phase function
// and the free-path decision of a segment that ran inside a scattering medium.  Small GSP_HD functions, each callable on its
// own (tests/devfn); shade_vertex<.., SCT = true> (pt_stages.h) is their one caller in the product.  Every expression is written
// in the order the header fixes, log / exp / sin / cos are the deterministic ones of pt_math.h.
#pragma once
#include "pt_shading.h"

namespace gsp {

// below this |g| the phase function is the isotropic one (the inverse CDF of HG divides by 2 g)
constexpr float kHgIsotropic = 1e-3f;

// Henyey-Greenstein, normalised over the sphere.  cos_theta = dot(direction the light travelled before, direction after): g > 0
// scatters forward
GSP_HD float hg_pdf(float g, float cos_theta) {
  if (gabs(g) < kHgIsotropic) return 1.0f / (4.0f * kPi);
  const float d = (1.0f + g * g) - (2.0f * g) * cos_theta;
  return (1.0f - g * g) / ((4.0f * kPi) * (d * gsqrt(d)));
}

// cos(theta) of the HG sample for u1: the inverse CDF, clamped to [-1, 1]
GSP_HD float hg_cos(float g, float u1) {
  if (gabs(g) < kHgIsotropic) return 1.0f - 2.0f * u1;
  const float sq = (1.0f - g * g) / ((1.0f - g) + (2.0f * g) * u1);
  return gclamp(((1.0f + g * g) - sq * sq) / (2.0f * g), -1.0f, 1.0f);
}

// a direction about the unit vector d (the frame of make_frame(d)), theta from u1, phi = 2 pi u2.  pdf = hg_pdf of it
GSP_HD f3 sample_hg(f3 d, float g, float u1, float u2, float& pdf) {
  const float ct = hg_cos(g, u1);
  const float st = gsqrt(gmax(0.0f, 1.0f - ct * ct));
  float sp, cp;
  det_sincosf((2.0f * kPi) * u2, sp, cp);
  pdf = hg_pdf(g, ct);
  return to_world(make_frame(d), mk3(st * cp, st * sp, ct));
}

// the channel whose sigma_t draws the free path
GSP_HD uint32_t medium_channel(float u_c) {
  const uint32_t c = (uint32_t)(u_c * 3.0f);
  return c < 2u ? c : 2u;
}

// the free path of u_d under sigma_t of the chosen channel; sigma_t == 0 never collides (+inf: the surface)
GSP_HD float medium_free_path(float sigma_t, float u_d) {
  if (sigma_t == 0.0f) return u2f(0x7f800000u);
  return -det_logf(1.0f - u_d) / sigma_t;
}

struct MediumEvent {
  bool scatter;  // a medium event at distance s (else the surface at t)
  bool valid;    // p is finite and not 0 (else the path ends)
  float s;
  f3 w;  // the path weight behind the event
};

// The decision over a segment of length t inside a medium (sigma_a, sigma_s): channel by u_c, free path by u_d, then the weight
// of the event against the density of the decision averaged over the three channels (the one-sample estimator over channels)
GSP_HD MediumEvent medium_event(f3 sigma_a, f3 sigma_s, float t, float u_c, float u_d, f3 weight) {
  const f3 sigma_t = sigma_a + sigma_s;
  const uint32_t c = medium_channel(u_c);
  MediumEvent ev;
  ev.s = medium_free_path(c == 0u ? sigma_t.x : (c == 1u ? sigma_t.y : sigma_t.z), u_d);
  ev.scatter = ev.s < t;
  float p;
  if (ev.scatter) {
    const f3 Tr = mk3(det_expf(-(sigma_t.x * ev.s)), det_expf(-(sigma_t.y * ev.s)), det_expf(-(sigma_t.z * ev.s)));
    p = ((sigma_t.x * Tr.x + sigma_t.y * Tr.y) + sigma_t.z * Tr.z) / 3.0f;
    ev.w = ((weight * sigma_s) * Tr) / p;
  } else {
    const f3 Tr = mk3(det_expf(-(sigma_t.x * t)), det_expf(-(sigma_t.y * t)), det_expf(-(sigma_t.z * t)));
    p = ((Tr.x + Tr.y) + Tr.z) / 3.0f;
    ev.w = (weight * Tr) / p;
  }
  ev.valid = gisvalid(p) && p != 0.0f;
  return ev;
}

}  // namespace gsp
