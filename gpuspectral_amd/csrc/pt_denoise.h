// pt_denoise.h -- the edge-avoiding a-trous denoiser (include/gpuspectral_pt.h, "Denoiser"): the per-pixel preparation, one tap of
// the dilated 5x5 stencil, the per-pixel finish, and the host-side resolution of a gsp_denoise into kernel constants.
//
// The GSP_HD functions compile for gfx950 (k_denoise_prepare / k_denoise_atrous, pt_render_kernels.inc) and for the host
// (tests/emu/denoise_emu.cpp): device and emulation are the same text.  All arithmetic is float32 in the order written; the file
// is compiled with -ffp-contract=off like the rest.
//
// A level works on three planes of 16 bytes per pixel:
//   E = {e.r, e.g, e.b, L}          the demodulated colour of this level's input and its luminance
//   A = {a'.r, a'.g, a'.b, valid}   the albedo with misses counted as 1; valid is 1.0f or 0.0f
//   G = {n.x, n.y, n.z, z}          the geom plane of the feature pass, as it is
// Only E changes from level to level.
#pragma once
#include <cmath>
#include <cstring>

#include "../../include/gpuspectral_pt.h"
#include "pt_display.h"
#include "pt_math.h"

namespace gsp {

constexpr uint32_t kDenoiseMaxIterations = 8;
constexpr uint32_t kDenoiseDefaultIterations = 5;
constexpr float kDenoiseSigmaColor = 0.5f, kDenoiseSigmaNormal = 0.3f, kDenoiseSigmaDepth = 0.05f, kDenoiseSigmaAlbedo = 0.1f;

// what a gsp_denoise comes to; passed to the kernels by value
struct DenoiseConsts {
  uint32_t iterations;                       // 1..8
  float inv_sc2, inv_sn2, inv_sz2, inv_sa2;  // 1 / sigma^2; 0 = the term is off
};

struct alignas(16) dn4 {
  float x, y, z, w;
};

struct DenoiseAcc {
  float w, r, g, b;  // sum_w, sum_k
};

// the B3-spline row {1, 4, 6, 4, 1} / 16; every product of two entries is exact in float32
GSP_HD float denoise_kernel(int d) { return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f); }

GSP_HD float denoise_floor_albedo(float a) { return a < 0.01f ? 0.01f : a; }  // A_k = max(a'_k, 0.01f)

// Prepare: c = the accumulate record, alb = {a.rgb, cov} -> E and A of level 0
GSP_HD void denoise_prepare(const dn4& c, const dn4& alb, dn4& E, dn4& A) {
  const bool valid = gisvalid(c.x) && gisvalid(c.y) && gisvalid(c.z);
  const float miss = 1.0f - alb.w;
  A.x = alb.x + miss;
  A.y = alb.y + miss;
  A.z = alb.z + miss;
  A.w = valid ? 1.0f : 0.0f;
  E.x = c.x / denoise_floor_albedo(A.x);
  E.y = c.y / denoise_floor_albedo(A.y);
  E.z = c.z / denoise_floor_albedo(A.z);
  E.w = display_luma(E.x, E.y, E.z);
}

// The guide differences of a tap: dn and da are squared distances, rz the relative depth difference
GSP_HD float denoise_dn(const dn4& Gp, const dn4& Gq) {
  const float nx = Gp.x - Gq.x, ny = Gp.y - Gq.y, nz = Gp.z - Gq.z;
  return (nx * nx + ny * ny) + nz * nz;
}
GSP_HD float denoise_rz(const dn4& Gp, const dn4& Gq) { return Gp.w == Gq.w ? 0.0f : (Gp.w - Gq.w) / (Gp.w + Gq.w); }
GSP_HD float denoise_da(const dn4& Ap, const dn4& Aq) {
  const float ar = Ap.x - Aq.x, ag = Ap.y - Aq.y, ab = Ap.z - Aq.z;
  return (ar * ar + ag * ag) + ab * ab;
}

// One tap q of centre p (both inside the frame; the centre is valid).  h = k[dx+2] * k[dy+2]; inv_sc2_level = inv_sc2 * 4^level.
// An invalid q adds nothing.
GSP_HD void denoise_tap(const DenoiseConsts& k, float inv_sc2_level, float h, const dn4& Ep, const dn4& Ap, const dn4& Gp, const dn4& Eq,
                        const dn4& Aq, const dn4& Gq, DenoiseAcc& acc) {
  if (Aq.w == 0.0f) return;
  const float dn = denoise_dn(Gp, Gq);
  const float rz = denoise_rz(Gp, Gq);
  const float da = denoise_da(Ap, Aq);
  const float rl = (Ep.w - Eq.w) / ((Ep.w + Eq.w) + 1e-3f);
  const float x = ((dn * k.inv_sn2 + rz * rz * k.inv_sz2) + da * k.inv_sa2) + (rl * rl) * inv_sc2_level;
  const float w = h * det_expf(-x);
  acc.w += w;
  acc.r += w * Eq.x;
  acc.g += w * Eq.y;
  acc.b += w * Eq.z;
}

// the level's output for a valid centre: e' = sum_k / sum_w and its luminance
GSP_HD dn4 denoise_level_result(const DenoiseAcc& acc) {
  dn4 o;
  o.x = acc.r / acc.w;
  o.y = acc.g / acc.w;
  o.z = acc.b / acc.w;
  o.w = display_luma(o.x, o.y, o.z);
  return o;
}

// Output: the remodulated colour of a valid pixel, the accumulate record itself (bit for bit) of an invalid one; out.w = c.w
GSP_HD dn4 denoise_finish(const dn4& E, const dn4& A, const dn4& c) {
  if (A.w == 0.0f) return c;
  dn4 o;
  o.x = E.x * denoise_floor_albedo(A.x);
  o.y = E.y * denoise_floor_albedo(A.y);
  o.z = E.z * denoise_floor_albedo(A.z);
  o.w = c.w;
  return o;
}

// One centre pixel of one level by a plain loop over fetch(x, y, E, A, G) -- what the emulation runs, and the order of summation
// the kernels follow: dy outer, dx inner, a tap outside the frame skipped.
template <class FETCH>
GSP_HD dn4 denoise_pixel_level(const DenoiseConsts& k, uint32_t level, int width, int height, int px, int py, FETCH fetch) {
  dn4 Ep, Ap, Gp;
  fetch(px, py, Ep, Ap, Gp);
  if (Ap.w == 0.0f) return Ep;
  const int s = 1 << level;
  const float c2 = k.inv_sc2 * (float)(1u << (2u * level));
  DenoiseAcc acc = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int dy = -2; dy <= 2; ++dy) {
    const int y = py + s * dy;
    if (y < 0 || y >= height) continue;
    for (int dx = -2; dx <= 2; ++dx) {
      const int x = px + s * dx;
      if (x < 0 || x >= width) continue;
      dn4 Eq, Aq, Gq;
      fetch(x, y, Eq, Aq, Gq);
      denoise_tap(k, c2, denoise_kernel(dx) * denoise_kernel(dy), Ep, Ap, Gp, Eq, Aq, Gq, acc);
    }
  }
  return denoise_level_result(acc);
}

// ---- host side: validation and constants (formed in double, rounded to float once) ----

// The host's struct under the struct_size rule (fields it does not have are 0; NULL and struct_size 0 = the zeroed struct = all
// defaults), validated as the header says.  Returns nullptr and the constants in `out`, or the text for gsp_last_error.
inline const char* resolve_denoise(const gsp_denoise* host, DenoiseConsts& out) {
  gsp_denoise d;
  std::memset(&d, 0, sizeof(d));
  if (host) std::memcpy(&d, host, host->struct_size < sizeof(d) ? host->struct_size : sizeof(d));
  if (d.iterations > kDenoiseMaxIterations) return "gsp_denoise.iterations must be 0 (the default, 5) or within 1 .. 8";
  if (!(d.sigma_color >= 0.0f)) return "gsp_denoise.sigma_color must be 0 (the default), positive or +Inf (the term is off)";
  if (!(d.sigma_normal >= 0.0f)) return "gsp_denoise.sigma_normal must be 0 (the default), positive or +Inf (the term is off)";
  if (!(d.sigma_depth >= 0.0f)) return "gsp_denoise.sigma_depth must be 0 (the default), positive or +Inf (the term is off)";
  if (!(d.sigma_albedo >= 0.0f)) return "gsp_denoise.sigma_albedo must be 0 (the default), positive or +Inf (the term is off)";
  const auto inv2 = [](float sigma, float dflt) {
    const double s = sigma == 0.0f ? (double)dflt : (double)sigma;
    if (std::isinf(s)) return 0.0f;
    const double v = 1.0 / (s * s);
    return v > 3.402823466e+38 ? 3.402823466e+38f : (float)v;  // (a finite constant: the centre tap's 0 * inv stays 0)
  };
  out.iterations = d.iterations ? d.iterations : kDenoiseDefaultIterations;
  out.inv_sc2 = inv2(d.sigma_color, kDenoiseSigmaColor);
  out.inv_sn2 = inv2(d.sigma_normal, kDenoiseSigmaNormal);
  out.inv_sz2 = inv2(d.sigma_depth, kDenoiseSigmaDepth);
  out.inv_sa2 = inv2(d.sigma_albedo, kDenoiseSigmaAlbedo);
  return nullptr;
}

}  // namespace gsp
