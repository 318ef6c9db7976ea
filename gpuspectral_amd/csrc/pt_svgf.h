// pt_svgf.h -- the variance-guided filter (include/gpuspectral_pt.h, "Variance-guided filter"): the luminance moments kept beside
// the temporal history, the per-pixel initial variance, one level of the a-trous filter whose luminance edge-stop is scaled by the
// local standard deviation, and the host-side resolution of a gsp_svgf into kernel constants.
//
// The GSP_HD functions compile for gfx950 (k_temporal_reproject_moments / k_svgf_variance / k_svgf_atrous, pt_render_kernels.inc)
// and for the host (tests/emu/svgf_emu.cpp): device and emulation are the same text.  All arithmetic is float32 in the order
// written; the file is compiled with -ffp-contract=off like the rest.
//
// Beside the denoiser's planes E, A, G (pt_denoise.h) and the history H, G, I (pt_temporal.h) there are
//   M = {m1, m2, r, 0}   16 bytes; the blended first and second luminance moments of the history and the sum of its squared
//                        frame weights
//   V                    4 bytes; the variance of a level's input luminance
#pragma once
#include <cmath>
#include <cstring>

#include "../../include/gpuspectral_pt.h"
#include "pt_denoise.h"
#include "pt_math.h"
#include "pt_temporal.h"

namespace gsp {

constexpr uint32_t kSvgfMinHistory = 4, kSvgfMinHistoryLimit = 65536;
constexpr float kSvgfSigmaVariance = 4.0f;
constexpr int kSvgfVarianceRadius = 3;  // the spatial estimate looks at 7 x 7 pixels

// what a gsp_denoise + gsp_svgf come to; passed to the kernels by value
struct SvgfConsts {
  uint32_t iterations;              // 1..8
  float inv_sn2, inv_sz2, inv_sa2;  // 1 / sigma^2 of the denoiser's guides; 0 = the term is off
  float min_history;                // 2 .. 65536, an exact float
  float sigma_v;                    // sigma_variance; not read when lum_on == 0
  uint32_t lum_on;                  // 0: sigma_variance is +Inf, inv_l = 0
};

struct SvgfAcc {
  float w, r, g, b, v;  // sum_w, sum_k, sum_v
};

struct SvgfLevelOut {
  dn4 E;
  float V;
};

struct TemporalMomentsOut {
  TemporalOut t;
  dn4 M;
};

GSP_HD float svgf_clamp0(float x) { return x > 0.0f ? x : 0.0f; }  // max(x, 0); a NaN gives 0

// ---- moments beside the history --------------------------------------------------------------------------------------------
// l = the luminance of the frame's demodulated colour: L of "Denoiser: Prepare" on (c, alb)
GSP_HD float svgf_frame_luminance(const dn4& c, const dn4& alb) {
  dn4 E, A;
  denoise_prepare(c, alb, E, A);
  return E.w;
}

// sm = the reprojected sums of M over the kept taps; history and acc as in temporal_blend
GSP_HD dn4 svgf_moments_blend(const TemporalParams& k, bool history, const TemporalAcc& acc, const dn4& sm, const dn4& c, float l) {
  const bool fin = temporal_finite3(c);
  if (!history) return fin ? dn4{l, l * l, 1.0f, 0.0f} : dn4{0.0f, 0.0f, 1.0f, 0.0f};
  const dn4 prev = {sm.x / acc.sw, sm.y / acc.sw, sm.z / acc.sw, 0.0f};
  if (!fin) return prev;
  float N;
  const float a = temporal_blend_weight(k, acc.sl / acc.sw, N);
  const float b = 1.0f - a;
  dn4 o;
  o.x = prev.x + (l - prev.x) * a;
  o.y = prev.y + (l * l - prev.y) * a;
  o.z = (b * b) * prev.z + a * a;
  o.w = 0.0f;
  return o;
}

// temporal_pixel with the moments: fetch(x, y, H, G, I, M) reads the PREVIOUS history.  H, G, I come from the very calls
// temporal_pixel makes in the order it makes them, so they are its bits; M is summed over the taps those calls keep.
template <class FETCH>
GSP_HD TemporalMomentsOut temporal_pixel_moments(const TemporalConsts& k, int px, int py, const dn4& c, const dn4& alb, const dn4& geom, uint32_t inst,
                                                 FETCH fetch) {
  const TemporalPixel p = temporal_classify(alb, geom, inst);
  TemporalAcc acc = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  dn4 sm = {0.0f, 0.0f, 0.0f, 0.0f};
  if (k.history_valid) {
    const TemporalProj pr = temporal_project(k, p, px, py);
    if (pr.ok) {
      dn4 Hq[4], Gq[4], Mq[4];
      uint32_t Iq[4];
      bool use[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int x = pr.x0 + (i & 1), y = pr.y0 + (i >> 1);
        use[i] = pr.w[i] != 0.0f && x >= 0 && x < (int)k.cur.width && y >= 0 && y < (int)k.cur.height;
        Hq[i] = dn4{0.0f, 0.0f, 0.0f, 0.0f};
        Gq[i] = Hq[i];
        Mq[i] = Hq[i];
        Iq[i] = 0u;
        if (use[i]) fetch(x, y, Hq[i], Gq[i], Iq[i], Mq[i]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (use[i]) {
          temporal_tap(k.p, p, pr.ze, pr.w[i], Hq[i], Gq[i], Iq[i], acc);
          if (temporal_tap_kept(k.p, p, pr.ze, Hq[i], Gq[i], Iq[i])) {
            sm.x += pr.w[i] * Mq[i].x;
            sm.y += pr.w[i] * Mq[i].y;
            sm.z += pr.w[i] * Mq[i].z;
          }
        }
    }
  }
  const bool history = k.history_valid != 0 && acc.sw >= 0.01f;
  TemporalMomentsOut o;
  o.t.H = temporal_blend(k.p, history, acc, c);
  o.t.G = dn4{p.n.x, p.n.y, p.n.z, p.z};
  o.t.I = p.inst;
  o.M = svgf_moments_blend(k.p, history, acc, sm, c, svgf_frame_luminance(c, alb));
  return o;
}

// ---- initial variance ------------------------------------------------------------------------------------------------------
// Is the temporal estimate used?  len = H.len of the pixel
GSP_HD bool svgf_variance_is_temporal(const SvgfConsts& k, float len, const dn4& M) { return len >= k.min_history && M.z < 1.0f; }

GSP_HD float svgf_variance_temporal(const dn4& M) { return svgf_clamp0(M.y - M.x * M.x) * (M.z / (1.0f - M.z)); }

// V0 of pixel (px, py): fetch(x, y, L, valid, G) reads a pixel inside the frame -- L = E.w, valid = A.w.
template <class FETCH>
GSP_HD float svgf_variance_pixel(const SvgfConsts& k, int width, int height, int px, int py, float len, const dn4& M, FETCH fetch) {
  float Lp, validp;
  dn4 Gp;
  fetch(px, py, Lp, validp, Gp);
  if (validp == 0.0f) return 0.0f;
  if (svgf_variance_is_temporal(k, len, M)) return svgf_variance_temporal(M);
  float sg = 0.0f, s1 = 0.0f, s2 = 0.0f;
  for (int dy = -kSvgfVarianceRadius; dy <= kSvgfVarianceRadius; ++dy) {
    const int y = py + dy;
    if (y < 0 || y >= height) continue;
    for (int dx = -kSvgfVarianceRadius; dx <= kSvgfVarianceRadius; ++dx) {
      const int x = px + dx;
      if (x < 0 || x >= width) continue;
      float Lq, validq;
      dn4 Gq;
      fetch(x, y, Lq, validq, Gq);
      if (validq == 0.0f) continue;
      const float rz = denoise_rz(Gp, Gq);
      const float g = det_expf(-(denoise_dn(Gp, Gq) * k.inv_sn2 + rz * rz * k.inv_sz2));
      sg += g;
      s1 += g * Lq;
      s2 += g * (Lq * Lq);
    }
  }
  const float m = s1 / sg;  // (the centre tap has g = 1: sg >= 1)
  return svgf_clamp0(s2 / sg - m * m);
}

// ---- one level ---------------------------------------------------------------------------------------------------------------
GSP_HD float svgf_tent(int d) { return d == 0 ? 0.5f : 0.25f; }

// One centre pixel of level `level` (step 2^level): fetch(x, y, E, A, G, V) reads a pixel inside the frame.  The order of
// summation: first the 3 x 3 variance prefilter (step 1), then the 25 taps, both dy outer, dx inner; a tap outside the frame is
// skipped before it is fetched.
template <class FETCH>
GSP_HD SvgfLevelOut svgf_pixel_level(const SvgfConsts& k, uint32_t level, int width, int height, int px, int py, FETCH fetch) {
  dn4 Ep, Ap, Gp;
  float Vp;
  fetch(px, py, Ep, Ap, Gp, Vp);
  if (Ap.w == 0.0f) return SvgfLevelOut{Ep, Vp};
  float inv_l = 0.0f;
  if (k.lum_on) {
    float sv = 0.0f, sk = 0.0f;
    for (int dy = -1; dy <= 1; ++dy) {
      const int y = py + dy;
      if (y < 0 || y >= height) continue;
      for (int dx = -1; dx <= 1; ++dx) {
        const int x = px + dx;
        if (x < 0 || x >= width) continue;
        dn4 Eq, Aq, Gq;
        float Vq;
        fetch(x, y, Eq, Aq, Gq, Vq);
        if (Aq.w == 0.0f) continue;
        const float t = svgf_tent(dx) * svgf_tent(dy);
        sk += t;
        sv += t * Vq;
      }
    }
    inv_l = 1.0f / (k.sigma_v * gsqrt(sv / sk) + 1e-4f);
  }
  const int s = 1 << level;
  SvgfAcc acc = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  for (int dy = -2; dy <= 2; ++dy) {
    const int y = py + s * dy;
    if (y < 0 || y >= height) continue;
    for (int dx = -2; dx <= 2; ++dx) {
      const int x = px + s * dx;
      if (x < 0 || x >= width) continue;
      dn4 Eq, Aq, Gq;
      float Vq;
      fetch(x, y, Eq, Aq, Gq, Vq);
      if (Aq.w == 0.0f) continue;
      const float h = denoise_kernel(dx) * denoise_kernel(dy);
      const float rz = denoise_rz(Gp, Gq);
      const float xx = ((denoise_dn(Gp, Gq) * k.inv_sn2 + rz * rz * k.inv_sz2) + denoise_da(Ap, Aq) * k.inv_sa2) + gabs(Ep.w - Eq.w) * inv_l;
      const float w = h * det_expf(-xx);
      acc.w += w;
      acc.r += w * Eq.x;
      acc.g += w * Eq.y;
      acc.b += w * Eq.z;
      acc.v += (w * w) * Vq;
    }
  }
  SvgfLevelOut o;
  o.E = denoise_level_result(DenoiseAcc{acc.w, acc.r, acc.g, acc.b});
  o.V = acc.v / (acc.w * acc.w);
  return o;
}

// ---- host side: validation and constants ------------------------------------------------------------------------------------
// The host's gsp_svgf under the struct_size rule and the gsp_denoise it goes with, validated as the header says.  Returns nullptr
// and the constants in `out`, or the text for gsp_last_error.
inline const char* resolve_svgf(const gsp_denoise* denoise_host, const gsp_svgf* host, SvgfConsts& out) {
  DenoiseConsts d;
  if (const char* why = resolve_denoise(denoise_host, d)) return why;  // (sigma_color is validated and not used)
  gsp_svgf s;
  std::memset(&s, 0, sizeof(s));
  if (host) std::memcpy(&s, host, host->struct_size < sizeof(s) ? host->struct_size : sizeof(s));
  if (s.min_history == 1 || s.min_history > kSvgfMinHistoryLimit) return "gsp_svgf.min_history must be 0 (the default, 4) or within 2 .. 65536";
  if (!(s.sigma_variance >= 0.0f)) return "gsp_svgf.sigma_variance must be 0 (the default, 4), positive or +Inf (the term is off)";
  out.iterations = d.iterations;
  out.inv_sn2 = d.inv_sn2;
  out.inv_sz2 = d.inv_sz2;
  out.inv_sa2 = d.inv_sa2;
  out.min_history = (float)(s.min_history ? s.min_history : kSvgfMinHistory);
  const float sv = s.sigma_variance == 0.0f ? kSvgfSigmaVariance : s.sigma_variance;
  out.lum_on = std::isinf(sv) ? 0u : 1u;
  out.sigma_v = out.lum_on ? sv : 0.0f;
  return nullptr;
}

}  // namespace gsp
