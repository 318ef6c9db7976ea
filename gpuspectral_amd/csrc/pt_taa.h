// pt_taa.h -- temporal anti-aliasing (include/gpuspectral_pt.h, "Temporal anti-aliasing"): the resolve of the tone-mapped frame
// over its own history D, per pixel -- the tone half of the LDR film on the source, YCoCg, the 3 x 3 neighbourhood box, the
// bilinear fetch of the older D through the motion plane V, the clamp into the box and the blend -- and the host-side resolution
// of a gsp_taa.
//
// The GSP_HD functions compile for gfx950 (k_taa_resolve; pt_render_kernels.inc) and for the host (tests/emu/taa_emu.cpp):
// device and emulation are the same text.  All arithmetic is float32 in the order written; the file is compiled with
// -ffp-contract=off like the rest.
//
//   D = {r, g, b, used}   16 bytes; display-linear colour (after the tone curve and the clamp to [0, 1], before the encode);
//                         used = 1 where the pixel was blended with its history, 0 where it is the frame's own
#pragma once
#include <cmath>
#include <cstring>

#include "../../include/gpuspectral_pt.h"
#include "pt_denoise.h"
#include "pt_display.h"
#include "pt_math.h"

namespace gsp {

constexpr float kTaaAlpha = 0.1f, kTaaSigmaClip = 1.0f;

// what a gsp_taa comes to; passed to the kernel by value
struct TaaParams {
  float alpha;       // (0, 1]
  float sigma_clip;  // > 0, finite
};

// ---- step 2: YCoCg, as dn4 {y, co, cg, w} (w is carried, not read) ------------------------------------------------------------
GSP_HD dn4 taa_ycocg(float r, float g, float b) { return dn4{(0.25f * r + 0.5f * g) + 0.25f * b, 0.5f * r - 0.5f * b, (-0.25f * r + 0.5f * g) - 0.25f * b, 0.0f}; }

GSP_HD void taa_rgb(const dn4& c, float& r, float& g, float& b) {
  const float t = c.x - c.z;
  r = t + c.y;
  g = c.x + c.z;
  b = t - c.y;
}

// steps 1-2 of one source pixel: X = YCoCg of the tone half of the LDR film (the curve is pt_display.h's, not restated)
template <uint32_t TONEMAP>
GSP_HD dn4 taa_source_t(const dn4& src, const DisplayConsts& k) {
  float r = src.x, g = src.y, b = src.z;
  display_tone_t<TONEMAP>(r, g, b, k);
  return taa_ycocg(r, g, b);
}

// the same through a run-time choice (host emulation)
GSP_HD dn4 taa_source(const dn4& src, const DisplayConsts& k) {
  if (k.tonemap == GSP_TONEMAP_ACES) return taa_source_t<GSP_TONEMAP_ACES>(src, k);
  if (k.tonemap == GSP_TONEMAP_REINHARD) return taa_source_t<GSP_TONEMAP_REINHARD>(src, k);
  return taa_source_t<GSP_TONEMAP_CLAMP>(src, k);
}

GSP_HD float taa_clip(float h, float lo, float hi) { return h < lo ? lo : (h > hi ? hi : h); }

// step 6, the blend: c + (x - c) * alpha; a frame of full weight is the frame itself, to the bit (c + (x - c) may round off x)
GSP_HD float taa_blend(float c, float x, float alpha) { return alpha == 1.0f ? x : c + (x - c) * alpha; }

// rgb of a YCoCg triple clamped to [0, 1] per channel, with `used` in .w
GSP_HD dn4 taa_store(const dn4& c, float used) {
  float r, g, b;
  taa_rgb(c, r, g, b);
  return dn4{display_clamp01(r), display_clamp01(g), display_clamp01(b), used};
}

// ---- steps 3-6 of one pixel ---------------------------------------------------------------------------------------------------
// D' of pixel (px, py).  V = the pixel's motion record {mx, my, sw, cls} of the frame's accumulate; taa_valid: there is an older D
// plane to read.  fetchX(x, y) returns X of the source and fetchD(x, y) D of the OLDER plane at a pixel inside the frame; neither
// is called for a pixel outside it.  The box is walked dy outer, dx inner; the four history taps are fetched before the first is
// used: the loads are independent and in flight together.
template <class FETCHX, class FETCHD>
GSP_HD dn4 taa_pixel(const TaaParams& a, bool taa_valid, int width, int height, int px, int py, const dn4& V, FETCHX fetchX, FETCHD fetchD) {
  const dn4 Xp = fetchX(px, py);
  bool history = taa_valid && V.w != 0.0f && !(V.z < 0.01f);
  const dn4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  dn4 Dq[4] = {zero, zero, zero, zero};
  float w[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  bool use[4] = {false, false, false, false};
  if (history) {
    const float fx = (float)px + V.x, fy = (float)py + V.y;
    // (outside (-1, W) x (-1, H) no tap lies inside the frame; NaN fails the test)
    if (fx > -1.0f && fx < (float)width && fy > -1.0f && fy < (float)height) {
      const float x0 = __builtin_floorf(fx), y0 = __builtin_floorf(fy);
      const float wx = fx - x0, wy = fy - y0;
      w[0] = (1.0f - wx) * (1.0f - wy);
      w[1] = wx * (1.0f - wy);
      w[2] = (1.0f - wx) * wy;
      w[3] = wx * wy;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int x = (int)x0 + (i & 1), y = (int)y0 + (i >> 1);
        use[i] = w[i] != 0.0f && x >= 0 && x < width && y >= 0 && y < height;
        if (use[i]) Dq[i] = fetchD(x, y);
      }
    }
  }
  float n = 0.0f;
  float s1y = 0.0f, s1o = 0.0f, s1g = 0.0f, s2y = 0.0f, s2o = 0.0f, s2g = 0.0f;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int x = px + dx, y = py + dy;
      if (x < 0 || x >= width || y < 0 || y >= height) continue;
      const dn4 Xq = fetchX(x, y);
      n += 1.0f;
      s1y += Xq.x;
      s1o += Xq.y;
      s1g += Xq.z;
      s2y += Xq.x * Xq.x;
      s2o += Xq.y * Xq.y;
      s2g += Xq.z * Xq.z;
    }
  float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (use[i]) {
      sw += w[i];
      sr += w[i] * Dq[i].x;
      sg += w[i] * Dq[i].y;
      sb += w[i] * Dq[i].z;
    }
  history = history && !(sw < 0.01f);
  if (!history) return taa_store(Xp, 0.0f);
  const dn4 Hc = taa_ycocg(sr / sw, sg / sw, sb / sw);
  const float my = s1y / n, mo = s1o / n, mg = s1g / n;
  const float sdy = gsqrt(gmax(s2y / n - my * my, 0.0f)), sdo = gsqrt(gmax(s2o / n - mo * mo, 0.0f)), sdg = gsqrt(gmax(s2g / n - mg * mg, 0.0f));
  const float cy = taa_clip(Hc.x, my - a.sigma_clip * sdy, my + a.sigma_clip * sdy);
  const float co = taa_clip(Hc.y, mo - a.sigma_clip * sdo, mo + a.sigma_clip * sdo);
  const float cg = taa_clip(Hc.z, mg - a.sigma_clip * sdg, mg + a.sigma_clip * sdg);
  return taa_store(dn4{taa_blend(cy, Xp.x, a.alpha), taa_blend(co, Xp.y, a.alpha), taa_blend(cg, Xp.z, a.alpha), 0.0f}, 1.0f);
}

// ---- host side: validation ----------------------------------------------------------------------------------------------------
// The host's struct under the struct_size rule (fields it does not have are 0; NULL and struct_size 0 = the zeroed struct = all
// defaults), validated as the header says.  Returns nullptr and the parameters in `out`, or the text for gsp_last_error.
inline const char* resolve_taa(const gsp_taa* host, TaaParams& out) {
  gsp_taa t;
  std::memset(&t, 0, sizeof(t));
  if (host) std::memcpy(&t, host, host->struct_size < sizeof(t) ? host->struct_size : sizeof(t));
  if (!(t.alpha >= 0.0f && t.alpha <= 1.0f)) return "gsp_taa.alpha must be 0 (the default, 0.1) or within (0, 1]";
  if (!(t.sigma_clip >= 0.0f) || !std::isfinite(t.sigma_clip)) return "gsp_taa.sigma_clip must be 0 (the default, 1.0) or positive and finite";
  out.alpha = t.alpha != 0.0f ? t.alpha : kTaaAlpha;
  out.sigma_clip = t.sigma_clip != 0.0f ? t.sigma_clip : kTaaSigmaClip;
  return nullptr;
}

}  // namespace gsp
