// pt_display.h -- the LDR film (include/gpuspectral_pt.h, "LDR film"): the per-pixel tone map + encode, the per-pixel frame
// statistic, and the host-side resolution of a gsp_display into kernel constants.
//
// The GSP_HD functions compile for gfx950 (k_display_map / k_display_stats, pt_render_kernels.inc) and for the host
// (tests/emu/display_emu.cpp): device and emulation are the same text.  All arithmetic is float32 in the order written; the file
// is compiled with -ffp-contract=off like the rest.
#pragma once
#include <cmath>
#include <cstring>

#include "../../include/gpuspectral_pt.h"
#include "pt_math.h"

namespace gsp {

// what a gsp_display + the frame's statistics come to; passed to k_display_map by value
struct DisplayConsts {
  uint32_t tonemap;      // GSP_TONEMAP_*
  uint32_t srgb;         // 1: the sRGB curve, 0: v^(inv_gamma)
  float exposure_scale;  // 2^exposure
  float inv_gamma;
  float scale;           // Reinhard: key / Lavg
  float inv_wp2;         // Reinhard: 1 / ((Lmax * scale)^2 * b^4)
};

// the 24-byte device record of k_display_stats: integer sum, count, and the max as a non-negative float's bit pattern
struct DisplayStatsRec {
  unsigned long long sum;  // two's complement of the int64 sum of q
  unsigned long long count;
  uint32_t max_bits;
  uint32_t pad_;
};

// step 1: a NaN channel and a negative channel (-Inf included) become 0; +Inf stays
GSP_HD float display_channel(float v) { return v > 0.0f ? v : 0.0f; }

GSP_HD float display_luma(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// The frame statistic of one pixel: false when a channel (or the luminance itself) is not finite -- the pixel does not count.
GSP_HD bool display_stat(float r, float g, float b, long long& q, float& Y) {
  if (!gisvalid(r) || !gisvalid(g) || !gisvalid(b)) return false;
  Y = display_luma(display_channel(r), display_channel(g), display_channel(b));
  if (!gisvalid(Y)) return false;
  q = (long long)grint(det_logf(Y + 1e-3f) * 1048576.0f);
  return true;
}

// step 4; a NaN here can only be an overflowed curve (Inf / Inf), i.e. a saturated pixel: it becomes 1
GSP_HD float display_clamp01(float v) { return v < 1.0f ? (v > 0.0f ? v : 0.0f) : 1.0f; }

template <bool SRGB>
GSP_HD float display_encode(float v, float inv_gamma) {
  if (SRGB) return v <= 0.0031308f ? 12.92f * v : 1.055f * det_expf(det_logf(v) * (1.0f / 2.4f)) - 0.055f;
  return v == 0.0f ? 0.0f : det_expf(det_logf(v) * inv_gamma);
}

GSP_HD float display_aces(float x) { return (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f); }

// steps 1-4 for one pixel, in place: display-linear colour, every channel finite in [0, 1]
template <uint32_t TONEMAP>
GSP_HD void display_tone_t(float& r, float& g, float& b, const DisplayConsts& k) {
  r = display_channel(r) * k.exposure_scale;
  g = display_channel(g) * k.exposure_scale;
  b = display_channel(b) * k.exposure_scale;
  if (TONEMAP == GSP_TONEMAP_ACES) {
    r = display_aces(r);
    g = display_aces(g);
    b = display_aces(b);
  } else if (TONEMAP == GSP_TONEMAP_REINHARD) {
    const float Y = display_luma(r, g, b);
    if (Y == 0.0f) {
      r = g = b = 0.0f;
    } else {
      const float Lp = Y * k.scale;
      const float Yp = (Lp * (1.0f + Lp * k.inv_wp2)) / (1.0f + Lp);
      const float ratio = Yp / Y;
      r = r * ratio;
      g = g * ratio;
      b = b * ratio;
    }
  }
  r = display_clamp01(r);
  g = display_clamp01(g);
  b = display_clamp01(b);
}

// steps 5-6 for one display-linear pixel (channels in [0, 1]): the RGBA8 word, R in bits 0-7, A = 255
template <bool SRGB>
GSP_HD uint32_t display_encode_word(float r, float g, float b, const DisplayConsts& k) {
  r = display_encode<SRGB>(r, k.inv_gamma);
  g = display_encode<SRGB>(g, k.inv_gamma);
  b = display_encode<SRGB>(b, k.inv_gamma);
  // (the encode of a value in [0, 1] stays in [0, 1 + 1 ulp]: the casts below cannot leave 0..255)
  const uint32_t R = (uint32_t)(r * 255.0f + 0.5f), G = (uint32_t)(g * 255.0f + 0.5f), B = (uint32_t)(b * 255.0f + 0.5f);
  return R | (G << 8) | (B << 16) | 0xff000000u;
}

// steps 1-6 for one pixel: the tone half, then the encode half
template <uint32_t TONEMAP, bool SRGB>
GSP_HD uint32_t display_pixel_t(float r, float g, float b, const DisplayConsts& k) {
  display_tone_t<TONEMAP>(r, g, b, k);
  return display_encode_word<SRGB>(r, g, b, k);
}

// the same through a run-time choice (host emulation, tests)
GSP_HD uint32_t display_pixel(float r, float g, float b, const DisplayConsts& k) {
  if (k.srgb) {
    if (k.tonemap == GSP_TONEMAP_ACES) return display_pixel_t<GSP_TONEMAP_ACES, true>(r, g, b, k);
    if (k.tonemap == GSP_TONEMAP_REINHARD) return display_pixel_t<GSP_TONEMAP_REINHARD, true>(r, g, b, k);
    return display_pixel_t<GSP_TONEMAP_CLAMP, true>(r, g, b, k);
  }
  if (k.tonemap == GSP_TONEMAP_ACES) return display_pixel_t<GSP_TONEMAP_ACES, false>(r, g, b, k);
  if (k.tonemap == GSP_TONEMAP_REINHARD) return display_pixel_t<GSP_TONEMAP_REINHARD, false>(r, g, b, k);
  return display_pixel_t<GSP_TONEMAP_CLAMP, false>(r, g, b, k);
}

// ---- host side: validation and constants (formed in double, rounded to float once) ----

// The host's struct under the struct_size rule (fields it does not have are 0; NULL and struct_size 0 = the zeroed struct),
// validated as the header says.  Returns nullptr and the display in `out`, or the text for gsp_last_error.
inline const char* resolve_display(const gsp_display* host, gsp_display& out) {
  gsp_display d;
  std::memset(&d, 0, sizeof(d));
  if (host) std::memcpy(&d, host, host->struct_size < sizeof(d) ? host->struct_size : sizeof(d));
  if (d.tonemap > GSP_TONEMAP_ACES) return "gsp_display.tonemap must be GSP_TONEMAP_CLAMP, _REINHARD or _ACES";
  if (!std::isfinite(d.exposure) || d.exposure < -64.0f || d.exposure > 64.0f) return "gsp_display.exposure must be finite, within -64 .. 64 f-stops";
  if (!(d.gamma >= 0.0f) || std::isinf(d.gamma)) return "gsp_display.gamma must be 0 (the sRGB curve) or a finite positive value";
  if (!(d.key >= 0.0f) || !(d.key <= 1.0f)) return "gsp_display.key must be within 0 .. 1 (0 = 0.18)";
  if (!(d.burn >= 0.0f) || !(d.burn <= 1.0f)) return "gsp_display.burn must be within 0 .. 1";
  if (!(d.log_avg_luminance >= 0.0f) || std::isinf(d.log_avg_luminance)) return "gsp_display.log_avg_luminance must be 0 (measure the frame) or a finite positive value";
  if (!(d.max_luminance >= 0.0f) || std::isinf(d.max_luminance)) return "gsp_display.max_luminance must be 0 (measure the frame) or a finite positive value";
  d.struct_size = (uint32_t)sizeof(gsp_display);
  out = d;
  return nullptr;
}

// does this (resolved) display need the frame's statistics?
inline bool display_needs_stats(const gsp_display& d) {
  return d.tonemap == GSP_TONEMAP_REINHARD && (d.log_avg_luminance == 0.0f || d.max_luminance == 0.0f);
}

// S, n, max bits -> the public record
inline gsp_luminance display_luminance(const DisplayStatsRec& r) {
  gsp_luminance l;
  l.log_sum_q20 = (int64_t)r.sum;
  l.pixels = r.count;
  l.max = u2f(r.max_bits);
  l.log_avg = r.count ? (float)std::exp((double)l.log_sum_q20 / (1048576.0 * (double)r.count)) : 0.0f;
  return l;
}

// `measured` is read only where display_needs_stats says so
inline DisplayConsts display_consts(const gsp_display& d, const gsp_luminance& measured) {
  DisplayConsts k;
  k.tonemap = d.tonemap;
  k.srgb = d.gamma == 0.0f ? 1u : 0u;
  k.exposure_scale = (float)std::exp2((double)d.exposure);
  k.inv_gamma = d.gamma == 0.0f ? 0.0f : (float)(1.0 / (double)d.gamma);
  k.scale = 1.0f;
  k.inv_wp2 = 0.0f;
  if (d.tonemap == GSP_TONEMAP_REINHARD) {
    const double lavg = d.log_avg_luminance > 0.0f ? (double)d.log_avg_luminance : (measured.pixels ? (double)measured.log_avg : 0.0);
    const double lmax = d.max_luminance > 0.0f ? (double)d.max_luminance : (measured.pixels ? (double)measured.max : 0.0);
    if (lavg > 0.0 && lmax > 0.0) {
      const double key = d.key == 0.0f ? 0.18 : (double)d.key;
      const double scale = key / lavg;
      double b = 1.0 - (double)d.burn;
      b = b < 1e-8 ? 1e-8 : (b > 1.0 ? 1.0 : b);
      const double wp = lmax * scale;
      k.scale = (float)scale;
      k.inv_wp2 = (float)(1.0 / ((wp * wp) * (b * b * b * b)));
    }
  }
  return k;
}

}  // namespace gsp
