// pt_antilag.h -- the temporal anti-lag (include/gpuspectral_pt.h, "Temporal anti-lag"): the fast history F beside the long one,
// the per-pixel driver that accumulates it with the accumulate's own reprojection (Step A), the per-pixel clamp of the long
// history into the box of F's window statistics (Step B), and the host-side resolution of a gsp_antilag.
//
// The GSP_HD functions compile for gfx950 (k_antilag_fast, k_antilag_clamp; pt_render_kernels.inc) and for the host
// (tests/emu/antilag_emu.cpp): device and emulation are the same text.  All arithmetic is float32 in the order written; the file
// is compiled with -ffp-contract=off like the rest.
//
// Beside the history planes H, G, I (pt_temporal.h) there is
//   F = {r, g, b, len}   16 bytes; the history whose length is capped at fast_history: colour, or illumination while the long
//                        history holds illumination (pt_illum.h)
#pragma once
#include <cmath>
#include <cstring>

#include "../../include/gpuspectral_pt.h"
#include "pt_denoise.h"
#include "pt_illum.h"
#include "pt_math.h"
#include "pt_motion.h"
#include "pt_temporal.h"

namespace gsp {

constexpr uint32_t kAntilagFastHistory = 4, kAntilagFastHistoryLimit = 64;
constexpr uint32_t kAntilagRadius = 2, kAntilagRadiusLimit = 3;
constexpr float kAntilagSigmaScale = 2.0f;

// what a gsp_antilag comes to; passed to the kernels by value
struct AntilagParams {
  float fast_history;  // 1 .. 64, an exact float
  int radius;          // 1 .. 3
  float sigma_scale;   // > 0, finite
};

struct AntilagClampOut {
  dn4 H;
  bool changed;  // some channel left its box: H differs from the record handed in and is to be stored
};

// ---- Step A: the fast history -----------------------------------------------------------------------------------------------
// The constants of Step A from those the frame's accumulate ran with: the cap of the length and whether there is a history to
// read.  Everything else -- both cameras, alpha, the tolerances -- is the accumulate's.
GSP_HD TemporalConsts antilag_fast_consts(const TemporalConsts& accumulate, const AntilagParams& a, bool fast_valid) {
  TemporalConsts k = accumulate;
  k.p.max_history = gmin(a.fast_history, accumulate.p.max_history);
  k.history_valid = accumulate.history_valid != 0 && fast_valid ? 1u : 0u;
  return k;
}

// F' of one pixel: what the accumulate computed for H' with F of the older fast plane in H's place.  The driver is the
// accumulate's own for the context state -- temporal_pixel, temporal_pixel_follow (FOLLOW) or illum_pixel (DEMOD) without the
// moments, whose H' does not depend on them -- so steps 1-7, the taps, their tests and weights and the blend are its operations
// in its order.  rec, wave_moved: as the accumulate's kernel hands them over (not read by temporal_pixel).
// fetch(x, y, F, G, I) reads F of the older fast plane and G, I of the older history set at a pixel inside the frame.
template <bool FOLLOW, bool DEMOD, class FETCH>
GSP_HD dn4 antilag_fast_pixel(const TemporalConsts& k, int px, int py, const dn4& c, const dn4& alb, const dn4& geom, uint32_t inst, const MotionRecord& rec,
                              bool wave_moved, FETCH fetch) {
  if constexpr (DEMOD) {
    return illum_pixel<false>(k, px, py, c, alb, geom, inst, rec, wave_moved, [&](int x, int y, dn4& F_, dn4& G_, uint32_t& I_, dn4&) { fetch(x, y, F_, G_, I_); })
        .t.H;
  } else if constexpr (FOLLOW) {
    return temporal_pixel_follow<false>(k, px, py, c, alb, geom, inst, rec, wave_moved,
                                        [&](int x, int y, dn4& F_, dn4& G_, uint32_t& I_, dn4&) { fetch(x, y, F_, G_, I_); })
        .t.H;
  } else {
    return temporal_pixel(k, px, py, c, alb, geom, inst, fetch).H;
  }
}

// ---- Step B: the clamp ------------------------------------------------------------------------------------------------------
// One pixel of the newest history: H = its record; fetch(x, y, F, G, I) reads F' and the newest set's G and I at a pixel inside
// the frame (of G only the normal is read).  The window is walked dy outer, dx inner; a pixel that is not processed, or whose
// window counts fewer than 2 radius + 1 records, or that lies inside its box comes back with changed == false.
template <class FETCH>
GSP_HD AntilagClampOut antilag_clamp_pixel(const AntilagParams& a, float normal_min, int width, int height, int px, int py, const dn4& H, FETCH fetch) {
  AntilagClampOut o;
  o.H = H;
  o.changed = false;
  if (!(H.w > 0.0f) || !temporal_finite3(H)) return o;
  dn4 Fp, Gp;
  uint32_t Ip;
  fetch(px, py, Fp, Gp, Ip);
  if (!(Fp.w > 0.0f) || !temporal_finite3(Fp)) return o;
  const bool surface = Ip != kTemporalBackground;
  float n = 0.0f;
  float s1r = 0.0f, s1g = 0.0f, s1b = 0.0f, s2r = 0.0f, s2g = 0.0f, s2b = 0.0f;
  for (int dy = -a.radius; dy <= a.radius; ++dy)
    for (int dx = -a.radius; dx <= a.radius; ++dx) {
      const int x = px + dx, y = py + dy;
      if (x < 0 || x >= width || y < 0 || y >= height) continue;
      dn4 Fq, Gq;
      uint32_t Iq;
      fetch(x, y, Fq, Gq, Iq);
      if (!(Fq.w > 0.0f) || !temporal_finite3(Fq)) continue;
      if (Iq != Ip) continue;
      if (surface && (Gp.x * Gq.x + Gp.y * Gq.y) + Gp.z * Gq.z < normal_min) continue;
      n += 1.0f;
      s1r += Fq.x;
      s1g += Fq.y;
      s1b += Fq.z;
      s2r += Fq.x * Fq.x;
      s2g += Fq.y * Fq.y;
      s2b += Fq.z * Fq.z;
    }
  if (n < (float)(2 * a.radius + 1)) return o;
  const float mr = s1r / n, mg = s1g / n, mb = s1b / n;
  const float sdr = gsqrt(gmax(s2r / n - mr * mr, 0.0f)), sdg = gsqrt(gmax(s2g / n - mg * mg, 0.0f)), sdb = gsqrt(gmax(s2b / n - mb * mb, 0.0f));
  const float lor = mr - a.sigma_scale * sdr, hir = mr + a.sigma_scale * sdr;
  const float log_ = mg - a.sigma_scale * sdg, hig = mg + a.sigma_scale * sdg;
  const float lob = mb - a.sigma_scale * sdb, hib = mb + a.sigma_scale * sdb;
  o.changed = H.x < lor || H.x > hir || H.y < log_ || H.y > hig || H.z < lob || H.z > hib;
  if (!o.changed) return o;
  o.H.x = H.x < lor ? lor : (H.x > hir ? hir : H.x);
  o.H.y = H.y < log_ ? log_ : (H.y > hig ? hig : H.y);
  o.H.z = H.z < lob ? lob : (H.z > hib ? hib : H.z);
  o.H.w = gmin(H.w, Fp.w);
  return o;
}

// ---- host side: validation ----------------------------------------------------------------------------------------------------
// The host's struct under the struct_size rule (fields it does not have are 0; NULL and struct_size 0 = the zeroed struct = all
// defaults), validated as the header says.  Returns nullptr and the parameters in `out`, or the text for gsp_last_error.
inline const char* resolve_antilag(const gsp_antilag* host, AntilagParams& out) {
  gsp_antilag t;
  std::memset(&t, 0, sizeof(t));
  if (host) std::memcpy(&t, host, host->struct_size < sizeof(t) ? host->struct_size : sizeof(t));
  if (t.fast_history > kAntilagFastHistoryLimit) return "gsp_antilag.fast_history must be 0 (the default, 4) or within 1 .. 64";
  if (t.radius > kAntilagRadiusLimit) return "gsp_antilag.radius must be 0 (the default, 2) or within 1 .. 3";
  if (!(t.sigma_scale >= 0.0f) || !std::isfinite(t.sigma_scale)) return "gsp_antilag.sigma_scale must be 0 (the default, 2.0) or positive and finite";
  out.fast_history = (float)(t.fast_history ? t.fast_history : kAntilagFastHistory);
  out.radius = (int)(t.radius ? t.radius : kAntilagRadius);
  out.sigma_scale = t.sigma_scale != 0.0f ? t.sigma_scale : kAntilagSigmaScale;
  return nullptr;
}

}  // namespace gsp
