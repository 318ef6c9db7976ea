// pt_temporal.h -- temporal accumulation (include/gpuspectral_pt.h, "Temporal accumulation"): the reprojection of a pixel into the
// previous camera, the test of one tap of the previous history, the blend, the per-pixel driver over a fetch(x, y) callable, and
// the host-side resolution of a gsp_temporal and of the two cameras into kernel constants.
//
// The GSP_HD functions compile for gfx950 (k_temporal_reproject, pt_render_kernels.inc) and for the host
// (tests/emu/temporal_emu.cpp): device and emulation are the same text.  All arithmetic is float32 in the order written; the file
// is compiled with -ffp-contract=off like the rest.
//
// A history set is three planes over the full frame:
//   H = {r, g, b, len}       16 bytes; len = the history length as a float, 0 = the pixel is nobody's history
//   G = {n.x, n.y, n.z, z}   16 bytes; zero for a background pixel
//   I = instance index       4 bytes; 0xffffffff = background
#pragma once
#include <cmath>
#include <cstring>

#include "../../include/gpuspectral_pt.h"
#include "pt_denoise.h"
#include "pt_math.h"
#include "pt_stages.h"

namespace gsp {

constexpr uint32_t kTemporalMaxHistoryLimit = 65536;
constexpr uint32_t kTemporalMaxHistory = 32;
constexpr double kTemporalAlpha = 0.2, kTemporalDepthTolerance = 0.02, kTemporalNormalMin = 0.9;
constexpr uint32_t kTemporalBackground = 0xffffffffu;

// what a gsp_temporal comes to
struct TemporalParams {
  float max_history;  // 1 .. 65536, an exact float
  float alpha, depth_tol, normal_min;
};

// ... plus the two cameras; passed to the kernel by value
struct TemporalConsts {
  RenderConstsBase cur;  // width, height, zplane, cam_origin and cam_to_world of THIS frame's camera (the rest is 0)
  TemporalParams p;
  uint32_t history_valid;  // 0: every pixel is without history and the previous planes are not read
  float eye_prev[3];
  float zplane_prev;
  float minv_prev[16];  // the inverse of the upper-left 3x3 of the previous to_world, in xform_dir's layout (m[4 * c + r])
};

struct TemporalPixel {  // a pixel's own data of this frame
  bool surface;
  f3 n;
  float z;
  uint32_t inst;  // 0xffffffff for a background pixel
};

struct TemporalProj {
  bool ok;  // false: no history (behind the previous camera, or no tap inside the previous frame)
  int x0, y0;
  float w[4];  // taps (x0,y0), (x0+1,y0), (x0,y0+1), (x0+1,y0+1)
  float ze;    // |v|: the distance from the previous eye (surface pixels)
};

struct TemporalAcc {
  float sw, r, g, b, sl;
};

struct TemporalOut {
  dn4 H, G;
  uint32_t I;
};

GSP_HD bool temporal_finite3(const dn4& c) { return gisvalid(c.x) && gisvalid(c.y) && gisvalid(c.z); }

GSP_HD TemporalPixel temporal_classify(const dn4& alb, const dn4& geom, uint32_t inst) {
  TemporalPixel p;
  const float cov = alb.w;
  p.surface = inst != kTemporalBackground && cov >= 0.5f;
  if (p.surface) {
    p.n = mk3(geom.x / cov, geom.y / cov, geom.z / cov);
    p.z = geom.w / cov;
    p.inst = inst;
  } else {
    p.n = mk3(0.0f, 0.0f, 0.0f);
    p.z = 0.0f;
    p.inst = kTemporalBackground;
  }
  return p;
}

// |f - rint(f)| < 1e-3f: f = rint(f)
GSP_HD float temporal_snap(float f) {
  const float r = grint(f);
  return gabs(f - r) < 1e-3f ? r : f;
}

// Steps 1-7 of the header: where pixel (px, py) was in the previous frame
GSP_HD TemporalProj temporal_project(const TemporalConsts& k, const TemporalPixel& p, int px, int py) {
  TemporalProj o;
  o.ok = false;
  o.x0 = o.y0 = 0;
  o.w[0] = o.w[1] = o.w[2] = o.w[3] = 0.0f;
  o.ze = 0.0f;
  const f3 d = camera_dir(k.cur, (float)px, (float)py);
  f3 v = d;
  if (p.surface) {
    const f3 P = mk3(k.cur.cam_origin[0] + d.x * p.z, k.cur.cam_origin[1] + d.y * p.z, k.cur.cam_origin[2] + d.z * p.z);
    v = mk3(P.x - k.eye_prev[0], P.y - k.eye_prev[1], P.z - k.eye_prev[2]);
    o.ze = length(v);
  }
  const f3 l = xform_dir(k.minv_prev, mk3(v.x, v.y * -1.0f, v.z));
  if (!(l.z > 0.0f)) return o;
  const float t = k.zplane_prev / l.z;
  const float W = (float)k.cur.width, H = (float)k.cur.height;
  float fx = W / 2.0f - l.x * t;
  float fy = H / 2.0f + l.y * t;
  fx = temporal_snap(fx);
  fy = temporal_snap(fy);
  // (-1, W) x (-1, H) is where at least one tap can lie inside the frame; NaN fails the test
  if (!(fx > -1.0f && fx < W && fy > -1.0f && fy < H)) return o;
  const float x0 = __builtin_floorf(fx), y0 = __builtin_floorf(fy);
  const float wx = fx - x0, wy = fy - y0;
  o.x0 = (int)x0;
  o.y0 = (int)y0;
  o.w[0] = (1.0f - wx) * (1.0f - wy);
  o.w[1] = wx * (1.0f - wy);
  o.w[2] = (1.0f - wx) * wy;
  o.w[3] = wx * wy;
  o.ok = true;
  return o;
}

// The test of one tap q inside the previous frame: is it this pixel's history?
GSP_HD bool temporal_tap_kept(const TemporalParams& k, const TemporalPixel& p, float ze, const dn4& Hq, const dn4& Gq, uint32_t Iq) {
  if (!(Hq.w > 0.0f) || !temporal_finite3(Hq)) return false;
  if (Iq != p.inst) return false;  // (a background pixel has inst = 0xffffffff)
  if (p.surface) {
    if (gabs(ze - Gq.w) > k.depth_tol * ze) return false;
    if (dot(p.n, mk3(Gq.x, Gq.y, Gq.z)) < k.normal_min) return false;
  }
  return true;
}

// One tap q inside the previous frame with weight w != 0: tested and, when kept, summed
GSP_HD void temporal_tap(const TemporalParams& k, const TemporalPixel& p, float ze, float w, const dn4& Hq, const dn4& Gq, uint32_t Iq,
                         TemporalAcc& acc) {
  if (!temporal_tap_kept(k, p, ze, Hq, Gq, Iq)) return;
  acc.sw += w;
  acc.r += w * Hq.x;
  acc.g += w * Hq.y;
  acc.b += w * Hq.z;
  acc.sl += w * Hq.w;
}

// The blend weight of a finite new frame on a history of length len: N = min(len + 1, max_history), a = max(alpha, 1 / N)
GSP_HD float temporal_blend_weight(const TemporalParams& k, float len, float& N) {
  N = gmin(len + 1.0f, k.max_history);
  return gmax(k.alpha, 1.0f / N);
}

// history = history_valid and sw >= 0.01f
GSP_HD dn4 temporal_blend(const TemporalParams& k, bool history, const TemporalAcc& acc, const dn4& c) {
  const bool fin = temporal_finite3(c);
  dn4 o;
  if (!history) {
    o.x = c.x;
    o.y = c.y;
    o.z = c.z;
    o.w = fin ? 1.0f : 0.0f;
    return o;
  }
  const float pr = acc.r / acc.sw, pg = acc.g / acc.sw, pb = acc.b / acc.sw;
  const float len = acc.sl / acc.sw;
  if (!fin) {
    o.x = pr;
    o.y = pg;
    o.z = pb;
    o.w = gmin(len, k.max_history);
    return o;
  }
  float N;
  const float a = temporal_blend_weight(k, len, N);
  o.x = pr + (c.x - pr) * a;
  o.y = pg + (c.y - pg) * a;
  o.z = pb + (c.z - pb) * a;
  o.w = N;
  return o;
}

// One pixel: c = its accumulate record, alb / geom / inst = its feature records of this frame (inst = ids.z);
// fetch(x, y, H, G, I) reads the PREVIOUS history at a pixel inside the frame.  Every kept-in-frame tap is fetched before the
// first one is tested: the loads are independent and in flight together.
template <class FETCH>
GSP_HD TemporalOut temporal_pixel(const TemporalConsts& k, int px, int py, const dn4& c, const dn4& alb, const dn4& geom, uint32_t inst, FETCH fetch) {
  const TemporalPixel p = temporal_classify(alb, geom, inst);
  TemporalAcc acc = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (k.history_valid) {
    const TemporalProj pr = temporal_project(k, p, px, py);
    if (pr.ok) {
      dn4 Hq[4], Gq[4];
      uint32_t Iq[4];
      bool use[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int x = pr.x0 + (i & 1), y = pr.y0 + (i >> 1);
        use[i] = pr.w[i] != 0.0f && x >= 0 && x < (int)k.cur.width && y >= 0 && y < (int)k.cur.height;
        Hq[i] = dn4{0.0f, 0.0f, 0.0f, 0.0f};
        Gq[i] = Hq[i];
        Iq[i] = 0u;
        if (use[i]) fetch(x, y, Hq[i], Gq[i], Iq[i]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (use[i]) temporal_tap(k.p, p, pr.ze, pr.w[i], Hq[i], Gq[i], Iq[i], acc);
    }
  }
  TemporalOut o;
  o.H = temporal_blend(k.p, k.history_valid != 0 && acc.sw >= 0.01f, acc, c);
  o.G = dn4{p.n.x, p.n.y, p.n.z, p.z};
  o.I = p.inst;
  return o;
}

// ---- host side: validation and constants (formed in double, rounded to float once) ----

// The host's struct under the struct_size rule (fields it does not have are 0; NULL and struct_size 0 = the zeroed struct = all
// defaults), validated as the header says.  Returns nullptr and the parameters in `out`, or the text for gsp_last_error.
inline const char* resolve_temporal(const gsp_temporal* host, TemporalParams& out) {
  gsp_temporal t;
  std::memset(&t, 0, sizeof(t));
  if (host) std::memcpy(&t, host, host->struct_size < sizeof(t) ? host->struct_size : sizeof(t));
  if (t.max_history > kTemporalMaxHistoryLimit) return "gsp_temporal.max_history must be 0 (the default, 32) or within 1 .. 65536";
  if (!(t.alpha >= 0.0f && t.alpha <= 1.0f)) return "gsp_temporal.alpha must be 0 (the default, 0.2) or within (0, 1]";
  if (!(t.depth_tolerance >= 0.0f)) return "gsp_temporal.depth_tolerance must be 0 (the default, 0.02) or positive";
  if (!(t.normal_min >= -1.0f && t.normal_min <= 1.0f)) return "gsp_temporal.normal_min must be 0 (the default, 0.9) or within [-1, 1]";
  out.max_history = (float)(t.max_history ? t.max_history : kTemporalMaxHistory);
  out.alpha = t.alpha != 0.0f ? t.alpha : (float)kTemporalAlpha;
  out.depth_tol = t.depth_tolerance != 0.0f ? t.depth_tolerance : (float)kTemporalDepthTolerance;
  out.normal_min = t.normal_min != 0.0f ? t.normal_min : (float)kTemporalNormalMin;
  return nullptr;
}

// zplane as gsp_focus_distance and render_consts form it
inline float temporal_zplane(uint32_t width, uint32_t height, float fov) {
  return (((float)width > (float)height ? (float)width : (float)height) / 2.0f) / tanf(fov / 2.0f);
}

// The kernel's constants of a frame of width x height under camera `cur`, whose history (when history_valid) belongs to camera
// `prev` and the same size.  Returns nullptr, or the text for gsp_last_error: the previous camera's 3x3 has no inverse.
inline const char* temporal_consts(const gsp_camera& cur, const gsp_camera* prev, bool history_valid, uint32_t width, uint32_t height,
                                   const TemporalParams& p, TemporalConsts& out) {
  std::memset(&out, 0, sizeof(out));
  out.cur.width = width;
  out.cur.height = height;
  out.cur.zplane = temporal_zplane(width, height, cur.fov);
  for (int i = 0; i < 16; ++i) out.cur.cam_to_world[i] = cur.to_world[i];
  for (int i = 0; i < 3; ++i) out.cur.cam_origin[i] = cur.to_world[12 + i];
  out.p = p;
  out.history_valid = history_valid && prev ? 1u : 0u;
  if (!out.history_valid) return nullptr;
  const float* m = prev->to_world;
  const double a = m[0], b = m[4], c = m[8], d = m[1], e = m[5], f = m[9], g = m[2], h = m[6], i = m[10];  // row-major names
  const double A = e * i - f * h, B = -(d * i - f * g), C = d * h - e * g;
  const double det = a * A + b * B + c * C;
  if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return "the camera the history belongs to has a singular to_world: no reprojection (gsp_temporal_reset starts over)";
  const double inv[3][3] = {{A / det, -(b * i - c * h) / det, (b * f - c * e) / det},
                            {B / det, (a * i - c * g) / det, -(a * f - c * d) / det},
                            {C / det, -(a * h - b * g) / det, (a * e - b * d) / det}};
  for (int r = 0; r < 3; ++r)
    for (int col = 0; col < 3; ++col) {
      const float v = (float)inv[r][col];
      if (!std::isfinite(v)) return "the camera the history belongs to has a singular to_world: no reprojection (gsp_temporal_reset starts over)";
      out.minv_prev[4 * col + r] = v;
    }
  for (int k = 0; k < 3; ++k) out.eye_prev[k] = m[12 + k];
  out.zplane_prev = temporal_zplane(width, height, prev->fov);
  return nullptr;
}

}  // namespace gsp
