// pt_illum.h -- the illumination history (include/gpuspectral_pt.h, "Illumination history"): the demodulated record (e, u) of a
// frame, the blend of it into a history that holds illumination, the per-pixel driver of the demodulated accumulate (plain, with
// moments, with the instances followed), Prepare for a demodulated history, the re-modulation of the image read-out and the
// feedback store of a filter level into the history.
//
// The GSP_HD functions compile for gfx950 (k_temporal_reproject_illum, k_illum_prepare, k_illum_image, k_svgf_atrous_feedback;
// pt_render_kernels.inc) and for the host (tests/emu/illum_emu.cpp): device and emulation are the same text.  All arithmetic is
// float32 in the order written; the file is compiled with -ffp-contract=off like the rest.
//
// No plane of its own: with demodulation on, H = {e.r, e.g, e.b, len} holds illumination in the 16 bytes pt_temporal.h gives it.
#pragma once
#include "../../include/gpuspectral_pt.h"
#include "pt_denoise.h"
#include "pt_math.h"
#include "pt_motion.h"
#include "pt_svgf.h"
#include "pt_temporal.h"

namespace gsp {

// The frame's demodulated record: (e, A) = "Denoiser: Prepare" of (c, alb); e.w = L, the luminance of e.
// u = c.rgb finite and e.rgb finite -- the second half guards a quotient that overflows.
struct IllumFrame {
  dn4 e;
  bool u;
};

GSP_HD IllumFrame illum_frame(const dn4& c, const dn4& alb) {
  IllumFrame f;
  dn4 A;
  denoise_prepare(c, alb, f.e, A);
  f.u = temporal_finite3(c) && temporal_finite3(f.e);
  return f;
}

// "Temporal accumulation: Blend" with u for "c finite" and e.k for c.k; history and acc as in temporal_blend
GSP_HD dn4 illum_blend(const TemporalParams& k, bool history, const TemporalAcc& acc, const dn4& c, const IllumFrame& f) {
  dn4 o;
  if (!history) {
    if (f.u) return dn4{f.e.x, f.e.y, f.e.z, 1.0f};
    return dn4{c.x, c.y, c.z, 0.0f};  // the raw record: nobody's history
  }
  const float pr = acc.r / acc.sw, pg = acc.g / acc.sw, pb = acc.b / acc.sw;
  const float len = acc.sl / acc.sw;
  if (!f.u) {
    o.x = pr;
    o.y = pg;
    o.z = pb;
    o.w = gmin(len, k.max_history);
    return o;
  }
  float N;
  const float a = temporal_blend_weight(k, len, N);
  o.x = pr + (f.e.x - pr) * a;
  o.y = pg + (f.e.y - pg) * a;
  o.z = pb + (f.e.z - pb) * a;
  o.w = N;
  return o;
}

// "Variance-guided filter: 1. Moments" with u for "c finite": l = f.e.w already is the luminance of e.  svgf_moments_blend reads
// of its c only whether it is finite, and e.rgb finite <=> u (a c that is not finite has no finite quotient).
GSP_HD dn4 illum_moments_blend(const TemporalParams& k, bool history, const TemporalAcc& acc, const dn4& sm, const IllumFrame& f) {
  const dn4 flag = f.u ? dn4{0.0f, 0.0f, 0.0f, 0.0f} : dn4{u2f(0x7fc00000u), 0.0f, 0.0f, 0.0f};
  return svgf_moments_blend(k, history, acc, sm, flag, f.e.w);
}

// temporal_pixel / temporal_pixel_moments / temporal_pixel_follow with the frame demodulated.  The reprojection, the taps and
// their tests, len, G', I' and V are temporal_pixel_follow's operations in its order (pt_motion.h; restated, not shared, for the
// reason given there), so they are its bits -- and, for a record of class 0 with wave_moved false, those of temporal_pixel /
// temporal_pixel_moments: what a context that does not follow instances passes.  Only the two blends differ.
template <bool MOMENTS, class FETCH>
GSP_HD MotionOut illum_pixel(const TemporalConsts& k, int px, int py, const dn4& c, const dn4& alb, const dn4& geom, uint32_t inst, const MotionRecord& rec,
                             bool wave_moved, FETCH fetch) {
  const TemporalPixel p = temporal_classify(alb, geom, inst);
  const uint32_t cls = p.surface ? motion_class(rec) : kMotionStatic;
  TemporalAcc acc = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  dn4 sm = {0.0f, 0.0f, 0.0f, 0.0f};
  dn4 V = {0.0f, 0.0f, 0.0f, 0.0f};
  if (k.history_valid && cls != kMotionNoHistory) {
    TemporalPixel pt = p;  // what the tap test sees: the normal of a followed pixel is n'
    TemporalProj pr;
    pr.ok = false;
    float fx = 0.0f, fy = 0.0f;
    bool have = true;
    const f3 d = camera_dir(k.cur, (float)px, (float)py);
    f3 v = d;  // (a background pixel: a point at infinity)
    float ze = 0.0f;
    if (p.surface) {
      const f3 P = motion_point(k, d, p.z);
      if (wave_moved && cls == kMotionMoved) {
        f3 n_prev;
        have = motion_apply(rec, k.eye_prev, P, p.n, v, ze, n_prev);
        if (have) pt.n = n_prev;
      } else {
        v = mk3(P.x - k.eye_prev[0], P.y - k.eye_prev[1], P.z - k.eye_prev[2]);
        ze = length(v);
      }
    }
    if (have) pr = motion_project_v(k, v, ze, fx, fy);
    if (have && pr.ok) {
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
          temporal_tap(k.p, pt, pr.ze, pr.w[i], Hq[i], Gq[i], Iq[i], acc);
          if (MOMENTS && temporal_tap_kept(k.p, pt, pr.ze, Hq[i], Gq[i], Iq[i])) {
            sm.x += pr.w[i] * Mq[i].x;
            sm.y += pr.w[i] * Mq[i].y;
            sm.z += pr.w[i] * Mq[i].z;
          }
        }
      V = dn4{fx - (float)px, fy - (float)py, acc.sw, cls == kMotionMoved ? 2.0f : 1.0f};
    }
  }
  const bool history = k.history_valid != 0 && acc.sw >= 0.01f;
  const IllumFrame f = illum_frame(c, alb);
  MotionOut o;
  o.t.H = illum_blend(k.p, history, acc, c, f);
  o.t.G = dn4{p.n.x, p.n.y, p.n.z, p.z};
  o.t.I = p.inst;
  o.M = dn4{0.0f, 0.0f, 0.0f, 0.0f};
  if (MOMENTS) o.M = illum_moments_blend(k.p, history, acc, sm, f);
  o.V = V;
  return o;
}

// Prepare of a demodulated history: e = H.rgb as it is, valid = H's three channels finite, A and a' from the albedo record as
// denoise_prepare forms them, L from e
GSP_HD void illum_prepare(const dn4& H, const dn4& alb, dn4& E, dn4& A) {
  const float miss = 1.0f - alb.w;
  A.x = alb.x + miss;
  A.y = alb.y + miss;
  A.z = alb.z + miss;
  A.w = temporal_finite3(H) ? 1.0f : 0.0f;
  E.x = H.x;
  E.y = H.y;
  E.z = H.z;
  E.w = display_luma(E.x, E.y, E.z);
}

// The image read-out of a demodulated history: H.k * A_k where H.len > 0, H as stored where H.len == 0; out.w = H.len
GSP_HD dn4 illum_image(const dn4& H, const dn4& alb) {
  if (!(H.w > 0.0f)) return H;
  const float miss = 1.0f - alb.w;
  dn4 o;
  o.x = H.x * denoise_floor_albedo(alb.x + miss);
  o.y = H.y * denoise_floor_albedo(alb.y + miss);
  o.z = H.z * denoise_floor_albedo(alb.z + miss);
  o.w = H.w;
  return o;
}

// The feedback store: the history record of a pixel after the level whose output is E; A = the pixel's record of the A plane.
// An invalid pixel keeps its bits, every pixel its len.
template <bool DEMOD>
GSP_HD dn4 illum_feedback(const dn4& E, const dn4& A, const dn4& H) {
  if (A.w == 0.0f) return H;
  dn4 o;
  if (DEMOD) {
    o.x = E.x;
    o.y = E.y;
    o.z = E.z;
  } else {
    o.x = E.x * denoise_floor_albedo(A.x);
    o.y = E.y * denoise_floor_albedo(A.y);
    o.z = E.z * denoise_floor_albedo(A.z);
  }
  o.w = H.w;
  return o;
}

}  // namespace gsp
