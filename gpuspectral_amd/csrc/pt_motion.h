// pt_motion.h -- temporal accumulation that follows moved instances (include/gpuspectral_pt.h, "Temporal accumulation: moved
// instances"): the per-instance record, its application to a pixel's world point and normal, the per-pixel driver over a
// record(i) and a fetch(x, y) callable, and the host-side table of the records of two transform arrays.
//
// The GSP_HD functions compile for gfx950 (k_temporal_reproject_follow, pt_render_kernels.inc) and for the host
// (tests/emu/motion_emu.cpp): device and emulation are the same text.  All arithmetic is float32 in the order written; the file
// is compiled with -ffp-contract=off like the rest.  A pixel of the background or of a static instance runs the very functions
// temporal_pixel / temporal_pixel_moments run, in their order, so its H', G', I' (and M') are their bits.
//
// Beside the history planes H, G, I (pt_temporal.h) and M (pt_svgf.h) there is
//   V = {fx - px, fy - py, sw, cls}   16 bytes; where the pixel was in the previous frame, the weight its kept taps sum to, and
//                                     0.0 = no reprojection, 1.0 = static path, 2.0 = followed
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/gpuspectral_pt.h"
#include "pt_denoise.h"
#include "pt_math.h"
#include "pt_svgf.h"
#include "pt_temporal.h"

namespace gsp {

constexpr uint32_t kMotionStatic = 0, kMotionMoved = 1, kMotionNoHistory = 2;
constexpr uint32_t kMotionRecordQuads = 6;

// One instance: 6 quads = 96 bytes.  A record of class 0 or 2 has b and n all zero.
struct MotionRecord {
  dn4 b[3];  // rows of B = T_prev * T_cur^-1: P'.r = ((b[r].x * P.x + b[r].y * P.y) + b[r].z * P.z) + b[r].w
  dn4 n[3];  // rows of N = transpose((B's 3x3)^-1) in .xyz; n[0].w = the bits of the class word, n[1].w = n[2].w = 0
};
static_assert(sizeof(MotionRecord) == kMotionRecordQuads * 16, "6 quads");

GSP_HD uint32_t motion_class(const MotionRecord& r) { return f2u(r.n[0].w); }

GSP_HD MotionRecord motion_record_of_class(uint32_t cls) {
  MotionRecord r;
  const dn4 z = {0.0f, 0.0f, 0.0f, 0.0f};
  r.b[0] = r.b[1] = r.b[2] = z;
  r.n[0] = r.n[1] = r.n[2] = z;
  r.n[0].w = u2f(cls);
  return r;
}

struct MotionOut {
  TemporalOut t;
  dn4 M;  // (MOMENTS only; zero otherwise)
  dn4 V;
};

// A class-1 pixel: its point P in the previous frame as v = P' - eye_prev with ze = |v|, and its normal there.  false: no history
GSP_HD bool motion_apply(const MotionRecord& r, const float* eye_prev, const f3& P, const f3& n, f3& v, float& ze, f3& n_prev) {
  const f3 Pp = mk3(((r.b[0].x * P.x + r.b[0].y * P.y) + r.b[0].z * P.z) + r.b[0].w, ((r.b[1].x * P.x + r.b[1].y * P.y) + r.b[1].z * P.z) + r.b[1].w,
                    ((r.b[2].x * P.x + r.b[2].y * P.y) + r.b[2].z * P.z) + r.b[2].w);
  v = mk3(Pp.x - eye_prev[0], Pp.y - eye_prev[1], Pp.z - eye_prev[2]);
  ze = length(v);
  const f3 m = mk3((r.n[0].x * n.x + r.n[0].y * n.y) + r.n[0].z * n.z, (r.n[1].x * n.x + r.n[1].y * n.y) + r.n[1].z * n.z,
                   (r.n[2].x * n.x + r.n[2].y * n.y) + r.n[2].z * n.z);
  const float s = (m.x * m.x + m.y * m.y) + m.z * m.z;
  if (!(s > 0.0f)) return false;
  const float q = gsqrt(s);
  n_prev = mk3(m.x / q, m.y / q, m.z / q);
  return true;
}

// Steps 3-7 of "Temporal accumulation" on a vector v from the previous eye (ze = |v| for a surface pixel, 0 for the background):
// temporal_project's operations in its order, so the same bits; fx, fy = the previous pixel coordinate after the snap (set when
// step 4 passes).  The text is restated here rather than shared because k_temporal_reproject compiled to another register
// allocation when temporal_project was split in two, and its instruction stream is to stay what it is.
GSP_HD TemporalProj motion_project_v(const TemporalConsts& k, const f3& v, float ze, float& fx, float& fy) {
  TemporalProj o;
  o.ok = false;
  o.x0 = o.y0 = 0;
  o.w[0] = o.w[1] = o.w[2] = o.w[3] = 0.0f;
  o.ze = ze;
  const f3 l = xform_dir(k.minv_prev, mk3(v.x, v.y * -1.0f, v.z));
  if (!(l.z > 0.0f)) return o;
  const float t = k.zplane_prev / l.z;
  const float W = (float)k.cur.width, H = (float)k.cur.height;
  fx = W / 2.0f - l.x * t;
  fy = H / 2.0f + l.y * t;
  fx = temporal_snap(fx);
  fy = temporal_snap(fy);
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

// Step 2: the world point of a surface pixel at distance z along its pinhole ray d
GSP_HD f3 motion_point(const TemporalConsts& k, const f3& d, float z) {
  return mk3(k.cur.cam_origin[0] + d.x * z, k.cur.cam_origin[1] + d.y * z, k.cur.cam_origin[2] + d.z * z);
}

// temporal_pixel / temporal_pixel_moments with the instances followed.  rec = the record of the pixel's instance (class 2 for an
// index the table does not have); fetch(x, y, H, G, I, M) reads the PREVIOUS history at a pixel inside the frame (M only read when MOMENTS).  wave_moved: some
// pixel this one shares its wave with is of class 1 (the host passes true); a wave without one skips the record arithmetic.
template <bool MOMENTS, class FETCH>
GSP_HD MotionOut temporal_pixel_follow(const TemporalConsts& k, int px, int py, const dn4& c, const dn4& alb, const dn4& geom, uint32_t inst,
                                       const MotionRecord& rec, bool wave_moved, FETCH fetch) {
  const TemporalPixel p = temporal_classify(alb, geom, inst);
  // a background pixel has no instance: the static path.  (The caller hands a surface pixel whose inst >= the table's size a
  // record of class 2.)
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
  MotionOut o;
  o.t.H = temporal_blend(k.p, history, acc, c);
  o.t.G = dn4{p.n.x, p.n.y, p.n.z, p.z};
  o.t.I = p.inst;
  o.M = dn4{0.0f, 0.0f, 0.0f, 0.0f};
  if (MOMENTS) o.M = svgf_moments_blend(k.p, history, acc, sm, c, svgf_frame_luminance(c, alb));
  o.V = V;
  return o;
}

// ---- host side: the table (formed in double, rounded to float once) ----------------------------------------------------------
namespace motion_detail {
// inverse of the row-major 3x3 a: adjugate / determinant.  false: the determinant is 0 or not finite
inline bool inverse3(const double a[3][3], double inv[3][3]) {
  const double A = a[1][1] * a[2][2] - a[1][2] * a[2][1], B = -(a[1][0] * a[2][2] - a[1][2] * a[2][0]), C = a[1][0] * a[2][1] - a[1][1] * a[2][0];
  const double det = a[0][0] * A + a[0][1] * B + a[0][2] * C;
  if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return false;
  inv[0][0] = A / det;
  inv[0][1] = -(a[0][1] * a[2][2] - a[0][2] * a[2][1]) / det;
  inv[0][2] = (a[0][1] * a[1][2] - a[0][2] * a[1][1]) / det;
  inv[1][0] = B / det;
  inv[1][1] = (a[0][0] * a[2][2] - a[0][2] * a[2][0]) / det;
  inv[1][2] = -(a[0][0] * a[1][2] - a[0][2] * a[1][0]) / det;
  inv[2][0] = C / det;
  inv[2][1] = -(a[0][0] * a[2][1] - a[0][1] * a[2][0]) / det;
  inv[2][2] = (a[0][0] * a[1][1] - a[0][1] * a[1][0]) / det;
  return true;
}
// the 3x3 (row-major) and the translation of a transform in glm memory order (t[4 * c + r]); its fourth row is taken as 0 0 0 1
inline void affine_of(const float* t, double a[3][3], double tr[3]) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) a[r][c] = t[4 * c + r];
    tr[r] = t[12 + r];
  }
}
}  // namespace motion_detail

// The record of one instance whose transform was t_prev (16 floats, glm memory order) in the frame the history belongs to and is
// t_cur now
inline MotionRecord motion_record(const float* t_prev, const float* t_cur) {
  using namespace motion_detail;
  if (std::memcmp(t_prev, t_cur, 16 * sizeof(float)) == 0) return motion_record_of_class(kMotionStatic);
  double ap[3][3], ac[3][3], tp[3], tc[3], ipv[3][3], icv[3][3];
  affine_of(t_prev, ap, tp);
  affine_of(t_cur, ac, tc);
  if (!inverse3(ap, ipv) || !inverse3(ac, icv)) return motion_record_of_class(kMotionNoHistory);
  MotionRecord rec = motion_record_of_class(kMotionMoved);
  bool finite = true;
  for (int r = 0; r < 3; ++r) {
    double b[3], n[3];
    for (int c = 0; c < 3; ++c) {
      b[c] = (ap[r][0] * icv[0][c] + ap[r][1] * icv[1][c]) + ap[r][2] * icv[2][c];  // B3 = A_prev * A_cur^-1
      n[c] = (ac[c][0] * ipv[0][r] + ac[c][1] * ipv[1][r]) + ac[c][2] * ipv[2][r];  // N = transpose(A_cur * A_prev^-1)
    }
    const double bt = tp[r] - ((b[0] * tc[0] + b[1] * tc[1]) + b[2] * tc[2]);
    const float bf[4] = {(float)b[0], (float)b[1], (float)b[2], (float)bt};
    const float nf[3] = {(float)n[0], (float)n[1], (float)n[2]};
    for (float f : bf) finite = finite && std::isfinite(f);
    for (float f : nf) finite = finite && std::isfinite(f);
    rec.b[r] = dn4{bf[0], bf[1], bf[2], bf[3]};
    rec.n[r].x = nf[0];
    rec.n[r].y = nf[1];
    rec.n[r].z = nf[2];
  }
  return finite ? rec : motion_record_of_class(kMotionNoHistory);
}

// The table of `count` instances: t_prev and t_cur hold 16 floats per instance
inline void motion_table(const float* t_prev, const float* t_cur, uint32_t count, MotionRecord* out) {
  for (uint32_t i = 0; i < count; ++i) out[i] = motion_record(t_prev + 16ull * i, t_cur + 16ull * i);
}

}  // namespace gsp
