// tests/emu/illum_emu.cpp -- TEST HARNESS, NOT A PRODUCT PATH.
//
// The illumination history of the library (include/gpuspectral_pt.h, "Illumination history") compiled for the host: the very text
// the kernels k_temporal_reproject_illum / k_illum_prepare / k_illum_image / k_svgf_atrous_feedback run (csrc/pt_illum.h), driven
// by plain loops over the frame.  With demod == 0 the accumulate runs the drivers the library runs with demodulation off
// (temporal_pixel, temporal_pixel_moments, temporal_pixel_follow), so that "off changes no bit" can be checked against
// TemporalEmu / SvgfEmu / MotionEmu.  Built into tests/emu/libillum_emu.so by the tests that use it (tests/illum_util.py).
#include <vector>

#include "../../gpuspectral_amd/csrc/pt_illum.h"

using namespace gsp;

namespace {
void put_error(const char* why, char* err, uint32_t cap) {
  if (err && cap) {
    std::strncpy(err, why, cap - 1);
    err[cap - 1] = 0;
  }
}
dn4 rec(const float* q, size_t i) { return dn4{q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]}; }
}  // namespace

extern "C" {

// One gsp_temporal_accumulate of a full frame under the context state (moments, follow, demod), as motion_emu_run: m_prev / m_out
// only with moments, table / v_out only with follow.  Returns 0, 1 (invalid gsp_temporal) or 2 (singular previous camera).
int illum_emu_run(const gsp_temporal* in, const gsp_camera* cur, const gsp_camera* prev, int history_valid, uint32_t width, uint32_t height, int moments,
                  int follow, int demod, const float* accum, const float* albedo, const float* geom, const uint32_t* ids, const float* h_prev,
                  const float* g_prev, const uint32_t* i_prev, const float* m_prev, const void* table, uint32_t num_records, float* h_out, float* g_out,
                  uint32_t* i_out, float* m_out, float* v_out, char* err, uint32_t cap) {
  TemporalParams p;
  if (const char* why = resolve_temporal(in, p)) {
    put_error(why, err, cap);
    return 1;
  }
  TemporalConsts k;
  if (const char* why = temporal_consts(*cur, prev, history_valid != 0, width, height, p, k)) {
    put_error(why, err, cap);
    return 2;
  }
  const MotionRecord* recs = (const MotionRecord*)table;
  auto fetch4 = [&](int x, int y, dn4& H_, dn4& G_, uint32_t& I_, dn4& M_) {
    const size_t q = (size_t)y * width + (size_t)x;
    H_ = rec(h_prev, q);
    G_ = rec(g_prev, q);
    I_ = i_prev[q];
    if (moments) M_ = rec(m_prev, q);
  };
  auto fetch3 = [&](int x, int y, dn4& H_, dn4& G_, uint32_t& I_) {
    const size_t q = (size_t)y * width + (size_t)x;
    H_ = rec(h_prev, q);
    G_ = rec(g_prev, q);
    I_ = i_prev[q];
  };
  for (int y = 0; y < (int)height; ++y)
    for (int x = 0; x < (int)width; ++x) {
      const size_t i = (size_t)y * width + (size_t)x;
      const uint32_t inst = ids[4 * i + 2];
      const dn4 c = rec(accum, i), a = rec(albedo, i), g = rec(geom, i);
      // what the kernels hand the driver: following, the instance's record (class 2 for an index the table does not have);
      // otherwise the constant of class 0 and no wave of moved pixels
      const MotionRecord r = !follow ? motion_record_of_class(kMotionStatic)
                                     : (k.history_valid && inst < num_records ? recs[inst] : motion_record_of_class(kMotionNoHistory));
      MotionOut o;
      if (demod) {
        o = moments ? illum_pixel<true>(k, x, y, c, a, g, inst, r, follow != 0, fetch4) : illum_pixel<false>(k, x, y, c, a, g, inst, r, follow != 0, fetch4);
      } else if (follow) {
        o = moments ? temporal_pixel_follow<true>(k, x, y, c, a, g, inst, r, true, fetch4) : temporal_pixel_follow<false>(k, x, y, c, a, g, inst, r, true, fetch4);
      } else if (moments) {
        const TemporalMomentsOut t = temporal_pixel_moments(k, x, y, c, a, g, inst, fetch4);
        o.t = t.t;
        o.M = t.M;
      } else {
        o.t = temporal_pixel(k, x, y, c, a, g, inst, fetch3);
      }
      std::memcpy(h_out + 4 * i, &o.t.H, 16);
      std::memcpy(g_out + 4 * i, &o.t.G, 16);
      i_out[i] = o.t.I;
      if (moments) std::memcpy(m_out + 4 * i, &o.M, 16);
      if (follow) std::memcpy(v_out + 4 * i, &o.V, 16);
    }
  return 0;
}

// gsp_download_temporal_image: n records of H and of this frame's albedo plane in, n records out
void illum_emu_image(const float* hist, const float* albedo, uint64_t n, int demod, float* out) {
  for (size_t i = 0; i < n; ++i) {
    const dn4 o = demod ? illum_image(rec(hist, i), rec(albedo, i)) : rec(hist, i);
    std::memcpy(out + 4 * i, &o, 16);
  }
}

// gsp_download_temporal_svgf (fb_levels == 0) or gsp_temporal_svgf_feedback (fb_levels > 0) of a full frame: hist, moments,
// albedo, geom, out and h_fb are width * height records of 4 floats; h_fb (only written with fb_levels > 0) receives the history
// after the feedback.  Returns 1 on invalid parameters, 3 on levels outside 1 .. iterations.
int illum_emu_svgf(const gsp_denoise* dn, const gsp_svgf* in, const float* hist, const float* moments, const float* albedo, const float* geom, uint32_t width,
                   uint32_t height, int demod, uint32_t fb_levels, int with_levels, float* out, float* h_fb) {
  SvgfConsts k;
  if (resolve_svgf(dn, in, k)) return 1;
  if (with_levels && (fb_levels < 1 || fb_levels > k.iterations)) return 3;
  const size_t n = (size_t)width * height;
  std::vector<dn4> E(n), E2(n), A(n), G(n);
  std::vector<float> V(n, 0.0f), V2(n);
  for (size_t i = 0; i < n; ++i) {
    if (demod) illum_prepare(rec(hist, i), rec(albedo, i), E[i], A[i]);
    else denoise_prepare(rec(hist, i), rec(albedo, i), E[i], A[i]);
    G[i] = rec(geom, i);
  }
  for (int y = 0; y < (int)height; ++y)
    for (int x = 0; x < (int)width; ++x) {
      const size_t i = (size_t)y * width + x;
      V[i] = svgf_variance_pixel(k, (int)width, (int)height, x, y, hist[4 * i + 3], rec(moments, i), [&](int qx, int qy, float& L_, float& valid_, dn4& G_) {
        const size_t q = (size_t)qy * width + qx;
        L_ = E[q].w;
        valid_ = A[q].w;
        G_ = G[q];
      });
    }
  for (uint32_t lvl = 0; lvl < k.iterations; ++lvl) {
    for (int y = 0; y < (int)height; ++y)
      for (int x = 0; x < (int)width; ++x) {
        const SvgfLevelOut o = svgf_pixel_level(k, lvl, (int)width, (int)height, x, y, [&](int qx, int qy, dn4& E_, dn4& A_, dn4& G_, float& V_) {
          const size_t q = (size_t)qy * width + qx;
          E_ = E[q];
          A_ = A[q];
          G_ = G[q];
          V_ = V[q];
        });
        E2[(size_t)y * width + x] = o.E;
        V2[(size_t)y * width + x] = o.V;
      }
    E.swap(E2);
    V.swap(V2);
    if (with_levels && lvl + 1 == fb_levels)
      for (size_t i = 0; i < n; ++i) {
        const dn4 o = demod ? illum_feedback<true>(E[i], A[i], rec(hist, i)) : illum_feedback<false>(E[i], A[i], rec(hist, i));
        std::memcpy(h_fb + 4 * i, &o, 16);
      }
  }
  for (size_t i = 0; i < n; ++i) {
    const dn4 o = denoise_finish(E[i], A[i], rec(hist, i));
    std::memcpy(out + 4 * i, &o, 16);
  }
  return 0;
}

// gsp_download_temporal_denoised of a full frame whose history is demodulated or not
int illum_emu_denoise(const gsp_denoise* in, const float* hist, const float* albedo, const float* geom, uint32_t width, uint32_t height, int demod,
                      float* out) {
  DenoiseConsts k;
  if (resolve_denoise(in, k)) return 1;
  const size_t n = (size_t)width * height;
  std::vector<dn4> E[2], A(n), G(n);
  E[0].resize(n);
  E[1].resize(n);
  for (size_t i = 0; i < n; ++i) {
    if (demod) illum_prepare(rec(hist, i), rec(albedo, i), E[0][i], A[i]);
    else denoise_prepare(rec(hist, i), rec(albedo, i), E[0][i], A[i]);
    G[i] = rec(geom, i);
  }
  for (uint32_t level = 0; level < k.iterations; ++level) {
    const std::vector<dn4>& in_ = E[level & 1u];
    std::vector<dn4>& out_ = E[(level + 1u) & 1u];
    for (int y = 0; y < (int)height; ++y)
      for (int x = 0; x < (int)width; ++x)
        out_[(size_t)y * width + x] = denoise_pixel_level(k, level, (int)width, (int)height, x, y, [&](int qx, int qy, dn4& E_, dn4& A_, dn4& G_) {
          const size_t q = (size_t)qy * width + qx;
          E_ = in_[q];
          A_ = A[q];
          G_ = G[q];
        });
  }
  const std::vector<dn4>& fin = E[k.iterations & 1u];
  for (size_t i = 0; i < n; ++i) {
    const dn4 o = denoise_finish(fin[i], A[i], rec(hist, i));
    std::memcpy(out + 4 * i, &o, 16);
  }
  return 0;
}

}  // extern "C"
