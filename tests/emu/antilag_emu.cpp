// tests/emu/antilag_emu.cpp -- TEST HARNESS, NOT A PRODUCT PATH.
//
// The temporal anti-lag of the library (include/gpuspectral_pt.h, "Temporal anti-lag") compiled for the host: the very text the
// kernels k_antilag_fast / k_antilag_clamp run (csrc/pt_antilag.h), driven by plain loops over the frame.  Built into
// tests/emu/libantilag_emu.so by the tests that use it (tests/antilag_util.py) and, with a main of its own, into the program of
// tests/emu/antilag_main.cpp.
#include <vector>

#include "../../gpuspectral_amd/csrc/pt_antilag.h"

using namespace gsp;

namespace {
void put_error(const char* why, char* err, uint32_t cap) {
  if (err && cap) {
    std::strncpy(err, why, cap - 1);
    err[cap - 1] = 0;
  }
}
dn4 rec(const float* q, size_t i) { return dn4{q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]}; }

// Step B over a full frame, in place on h
void clamp_frame(const AntilagParams& a, float normal_min, uint32_t width, uint32_t height, const float* f, const float* g, const uint32_t* ids, float* h) {
  for (int y = 0; y < (int)height; ++y)
    for (int x = 0; x < (int)width; ++x) {
      const size_t i = (size_t)y * width + (size_t)x;
      const AntilagClampOut o = antilag_clamp_pixel(a, normal_min, (int)width, (int)height, x, y, rec(h, i), [&](int qx, int qy, dn4& F_, dn4& G_, uint32_t& I_) {
        const size_t q = (size_t)qy * width + (size_t)qx;
        F_ = rec(f, q);
        G_ = rec(g, q);
        I_ = ids[q];
      });
      if (o.changed) std::memcpy(h + 4 * i, &o.H, 16);
    }
}
}  // namespace

extern "C" {

// What a gsp_antilag comes to: out = {fast_history, radius, sigma_scale}.  Returns 0, or 4 and the refusal's text.
int antilag_emu_resolve(const gsp_antilag* in, float* out, char* err, uint32_t cap) {
  AntilagParams a;
  if (const char* why = resolve_antilag(in, a)) {
    put_error(why, err, cap);
    return 4;
  }
  out[0] = a.fast_history;
  out[1] = (float)a.radius;
  out[2] = a.sigma_scale;
  return 0;
}

// Step B alone on given planes: f = F', g and ids = G and I of the newest set, h = its H (clamped in place)
int antilag_emu_clamp(const gsp_antilag* in, float normal_min, uint32_t width, uint32_t height, const float* f, const float* g, const uint32_t* ids, float* h) {
  AntilagParams a;
  if (resolve_antilag(in, a)) return 4;
  clamp_frame(a, normal_min, width, height, f, g, ids, h);
  return 0;
}

// One gsp_temporal_antilag after the gsp_temporal_accumulate of a full frame under the context state (follow, demod).  The
// accumulate's own arguments: temporal, the two cameras, history_valid, the frame's planes, the table.  f_prev (the older fast
// plane; only read with fast_valid), g_prev / i_prev (the older history set; only read with history_valid and fast_valid);
// h_new (clamped in place), g_new, i_new: the set the accumulate wrote; f_out: F'.
// Returns 0, 1 (invalid gsp_temporal), 2 (singular previous camera) or 4 (invalid gsp_antilag).
int antilag_emu_run(const gsp_antilag* al, const gsp_temporal* in, const gsp_camera* cur, const gsp_camera* prev, int history_valid, int fast_valid, uint32_t width,
                    uint32_t height, int follow, int demod, const float* accum, const float* albedo, const float* geom, const uint32_t* ids, const float* f_prev,
                    const float* g_prev, const uint32_t* i_prev, const void* table, uint32_t num_records, float* h_new, const float* g_new, const uint32_t* i_new,
                    float* f_out, char* err, uint32_t cap) {
  TemporalParams p;
  if (const char* why = resolve_temporal(in, p)) {
    put_error(why, err, cap);
    return 1;
  }
  AntilagParams a;
  if (const char* why = resolve_antilag(al, a)) {
    put_error(why, err, cap);
    return 4;
  }
  TemporalConsts ka;
  if (const char* why = temporal_consts(*cur, prev, history_valid != 0, width, height, p, ka)) {
    put_error(why, err, cap);
    return 2;
  }
  const TemporalConsts k = antilag_fast_consts(ka, a, fast_valid != 0);
  const MotionRecord* recs = (const MotionRecord*)table;
  auto fetch = [&](int x, int y, dn4& F_, dn4& G_, uint32_t& I_) {
    const size_t q = (size_t)y * width + (size_t)x;
    F_ = rec(f_prev, q);
    G_ = rec(g_prev, q);
    I_ = i_prev[q];
  };
  for (int y = 0; y < (int)height; ++y)
    for (int x = 0; x < (int)width; ++x) {
      const size_t i = (size_t)y * width + (size_t)x;
      const uint32_t inst = ids[4 * i + 2];
      const dn4 c = rec(accum, i), al_ = rec(albedo, i), g = rec(geom, i);
      // what the kernel hands the driver: following, the instance's record of the accumulate's table (class 2 for an index it
      // does not have); otherwise the constant of class 0 and no wave of moved pixels
      const MotionRecord r = !follow ? motion_record_of_class(kMotionStatic)
                                     : (ka.history_valid && inst < num_records ? recs[inst] : motion_record_of_class(kMotionNoHistory));
      dn4 F;
      if (demod) {
        F = follow ? antilag_fast_pixel<true, true>(k, x, y, c, al_, g, inst, r, true, fetch) : antilag_fast_pixel<false, true>(k, x, y, c, al_, g, inst, r, false, fetch);
      } else {
        F = follow ? antilag_fast_pixel<true, false>(k, x, y, c, al_, g, inst, r, true, fetch) : antilag_fast_pixel<false, false>(k, x, y, c, al_, g, inst, r, false, fetch);
      }
      std::memcpy(f_out + 4 * i, &F, 16);
    }
  clamp_frame(a, k.p.normal_min, width, height, f_out, g_new, i_new, h_new);
  return 0;
}

}  // extern "C"
