// tests/emu/motion_emu.cpp -- TEST HARNESS, NOT A PRODUCT PATH.
//
// Temporal accumulation with the moved instances followed (include/gpuspectral_pt.h, "Temporal accumulation: moved instances")
// compiled for the host: the very text the kernel k_temporal_reproject_follow runs (csrc/pt_motion.h), driven by a plain loop over
// the frame, plus the host-side table of the per-instance records.  Built into tests/emu/libmotion_emu.so by the tests that use
// it (tests/motion_util.py).
#include <vector>

#include "../../gpuspectral_amd/csrc/pt_motion.h"

using namespace gsp;

namespace {
void put_error(const char* why, char* err, uint32_t cap) {
  if (err && cap) {
    std::strncpy(err, why, cap - 1);
    err[cap - 1] = 0;
  }
}
}  // namespace

extern "C" {

// motion_table: t_prev / t_cur hold 16 floats per instance, out 24 words per instance (the record as the device reads it)
void motion_emu_table(const float* t_prev, const float* t_cur, uint32_t count, void* out) { motion_table(t_prev, t_cur, count, (MotionRecord*)out); }

// One followed gsp_temporal_accumulate of a full frame, as temporal_emu_run / svgf_emu_accumulate: m_prev / m_out only with
// moments != 0; table = num_records records (not read when history_valid == 0); v_out = the motion plane.  Returns 0, 1 (invalid
// gsp_temporal) or 2 (singular previous camera), with the text in err.
int motion_emu_run(const gsp_temporal* in, const gsp_camera* cur, const gsp_camera* prev, int history_valid, uint32_t width, uint32_t height, int moments,
                   const float* accum, const float* albedo, const float* geom, const uint32_t* ids, const float* h_prev, const float* g_prev,
                   const uint32_t* i_prev, const float* m_prev, const void* table, uint32_t num_records, float* h_out, float* g_out, uint32_t* i_out,
                   float* m_out, float* v_out, char* err, uint32_t cap) {
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
  auto rec = [](const float* q, size_t i) { return dn4{q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]}; };
  auto fetch = [&](int x, int y, dn4& H_, dn4& G_, uint32_t& I_, dn4& M_) {
    const size_t q = (size_t)y * width + (size_t)x;
    H_ = rec(h_prev, q);
    G_ = rec(g_prev, q);
    I_ = i_prev[q];
    if (moments) M_ = rec(m_prev, q);
  };
  for (int y = 0; y < (int)height; ++y)
    for (int x = 0; x < (int)width; ++x) {
      const size_t i = (size_t)y * width + (size_t)x;
      const uint32_t inst = ids[4 * i + 2];
      const MotionRecord r = k.history_valid && inst < num_records ? recs[inst] : motion_record_of_class(kMotionNoHistory);
      const MotionOut o = moments ? temporal_pixel_follow<true>(k, x, y, rec(accum, i), rec(albedo, i), rec(geom, i), inst, r, true, fetch)
                                  : temporal_pixel_follow<false>(k, x, y, rec(accum, i), rec(albedo, i), rec(geom, i), inst, r, true, fetch);
      std::memcpy(h_out + 4 * i, &o.t.H, 16);
      std::memcpy(g_out + 4 * i, &o.t.G, 16);
      i_out[i] = o.t.I;
      if (moments) std::memcpy(m_out + 4 * i, &o.M, 16);
      std::memcpy(v_out + 4 * i, &o.V, 16);
    }
  return 0;
}

}  // extern "C"
