// tests/emu/temporal_emu.cpp -- TEST HARNESS, NOT A PRODUCT PATH.
//
// Temporal accumulation of the library (include/gpuspectral_pt.h, "Temporal accumulation") compiled for the host: the very text
// the kernel k_temporal_reproject runs (csrc/pt_temporal.h), driven by a plain loop over the frame, plus gsp_temporal_accumulate's
// validation and the resolution of a gsp_temporal and of the two cameras into the kernel's constants.  Built into
// tests/emu/libtemporal_emu.so by the tests that use it (tests/temporal_util.py).
#include <vector>

#include "../../gpuspectral_amd/csrc/pt_temporal.h"

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

// the validation + struct_size rule.  Returns 0 and out4 = {bits(max_history as float), bits(alpha), bits(depth_tol), bits(normal_min)},
// or 1 and the error text in err (cap bytes)
int temporal_emu_resolve(const gsp_temporal* in, uint32_t* out4, char* err, uint32_t cap) {
  TemporalParams p;
  if (const char* why = resolve_temporal(in, p)) {
    put_error(why, err, cap);
    return 1;
  }
  out4[0] = f2u(p.max_history);
  out4[1] = f2u(p.alpha);
  out4[2] = f2u(p.depth_tol);
  out4[3] = f2u(p.normal_min);
  return 0;
}

// One gsp_temporal_accumulate of a full frame.  accum, albedo, geom: width * height records of 4 floats, ids: of 4 words (the
// frame and its feature planes); {h, g, i}_prev: the history read (may be NULL when history_valid == 0), {h, g, i}_out: the
// history written.  kept (optional): per pixel, bit i set = tap i passed the tap test, bit 7 = the projection found a tap inside
// the frame.  Returns 0, 1 (invalid gsp_temporal) or 2 (singular previous camera), with the text in err.
int temporal_emu_run(const gsp_temporal* in, const gsp_camera* cur, const gsp_camera* prev, int history_valid, uint32_t width, uint32_t height,
                     const float* accum, const float* albedo, const float* geom, const uint32_t* ids, const float* h_prev, const float* g_prev,
                     const uint32_t* i_prev, float* h_out, float* g_out, uint32_t* i_out, uint8_t* kept, char* err, uint32_t cap) {
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
  auto rec = [](const float* q, size_t i) { return dn4{q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]}; };
  auto fetch = [&](int x, int y, dn4& H_, dn4& G_, uint32_t& I_) {
    const size_t q = (size_t)y * width + (size_t)x;
    H_ = rec(h_prev, q);
    G_ = rec(g_prev, q);
    I_ = i_prev[q];
  };
  for (int y = 0; y < (int)height; ++y)
    for (int x = 0; x < (int)width; ++x) {
      const size_t i = (size_t)y * width + (size_t)x;
      const TemporalOut o = temporal_pixel(k, x, y, rec(accum, i), rec(albedo, i), rec(geom, i), ids[4 * i + 2], fetch);
      std::memcpy(h_out + 4 * i, &o.H, 16);
      std::memcpy(g_out + 4 * i, &o.G, 16);
      i_out[i] = o.I;
      if (kept) {
        uint8_t m = 0;
        if (k.history_valid) {
          const TemporalPixel px = temporal_classify(rec(albedo, i), rec(geom, i), ids[4 * i + 2]);
          const TemporalProj pr = temporal_project(k, px, x, y);
          if (pr.ok) {
            m = 0x80;
            for (int t = 0; t < 4; ++t) {
              const int qx = pr.x0 + (t & 1), qy = pr.y0 + (t >> 1);
              if (pr.w[t] == 0.0f || qx < 0 || qx >= (int)width || qy < 0 || qy >= (int)height) continue;
              dn4 H_, G_;
              uint32_t I_;
              fetch(qx, qy, H_, G_, I_);
              TemporalAcc acc = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
              temporal_tap(k.p, px, pr.ze, pr.w[t], H_, G_, I_, acc);
              if (acc.sw != 0.0f) m |= (uint8_t)(1u << t);
            }
          }
        }
        kept[i] = m;
      }
    }
  return 0;
}

}  // extern "C"
