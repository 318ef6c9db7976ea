// tests/devfn/medium_bodies.h -- TEST HARNESS, NOT A PRODUCT PATH.
//
// One vector of each function of gpuspectral_amd/csrc/pt_medium.h (include/gpuspectral_pt.h "Scattering media"), written once and
// compiled twice: for gfx950 by medium_devfn.hip and for the host by tests/emu/scatter_emu.cpp.  The tests compare the two word
// for word.  The bodies read and write only element i of their arrays.
#pragma once
#include "devfn_bodies.h"

namespace devfn {

// out4 = {direction, pdf}
GSP_HD void sample_hg1(uint64_t i, const float* d, const float* g, const float* u1, const float* u2, float* out4) {
  float pdf;
  const f3 r = sample_hg(ld3(d + 3 * i), g[i], u1[i], u2[i], pdf);
  put3(out4 + 4 * i, r);
  out4[4 * i + 3] = pdf;
}

GSP_HD void hg_pdf1(uint64_t i, const float* g, const float* cos_theta, float* pdf) { pdf[i] = hg_pdf(g[i], cos_theta[i]); }

// out6 = {scatter (0 / 1), valid (0 / 1), s, w.r, w.g, w.b}
GSP_HD void medium_event1(uint64_t i, const float* sigma_a, const float* sigma_s, const float* t, const float* u_c, const float* u_d,
                          const float* weight, float* out6) {
  const MediumEvent ev = medium_event(ld3(sigma_a + 3 * i), ld3(sigma_s + 3 * i), t[i], u_c[i], u_d[i], ld3(weight + 3 * i));
  float* o = out6 + 6 * i;
  o[0] = ev.scatter ? 1.0f : 0.0f;
  o[1] = ev.valid ? 1.0f : 0.0f;
  o[2] = ev.s;
  put3(o + 3, ev.w);
}

}  // namespace devfn
