// tests/devfn/delta_bodies.h -- TEST HARNESS, NOT A PRODUCT PATH.
//
// One vector of each function of gpuspectral_amd/csrc/pt_deltalight.h (include/gpuspectral_pt.h "Delta lights"), written once and
// compiled twice: for gfx950 by delta_devfn.hip and for the host by tests/emu/delta_emu.cpp.  The tests compare the two word
// for word.  The bodies read and write only element i of their arrays.
#pragma once
#include "devfn_bodies.h"

namespace devfn {

GSP_HD void spot_falloff1(uint64_t i, const float* c, const float* cos_cutoff, const float* cos_beam, float* out) {
  out[i] = spot_falloff(c[i], cos_cutoff[i], cos_beam[i]);
}

// rec16 = one gsp_delta_light as 16 words; out8 = {L, Ldist, emission, pdf}
GSP_HD void sample_delta_light1(uint64_t i, const float* rec16, const float* pos, const float* pmf, float* out8) {
  const DeltaSample ds = sample_delta_light(*(const gsp_delta_light*)(rec16 + 16 * i), ld3(pos + 3 * i), pmf[i]);
  float* o = out8 + 8 * i;
  put3(o, ds.L);
  o[3] = ds.Ldist;
  put3(o + 4, ds.emission);
  o[7] = ds.pdf;
}

}  // namespace devfn
