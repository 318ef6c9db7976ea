// tests/devfn/lights_bodies.h -- TEST HARNESS, NOT A PRODUCT PATH.
//
// One vector of sample_light_power (gpuspectral_amd/csrc/pt_shading.h; include/gpuspectral_pt.h "Light selection"), written once
// and compiled twice: for gfx950 by lights_devfn.hip and for the host by tests/emu/lights_emu.cpp.  The tests compare the two
// word for word.  Index checks happen on the host, before any launch (ok_light_pick).
#pragma once
#include "devfn_bodies.h"

namespace devfn {

// image: num_lights BAKED light records with their pick table straight behind (the layout of the resident table image).
// out8 = {position, emission, pdf, rng after the three draws}
GSP_HD void light_power1(uint64_t i, const gsp_triangle_light* image, uint32_t num_lights, const float* pos, const uint32_t* seeds,
                         float* out8) {
  uint32_t rng = seeds[i];
  const LightSample r = sample_light_power(image, (const gsp_light_pick*)(image + num_lights), num_lights, rng, ld3(pos + 3 * i));
  float* o = out8 + 8 * i;
  put3(o, r.position);
  put3(o + 3, r.emission);
  o[6] = r.pdf;
  o[7] = u2f(rng);
}

// every alias of the table names a light of the table
inline bool ok_light_pick(const gsp_light_pick* pick, uint32_t num_lights) {
  for (uint32_t j = 0; j < num_lights; ++j)
    if (pick[j].alias >= num_lights) return false;
  return true;
}

}  // namespace devfn
