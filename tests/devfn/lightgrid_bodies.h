// tests/devfn/lightgrid_bodies.h -- TEST HARNESS, NOT A PRODUCT PATH.
//
// One vector of each device function of gpuspectral_amd/csrc/pt_lightgrid.h (include/gpuspectral_pt.h "Light grid"), written once
// and compiled twice: for gfx950 by lightgrid_devfn.hip and for the host by tests/emu/lightgrid_emu.cpp.  The tests compare the two
// word for word.  The bodies read the shared grid image and fallback table, and read and write only element i of their arrays.
#pragma once
#include "devfn_bodies.h"

#include "../../gpuspectral_amd/csrc/pt_lightgrid.h"

namespace devfn {

// out4 = {cell number (0xffffffff: the fallback), ix, iy, iz}
GSP_HD void lightgrid_cell1(uint64_t i, const uint8_t* grid, const float* pos3, uint32_t* out4) {
  const LightGridHeader g = *(const LightGridHeader*)grid;
  uint32_t* o = out4 + 4 * i;
  o[0] = lightgrid_cell(g, ld3(pos3 + 3 * i), o[1], o[2], o[3]);
}

// out2 = {light index, bits(pmf)} of the draw r[i] at pos3[i]
GSP_HD void lightgrid_pick1(uint64_t i, const uint8_t* grid, const gsp_light_pick* fallback, uint32_t num_lights, const float* pos3, const uint32_t* r, uint32_t* out2) {
  float pmf;
  out2[2 * i] = lightgrid_pick(grid, fallback, num_lights, ld3(pos3 + 3 * i), r[i], pmf);
  out2[2 * i + 1] = f2u(pmf);
}

// tri12 = {v0, v1, v2, emission}; out1 = p_sel of that triangle hit by a ray from pos3[i]
GSP_HD void lightgrid_hit_pmf1(uint64_t i, const uint8_t* grid, const gsp_light_pick* fallback, uint32_t num_lights, const float* pos3, const float* tri12, float* out1) {
  const float* t = tri12 + 12 * i;
  const f3 v0 = ld3(t), v1 = ld3(t + 3), v2 = ld3(t + 6);
  out1[i] = lightgrid_hit_select_pmf(grid, fallback, num_lights, 1.0f / (float)num_lights, ld3(pos3 + 3 * i), v0, v1, v2, ld3(t + 9), light_hit_area(v0, v1, v2));
}

}  // namespace devfn
