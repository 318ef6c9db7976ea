// tests/devfn/envlight_bodies.h -- TEST HARNESS, NOT A PRODUCT PATH.
//
// One vector of each device function of gpuspectral_amd/csrc/pt_envlight.h (include/gpuspectral_pt.h "Environment light"), written
// once and compiled twice: for gfx950 by envlight_devfn.hip and for the host by tests/emu/envlight_emu.cpp.  The tests compare the
// two word for word.  The bodies read the shared map, cell table and record, and read and write only element i of their arrays.
#pragma once
#include "devfn_bodies.h"

namespace devfn {

// out5 = {radiance, density, bits(cell)}
GSP_HD void env_eval1(uint64_t i, const TextureView& T, const gsp_light_pick* cells, const float* rec16, const float* dirs, float* out5) {
  const EnvLightRecord& rec = *(const EnvLightRecord*)rec16;
  const EnvEval ev = env_eval(T, cells, rec.cw, rec.ch, ld3(dirs + 3 * i));
  float* o = out5 + 5 * i;
  put3(o, ev.radiance);
  o[3] = ev.density;
  o[4] = u2f(ev.cell);
}

// draws3 = {bits(r2), e1, e2}; out9 = {L, emission, pdf, bits(cell picked), bits(cell of L)}
GSP_HD void sample_env_light1(uint64_t i, const TextureView& T, const gsp_light_pick* cells, const float* rec16, const float* draws3, float* out9) {
  const float* d = draws3 + 3 * i;
  const EnvSample es = sample_env_light(T, cells, *(const EnvLightRecord*)rec16, f2u(d[0]), d[1], d[2]);
  float* o = out9 + 9 * i;
  put3(o, es.L);
  put3(o + 3, es.emission);
  o[6] = es.pdf;
  o[7] = u2f(es.cell_picked);
  o[8] = u2f(es.cell_of_L);
}

}  // namespace devfn
