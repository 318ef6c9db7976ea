// tests/emu/envlight_builder_main.cpp -- TEST HARNESS, NOT A PRODUCT PATH.
//
// The host side of the environment light (gpuspectral_amd/csrc/pt_envlight.h: the cell weights, the radiant sum, the record, the
// frame check) and the alias builder it feeds (pt_lightpick.h) as a stand-alone program for the sanitizers
// (tests/test_envlight_cpu.py builds it with -fsanitize=address,undefined): maps from 1 x 1 to beyond both cell caps, with NaN,
// infinite and negative texels; every table is checked, and the sampler and the shared function are run over it on the host.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../gpuspectral_amd/csrc/pt_lightpick.h"
#include "../../gpuspectral_amd/csrc/pt_envlight.h"

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static double urand() {  // xorshift64*, [0, 1)
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return (double)((g_state * 0x2545f4914f6cdd1dull) >> 11) / 9007199254740992.0;
}

int main() {
  using namespace gsp;
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const uint32_t sizes[][2] = {{1, 1}, {2, 1}, {1, 2}, {16, 8}, {13, 7}, {1030, 3}, {3, 300}, {512, 256}, {513, 257}, {600, 300}};
  unsigned maps = 0;
  for (const auto& sz : sizes) {
    for (int kind = 0; kind < 4; ++kind) {
      const uint32_t w = sz[0], h = sz[1];
      std::vector<float> texels(4 * (size_t)w * h);
      for (size_t i = 0; i < texels.size(); ++i) {
        const double u = urand();
        switch (kind) {
          case 0: texels[i] = (float)(u * 2.0); break;
          case 1: texels[i] = 0.0f; break;                                                    // black: the table falls back to uniform
          case 2: texels[i] = urand() < 0.05 ? nan : (urand() < 0.05 ? inf : (float)(u - 0.3)); break;  // nothing to rely on
          default: texels[i] = (i / 4) == (size_t)(w * (h / 2)) ? 1e30f : 1e-30f; break;      // one texel owns everything
        }
      }
      uint32_t cw = 0, ch = 0;
      const std::vector<double> wt = env_cell_weights(texels.data(), w, h, cw, ch);
      if (cw != (w < 512u ? w : 512u) || ch != (h < 256u ? h : 256u) || wt.size() != (size_t)cw * ch) return std::printf("%u x %u: wrong cell grid\n", w, h), 1;
      for (double x : wt)
        if (!(x >= 0.0) || !std::isfinite(x)) return std::printf("%u x %u: a weight is negative or not finite\n", w, h), 1;
      std::vector<gsp_light_pick> cells(wt.size());
      build_light_pick_from_weights(wt.data(), (uint32_t)wt.size(), cells.data());
      double sum = 0.0;
      for (const gsp_light_pick& c : cells) {
        if (c.alias >= cells.size()) return std::printf("%u x %u: alias out of range\n", w, h), 1;
        sum += (double)c.pmf_self;
      }
      if (std::fabs(sum - 1.0) > 1e-5) return std::printf("%u x %u: pmfs sum to %.9g\n", w, h, sum), 1;
      const double radiant = env_radiant_sum(texels.data(), w, h);
      if (!(radiant >= 0.0)) return std::printf("%u x %u: radiant sum %g\n", w, h, radiant), 1;
      (void)env_power_weight(radiant, 2.0f);
      float frame[16] = {0.8f, 0.0f, -0.6f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.6f, 0.0f, 0.8f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
      if (!env_frame_is_rotation(frame)) return std::printf("a rotation was refused\n"), 1;
      const EnvLightRecord rec = make_env_record(frame, cw, ch, 0.5f);
      TextureView T;
      T.env_texels = texels.data();
      T.env_width = w;
      T.env_height = h;
      for (int k = 0; k < 16; ++k) T.env_to_local[k] = frame[k];
      for (int s = 0; s < 2000; ++s) {  // the sampler and the shared function read nothing beyond the map and the table
        const EnvSample es = sample_env_light(T, cells.data(), rec, (uint32_t)(urand() * 4294967296.0), (float)urand(), (float)urand());
        if (es.cell_picked >= cells.size() || es.cell_of_L >= cells.size()) return std::printf("%u x %u: cell out of range\n", w, h), 1;
        const f3 odd = s % 3 == 0 ? mk3(nan, 0.0f, 1.0f) : (s % 3 == 1 ? mk3(0.0f, s % 2 ? 1.0f : -1.0f, 0.0f) : mk3(inf, -inf, 0.0f));
        if (env_eval(T, cells.data(), cw, ch, odd).cell >= cells.size()) return std::printf("%u x %u: cell out of range\n", w, h), 1;
      }
      ++maps;
    }
  }
  float scaled[16] = {1.01f, 0, 0, 0, 0, 1.01f, 0, 0, 0, 0, 1.01f, 0, 0, 0, 0, 1};
  if (env_frame_is_rotation(scaled)) return std::printf("a scale passed for a rotation\n"), 1;
  std::printf("%u maps ok\n", maps);
  return 0;
}
