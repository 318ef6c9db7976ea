// tests/emu/lightpick_main.cpp -- TEST HARNESS, NOT A PRODUCT PATH.
//
// The light pick table builder (gpuspectral_amd/csrc/pt_lightpick.h) as a stand-alone program for the sanitizers
// (tests/test_lights_cpu.py builds it with -fsanitize=address,undefined): random and degenerate weight vectors and light records,
// n = 1 .. 4096, every table checked against the invariants of include/gpuspectral_pt.h "Light selection".
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../gpuspectral_amd/csrc/pt_lightpick.h"

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static double urand() {  // xorshift64*, [0, 1)
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return (double)((g_state * 0x2545f4914f6cdd1dull) >> 11) / 9007199254740992.0;
}

static int check(const std::vector<double>& w, const std::vector<gsp_light_pick>& t, const char* what) {
  const uint32_t n = (uint32_t)w.size();
  const double two32 = 4294967296.0;
  std::vector<double> mass(n);
  bool any = false;
  for (uint32_t j = 0; j < n; ++j) any = any || (std::isfinite(w[j]) && w[j] > 0.0);
  for (uint32_t j = 0; j < n; ++j) {
    if (t[j].alias >= n) return std::printf("%s: n = %u: alias out of range\n", what, n), 1;
    if (t[j].threshold == 0xffffffffu && t[j].alias != j) return std::printf("%s: n = %u: saturated entry with a foreign alias\n", what, n), 1;
    mass[j] = t[j].threshold == 0xffffffffu ? two32 : (double)t[j].threshold;
  }
  for (uint32_t j = 0; j < n; ++j)
    if (t[j].alias != j) mass[t[j].alias] += two32 - (double)t[j].threshold;
  double sum = 0.0;
  for (uint32_t j = 0; j < n; ++j) {
    const double p = mass[j] / ((double)n * two32);
    sum += p;
    const bool zero = any && !(std::isfinite(w[j]) && w[j] > 0.0);
    if (zero && p != 0.0) return std::printf("%s: n = %u: a light of weight 0 has probability %g\n", what, n, p), 1;
    if (t[j].pmf_self != (float)p) return std::printf("%s: n = %u: pmf_self is not float32(p)\n", what, n), 1;
  }
  if (std::fabs(sum - 1.0) > 1e-12) return std::printf("%s: n = %u: sum p = %.17g\n", what, n, sum), 1;
  return 0;
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  unsigned tables = 0;
  const uint32_t sizes[] = {1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 66, 127, 255, 256, 336, 1000, 1023, 1024, 4095, 4096};
  for (uint32_t n : sizes) {
    for (int kind = 0; kind < 8; ++kind) {
      std::vector<double> w(n);
      for (uint32_t i = 0; i < n; ++i) {
        const double u = urand();
        switch (kind) {
          case 0: w[i] = std::pow(10.0, -6.0 + 10.0 * u); break;                      // 1e-6 .. 1e4
          case 1: w[i] = urand() < 0.3 ? 0.0 : u; break;                              // zeros
          case 2: w[i] = 0.0; break;                                                  // all zero
          case 3: w[i] = i % 3 == 0 ? nan : (i % 3 == 1 ? inf : -u); break;           // nothing usable
          case 4: w[i] = 1.0; break;                                                  // all equal: every entry saturated
          case 5: w[i] = i == 0 ? 1e300 : 1e-300; break;                              // one light owns everything
          case 6: w[i] = i % 2 ? 1e308 : 1e307; break;                                // a sum beyond double
          default: w[i] = urand() < 0.1 ? nan : (urand() < 0.1 ? -1.0 : std::pow(2.0, -40.0 * u)); break;
        }
      }
      std::vector<gsp_light_pick> t(n);
      gsp::build_light_pick_from_weights(w.data(), n, t.data());
      if (kind == 6) {
        for (double& x : w) x /= 1e308;  // (the builder scales such a vector down; the shares are what counts)
      }
      if (check(w, t, "weights")) return 1;
      ++tables;
    }
    // light records, some degenerate
    std::vector<gsp_triangle_light> L(n);
    std::vector<double> w(n);
    for (uint32_t i = 0; i < n; ++i) {
      for (int v = 0; v < 3; ++v)
        for (int c = 0; c < 4; ++c) L[i].positions[v][c] = (float)(urand() * 4.0 - 2.0);
      for (int c = 0; c < 4; ++c) L[i].radiance[c] = (float)(urand() * 50.0);
      if (i % 11 == 3) L[i].radiance[1] = (float)nan;
      if (i % 13 == 5) L[i].positions[1][0] = (float)inf;
      if (i % 17 == 7)
        for (int c = 0; c < 3; ++c) L[i].positions[2][c] = L[i].positions[0][c];
      w[i] = gsp::light_pick_weight(L[i]);
    }
    std::vector<gsp_light_pick> t(n);
    gsp::build_light_pick(L.data(), n, t.data());
    if (check(w, t, "records")) return 1;
    ++tables;
  }
  gsp::build_light_pick(nullptr, 0, nullptr);  // no lights: nothing is touched
  std::printf("%u tables ok\n", tables);
  return 0;
}
