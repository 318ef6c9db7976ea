// tests/emu/motion_table_main.cpp -- TEST HARNESS, NOT A PRODUCT PATH.
//
// motion_table of csrc/pt_motion.h as a program of its own, for a run under AddressSanitizer / UndefinedBehaviorSanitizer
// (tests/test_motion_cpu.py): random rigid, affine, singular and non-finite transform pairs, the classes counted.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../gpuspectral_amd/csrc/pt_motion.h"

using namespace gsp;

int main(int argc, char** argv) {
  const unsigned seed = argc > 1 ? (unsigned)std::strtoul(argv[1], nullptr, 10) : 1u;
  const uint32_t count = argc > 2 ? (uint32_t)std::strtoul(argv[2], nullptr, 10) : 1000u;
  std::mt19937 rng(seed);
  std::uniform_real_distribution<float> u(-2.0f, 2.0f);
  std::vector<float> prev(16ull * count), cur(16ull * count);
  for (uint32_t i = 0; i < count; ++i) {
    float* p = &prev[16ull * i];
    float* c = &cur[16ull * i];
    for (int k = 0; k < 16; ++k) p[k] = c[k] = (k % 5 == 0) ? 1.0f + 0.25f * u(rng) : (k < 12 && k % 4 != 3 ? 0.2f * u(rng) : 0.0f);
    for (int k = 12; k < 15; ++k) p[k] = c[k] = u(rng);
    p[15] = c[15] = 1.0f;
    switch (i % 6) {
      case 0: break;  // static
      case 1: c[12] += u(rng); break;
      case 2: for (int k = 0; k < 12; ++k) if (k % 4 != 3) c[k] += 0.1f * u(rng); break;
      case 3: for (int k = 0; k < 3; ++k) c[4 + k] = 0.0f; break;  // scaled to nothing along one axis
      case 4: p[rng() % 15] = NAN; break;
      default: c[12] = INFINITY; break;
    }
  }
  std::vector<MotionRecord> out(count);
  motion_table(prev.data(), cur.data(), count, out.data());
  uint32_t n[3] = {0, 0, 0};
  for (const MotionRecord& r : out) {
    const uint32_t cls = motion_class(r);
    if (cls > 2) return 1;
    ++n[cls];
    for (int k = 0; k < 3; ++k) {
      const float f[7] = {r.b[k].x, r.b[k].y, r.b[k].z, r.b[k].w, r.n[k].x, r.n[k].y, r.n[k].z};
      for (float x : f)
        if (!std::isfinite(x) || (cls != kMotionMoved && x != 0.0f)) return 2;
    }
  }
  std::printf("%u static, %u moved, %u without history\n", n[0], n[1], n[2]);
  return 0;
}
