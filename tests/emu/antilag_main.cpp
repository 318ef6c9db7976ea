// tests/emu/antilag_main.cpp -- TEST HARNESS, NOT A PRODUCT PATH.
//
// The emulation of the temporal anti-lag (tests/emu/antilag_emu.cpp, i.e. csrc/pt_antilag.h on the host) as a program of its own,
// for a run under AddressSanitizer / UndefinedBehaviorSanitizer (tests/test_antilag_cpu.py): a 33 x 9 and a 1 x 1 frame at radius
// 3, two calls each (without and with a fast history) in every context state, on planes of exactly the frame's size.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "antilag_emu.cpp"

namespace {
int run(uint32_t w, uint32_t h, unsigned seed) {
  std::mt19937 rng(seed);
  std::uniform_real_distribution<float> u(0.0f, 1.0f);
  const size_t n = (size_t)w * h;
  gsp_camera cam{};
  for (int i = 0; i < 4; ++i) cam.to_world[5 * i] = 1.0f;
  cam.to_world[14] = 5.0f;
  cam.fov = 0.6f;
  gsp_camera cam2 = cam;
  cam2.to_world[12] = 0.01f;
  gsp_antilag al{};
  al.struct_size = sizeof(al);
  al.radius = 3;
  al.fast_history = 2;
  std::vector<float> accum(4 * n), albedo(4 * n), geom(4 * n), f0(4 * n), f1(4 * n), g0(4 * n), g1(4 * n), hist(4 * n);
  std::vector<uint32_t> ids(4 * n), i0(n), i1(n);
  std::vector<MotionRecord> table(3);
  const float still[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  float shifted[16];
  std::memcpy(shifted, still, sizeof(still));
  shifted[12] = 0.02f;
  table[0] = motion_record(still, still);
  table[1] = motion_record(still, shifted);
  table[2] = motion_record_of_class(kMotionNoHistory);
  size_t touched = 0;
  for (int follow = 0; follow < 2; ++follow)
    for (int demod = 0; demod < 2; ++demod) {
      for (size_t i = 0; i < n; ++i) {
        const bool surf = u(rng) < 0.85f;
        const uint32_t inst = surf ? rng() % 4 : kTemporalBackground;  // (3: an index the table does not have)
        const float z = 4.0f + u(rng);
        const float c[4] = {u(rng) < 0.05f ? NAN : 4.0f * u(rng), u(rng), u(rng), 1.0f};
        const float a[4] = {surf ? u(rng) : 0.0f, surf ? u(rng) : 0.0f, surf ? u(rng) : 0.0f, surf ? 1.0f : 0.0f};
        const float g[4] = {0.0f, 0.0f, surf ? -1.0f : 0.0f, surf ? z : 0.0f};
        for (int k = 0; k < 4; ++k) {
          accum[4 * i + k] = c[k];
          albedo[4 * i + k] = a[k];
          geom[4 * i + k] = g[k];
          g0[4 * i + k] = g1[4 * i + k] = g[k];
          hist[4 * i + k] = k < 3 ? 2.0f * u(rng) : (u(rng) < 0.1f ? 0.0f : 5.0f);
          ids[4 * i + k] = k == 2 ? inst : 0u;
        }
        i0[i] = i1[i] = inst;
      }
      char err[128];
      int rc = antilag_emu_run(&al, nullptr, &cam, nullptr, 0, 0, w, h, follow, demod, accum.data(), albedo.data(), geom.data(), ids.data(), nullptr, nullptr, nullptr,
                               nullptr, 0, hist.data(), g1.data(), i1.data(), f0.data(), err, sizeof(err));
      if (rc) return 10 + rc;
      for (size_t i = 0; i < n; ++i)
        if (f0[4 * i + 3] != (std::isfinite(accum[4 * i]) ? 1.0f : 0.0f)) return 3;
      rc = antilag_emu_run(&al, nullptr, &cam2, &cam, 1, 1, w, h, follow, demod, accum.data(), albedo.data(), geom.data(), ids.data(), f0.data(), g0.data(), i0.data(),
                           follow ? table.data() : nullptr, follow ? 3u : 0u, hist.data(), g1.data(), i1.data(), f1.data(), err, sizeof(err));
      if (rc) return 20 + rc;
      for (size_t i = 0; i < n; ++i) {
        if (!(f1[4 * i + 3] >= 0.0f && f1[4 * i + 3] <= 2.0f)) return 4;
        touched += f1[4 * i + 3] == 2.0f;
      }
    }
  std::printf("%u x %u: %zu records of length 2\n", w, h, touched);
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  const unsigned seed = argc > 1 ? (unsigned)std::strtoul(argv[1], nullptr, 10) : 1u;
  if (int rc = run(33, 9, seed)) return rc;
  return run(1, 1, seed + 1);
}
