// tests/emu/taa_main.cpp -- TEST HARNESS, NOT A PRODUCT PATH.
//
// The emulation of temporal anti-aliasing (tests/emu/taa_emu.cpp, i.e. csrc/pt_taa.h on the host) as a program of its own, for a
// run under AddressSanitizer / UndefinedBehaviorSanitizer (tests/test_taa_cpu.py): a 33 x 9 and a 1 x 1 frame, three resolves each
// (without and with a history) under every tone map and both encodes, on planes of exactly the frame's size, with motion records
// that point out of the frame, carry a zero class, a small weight, NaN and huge offsets, and sources with NaN, Inf and negatives.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "taa_emu.cpp"

namespace {
int run(uint32_t w, uint32_t h, unsigned seed) {
  std::mt19937 rng(seed);
  std::uniform_real_distribution<float> u(0.0f, 1.0f);
  const size_t n = (size_t)w * h;
  std::vector<float> src(4 * n), motion(4 * n), d0(4 * n), d1(4 * n);
  std::vector<uint32_t> words(n);
  size_t blended = 0;
  for (uint32_t tonemap = 0; tonemap < 3; ++tonemap)
    for (int srgb = 0; srgb < 2; ++srgb) {
      gsp_display disp{};
      disp.struct_size = sizeof(disp);
      disp.tonemap = tonemap;
      disp.gamma = srgb ? 0.0f : 2.2f;
      disp.exposure = 0.5f;
      gsp_taa taa{};
      taa.struct_size = sizeof(taa);
      taa.alpha = 0.25f;
      taa.sigma_clip = 1.5f;
      for (int frame = 0; frame < 3; ++frame) {
        for (size_t i = 0; i < n; ++i) {
          const float odd = u(rng);
          src[4 * i + 0] = odd < 0.03f ? NAN : (odd < 0.06f ? INFINITY : (odd < 0.09f ? -1.0f : 3.0f * u(rng)));
          src[4 * i + 1] = 2.0f * u(rng);
          src[4 * i + 2] = u(rng);
          src[4 * i + 3] = NAN;  // (not read)
          const float kind = u(rng);
          motion[4 * i + 0] = kind < 0.05f ? NAN : (kind < 0.1f ? 3.0e9f : (kind < 0.2f ? -40.0f : 3.0f * (u(rng) - 0.5f)));
          motion[4 * i + 1] = kind > 0.95f ? -3.0e9f : 3.0f * (u(rng) - 0.5f);
          motion[4 * i + 2] = kind > 0.85f && kind < 0.9f ? 0.005f : 1.0f;
          motion[4 * i + 3] = kind > 0.75f && kind < 0.8f ? 0.0f : (u(rng) < 0.5f ? 1.0f : 2.0f);
        }
        char err[128];
        std::vector<float>& out = frame & 1 ? d1 : d0;
        const std::vector<float>& prev = frame & 1 ? d0 : d1;
        const int rc = taa_emu_run(&taa, &disp, frame > 0, w, h, src.data(), motion.data(), frame > 0 ? prev.data() : nullptr, out.data(), words.data(), err, sizeof(err));
        if (rc) return 10 + rc;
        for (size_t i = 0; i < n; ++i) {
          for (int k = 0; k < 3; ++k)
            if (!(out[4 * i + k] >= 0.0f && out[4 * i + k] <= 1.0f)) return 3;
          if (out[4 * i + 3] != 0.0f && out[4 * i + 3] != 1.0f) return 4;
          if (frame == 0 && out[4 * i + 3] != 0.0f) return 5;
          if ((words[i] >> 24) != 0xffu) return 6;
          blended += out[4 * i + 3] == 1.0f;
        }
      }
    }
  std::printf("%u x %u: %zu pixels blended with their history\n", w, h, blended);
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  const unsigned seed = argc > 1 ? (unsigned)std::strtoul(argv[1], nullptr, 10) : 1u;
  if (int rc = run(33, 9, seed)) return rc;
  return run(1, 1, seed + 1);
}
