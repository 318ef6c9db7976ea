// Kernel time of k_taa_resolve<ACES> against k_antilag_clamp<1> at 1920 x 1080 from HIP events: the library's translation unit with a
// main of its own.  Three sets of planes per kernel (about 400 MB each family) are rotated so that no launch finds its planes in the
// 256 MB Infinity Cache; the two kernels alternate in windows of 300 launches, five windows each.  (profiles/taa_cost.txt, DESIGN.md
// section 24.)  Not part of the library or the suite.  After `make -C gpuspectral_amd/csrc`, from the repository root:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-slp-vectorize -c tests/tools/taa_kernel_times.hip -o /tmp/taa_kernel_times.o
//   hipcc --offload-arch=gfx950 /tmp/taa_kernel_times.o gpuspectral_amd/csrc/build/pt_bvh.o gpuspectral_amd/csrc/build/pt_multi.o \
//         gpuspectral_amd/csrc/build/pt_buildinfo.o -ldl -o /tmp/taa_kernel_times && /tmp/taa_kernel_times
#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

#include "../../gpuspectral_amd/csrc/pt_render.hip"

using namespace gsp;

#define CK(x)                                                                  \
  do {                                                                         \
    hipError_t e_ = (x);                                                       \
    if (e_ != hipSuccess) {                                                    \
      std::printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); \
      return 1;                                                                \
    }                                                                          \
  } while (0)

int main() {
  const int W = 1920, H = 1080, SETS = 3, WINDOW = 300, REPS = 5;
  const size_t n = (size_t)W * H;
  std::mt19937 rng(1);
  std::uniform_real_distribution<float> u(0.0f, 1.0f);
  std::vector<float> src(4 * n), mot(4 * n), d(4 * n), f(4 * n), g(4 * n), hh(4 * n);
  std::vector<uint32_t> ids(n, 3u);
  for (size_t i = 0; i < n; ++i) {
    for (int k = 0; k < 3; ++k) {
      src[4 * i + k] = 2.0f * u(rng);
      d[4 * i + k] = u(rng);
      f[4 * i + k] = u(rng);
      hh[4 * i + k] = u(rng);
    }
    src[4 * i + 3] = 1.0f;
    d[4 * i + 3] = 1.0f;
    f[4 * i + 3] = 3.0f;
    hh[4 * i + 3] = 7.0f;
    mot[4 * i + 0] = 3.0f * (u(rng) - 0.5f);
    mot[4 * i + 1] = 3.0f * (u(rng) - 0.5f);
    mot[4 * i + 2] = 1.0f;
    mot[4 * i + 3] = 1.0f;
    g[4 * i + 0] = 0.0f;
    g[4 * i + 1] = 0.0f;
    g[4 * i + 2] = -1.0f;
    g[4 * i + 3] = 5.0f;
  }
  v4f *dsrc[SETS], *dmot[SETS], *dd0[SETS], *dd1[SETS], *df[SETS], *dg[SETS], *dh[SETS];
  uint32_t* di[SETS];
  for (int s = 0; s < SETS; ++s) {
    for (v4f** p : {&dsrc[s], &dmot[s], &dd0[s], &dd1[s], &df[s], &dg[s], &dh[s]}) CK(hipMalloc((void**)p, n * 16));
    CK(hipMalloc((void**)&di[s], n * 4));
    CK(hipMemcpy(dsrc[s], src.data(), n * 16, hipMemcpyHostToDevice));
    CK(hipMemcpy(dmot[s], mot.data(), n * 16, hipMemcpyHostToDevice));
    CK(hipMemcpy(dd0[s], d.data(), n * 16, hipMemcpyHostToDevice));
    CK(hipMemset(dd1[s], 0, n * 16));
    CK(hipMemcpy(df[s], f.data(), n * 16, hipMemcpyHostToDevice));
    CK(hipMemcpy(dg[s], g.data(), n * 16, hipMemcpyHostToDevice));
    CK(hipMemcpy(dh[s], hh.data(), n * 16, hipMemcpyHostToDevice));
    CK(hipMemcpy(di[s], ids.data(), n * 4, hipMemcpyHostToDevice));
  }
  gsp_display disp{};
  disp.struct_size = sizeof(disp);
  disp.tonemap = GSP_TONEMAP_ACES;
  gsp_display rd;
  if (resolve_display(&disp, rd)) return 2;
  const DisplayConsts k = display_consts(rd, gsp_luminance{});
  TaaParams ta;
  if (resolve_taa(nullptr, ta)) return 2;
  AntilagParams al;
  if (resolve_antilag(nullptr, al)) return 2;
  al.radius = 1;
  const dim3 grid = tile_grid(W, H), block(kBlock);
  hipStream_t stream;
  CK(hipStreamCreate(&stream));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  auto taa = [&](int s) {
    hipLaunchKernelGGL((k_taa_resolve<GSP_TONEMAP_ACES>), grid, block, 0, stream, (const v4f*)dsrc[s], (const v4f*)dmot[s], (const v4f*)dd0[s], dd1[s], ta, k, 1, W, H);
  };
  auto clamp = [&](int s) {
    hipLaunchKernelGGL((k_antilag_clamp<1>), grid, block, 0, stream, (const v4f*)df[s], (const v4f*)dg[s], (const uint32_t*)di[s], dh[s], al, 0.9f, W, H);
  };
  for (int i = 0; i < 12; ++i) {  // warm-up of both on every set
    taa(i % SETS);
    clamp(i % SETS);
  }
  CK(hipGetLastError());
  CK(hipStreamSynchronize(stream));
  std::vector<float> t_taa, t_clamp;
  for (int r = 0; r < REPS; ++r)
    for (int which = 0; which < 2; ++which) {
      CK(hipEventRecord(e0, stream));
      for (int i = 0; i < WINDOW; ++i) which ? clamp(i % SETS) : taa(i % SETS);
      CK(hipEventRecord(e1, stream));
      CK(hipGetLastError());
      CK(hipEventSynchronize(e1));
      float ms = 0.0f;
      CK(hipEventElapsedTime(&ms, e0, e1));
      (which ? t_clamp : t_taa).push_back(1000.0f * ms / WINDOW);
    }
  std::sort(t_taa.begin(), t_taa.end());
  std::sort(t_clamp.begin(), t_clamp.end());
  const double bytes_taa = 64.0 * (double)n, bytes_clamp = 52.0 * (double)n;
  std::printf("1920 x 1080, %d windows of %d launches each, planes rotated over %d sets\n", REPS, WINDOW, SETS);
  std::printf("k_taa_resolve<ACES>   us per launch: min %.2f median %.2f max %.2f   (64 B/pixel = %.1f MB: %.2f TB/s at the median)\n", t_taa.front(), t_taa[REPS / 2],
              t_taa.back(), bytes_taa / 1e6, bytes_taa / (t_taa[REPS / 2] * 1e-6) / 1e12);
  std::printf("k_antilag_clamp<1>    us per launch: min %.2f median %.2f max %.2f   (52 B/pixel read = %.1f MB: %.2f TB/s at the median)\n", t_clamp.front(),
              t_clamp[REPS / 2], t_clamp.back(), bytes_clamp / 1e6, bytes_clamp / (t_clamp[REPS / 2] * 1e-6) / 1e12);
  std::vector<float> back(4 * n);
  CK(hipMemcpy(back.data(), dd1[0], n * 16, hipMemcpyDeviceToHost));
  size_t used = 0;
  for (size_t i = 0; i < n; ++i) used += back[4 * i + 3] == 1.0f;
  std::printf("resolved pixels with a history: %zu of %zu\n", used, n);
  return 0;
}
