// tests/devfn/medium_devfn.hip -- TEST HARNESS, NOT A PRODUCT PATH.
//
// The functions of gpuspectral_amd/csrc/pt_medium.h (sample_hg, hg_pdf, medium_event) compiled for gfx950 with the product's own
// flags and called with chosen arguments: one thread per vector, plain loads and stores, as pt_devfn.hip does for the other device
// functions.  Built into tests/devfn/libmedium_devfn.so by tests/devfn/medium.mk; it never links against libgpuspectral_pt.so,
// and nothing shipped loads it.  tests/test_gpu_scatter_devfn.py compares what comes back with the host compile of the same
// bodies (medium_bodies.h through tests/emu/scatter_emu.cpp).
#include <hip/hip_runtime.h>

#include <vector>

#include "medium_bodies.h"

using namespace devfn;

#ifndef DEVFN_BUILD_INFO
#error "build with tests/devfn/medium.mk: it stamps DEVFN_BUILD_INFO"
#endif

namespace {
constexpr uint32_t kThreads = 256;
constexpr uint64_t kMaxVectors = 1ull << 24;

__global__ __launch_bounds__(kThreads) void k_sample_hg(uint64_t n, const float* d, const float* g, const float* u1, const float* u2, float* out4) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) sample_hg1(i, d, g, u1, u2, out4);
}
__global__ __launch_bounds__(kThreads) void k_hg_pdf(uint64_t n, const float* g, const float* c, float* pdf) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) hg_pdf1(i, g, c, pdf);
}
__global__ __launch_bounds__(kThreads) void k_medium_event(uint64_t n, const float* sigma_a, const float* sigma_s, const float* t, const float* u_c,
                                                           const float* u_d, const float* weight, float* out6) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) medium_event1(i, sigma_a, sigma_s, t, u_c, u_d, weight, out6);
}

// device copies of the inputs ({host pointer, floats per vector}) and one output array, freed on every path
struct Arrays {
  std::vector<float*> in;
  float* out = nullptr;
  hipError_t err = hipSuccess;
  Arrays(uint64_t n, std::initializer_list<std::pair<const float*, uint32_t>> inputs, uint32_t out_floats) {
    for (const auto& a : inputs) {
      float* p = nullptr;
      if (err == hipSuccess) err = hipMalloc((void**)&p, sizeof(float) * a.second * n);
      if (err == hipSuccess) err = hipMemcpy(p, a.first, sizeof(float) * a.second * n, hipMemcpyHostToDevice);
      in.push_back(p);
    }
    if (err == hipSuccess) err = hipMalloc((void**)&out, sizeof(float) * out_floats * n);
  }
  int finish(float* host_out, uint32_t out_floats, uint64_t n) {
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err == hipSuccess) err = hipMemcpy(host_out, out, sizeof(float) * out_floats * n, hipMemcpyDeviceToHost);
    for (float* p : in)
      if (p) (void)hipFree(p);
    if (out) (void)hipFree(out);
    return (int)err;
  }
};
dim3 grid_for(uint64_t n) { return dim3((uint32_t)((n + kThreads - 1) / kThreads)); }
}  // namespace

extern "C" {

const char* medium_devfn_build_info() { return DEVFN_BUILD_INFO; }

// Each returns 0, kBadIndex (nothing launched), or the first non-zero hipError_t.
int medium_devfn_sample_hg(uint64_t n, const float* d, const float* g, const float* u1, const float* u2, float* out4) {
  if (n == 0 || n > kMaxVectors) return kBadIndex;
  Arrays a(n, {{d, 3u}, {g, 1u}, {u1, 1u}, {u2, 1u}}, 4);
  if (a.err == hipSuccess) hipLaunchKernelGGL(k_sample_hg, grid_for(n), dim3(kThreads), 0, 0, n, a.in[0], a.in[1], a.in[2], a.in[3], a.out);
  return a.finish(out4, 4, n);
}
int medium_devfn_hg_pdf(uint64_t n, const float* g, const float* c, float* pdf) {
  if (n == 0 || n > kMaxVectors) return kBadIndex;
  Arrays a(n, {{g, 1u}, {c, 1u}}, 1);
  if (a.err == hipSuccess) hipLaunchKernelGGL(k_hg_pdf, grid_for(n), dim3(kThreads), 0, 0, n, a.in[0], a.in[1], a.out);
  return a.finish(pdf, 1, n);
}
int medium_devfn_medium_event(uint64_t n, const float* sigma_a, const float* sigma_s, const float* t, const float* u_c, const float* u_d,
                              const float* weight, float* out6) {
  if (n == 0 || n > kMaxVectors) return kBadIndex;
  Arrays a(n, {{sigma_a, 3u}, {sigma_s, 3u}, {t, 1u}, {u_c, 1u}, {u_d, 1u}, {weight, 3u}}, 6);
  if (a.err == hipSuccess)
    hipLaunchKernelGGL(k_medium_event, grid_for(n), dim3(kThreads), 0, 0, n, a.in[0], a.in[1], a.in[2], a.in[3], a.in[4], a.in[5], a.out);
  return a.finish(out6, 6, n);
}
}
