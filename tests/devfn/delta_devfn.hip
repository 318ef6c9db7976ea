// tests/devfn/delta_devfn.hip -- TEST HARNESS, NOT A PRODUCT PATH.
//
// The functions of gpuspectral_amd/csrc/pt_deltalight.h (spot_falloff, sample_delta_light) compiled for gfx950 with the product's own
// flags and called with chosen arguments: one thread per vector, plain loads and stores, as medium_devfn.hip does for pt_medium.h.
// Built into tests/devfn/libdelta_devfn.so by tests/devfn/delta.mk; it never links against libgpuspectral_pt.so, and nothing
// shipped loads it.  tests/test_gpu_delta_devfn.py compares what comes back with the host compile of the same bodies
// (delta_bodies.h through tests/emu/delta_emu.cpp).
#include <hip/hip_runtime.h>

#include <vector>

#include "delta_bodies.h"

using namespace devfn;

#ifndef DEVFN_BUILD_INFO
#error "build with tests/devfn/delta.mk: it stamps DEVFN_BUILD_INFO"
#endif

namespace {
constexpr uint32_t kThreads = 256;
constexpr uint64_t kMaxVectors = 1ull << 24;

__global__ __launch_bounds__(kThreads) void k_spot_falloff(uint64_t n, const float* c, const float* cos_cutoff, const float* cos_beam, float* out) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) spot_falloff1(i, c, cos_cutoff, cos_beam, out);
}
__global__ __launch_bounds__(kThreads) void k_sample_delta_light(uint64_t n, const float* rec16, const float* pos, const float* pmf, float* out8) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) sample_delta_light1(i, rec16, pos, pmf, out8);
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

const char* delta_devfn_build_info() { return DEVFN_BUILD_INFO; }

// Each returns 0, kBadIndex (nothing launched), or the first non-zero hipError_t.
int delta_devfn_spot_falloff(uint64_t n, const float* c, const float* cos_cutoff, const float* cos_beam, float* out) {
  if (n == 0 || n > kMaxVectors) return kBadIndex;
  Arrays a(n, {{c, 1u}, {cos_cutoff, 1u}, {cos_beam, 1u}}, 1);
  if (a.err == hipSuccess) hipLaunchKernelGGL(k_spot_falloff, grid_for(n), dim3(kThreads), 0, 0, n, a.in[0], a.in[1], a.in[2], a.out);
  return a.finish(out, 1, n);
}
int delta_devfn_sample_delta_light(uint64_t n, const float* rec16, const float* pos, const float* pmf, float* out8) {
  if (n == 0 || n > kMaxVectors) return kBadIndex;
  Arrays a(n, {{rec16, 16u}, {pos, 3u}, {pmf, 1u}}, 8);
  if (a.err == hipSuccess) hipLaunchKernelGGL(k_sample_delta_light, grid_for(n), dim3(kThreads), 0, 0, n, a.in[0], a.in[1], a.in[2], a.out);
  return a.finish(out8, 8, n);
}
}
