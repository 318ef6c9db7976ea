// tests/devfn/lightgrid_devfn.hip -- TEST HARNESS, NOT A PRODUCT PATH.
//
// The device functions of gpuspectral_amd/csrc/pt_lightgrid.h (lightgrid_cell, lightgrid_pick, lightgrid_hit_select_pmf) compiled for
// gfx950 with the product's own flags and called with chosen arguments: one thread per vector, plain loads and stores, as
// envlight_devfn.hip does for pt_envlight.h.  Built into tests/devfn/liblightgrid_devfn.so by tests/devfn/lightgrid.mk; it never
// links against libgpuspectral_pt.so, and nothing shipped loads it.  tests/test_gpu_lightgrid_devfn.py compares what comes back with
// the host compile of the same bodies (lightgrid_bodies.h through tests/emu/lightgrid_emu.cpp).
#include <hip/hip_runtime.h>

#include <vector>

#include "lightgrid_bodies.h"

using namespace devfn;

#ifndef DEVFN_BUILD_INFO
#error "build with tests/devfn/lightgrid.mk: it stamps DEVFN_BUILD_INFO"
#endif

namespace {
constexpr uint32_t kThreads = 256;
constexpr uint64_t kMaxVectors = 1ull << 24;

__global__ __launch_bounds__(kThreads) void k_cell(uint64_t n, const uint8_t* grid, const float* pos3, uint32_t* out4) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) lightgrid_cell1(i, grid, pos3, out4);
}
__global__ __launch_bounds__(kThreads) void k_pick(uint64_t n, const uint8_t* grid, const gsp_light_pick* fallback, uint32_t num_lights, const float* pos3, const uint32_t* r,
                                                   uint32_t* out2) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) lightgrid_pick1(i, grid, fallback, num_lights, pos3, r, out2);
}
__global__ __launch_bounds__(kThreads) void k_hit_pmf(uint64_t n, const uint8_t* grid, const gsp_light_pick* fallback, uint32_t num_lights, const float* pos3,
                                                      const float* tri12, float* out1) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) lightgrid_hit_pmf1(i, grid, fallback, num_lights, pos3, tri12, out1);
}

// device copies of the grid image, the fallback table (+ tail), two per-vector inputs and one output array, freed on every path
struct Arrays {
  void* p[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // grid, fallback, input a, input b, output
  hipError_t err = hipSuccess;
  void put(int k, const void* src, size_t bytes) {
    if (err == hipSuccess) err = hipMalloc(&p[k], bytes ? bytes : 16);
    if (err == hipSuccess && src && bytes) err = hipMemcpy(p[k], src, bytes, hipMemcpyHostToDevice);
  }
  int finish(void* host_out, size_t out_bytes) {
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err == hipSuccess) err = hipMemcpy(host_out, p[4], out_bytes, hipMemcpyDeviceToHost);
    for (void* q : p)
      if (q) (void)hipFree(q);
    return (int)err;
  }
};
dim3 grid_for(uint64_t n) { return dim3((uint32_t)((n + kThreads - 1) / kThreads)); }
// The image is what its header says, entry for entry: the bodies then index nothing beyond the copies above.  grid_bytes = the
// caller's size of the image; fallback: num_lights entries + the tail.  Every alias of every table names a light
bool shapes_ok(const uint8_t* grid, uint64_t grid_bytes, const gsp_light_pick* fallback, uint32_t num_lights) {
  if (!grid || grid_bytes < sizeof(LightGridHeader) || num_lights == 0) return false;
  LightGridHeader g;
  std::memcpy(&g, grid, sizeof(g));
  if (g.nx == 0 || g.ny == 0 || g.nz == 0 || g.nx > kLightGridMaxAxis || g.ny > kLightGridMaxAxis || g.nz > kLightGridMaxAxis) return false;
  const uint64_t cells = ((uint64_t)g.nx * g.ny) * g.nz;
  if (cells * num_lights > kLightGridMaxEntries || grid_bytes != lightgrid_bytes(g.nx, g.ny, g.nz, num_lights)) return false;
  for (uint64_t c = 0; c < cells; ++c) {
    const gsp_light_pick* t = (const gsp_light_pick*)(grid + sizeof(LightGridHeader) + c * lightgrid_cell_bytes(num_lights));
    for (uint32_t j = 0; j < num_lights; ++j)
      if (t[j].alias >= num_lights) return false;
  }
  if (fallback)
    for (uint32_t j = 0; j < num_lights; ++j)
      if (fallback[j].alias >= num_lights) return false;
  return true;
}
}  // namespace

extern "C" {

const char* lightgrid_devfn_build_info() { return DEVFN_BUILD_INFO; }

// Each returns 0, kBadIndex (nothing launched), or the first non-zero hipError_t.
int lightgrid_devfn_cell(uint64_t n, const uint8_t* grid, uint64_t grid_bytes, const float* pos3, uint32_t* out4) {
  if (n == 0 || n > kMaxVectors || !grid || grid_bytes < sizeof(LightGridHeader)) return kBadIndex;
  Arrays a;
  a.put(0, grid, sizeof(LightGridHeader));  // (the cell lookup reads the header alone)
  a.put(2, pos3, sizeof(float) * 3 * n);
  a.put(4, nullptr, sizeof(uint32_t) * 4 * n);
  if (a.err == hipSuccess) hipLaunchKernelGGL(k_cell, grid_for(n), dim3(kThreads), 0, 0, n, (const uint8_t*)a.p[0], (const float*)a.p[2], (uint32_t*)a.p[4]);
  return a.finish(out4, sizeof(uint32_t) * 4 * n);
}
int lightgrid_devfn_pick(uint64_t n, const uint8_t* grid, uint64_t grid_bytes, const gsp_light_pick* fallback, uint32_t num_lights, const float* pos3, const uint32_t* r,
                         uint32_t* out2) {
  if (n == 0 || n > kMaxVectors || !fallback || !shapes_ok(grid, grid_bytes, fallback, num_lights)) return kBadIndex;
  Arrays a;
  a.put(0, grid, grid_bytes);
  a.put(1, fallback, sizeof(gsp_light_pick) * ((size_t)num_lights + 1u));
  a.put(2, pos3, sizeof(float) * 3 * n);
  a.put(3, r, sizeof(uint32_t) * n);
  a.put(4, nullptr, sizeof(uint32_t) * 2 * n);
  if (a.err == hipSuccess)
    hipLaunchKernelGGL(k_pick, grid_for(n), dim3(kThreads), 0, 0, n, (const uint8_t*)a.p[0], (const gsp_light_pick*)a.p[1], num_lights, (const float*)a.p[2],
                       (const uint32_t*)a.p[3], (uint32_t*)a.p[4]);
  return a.finish(out2, sizeof(uint32_t) * 2 * n);
}
int lightgrid_devfn_hit_pmf(uint64_t n, const uint8_t* grid, uint64_t grid_bytes, const gsp_light_pick* fallback, uint32_t num_lights, const float* pos3,
                            const float* tri12, float* out1) {
  if (n == 0 || n > kMaxVectors || !fallback || !shapes_ok(grid, grid_bytes, fallback, num_lights)) return kBadIndex;
  Arrays a;
  a.put(0, grid, grid_bytes);
  a.put(1, fallback, sizeof(gsp_light_pick) * ((size_t)num_lights + 1u));
  a.put(2, pos3, sizeof(float) * 3 * n);
  a.put(3, tri12, sizeof(float) * 12 * n);
  a.put(4, nullptr, sizeof(float) * n);
  if (a.err == hipSuccess)
    hipLaunchKernelGGL(k_hit_pmf, grid_for(n), dim3(kThreads), 0, 0, n, (const uint8_t*)a.p[0], (const gsp_light_pick*)a.p[1], num_lights, (const float*)a.p[2],
                       (const float*)a.p[3], (float*)a.p[4]);
  return a.finish(out1, sizeof(float) * n);
}
}
