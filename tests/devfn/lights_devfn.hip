// tests/devfn/lights_devfn.hip -- TEST HARNESS, NOT A PRODUCT PATH.
//
// sample_light_power (gpuspectral_amd/csrc/pt_shading.h) compiled for gfx950 with the product's own flags and called with chosen
// arguments: one thread per vector, plain loads and stores, as pt_devfn.hip does for the other device functions.  Built into
// tests/devfn/liblights_devfn.so by tests/devfn/lights.mk; it never links against libgpuspectral_pt.so, and nothing shipped
// loads it.  tests/test_gpu_lights_devfn.py compares what comes back with the host compile of the same body (lights_bodies.h
// through tests/emu/lights_emu.cpp).
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "lights_bodies.h"
#include "../../gpuspectral_amd/csrc/pt_lightpick.h"

using namespace devfn;

#ifndef DEVFN_BUILD_INFO
#error "build with tests/devfn/lights.mk: it stamps DEVFN_BUILD_INFO"
#endif

namespace {
constexpr uint32_t kThreads = 256;

__global__ __launch_bounds__(kThreads) void k_bake(uint64_t n, gsp_triangle_light* lights) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) bake_light1(i, lights);
}
__global__ __launch_bounds__(kThreads) void k_light_power(uint64_t n, const gsp_triangle_light* image, uint32_t num_lights, const float* pos,
                                                          const uint32_t* seeds, float* out8) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) light_power1(i, image, num_lights, pos, seeds, out8);
}
}  // namespace

extern "C" {

const char* lights_devfn_build_info() { return DEVFN_BUILD_INFO; }

// lights: num_lights records as a scene gives them.  The pick table is built from them on the host (pt_lightpick.h) and laid
// behind the records; the records are baked on the device (bake_light), then one vector per thread.  pick_out (optional) receives
// the table.  Returns 0, kBadIndex (nothing launched), or the first non-zero hipError_t.
int lights_devfn_power(const gsp_triangle_light* lights, uint32_t num_lights, const float* pos, const uint32_t* seeds, uint64_t n, float* out8,
                       gsp_light_pick* pick_out) {
  if (num_lights == 0 || num_lights > (1u << 20) || n > (1ull << 24)) return kBadIndex;
  std::vector<gsp_light_pick> pick(num_lights);
  gsp::build_light_pick(lights, num_lights, pick.data());
  if (!ok_light_pick(pick.data(), num_lights)) return kBadIndex;
  if (pick_out) std::memcpy(pick_out, pick.data(), sizeof(gsp_light_pick) * num_lights);
  const size_t lbytes = sizeof(gsp_triangle_light) * (size_t)num_lights, pbytes = sizeof(gsp_light_pick) * (size_t)num_lights;
  uint8_t* image = nullptr;
  float *dpos = nullptr, *dout = nullptr;
  uint32_t* dseeds = nullptr;
  hipError_t err = hipMalloc((void**)&image, lbytes + pbytes);
  if (err == hipSuccess) err = hipMalloc((void**)&dpos, sizeof(float) * 3 * (n ? n : 1));
  if (err == hipSuccess) err = hipMalloc((void**)&dseeds, sizeof(uint32_t) * (n ? n : 1));
  if (err == hipSuccess) err = hipMalloc((void**)&dout, sizeof(float) * 8 * (n ? n : 1));
  if (err == hipSuccess) err = hipMemcpy(image, lights, lbytes, hipMemcpyHostToDevice);
  if (err == hipSuccess) err = hipMemcpy(image + lbytes, pick.data(), pbytes, hipMemcpyHostToDevice);
  if (err == hipSuccess && n) err = hipMemcpy(dpos, pos, sizeof(float) * 3 * n, hipMemcpyHostToDevice);
  if (err == hipSuccess && n) err = hipMemcpy(dseeds, seeds, sizeof(uint32_t) * n, hipMemcpyHostToDevice);
  if (err == hipSuccess) {
    hipLaunchKernelGGL(k_bake, dim3((num_lights + kThreads - 1) / kThreads), dim3(kThreads), 0, 0, (uint64_t)num_lights, (gsp_triangle_light*)image);
    err = hipGetLastError();
  }
  if (err == hipSuccess && n) {
    hipLaunchKernelGGL(k_light_power, dim3((uint32_t)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, 0, n, (const gsp_triangle_light*)image, num_lights,
                       (const float*)dpos, (const uint32_t*)dseeds, dout);
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err == hipSuccess && n) err = hipMemcpy(out8, dout, sizeof(float) * 8 * n, hipMemcpyDeviceToHost);
  for (void* p : {(void*)image, (void*)dpos, (void*)dseeds, (void*)dout}) {
    if (!p) continue;
    const hipError_t e = hipFree(p);
    if (err == hipSuccess) err = e;
  }
  return (int)err;
}
}
