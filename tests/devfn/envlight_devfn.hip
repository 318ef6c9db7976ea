// tests/devfn/envlight_devfn.hip -- TEST HARNESS, NOT A PRODUCT PATH.
//
// The device functions of gpuspectral_amd/csrc/pt_envlight.h (env_eval, sample_env_light) compiled for gfx950 with the product's own
// flags and called with chosen arguments: one thread per vector, plain loads and stores, as delta_devfn.hip does for pt_deltalight.h.
// Built into tests/devfn/libenvlight_devfn.so by tests/devfn/envlight.mk; it never links against libgpuspectral_pt.so, and nothing
// shipped loads it.  tests/test_gpu_envlight_devfn.py compares what comes back with the host compile of the same bodies
// (envlight_bodies.h through tests/emu/envlight_emu.cpp).
#include <hip/hip_runtime.h>

#include <vector>

#include "envlight_bodies.h"

using namespace devfn;

#ifndef DEVFN_BUILD_INFO
#error "build with tests/devfn/envlight.mk: it stamps DEVFN_BUILD_INFO"
#endif

namespace {
constexpr uint32_t kThreads = 256;
constexpr uint64_t kMaxVectors = 1ull << 24;

__global__ __launch_bounds__(kThreads) void k_env_eval(uint64_t n, TextureView T, const gsp_light_pick* cells, const float* rec16, const float* dirs, float* out5) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) env_eval1(i, T, cells, rec16, dirs, out5);
}
__global__ __launch_bounds__(kThreads) void k_sample_env_light(uint64_t n, TextureView T, const gsp_light_pick* cells, const float* rec16, const float* draws3, float* out9) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) sample_env_light1(i, T, cells, rec16, draws3, out9);
}

// device copies of the shared map, cell table and record, of one per-vector input and of one output array, freed on every path
struct Arrays {
  void* p[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // texels, cells, record, input, output
  hipError_t err = hipSuccess;
  void put(int k, const void* src, size_t bytes) {
    if (err == hipSuccess) err = hipMalloc(&p[k], bytes ? bytes : 16);
    if (err == hipSuccess && src) err = hipMemcpy(p[k], src, bytes, hipMemcpyHostToDevice);
  }
  Arrays(const float* texels, uint32_t width, uint32_t height, const gsp_light_pick* cells, const float* rec16, const float* in, uint32_t in_floats, uint32_t out_floats,
         uint64_t n) {
    const EnvLightRecord& rec = *(const EnvLightRecord*)rec16;
    put(0, texels, sizeof(float) * 4 * (size_t)width * height);
    put(1, cells, sizeof(gsp_light_pick) * (size_t)rec.cw * rec.ch);
    put(2, rec16, sizeof(EnvLightRecord));
    put(3, in, sizeof(float) * in_floats * n);
    put(4, nullptr, sizeof(float) * out_floats * n);
  }
  TextureView view(uint32_t width, uint32_t height, const float* to_local) const {
    TextureView T;
    T.env_texels = (const float*)p[0];
    T.env_width = width;
    T.env_height = height;
    for (int k = 0; k < 16; ++k) T.env_to_local[k] = to_local[k];
    return T;
  }
  int finish(float* host_out, uint32_t out_floats, uint64_t n) {
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err == hipSuccess) err = hipMemcpy(host_out, p[4], sizeof(float) * out_floats * n, hipMemcpyDeviceToHost);
    for (void* q : p)
      if (q) (void)hipFree(q);
    return (int)err;
  }
};
dim3 grid_for(uint64_t n) { return dim3((uint32_t)((n + kThreads - 1) / kThreads)); }
// the record names a cell grid of the map's own size class, and the map is not empty: the bodies index nothing beyond the copies above
bool shapes_ok(uint32_t width, uint32_t height, const float* rec16) {
  const EnvLightRecord& rec = *(const EnvLightRecord*)rec16;
  return width != 0 && height != 0 && width <= 32768u && height <= 32768u && rec.cw != 0 && rec.ch != 0 && rec.cw <= kEnvCellsU && rec.ch <= kEnvCellsV;
}
}  // namespace

extern "C" {

const char* envlight_devfn_build_info() { return DEVFN_BUILD_INFO; }

// Each returns 0, kBadIndex (nothing launched), or the first non-zero hipError_t.
int envlight_devfn_env_eval(uint64_t n, const float* texels, uint32_t width, uint32_t height, const float* to_local, const gsp_light_pick* cells, const float* rec16,
                            const float* dirs, float* out5) {
  if (n == 0 || n > kMaxVectors || !shapes_ok(width, height, rec16)) return kBadIndex;
  Arrays a(texels, width, height, cells, rec16, dirs, 3, 5, n);
  if (a.err == hipSuccess)
    hipLaunchKernelGGL(k_env_eval, grid_for(n), dim3(kThreads), 0, 0, n, a.view(width, height, to_local), (const gsp_light_pick*)a.p[1], (const float*)a.p[2],
                       (const float*)a.p[3], (float*)a.p[4]);
  return a.finish(out5, 5, n);
}
int envlight_devfn_sample_env_light(uint64_t n, const float* texels, uint32_t width, uint32_t height, const float* to_local, const gsp_light_pick* cells,
                                    const float* rec16, const float* draws3, float* out9) {
  if (n == 0 || n > kMaxVectors || !shapes_ok(width, height, rec16)) return kBadIndex;
  Arrays a(texels, width, height, cells, rec16, draws3, 3, 9, n);
  if (a.err == hipSuccess)
    hipLaunchKernelGGL(k_sample_env_light, grid_for(n), dim3(kThreads), 0, 0, n, a.view(width, height, to_local), (const gsp_light_pick*)a.p[1], (const float*)a.p[2],
                       (const float*)a.p[3], (float*)a.p[4]);
  return a.finish(out9, 9, n);
}
}
