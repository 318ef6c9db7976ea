// tests/devfn/pt_devfn.hip -- TEST HARNESS, NOT A PRODUCT PATH.
//
// The device functions of the render kernels (gpuspectral_amd/csrc/pt_math.h, pt_shading.h, pt_trace.h, pt_stages.h), compiled for
// gfx950 with the product's own flags and called one by one with chosen arguments: one thread per vector, plain loads and
// stores.  tests/test_gpu_devfn.py compares what comes back with the host compile of the same bodies (devfn_bodies.h through
// tests/emu) and with the function vectors of tests/golden.  Built into tests/devfn/libpt_devfn.so; it never links against
// or calls into libgpuspectral_pt.so, and nothing shipped loads it.
//
// Every entry point takes host arrays, checks every index its vectors carry (devfn::kBadIndex, before any HIP call), then:
// hipMalloc, copy in, one launch (two where tables are baked first: devfn_bsdf, devfn_lights), hipDeviceSynchronize, copy out,
// hipFree; it returns the first non-zero hipError_t.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "devfn_bodies.h"

using namespace devfn;

#ifndef DEVFN_BUILD_INFO
#error "build with tests/devfn/Makefile: it stamps DEVFN_BUILD_INFO"
#endif

namespace {

constexpr uint32_t kThreads = 256;
uint64_t g_runs = 0;  // entry points that got past their index checks (devfn_run_count)

template <class F>
__global__ __launch_bounds__(kThreads) void k_each(uint64_t n, F f) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) f(i);
}

struct Run {
  struct Buf {
    void* dev;
    void* host_out;
    size_t bytes;
  };
  hipError_t err = hipSuccess;
  std::vector<Buf> bufs;
  Run() { ++g_runs; }
  void* alloc(const void* src, void* dst, size_t bytes) {
    if (err != hipSuccess) return nullptr;
    void* d = nullptr;
    err = hipMalloc(&d, bytes ? bytes : 16);
    if (err != hipSuccess) return nullptr;
    bufs.push_back(Buf{d, dst, bytes});
    if (bytes) err = src ? hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) : hipMemset(d, 0, bytes);
    return d;
  }
  template <class T>
  const T* in(const T* h, size_t count) { return (const T*)alloc(h, nullptr, count * sizeof(T)); }
  template <class T>
  T* out(T* h, size_t count) { return (T*)alloc(nullptr, h, count * sizeof(T)); }
  template <class T>
  T* inout(T* h, size_t count) { return (T*)alloc(h, h, count * sizeof(T)); }
  template <class F>
  void launch(uint64_t n, F f) {
    if (err != hipSuccess || n == 0) return;
    hipLaunchKernelGGL(k_each<F>, dim3((uint32_t)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, 0, n, f);
    err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
  }
  int finish() {
    for (const Buf& b : bufs)
      if (err == hipSuccess && b.host_out && b.bytes) err = hipMemcpy(b.host_out, b.dev, b.bytes, hipMemcpyDeviceToHost);
    for (const Buf& b : bufs) {
      const hipError_t e = hipFree(b.dev);
      if (err == hipSuccess) err = e;
    }
    return (int)err;
  }
};

}  // namespace

extern "C" {

const char* devfn_build_info() { return DEVFN_BUILD_INFO; }
uint64_t devfn_run_count() { return g_runs; }
int devfn_device_count() {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}
// byte offsets of the derived quads and of the first record of every table in the image devfn_bsdf returns; the image's size
uint64_t devfn_table_layout(const uint32_t* num, uint64_t* quad_off, uint64_t* rec_off) {
  const TableLayout L = table_layout(num);
  for (int t = 0; t < GSP_BSDF_TYPE_COUNT; ++t) quad_off[t] = L.quad_off[t], rec_off[t] = L.rec_off[t];
  return L.total;
}

int devfn_math(const float* x, uint64_t n, float* s, float* c, float* lg, float* ex, float* sq, float* rc) {
  Run r;
  const float* dx = r.in(x, n);
  float *ds = r.out(s, n), *dc = r.out(c, n), *dl = r.out(lg, n), *de = r.out(ex, n), *dq = r.out(sq, n), *dr = r.out(rc, n);
  r.launch(n, [=] __device__(uint64_t i) { math1(i, dx, ds, dc, dl, de, dq, dr); });
  return r.finish();
}
int devfn_atan2(const float* y, const float* x, uint64_t n, float* out) {
  Run r;
  const float *dy = r.in(y, n), *dx = r.in(x, n);
  float* d = r.out(out, n);
  r.launch(n, [=] __device__(uint64_t i) { atan2_1(i, dy, dx, d); });
  return r.finish();
}
int devfn_normalize(const float* v, uint64_t n, float* out3) {
  Run r;
  const float* dv = r.in(v, 3 * n);
  float* d = r.out(out3, 3 * n);
  r.launch(n, [=] __device__(uint64_t i) { normalize1(i, dv, d); });
  return r.finish();
}
int devfn_rng(const uint32_t* a, const uint32_t* b, uint64_t n, uint32_t* out7) {
  Run r;
  const uint32_t *da = r.in(a, n), *db = r.in(b, n);
  uint32_t* d = r.out(out7, 7 * n);
  r.launch(n, [=] __device__(uint64_t i) { rng1(i, da, db, d); });
  return r.finish();
}
int devfn_onb(const float* nrm, const float* v, uint64_t n, float* out15) {
  Run r;
  const float *dn = r.in(nrm, 3 * n), *dv = r.in(v, 3 * n);
  float* d = r.out(out15, 15 * n);
  r.launch(n, [=] __device__(uint64_t i) { onb1(i, dn, dv, d); });
  return r.finish();
}
int devfn_helpers(const float* f, const float* g, const uint32_t* h, uint64_t n, uint32_t* out3) {
  Run r;
  const float *df = r.in(f, n), *dg = r.in(g, n);
  const uint32_t* dh = r.in(h, n);
  uint32_t* d = r.out(out3, 3 * n);
  r.launch(n, [=] __device__(uint64_t i) { helpers1(i, df, dg, dh, d); });
  return r.finish();
}
int devfn_samplers(const uint32_t* seeds, const float* alpha, uint64_t n, float* out8) {
  Run r;
  const uint32_t* ds = r.in(seeds, n);
  const float* da = r.in(alpha, n);
  float* d = r.out(out8, 8 * n);
  r.launch(n, [=] __device__(uint64_t i) { samplers1(i, ds, da, d); });
  return r.finish();
}

// recs[t] / num[t]: the records of BSDF type t as a scene gives them.  They are laid out as the product lays its resident
// tables out (devfn_table_layout) and baked on the device as k_bake_tables does; `image` (devfn_table_layout bytes) receives the
// baked tables.  Then one vector per thread: out9 = bsdf_sample, out5 = bsdf_eval at wi.
int devfn_bsdf(const void* const* recs, const uint32_t* num, const uint32_t* handles, const float* wo, const uint32_t* seeds,
               const float* wi, uint64_t n, float* out9, float* out5, uint8_t* image) {
  for (int t = 0; t < GSP_BSDF_TYPE_COUNT; ++t)
    if (num[t] > 0x10000u) return kBadIndex;
  if (!ok_handles(handles, n, num)) return kBadIndex;
  const TableLayout L = table_layout(num);
  std::memset(image, 0, L.total);
  uint32_t most = 0;
  for (int t = 0; t < GSP_BSDF_TYPE_COUNT; ++t) {
    if (num[t]) std::memcpy(image + L.rec_off[t], recs[t], (size_t)num[t] * kRecBytes[t]);
    most = num[t] > most ? num[t] : most;
  }
  Run r;
  uint8_t* base = r.inout(image, L.total);
  const uint32_t* dh = r.in(handles, n);
  const float *dwo = r.in(wo, 3 * n), *dwi = r.in(wi, 3 * n);
  const uint32_t* ds = r.in(seeds, n);
  float *d9 = r.out(out9, 9 * n), *d5 = r.out(out5, 5 * n);
  r.launch(most, [=] __device__(uint64_t i) { bake_tables1(i, base, L); });
  r.launch(n, [=] __device__(uint64_t i) { bsdf1(i, tables_at(base, L), dh, dwo, ds, dwi, d9, d5); });
  return r.finish();
}

// lights: `capacity` records as a scene gives them, baked in place on the device (bake_light) and returned; sample_light draws
// among the first num_lights of them
int devfn_lights(gsp_triangle_light* lights, uint32_t capacity, uint32_t num_lights, const float* pos, const uint32_t* seeds, uint64_t n,
                 float* out8) {
  if (num_lights > capacity) return kBadIndex;
  Run r;
  gsp_triangle_light* dl = r.inout(lights, capacity);
  const float* dp = r.in(pos, 3 * n);
  const uint32_t* ds = r.in(seeds, n);
  float* d = r.out(out8, 8 * n);
  const float inv = num_lights ? 1.0f / (float)num_lights : 0.0f;  // as gsp_context::view()
  r.launch(capacity, [=] __device__(uint64_t i) { bake_light1(i, dl); });
  r.launch(n, [=] __device__(uint64_t i) { light1(i, dl, num_lights, inv, dp, ds, d); });
  return r.finish();
}

int devfn_texture(const gsp_texture* textures, uint32_t num_textures, const uint32_t* texels, uint64_t num_texels, const float* decode,
                  const uint32_t* ids, const float* uv, uint64_t n, float* out3) {
  if (!ok_textures(textures, num_textures, num_texels, ids, n)) return kBadIndex;
  Run r;
  TextureView T;
  T.textures = r.in(textures, num_textures);
  T.texels = r.in(texels, num_texels);
  T.decode = r.in(decode, 256);
  T.num_textures = num_textures;
  const uint32_t* di = r.in(ids, n);
  const float* duv = r.in(uv, 2 * n);
  float* d = r.out(out3, 3 * n);
  r.launch(n, [=] __device__(uint64_t i) { texture1(i, T, di, duv, d); });
  return r.finish();
}
int devfn_envmap(const float* env_texels, uint32_t width, uint32_t height, const float* to_local, const float* dirs, uint64_t n,
                 float* out3) {
  if (width == 0 || height == 0 || width > 32768u || height > 32768u) return kBadIndex;
  Run r;
  TextureView T;
  T.env_texels = r.in(env_texels, 4 * (size_t)width * height);
  T.env_width = width;
  T.env_height = height;
  for (int k = 0; k < 16; ++k) T.env_to_local[k] = to_local[k];
  const float* dd = r.in(dirs, 3 * n);
  float* d = r.out(out3, 3 * n);
  r.launch(n, [=] __device__(uint64_t i) { envmap1(i, T, dd, d); });
  return r.finish();
}

int devfn_tri_tests(const float* rays, const float* tris, uint64_t n, float* out_ref, float* out_rot) {
  Run r;
  const float *dr = r.in(rays, 8 * n), *dt = r.in(tris, 9 * n);
  float *da = r.out(out_ref, 4 * n), *db = r.out(out_rot, 4 * n);
  r.launch(n, [=] __device__(uint64_t i) { tri1(i, dr, dt, da, db); });
  return r.finish();
}
int devfn_shears(const float* d3, uint64_t n, uint32_t* out12) {
  Run r;
  const float* dd = r.in(d3, 3 * n);
  uint32_t* d = r.out(out12, 12 * n);
  r.launch(n, [=] __device__(uint64_t i) { shear1(i, dd, d); });
  return r.finish();
}
int devfn_encode_nodes(const float* boxes, const int32_t* counts, uint64_t n, uint32_t* out_ref, uint32_t* out_fast) {
  if (!ok_child_counts(counts, n)) return kBadIndex;
  Run r;
  const float* db = r.in(boxes, 24 * n);
  const int32_t* dc = r.in(counts, 2 * n);
  uint32_t *da = r.out(out_ref, 16 * n), *df = r.out(out_fast, 16 * n);
  r.launch(n, [=] __device__(uint64_t i) { encode1(i, db, dc, da, df); });
  return r.finish();
}
int devfn_node_tests(const uint32_t* nodes, uint64_t num_nodes, const uint32_t* node_idx, const float* rays, uint64_t n, uint32_t* out12) {
  if (!ok_node_indices(node_idx, n, num_nodes)) return kBadIndex;
  Run r;
  const uint32_t *dn = r.in(nodes, 16 * num_nodes), *di = r.in(node_idx, n);
  const float* dr = r.in(rays, 8 * n);
  uint32_t* d = r.out(out12, 12 * n);
  r.launch(n, [=] __device__(uint64_t i) { nodetest1(i, dn, di, dr, d); });
  return r.finish();
}
}
