// tests/emu/denoise_emu.cpp -- TEST HARNESS, NOT A PRODUCT PATH.
//
// The denoiser of the library (include/gpuspectral_pt.h, "Denoiser") compiled for the host: the very text the kernels
// k_denoise_prepare / k_denoise_atrous run (csrc/pt_denoise.h), driven by plain loops over the frame, plus gsp_*_denoised's
// validation and the resolution of a gsp_denoise into the kernels' constants.  Built into tests/emu/libdenoise_emu.so by the tests
// that use it (tests/denoise_util.py).
#include <vector>

#include "../../gpuspectral_amd/csrc/pt_denoise.h"

using namespace gsp;

extern "C" {

// the validation + struct_size rule.  Returns 0 and out5 = {iterations, bits(inv_sc2), bits(inv_sn2), bits(inv_sz2), bits(inv_sa2)},
// or 1 and the error text in err (cap bytes)
int denoise_emu_resolve(const gsp_denoise* in, uint32_t* out5, char* err, uint32_t cap) {
  DenoiseConsts k;
  const char* why = resolve_denoise(in, k);
  if (why) {
    if (err && cap) {
      std::strncpy(err, why, cap - 1);
      err[cap - 1] = 0;
    }
    return 1;
  }
  out5[0] = k.iterations;
  out5[1] = f2u(k.inv_sc2);
  out5[2] = f2u(k.inv_sn2);
  out5[3] = f2u(k.inv_sz2);
  out5[4] = f2u(k.inv_sa2);
  return 0;
}

// gsp_download_denoised of a full frame: accum, albedo, geom and out are width * height records of 4 floats.  Returns 1 on an
// invalid gsp_denoise
int denoise_emu_run(const gsp_denoise* in, const float* accum, const float* albedo, const float* geom, uint32_t width, uint32_t height, float* out) {
  DenoiseConsts k;
  if (resolve_denoise(in, k)) return 1;
  const size_t n = (size_t)width * height;
  std::vector<dn4> E[2], A(n), G(n);
  E[0].resize(n);
  E[1].resize(n);
  auto rec = [](const float* p, size_t i) { return dn4{p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3]}; };
  for (size_t i = 0; i < n; ++i) {
    denoise_prepare(rec(accum, i), rec(albedo, i), E[0][i], A[i]);
    G[i] = rec(geom, i);
  }
  for (uint32_t level = 0; level < k.iterations; ++level) {
    const std::vector<dn4>& in_ = E[level & 1u];
    std::vector<dn4>& out_ = E[(level + 1u) & 1u];
    for (int y = 0; y < (int)height; ++y)
      for (int x = 0; x < (int)width; ++x)
        out_[(size_t)y * width + x] = denoise_pixel_level(k, level, (int)width, (int)height, x, y, [&](int qx, int qy, dn4& E_, dn4& A_, dn4& G_) {
          const size_t q = (size_t)qy * width + qx;
          E_ = in_[q];
          A_ = A[q];
          G_ = G[q];
        });
  }
  const std::vector<dn4>& fin = E[k.iterations & 1u];
  for (size_t i = 0; i < n; ++i) {
    const dn4 o = denoise_finish(fin[i], A[i], rec(accum, i));
    std::memcpy(out + 4 * i, &o, 16);
  }
  return 0;
}

}  // extern "C"
