// tests/emu/svgf_emu.cpp -- TEST HARNESS, NOT A PRODUCT PATH.
//
// The variance-guided filter of the library (include/gpuspectral_pt.h, "Variance-guided filter") compiled for the host: the very
// text the kernels k_temporal_reproject_moments / k_svgf_variance / k_svgf_atrous run (csrc/pt_svgf.h), driven by plain loops over
// the frame, plus the validation and the resolution of a gsp_denoise + gsp_svgf into the kernels' constants.  Built into
// tests/emu/libsvgf_emu.so by the tests that use it (tests/svgf_util.py).
#include <vector>

#include "../../gpuspectral_amd/csrc/pt_svgf.h"

using namespace gsp;

namespace {
void put_error(const char* why, char* err, uint32_t cap) {
  if (err && cap) {
    std::strncpy(err, why, cap - 1);
    err[cap - 1] = 0;
  }
}
dn4 rec(const float* q, size_t i) { return dn4{q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]}; }

struct Planes {
  std::vector<dn4> E, A, G;
  std::vector<float> V;
};

void prepare(const float* hist, const float* albedo, const float* geom, size_t n, Planes& p) {
  p.E.resize(n);
  p.A.resize(n);
  p.G.resize(n);
  p.V.assign(n, 0.0f);
  for (size_t i = 0; i < n; ++i) {
    denoise_prepare(rec(hist, i), rec(albedo, i), p.E[i], p.A[i]);
    p.G[i] = rec(geom, i);
  }
}

void variance(const SvgfConsts& k, const float* hist, const float* moments, uint32_t width, uint32_t height, Planes& p) {
  for (int y = 0; y < (int)height; ++y)
    for (int x = 0; x < (int)width; ++x) {
      const size_t i = (size_t)y * width + x;
      p.V[i] = svgf_variance_pixel(k, (int)width, (int)height, x, y, hist[4 * i + 3], rec(moments, i), [&](int qx, int qy, float& L_, float& valid_, dn4& G_) {
        const size_t q = (size_t)qy * width + qx;
        L_ = p.E[q].w;
        valid_ = p.A[q].w;
        G_ = p.G[q];
      });
    }
}

void level(const SvgfConsts& k, uint32_t lvl, uint32_t width, uint32_t height, const Planes& in, std::vector<dn4>& Eout, std::vector<float>& Vout) {
  for (int y = 0; y < (int)height; ++y)
    for (int x = 0; x < (int)width; ++x) {
      const SvgfLevelOut o = svgf_pixel_level(k, lvl, (int)width, (int)height, x, y, [&](int qx, int qy, dn4& E_, dn4& A_, dn4& G_, float& V_) {
        const size_t q = (size_t)qy * width + qx;
        E_ = in.E[q];
        A_ = in.A[q];
        G_ = in.G[q];
        V_ = in.V[q];
      });
      Eout[(size_t)y * width + x] = o.E;
      Vout[(size_t)y * width + x] = o.V;
    }
}
}  // namespace

extern "C" {

// the validation + struct_size rule.  Returns 0 and out7 = {iterations, bits(inv_sn2), bits(inv_sz2), bits(inv_sa2), bits(min_history
// as float), bits(sigma_v), lum_on}, or 1 and the error text in err (cap bytes)
int svgf_emu_resolve(const gsp_denoise* dn, const gsp_svgf* in, uint32_t* out7, char* err, uint32_t cap) {
  SvgfConsts k;
  if (const char* why = resolve_svgf(dn, in, k)) {
    put_error(why, err, cap);
    return 1;
  }
  out7[0] = k.iterations;
  out7[1] = f2u(k.inv_sn2);
  out7[2] = f2u(k.inv_sz2);
  out7[3] = f2u(k.inv_sa2);
  out7[4] = f2u(k.min_history);
  out7[5] = f2u(k.sigma_v);
  out7[6] = k.lum_on;
  return 0;
}

// One gsp_temporal_accumulate of a full frame with tracking on: temporal_emu_run's arguments plus the moments plane read and
// written (width * height records of 4 floats).  Returns 0, 1 (invalid gsp_temporal) or 2 (singular previous camera).
int svgf_emu_accumulate(const gsp_temporal* in, const gsp_camera* cur, const gsp_camera* prev, int history_valid, uint32_t width, uint32_t height,
                        const float* accum, const float* albedo, const float* geom, const uint32_t* ids, const float* h_prev, const float* g_prev,
                        const uint32_t* i_prev, const float* m_prev, float* h_out, float* g_out, uint32_t* i_out, float* m_out, char* err, uint32_t cap) {
  TemporalParams p;
  if (const char* why = resolve_temporal(in, p)) {
    put_error(why, err, cap);
    return 1;
  }
  TemporalConsts k;
  if (const char* why = temporal_consts(*cur, prev, history_valid != 0, width, height, p, k)) {
    put_error(why, err, cap);
    return 2;
  }
  auto fetch = [&](int x, int y, dn4& H_, dn4& G_, uint32_t& I_, dn4& M_) {
    const size_t q = (size_t)y * width + (size_t)x;
    H_ = rec(h_prev, q);
    G_ = rec(g_prev, q);
    I_ = i_prev[q];
    M_ = rec(m_prev, q);
  };
  for (int y = 0; y < (int)height; ++y)
    for (int x = 0; x < (int)width; ++x) {
      const size_t i = (size_t)y * width + (size_t)x;
      const TemporalMomentsOut o = temporal_pixel_moments(k, x, y, rec(accum, i), rec(albedo, i), rec(geom, i), ids[4 * i + 2], fetch);
      std::memcpy(h_out + 4 * i, &o.t.H, 16);
      std::memcpy(g_out + 4 * i, &o.t.G, 16);
      i_out[i] = o.t.I;
      std::memcpy(m_out + 4 * i, &o.M, 16);
    }
  return 0;
}

// gsp_download_temporal_svgf of a full frame: hist, moments, albedo, geom and out are width * height records of 4 floats; v0_out
// and v_out (optional, width * height floats): the initial variance and the input variance of the LAST level.  Returns 1 on
// invalid parameters.
int svgf_emu_run(const gsp_denoise* dn, const gsp_svgf* in, const float* hist, const float* moments, const float* albedo, const float* geom, uint32_t width,
                 uint32_t height, float* out, float* v0_out, float* v_out) {
  SvgfConsts k;
  if (resolve_svgf(dn, in, k)) return 1;
  const size_t n = (size_t)width * height;
  Planes p;
  prepare(hist, albedo, geom, n, p);
  variance(k, hist, moments, width, height, p);
  if (v0_out) std::memcpy(v0_out, p.V.data(), n * sizeof(float));
  std::vector<dn4> E2(n);
  std::vector<float> V2(n);
  for (uint32_t lvl = 0; lvl < k.iterations; ++lvl) {
    if (v_out && lvl + 1 == k.iterations) std::memcpy(v_out, p.V.data(), n * sizeof(float));
    level(k, lvl, width, height, p, E2, V2);
    p.E.swap(E2);
    p.V.swap(V2);
  }
  for (size_t i = 0; i < n; ++i) {
    const dn4 o = denoise_finish(p.E[i], p.A[i], rec(hist, i));
    std::memcpy(out + 4 * i, &o, 16);
  }
  return 0;
}

// One level on planes given as they are: E, A, G (records of 4 floats) and V (floats) in, E and V out.
int svgf_emu_level(const gsp_denoise* dn, const gsp_svgf* in, uint32_t lvl, const float* E, const float* A, const float* G, const float* V, uint32_t width,
                   uint32_t height, float* e_out, float* v_out) {
  SvgfConsts k;
  if (resolve_svgf(dn, in, k)) return 1;
  const size_t n = (size_t)width * height;
  Planes p;
  p.E.resize(n);
  p.A.resize(n);
  p.G.resize(n);
  p.V.assign(V, V + n);
  for (size_t i = 0; i < n; ++i) {
    p.E[i] = rec(E, i);
    p.A[i] = rec(A, i);
    p.G[i] = rec(G, i);
  }
  std::vector<dn4> E2(n);
  std::vector<float> V2(n);
  level(k, lvl, width, height, p, E2, V2);
  std::memcpy(e_out, E2.data(), n * 16);
  std::memcpy(v_out, V2.data(), n * sizeof(float));
  return 0;
}

}  // extern "C"
