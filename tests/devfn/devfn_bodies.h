// tests/devfn/devfn_bodies.h -- TEST HARNESS, NOT A PRODUCT PATH.
//
// One vector of every function family, stated once: pt_devfn.hip runs these bodies on the GPU (one thread per vector),
// tests/emu/pt_emu.cpp runs the same text on the host (a loop).  What is compared is therefore the two compiles of the
// product's headers (gfx950 through hipcc, x86 through g++), never two statements of the calling protocol.
// The bodies read and write only element i of their arrays (and the tables they are given); the entry points validate
// every index a vector carries before they call a body.
#pragma once
#include "../../gpuspectral_amd/csrc/pt_stages.h"

namespace devfn {
using namespace gsp;

constexpr int kBadIndex = -2;  // an entry point refused a vector (no HIP call was made); hipError_t values are positive

// ---- resident BSDF tables: per type, one derived quad per record in reverse order in FRONT of the records (derived_of) ----
constexpr uint32_t kRecBytes[GSP_BSDF_TYPE_COUNT] = {sizeof(gsp_diffuse_bsdf),         sizeof(gsp_smooth_dielectric_bsdf),
                                                     sizeof(gsp_smooth_conductor_bsdf), sizeof(gsp_smooth_plastic_bsdf),
                                                     sizeof(gsp_rough_conductor_bsdf),  sizeof(gsp_smooth_floor_bsdf),
                                                     sizeof(gsp_rough_floor_bsdf),      sizeof(gsp_rough_plastic_bsdf)};
struct TableLayout {
  uint64_t quad_off[GSP_BSDF_TYPE_COUNT], rec_off[GSP_BSDF_TYPE_COUNT], total;
  uint32_t num[GSP_BSDF_TYPE_COUNT];
};
inline TableLayout table_layout(const uint32_t* num) {
  TableLayout L;
  uint64_t cur = 0;
  for (int t = 0; t < GSP_BSDF_TYPE_COUNT; ++t) {
    L.num[t] = num[t];
    L.quad_off[t] = cur;
    cur += 16ull * num[t];
    L.rec_off[t] = cur;
    cur += ((uint64_t)num[t] * kRecBytes[t] + 15ull) & ~15ull;
  }
  L.total = cur + 16;
  return L;
}
GSP_HD BsdfTables tables_at(const uint8_t* base, const TableLayout& L) {
  BsdfTables T;
  T.diffuse = (const gsp_diffuse_bsdf*)(base + L.rec_off[0]);
  T.smooth_dielectric = (const gsp_smooth_dielectric_bsdf*)(base + L.rec_off[1]);
  T.smooth_conductor = (const gsp_smooth_conductor_bsdf*)(base + L.rec_off[2]);
  T.smooth_plastic = (const gsp_smooth_plastic_bsdf*)(base + L.rec_off[3]);
  T.rough_conductor = (const gsp_rough_conductor_bsdf*)(base + L.rec_off[4]);
  T.smooth_floor = (const gsp_smooth_floor_bsdf*)(base + L.rec_off[5]);
  T.rough_floor = (const gsp_rough_floor_bsdf*)(base + L.rec_off[6]);
  T.rough_plastic = (const gsp_rough_plastic_bsdf*)(base + L.rec_off[7]);
  return T;
}
// record i of every table, as k_bake_tables: the derived quads first (bake_bsdf reads the records as uploaded), then the
// diffuse record in place
GSP_HD void bake_tables1(uint64_t i, uint8_t* base, const TableLayout& L) {
  for (uint32_t t = 0; t < GSP_BSDF_TYPE_COUNT; ++t)
    if (i < L.num[t]) ((q4s*)(base + L.rec_off[t]))[-1 - (int32_t)i] = bake_bsdf(t, base + L.rec_off[t] + i * kRecBytes[t]);
  if (i < L.num[0]) {
    gsp_diffuse_bsdf* d = (gsp_diffuse_bsdf*)(base + L.rec_off[0]) + i;
    gsp_diffuse_bsdf b = *d;
    bake_diffuse(b);
    *d = b;
  }
}
GSP_HD void bake_light1(uint64_t i, gsp_triangle_light* lights) {
  gsp_triangle_light L = lights[i];
  bake_light(L);
  lights[i] = L;
}

GSP_HD void put3(float* o, f3 v) {
  o[0] = v.x;
  o[1] = v.y;
  o[2] = v.z;
}

// ---- math ----
GSP_HD void math1(uint64_t i, const float* x, float* s, float* c, float* lg, float* ex, float* sq, float* rc) {
  det_sincosf(x[i], s[i], c[i]);
  lg[i] = det_logf(x[i]);
  ex[i] = det_expf(x[i]);
  sq[i] = gsqrt(x[i]);
  rc[i] = 1.0f / x[i];
}
GSP_HD void atan2_1(uint64_t i, const float* y, const float* x, float* out) { out[i] = det_atan2f(y[i], x[i]); }
GSP_HD void normalize1(uint64_t i, const float* v, float* out) { put3(out + 3 * i, normalize(ld3(v + 3 * i))); }

// ---- rng: out7 = {tea(a, b), pcg_hash(a), from state a: pcg_next, pcg_next, rand_uniform bits, state afterwards, and the
// frame seed of pixel index a at timestamp b (generate_path, pt_stages.h)}
GSP_HD void rng1(uint64_t i, const uint32_t* a, const uint32_t* b, uint32_t* out7) {
  uint32_t* o = out7 + 7 * i;
  o[0] = tea(a[i], b[i]);
  o[1] = pcg_hash(a[i]);
  uint32_t st = a[i];
  o[2] = pcg_next(st);
  o[3] = pcg_next(st);
  o[4] = f2u(rand_uniform(st));
  o[5] = st;
  o[6] = pcg_hash(tea(a[i], b[i]));
}

// ---- frame and helpers ----
GSP_HD void onb1(uint64_t i, const float* nrm, const float* v, float* out15) {
  const Frame f = make_frame(ld3(nrm + 3 * i));
  const f3 w = ld3(v + 3 * i);
  float* o = out15 + 15 * i;
  put3(o, f.t);
  put3(o + 3, f.b);
  put3(o + 6, f.n);
  put3(o + 9, to_local(f, w));
  put3(o + 12, to_world(f, w));
}
GSP_HD void helpers1(uint64_t i, const float* f, const float* g, const uint32_t* h, uint32_t* out3) {
  out3[3 * i] = f2u(power_heuristic(f[i], g[i]));
  out3[3 * i + 1] = f2u(cosine_pdf(mk3(0.0f, 0.0f, f[i])));
  out3[3 * i + 2] = bsdf_transmits(h[i]) ? 1u : 0u;
}
// out8 = {sample_cosine_hemisphere xyz, state afterwards, sample_half_beckmann xyz, state afterwards}, both from `seed`
GSP_HD void samplers1(uint64_t i, const uint32_t* seeds, const float* alpha, float* out8) {
  float* o = out8 + 8 * i;
  uint32_t rng = seeds[i];
  put3(o, sample_cosine_hemisphere(rng));
  o[3] = u2f(rng);
  rng = seeds[i];
  put3(o + 4, sample_half_beckmann(rng, alpha[i]));
  o[7] = u2f(rng);
}

// ---- bsdf: out9 as emu_bsdf_sample; out5 as emu_bsdf_eval (the sampler of the same vertex runs first, with state 1, and hands
// its BsdfCarry to the evaluation)
GSP_HD void bsdf1(uint64_t i, const BsdfTables& T, const uint32_t* handles, const float* wo, const uint32_t* seeds, const float* wi,
                  float* out9, float* out5) {
  const f3 o = ld3(wo + 3 * i);
  {
    uint32_t rng = seeds[i];
    f3 w;
    BsdfResult r;
    BsdfCarry cy;
    bsdf_sample(T, handles[i], rng, o, w, r, cy);
    float* q = out9 + 9 * i;
    put3(q, w);
    put3(q + 3, r.f);
    q[6] = r.pdf;
    q[7] = r.delta ? 1.0f : 0.0f;
    q[8] = u2f(rng);
  }
  {
    uint32_t rng = 1u;
    f3 w0;
    BsdfResult r0, r;
    BsdfCarry cy;
    bsdf_sample(T, handles[i], rng, o, w0, r0, cy);
    bsdf_eval(T, handles[i], o, ld3(wi + 3 * i), r, cy);
    float* q = out5 + 5 * i;
    put3(q, r.f);
    q[3] = r.pdf;
    q[4] = r.delta ? 1.0f : 0.0f;
  }
}

// ---- light: out8 as emu_sample_light; `lights` are baked records
GSP_HD void light1(uint64_t i, const gsp_triangle_light* lights, uint32_t num_lights, float inv_num_lights, const float* pos,
                   const uint32_t* seeds, float* out8) {
  uint32_t rng = seeds[i];
  const LightSample r = sample_light(lights, num_lights, inv_num_lights, rng, ld3(pos + 3 * i));
  float* o = out8 + 8 * i;
  put3(o, r.position);
  put3(o + 3, r.emission);
  o[6] = r.pdf;
  o[7] = u2f(rng);
}

// ---- texture ----
GSP_HD void texture1(uint64_t i, const TextureView& T, const uint32_t* ids, const float* uv, float* out3) {
  put3(out3 + 3 * i, sample_texture(T, ids[i], uv[2 * i], uv[2 * i + 1]));
}
GSP_HD void envmap1(uint64_t i, const TextureView& T, const float* dirs, float* out3) {
  put3(out3 + 3 * i, sample_envmap(T, ld3(dirs + 3 * i)));
}

// ---- trace ----
// rays: {o.xyz, d.xyz, tmin, tmax}, tris: 9 floats; out: {hit, t, u, v} of intersect_tri and of intersect_tri_rot (emu_tri_tests)
GSP_HD void tri1(uint64_t i, const float* rays, const float* tris, float* out_ref, float* out_rot) {
  const float* r = rays + 8 * i;
  const float* p = tris + 9 * i;
  const f3 o = ld3(r), d = ld3(r + 3);
  const f3 v0 = ld3(p), v1 = ld3(p + 3), v2 = ld3(p + 6);
  float t = 0.0f, u = 0.0f, v = 0.0f;
  const RayShear rs = make_shear(d);
  const bool h0 = intersect_tri(v0, v1, v2, o, rs, r[6], r[7], t, u, v);
  out_ref[4 * i + 0] = h0 ? 1.0f : 0.0f;
  out_ref[4 * i + 1] = h0 ? t : 0.0f;
  out_ref[4 * i + 2] = h0 ? u : 0.0f;
  out_ref[4 * i + 3] = h0 ? v : 0.0f;
  const RayShearRot rr = make_shear_rot(d);
  const bool h1 = intersect_tri_rot(v0, v1, v2, o, rr, r[6], r[7], t, u, v);
  out_rot[4 * i + 0] = h1 ? 1.0f : 0.0f;
  out_rot[4 * i + 1] = h1 ? t : 0.0f;
  out_rot[4 * i + 2] = h1 ? u : 0.0f;
  out_rot[4 * i + 3] = h1 ? v : 0.0f;
}
// out12 = make_shear {kx, ky, kz, Sx, Sy, Sz}, make_shear_rot {m0, m1, ms, Sx, Sy, Sz} (words)
GSP_HD void shear1(uint64_t i, const float* d, uint32_t* out12) {
  uint32_t* o = out12 + 12 * i;
  const RayShear a = make_shear(ld3(d + 3 * i));
  o[0] = (uint32_t)a.kx;
  o[1] = (uint32_t)a.ky;
  o[2] = (uint32_t)a.kz;
  o[3] = f2u(a.Sx);
  o[4] = f2u(a.Sy);
  o[5] = f2u(a.Sz);
  const RayShearRot b = make_shear_rot(ld3(d + 3 * i));
  o[6] = b.m0;
  o[7] = b.m1;
  o[8] = b.ms;
  o[9] = f2u(b.Sx);
  o[10] = f2u(b.Sy);
  o[11] = f2u(b.Sz);
}
// boxes: 4 x {lo.xyz, hi.xyz}; counts: {ni, nl}; out: 16 words of encode_node_w4_ref and of encode_node_w4 (emu_encode_nodes)
GSP_HD void encode1(uint64_t i, const float* boxes, const int32_t* counts, uint32_t* out_ref, uint32_t* out_fast) {
  WideChild wc[4];
  for (int k = 0; k < 4; ++k) {
    const float* b = boxes + 24 * i + 6 * k;
    wc[k].lo = make_q4(b[0], b[1], b[2], 0.0f);
    wc[k].hi = make_q4(b[3], b[4], b[5], 0.0f);
  }
  q4 a[4], c[4];
  const int ni = counts[2 * i], nl = counts[2 * i + 1];
  encode_node_w4_ref(a, wc, ni, nl, 1000u + (uint32_t)i, 77u + (uint32_t)i);
  encode_node_w4(c, wc, ni, nl, 1000u + (uint32_t)i, 77u + (uint32_t)i);
  for (int k = 0; k < 4; ++k) {
    const float ra[4] = {a[k].x, a[k].y, a[k].z, a[k].w}, rc[4] = {c[k].x, c[k].y, c[k].z, c[k].w};
    for (int j = 0; j < 4; ++j) {
      out_ref[16 * i + 4 * k + j] = f2u(ra[j]);
      out_fast[16 * i + 4 * k + j] = f2u(rc[j]);
    }
  }
}
// nodes: 16 words per record; rays: {o.xyz, d.xyz, tmin, tfar}; out12 = {node_test mask, make_raybox: inv.xyz, invc.xyz,
// negx | negy << 1 | negz << 2 | octhi << 3, octshift, mx & 1 | my & 2 | mz & 4}, one spare word
GSP_HD void nodetest1(uint64_t i, const uint32_t* nodes, const uint32_t* node_idx, const float* rays, uint32_t* out12) {
  const float* r = rays + 8 * i;
  const RayBox rb = make_raybox(ld3(r), ld3(r + 3));
  q4 n[4];
  const uint32_t* w = nodes + 16ull * node_idx[i];
  for (int k = 0; k < 4; ++k) n[k] = make_q4(u2f(w[4 * k]), u2f(w[4 * k + 1]), u2f(w[4 * k + 2]), u2f(w[4 * k + 3]));
  uint32_t* o = out12 + 12 * i;
  o[0] = node_test(n, rb, r[6], r[7]);
  o[1] = f2u(rb.inv.x);
  o[2] = f2u(rb.inv.y);
  o[3] = f2u(rb.inv.z);
  o[4] = f2u(rb.invc.x);
  o[5] = f2u(rb.invc.y);
  o[6] = f2u(rb.invc.z);
  o[7] = (rb.negx ? 1u : 0u) | (rb.negy ? 2u : 0u) | (rb.negz ? 4u : 0u) | (rb.octhi ? 8u : 0u);
  o[8] = rb.octshift;
  o[9] = (rb.mx & 1u) | (rb.my & 2u) | (rb.mz & 4u);
  o[10] = f2u(rb.o.x);
  o[11] = 0u;
}

// ---- what the entry points check on the host before any vector runs: no vector may index outside its arrays ----
inline bool ok_handles(const uint32_t* handles, uint64_t n, const uint32_t* num) {
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t t = handles[i] >> 16, k = handles[i] & 0xffffu;
    if (t >= GSP_BSDF_TYPE_COUNT || k >= num[t]) return false;
  }
  return true;
}
inline bool ok_textures(const gsp_texture* tx, uint32_t num_textures, uint64_t num_texels, const uint32_t* ids, uint64_t n) {
  for (uint32_t k = 0; k < num_textures; ++k) {
    if (tx[k].width == 0 || tx[k].height == 0 || tx[k].width > 32768u || tx[k].height > 32768u) return false;
    if (tx[k].first_texel > num_texels || (uint64_t)tx[k].width * tx[k].height > num_texels - tx[k].first_texel) return false;
  }
  for (uint64_t i = 0; i < n; ++i)
    if (ids[i] >= num_textures) return false;
  return true;
}
inline bool ok_child_counts(const int32_t* counts, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i) {
    const int32_t ni = counts[2 * i], nl = counts[2 * i + 1];
    if (ni < 0 || nl < 0 || ni + nl > kWide) return false;
  }
  return true;
}
inline bool ok_node_indices(const uint32_t* idx, uint64_t n, uint64_t num_nodes) {
  for (uint64_t i = 0; i < n; ++i)
    if (idx[i] >= num_nodes) return false;
  return true;
}

}  // namespace devfn
