// pt_hostmath.h -- host-side float32 linear algebra of gsp_upload_scene.
#pragma once
#include <cmath>
#include <cstring>

#include "../../include/gpuspectral_pt.h"

namespace gsp {

// gsp_set_lens: the host's struct under the struct_size rule (fields it does not have are 0; NULL = pinhole), validated as
// include/gpuspectral_pt.h "Thin lens" says.  Returns nullptr and the lens in `out`, or the text for gsp_last_error.
inline const char* resolve_lens(const gsp_lens* host, gsp_lens& out) {
  gsp_lens l;
  std::memset(&l, 0, sizeof(l));
  if (host) {
    if (host->struct_size < sizeof(uint32_t)) return "gsp_lens.struct_size is smaller than the field itself: set it to sizeof(gsp_lens)";
    std::memcpy(&l, host, host->struct_size < sizeof(l) ? host->struct_size : sizeof(l));
  }
  if (!(l.radius >= 0.0f) || std::isinf(l.radius)) return "gsp_lens.radius must be 0 (pinhole) or a finite positive value";
  if (l.radius > 0.0f && (!(l.focus_distance > 0.0f) || std::isinf(l.focus_distance)))
    return "gsp_lens.focus_distance must be finite and positive when radius > 0";
  if (l.blades != 0u && (l.blades < 3u || l.blades > 16u)) return "gsp_lens.blades must be 0 (circular aperture) or 3..16";
  if (!std::isfinite(l.rotation)) return "gsp_lens.rotation must be finite";
  l.struct_size = (uint32_t)sizeof(gsp_lens);
  out = l;
  return nullptr;
}

// gsp_set_media: the table as include/gpuspectral_pt.h "Interior media" wants it (NULL or 0 entries = none).  Returns nullptr or
// the text for gsp_last_error.
inline const char* check_media(const gsp_medium* media, uint32_t num_media) {
  if (!media || num_media == 0u) return nullptr;
  if (num_media > GSP_MAX_MEDIA) return "gsp_set_media: at most 4095 media (the medium number is 12 bits of the BSDF handle)";
  for (uint32_t k = 0; k < num_media; ++k)
    for (int c = 0; c < 3; ++c)
      if (!(media[k].sigma_a[c] >= 0.0f) || std::isinf(media[k].sigma_a[c])) return "gsp_medium.sigma_a must be finite and >= 0";
  return nullptr;
}
// gsp_set_media_scattering: the table parallel to the context's `have` media (include/gpuspectral_pt.h, "Scattering media"; NULL or
// 0 entries = none).  Returns nullptr or the text for gsp_last_error.
inline const char* check_media_scattering(const gsp_medium_scatter* scatter, uint32_t n, uint32_t have) {
  if (!scatter || n == 0u) return nullptr;
  if (n != have) return "gsp_set_media_scattering: the count must be 0 or the context's media count (the table is parallel to gsp_set_media's)";
  for (uint32_t k = 0; k < n; ++k) {
    for (int c = 0; c < 3; ++c)
      if (!(scatter[k].sigma_s[c] >= 0.0f) || std::isinf(scatter[k].sigma_s[c])) return "gsp_medium_scatter.sigma_s must be finite and >= 0";
    if (!(std::fabs(scatter[k].g) < 1.0f)) return "gsp_medium_scatter.g must be finite with |g| < 1";
  }
  return nullptr;
}
// does any medium of the table scatter?  (selects the <SCT> kernels)
inline bool any_scattering(const gsp_medium_scatter* scatter, size_t n) {
  for (size_t k = 0; k < n; ++k)
    if (scatter[k].sigma_s[0] != 0.0f || scatter[k].sigma_s[1] != 0.0f || scatter[k].sigma_s[2] != 0.0f) return true;
  return false;
}
// the largest medium number the instances name (bits 19..30 of gsp_instance.bsdf)
inline uint32_t max_medium_number(const gsp_instance* inst, size_t n) {
  uint32_t m = 0;
  for (size_t i = 0; i < n; ++i) m = ((inst[i].bsdf >> 19) & 0xfffu) > m ? ((inst[i].bsdf >> 19) & 0xfffu) : m;
  return m;
}

// ---- host-side linear algebra for PathTracer::prepareScene (PathTracer.cpp:62) ------
// glm::inverse(glm::transpose(M)); cofactor expansion in glm's order so the
// float32 result matches a glm build of the reference.
inline void transpose4(const float* m, float* o) {
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) o[4 * c + r] = m[4 * r + c];
}
inline void inverse4(const float* a, float* o) {
  auto M = [&](int c, int r) { return a[4 * c + r]; };
  const float c00 = M(2, 2) * M(3, 3) - M(3, 2) * M(2, 3), c02 = M(1, 2) * M(3, 3) - M(3, 2) * M(1, 3),
              c03 = M(1, 2) * M(2, 3) - M(2, 2) * M(1, 3), c04 = M(2, 1) * M(3, 3) - M(3, 1) * M(2, 3),
              c06 = M(1, 1) * M(3, 3) - M(3, 1) * M(1, 3), c07 = M(1, 1) * M(2, 3) - M(2, 1) * M(1, 3),
              c08 = M(2, 1) * M(3, 2) - M(3, 1) * M(2, 2), c10 = M(1, 1) * M(3, 2) - M(3, 1) * M(1, 2),
              c11 = M(1, 1) * M(2, 2) - M(2, 1) * M(1, 2), c12 = M(2, 0) * M(3, 3) - M(3, 0) * M(2, 3),
              c14 = M(1, 0) * M(3, 3) - M(3, 0) * M(1, 3), c15 = M(1, 0) * M(2, 3) - M(2, 0) * M(1, 3),
              c16 = M(2, 0) * M(3, 2) - M(3, 0) * M(2, 2), c18 = M(1, 0) * M(3, 2) - M(3, 0) * M(1, 2),
              c19 = M(1, 0) * M(2, 2) - M(2, 0) * M(1, 2), c20 = M(2, 0) * M(3, 1) - M(3, 0) * M(2, 1),
              c22 = M(1, 0) * M(3, 1) - M(3, 0) * M(1, 1), c23 = M(1, 0) * M(2, 1) - M(2, 0) * M(1, 1);
  const float f0[4] = {c00, c00, c02, c03}, f1[4] = {c04, c04, c06, c07}, f2[4] = {c08, c08, c10, c11},
              f3_[4] = {c12, c12, c14, c15}, f4[4] = {c16, c16, c18, c19}, f5[4] = {c20, c20, c22, c23};
  const float v0[4] = {M(1, 0), M(0, 0), M(0, 0), M(0, 0)}, v1[4] = {M(1, 1), M(0, 1), M(0, 1), M(0, 1)},
              v2[4] = {M(1, 2), M(0, 2), M(0, 2), M(0, 2)}, v3[4] = {M(1, 3), M(0, 3), M(0, 3), M(0, 3)};
  const float sa[4] = {1.0f, -1.0f, 1.0f, -1.0f}, sb[4] = {-1.0f, 1.0f, -1.0f, 1.0f};
  float inv[4][4];
  for (int i = 0; i < 4; ++i) {
    inv[0][i] = ((v1[i] * f0[i] - v2[i] * f1[i]) + v3[i] * f2[i]) * sa[i];
    inv[1][i] = ((v0[i] * f0[i] - v2[i] * f3_[i]) + v3[i] * f4[i]) * sb[i];
    inv[2][i] = ((v0[i] * f1[i] - v1[i] * f3_[i]) + v3[i] * f5[i]) * sa[i];
    inv[3][i] = ((v0[i] * f2[i] - v1[i] * f4[i]) + v2[i] * f5[i]) * sb[i];
  }
  const float d0 = M(0, 0) * inv[0][0], d1 = M(0, 1) * inv[1][0], d2 = M(0, 2) * inv[2][0], d3 = M(0, 3) * inv[3][0];
  const float ood = 1.0f / ((d0 + d1) + (d2 + d3));
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) o[4 * c + r] = inv[c][r] * ood;
}


}  // namespace gsp
