// pt_features.h -- first-hit feature buffers (include/gpuspectral_pt.h, "Feature buffers"): what one feature sample -- the camera
// ray of a beauty sample, traced to its closest hit -- contributes to the albedo / normal / depth / id planes, and the running
// mean.  GSP_HD: k_features (pt_render_kernels.inc) and the host emulation (tests/emu/features_emu.cpp) compile this text.
//
// The normal is shade_vertex's SN (pt_stages.h; rayhit.rchit:690-707), operation for operation: the same packet reads, the same
// barycentric sum, the same two-faced flip.  No existing function is touched: shade_vertex stays what it is.
#pragma once
#include "pt_stages.h"

namespace gsp {

struct FeatureSample {
  f3 albedo;
  float coverage;  // 1 on a hit; a miss is all zero
  f3 normal;
  float depth;     // the hit's t
  uint32_t bsdf;   // BSDF handle of the hit triangle (0xffffffff on a miss)
};

GSP_HD FeatureSample feature_miss() {
  FeatureSample f;
  f.albedo = splat(0.0f);
  f.coverage = 0.0f;
  f.normal = splat(0.0f);
  f.depth = 0.0f;
  f.bsdf = 0xffffffffu;
  return f;
}

// the kD of a record as uploaded: the header's albedo table (the resident diffuse record holds reflectance / pi, bake_diffuse)
GSP_HD f3 feature_record_albedo(const BsdfTables& T, uint32_t handle) {
  const uint32_t i = handle & 0xffffu;
  switch (handle >> 16) {
    case GSP_BSDF_DIFFUSE: return ld3(T.diffuse[i].reflectance) * kPi;
    case GSP_BSDF_SMOOTH_PLASTIC: return ld3(T.smooth_plastic[i].diffuse);
    case GSP_BSDF_ROUGH_CONDUCTOR: return ld3(T.rough_conductor[i].reflectance);
    case GSP_BSDF_SMOOTH_FLOOR: return ld3(T.smooth_floor[i].diffuse);
    case GSP_BSDF_ROUGH_FLOOR: return ld3(T.rough_floor[i].diffuse);
    case GSP_BSDF_ROUGH_PLASTIC: return ld3(T.rough_plastic[i].diffuse);
    default: return splat(1.0f);  // SMOOTH_CONDUCTOR, SMOOTH_DIELECTRIC
  }
}

// sp: the four quads of the hit triangle's shading packet; uv: its two quads of texture coordinates (TEX only, may be null)
template <bool TEX>
GSP_HD FeatureSample feature_vertex(const BsdfTables& T, const TextureView& tex, const q4* sp, const q4* uv, f3 rayDir, const HitRec& hit) {
  const q4 s0 = sp[0], s1 = sp[1], s2 = sp[2], s3 = sp[3];
  const uint32_t material = f2u(s0.w);
  const uint32_t bsdf = material & 0x0007ffffu;  // (without the medium number of bits 19..30: "Interior media")
  const bool twofaced = (material >> 31) != 0u;
  const f3 emission = mk3(s1.w, s2.w, s3.w);
  const float b0 = (1.0f - hit.u) - hit.v;                                // :690
  f3 SN = normalize((b0 * mk3(s1.x, s1.y, s1.z) + hit.u * mk3(s2.x, s2.y, s2.z)) + hit.v * mk3(s3.x, s3.y, s3.z));
  const f3 N = mk3(s0.x, s0.y, s0.z);
  const bool emits = !(emission.x == 0.0f && emission.y == 0.0f && emission.z == 0.0f);
  if (dot(N, -rayDir) < 0.0f) {                                           // :698-707
    if (twofaced && !emits) SN = SN * -1.0f;
  }
  FeatureSample f;
  f.coverage = 1.0f;
  f.normal = SN;
  f.depth = hit.t;
  f.bsdf = bsdf;
  if (emits) {
    f.albedo = mk3(gmin(emission.x, 1.0f), gmin(emission.y, 1.0f), gmin(emission.z, 1.0f));
    return f;
  }
  if (TEX) {  // the kd of shade_vertex<true>
    const uint32_t tid = bsdf_texture(T, bsdf);
    if (tid != 0u && tid <= tex.num_textures && uv != nullptr) {
      const q4 ua = uv[0], ub2 = uv[1];
      const float tu = (b0 * ua.x + hit.u * ua.z) + hit.v * ub2.x;
      const float tv = (b0 * ua.y + hit.u * ua.w) + hit.v * ub2.y;
      f.albedo = sample_texture(tex, tid - 1u, tu, tv);
      return f;
    }
  }
  f.albedo = feature_record_albedo(T, bsdf);
  return f;
}

// instance of scene triangle g: the last one with tri_first <= g (tri_first is ascending, num_instances + 1 entries)
GSP_HD uint32_t feature_instance(const uint32_t* tri_first, uint32_t num_instances, uint32_t g) {
  uint32_t lo = 0, hi = num_instances;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (tri_first[mid] <= g) lo = mid;
    else hi = mid;
  }
  return lo;
}

// the running mean of a channel after n folded samples: mix(prev, x, 1 / (n + 1)) in the form prev + (x - prev) * a, which
// returns prev exactly when x == prev (the unfiltered pinhole: every sample of a pixel is the same) and x exactly when n == 0
GSP_HD float feature_mix(float prev, float x, float a) { return prev + (x - prev) * a; }

// the three planes of one pixel, held in registers over a call's timestamps
struct FeaturePixel {
  q4 albedo;  // {r, g, b, coverage}
  q4 geom;    // {nx, ny, nz, depth}
  uint32_t tri, bsdf, inst, n;
};

GSP_HD void feature_fold(FeaturePixel& p, const FeatureSample& f, uint32_t tri, uint32_t inst) {
  const float a = 1.0f / (float)(p.n + 1u);
  p.albedo.x = feature_mix(p.albedo.x, f.albedo.x, a);
  p.albedo.y = feature_mix(p.albedo.y, f.albedo.y, a);
  p.albedo.z = feature_mix(p.albedo.z, f.albedo.z, a);
  p.albedo.w = feature_mix(p.albedo.w, f.coverage, a);
  p.geom.x = feature_mix(p.geom.x, f.normal.x, a);
  p.geom.y = feature_mix(p.geom.y, f.normal.y, a);
  p.geom.z = feature_mix(p.geom.z, f.normal.z, a);
  p.geom.w = feature_mix(p.geom.w, f.depth, a);
  if (p.n == 0u) {  // the ids are those of the first sample folded in this frame
    p.tri = tri;
    p.bsdf = f.bsdf;
    p.inst = inst;
  }
  p.n += 1u;
}

}  // namespace gsp
