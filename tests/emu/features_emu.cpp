// tests/emu/features_emu.cpp -- TEST HARNESS, NOT A PRODUCT PATH.
//
// The feature-buffer side of the host emulation (include/gpuspectral_pt.h, "Feature buffers").  It includes lens_emu.cpp textually
// -- and through it filter_emu.cpp and pt_emu.cpp: scene, BVH, per-ray traversal, the filter's and the lens's constants -- and adds
// the loop of k_features over the product's own pt_features.h: generate_path, the emulation's traversal, feature_vertex,
// feature_fold.  Built into tests/emu/libfeatures_emu.so by the tests that use it (tests/features_util.py).
#include "lens_emu.cpp"

#include "../../gpuspectral_amd/csrc/pt_features.h"

extern "C" {

// gsp_render_features on the compact planes (npix records of 16 bytes each, read and written: a second call continues the means)
int features_emu_render(void* h, uint32_t width, uint32_t height, const uint32_t* pixel_ids, uint64_t num_pixels,
                        const gsp_render_params* rp, const gsp_lens* lens, float* albedo, float* geom, uint32_t* ids) {
  Emu* e = (Emu*)h;
  const RenderConstsLens rc = lens_consts_for(width, height, e->sc.camera.fov, e->sc.camera.to_world, rp->pixel_filter, rp->pixel_filter_param, lens);
  const uint64_t npix = pixel_ids ? num_pixels : (uint64_t)width * height;
  const SceneView& S = e->view;
  std::vector<uint32_t> tri_first(e->sc.num_instances + 1ull);
  uint32_t acc = 0;
  for (uint32_t i = 0; i < e->sc.num_instances; ++i) tri_first[i] = acc, acc += e->instances[i].vertex_count / 3;
  tri_first[e->sc.num_instances] = acc;
  for (uint64_t lp = 0; lp < npix; ++lp) {
    const uint32_t gid = pixel_ids ? pixel_ids[lp] : (uint32_t)lp;
    FeaturePixel px;
    px.albedo = mkq(albedo[4 * lp], albedo[4 * lp + 1], albedo[4 * lp + 2], albedo[4 * lp + 3]);
    px.geom = mkq(geom[4 * lp], geom[4 * lp + 1], geom[4 * lp + 2], geom[4 * lp + 3]);
    px.tri = ids[4 * lp];
    px.bsdf = ids[4 * lp + 1];
    px.inst = ids[4 * lp + 2];
    px.n = ids[4 * lp + 3];
    for (uint32_t s = 0; s < rp->spp; ++s) {
      PathState p;
      generate_path(rc, gid, rp->first_timestamp + s, 0, p);
      HitRec hit;
      uint32_t aux;
      trace1<false>(S, p.o, p.d, 0.0f, 1e10f, hit, aux);
      if (hit.slot < 0 || e->sc.num_vertices == 0) {
        feature_fold(px, feature_miss(), 0xffffffffu, 0xffffffffu);
        continue;
      }
      const q4* sp = S.tri_shade + 4ll * hit.slot;
      const q4* uv = (e->textured && S.tex.tri_uv != nullptr) ? (const q4*)S.tex.tri_uv + 2ll * hit.slot : nullptr;
      const FeatureSample f = e->textured ? feature_vertex<true>(S.bsdf, S.tex, sp, uv, p.d, hit) : feature_vertex<false>(S.bsdf, S.tex, sp, uv, p.d, hit);
      const uint32_t tri = e->slot_to_global[hit.slot];
      feature_fold(px, f, tri, feature_instance(tri_first.data(), e->sc.num_instances, tri));
    }
    const float a4[4] = {px.albedo.x, px.albedo.y, px.albedo.z, px.albedo.w}, g4[4] = {px.geom.x, px.geom.y, px.geom.z, px.geom.w};
    const uint32_t i4[4] = {px.tri, px.bsdf, px.inst, px.n};
    std::memcpy(albedo + 4 * lp, a4, sizeof(a4));
    std::memcpy(geom + 4 * lp, g4, sizeof(g4));
    std::memcpy(ids + 4 * lp, i4, sizeof(i4));
  }
  return 0;
}
}
