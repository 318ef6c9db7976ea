// tests/emu/estimator_emu.cpp -- TEST HARNESS, NOT A PRODUCT PATH.
//
// The estimator side of the host emulation (include/gpuspectral_pt.h, "Estimator").  It includes pt_emu.cpp textually -- scene,
// BVH, per-ray traversal -- and adds a render loop that is emu_render's around the product's shade_vertex<TEX, false, MED, LSEL, EST>,
// with the table image of the context's two modes behind the light records (the alias table under GSP_LIGHTS_POWER, and behind it
// the trailing record with 1 / sum(w) when GSP_ESTIMATOR_TEXTBOOK is on too), and with the commit rule of the mode: in textbook mode
// the verdict of the shadow ray does not touch the continuing path's directWeight field (it carries lastPdf), as k_finish<.., EST>
// and the textbook any-hit sources of k_trace have it.  Also: the product's selection probability of a light that was hit
// (light_hit_select_pmf over light_pick_inv_sum) for chosen records.  Built into tests/emu/libestimator_emu.so by the tests that
// use it (tests/estimator_util.py).
#include "pt_emu.cpp"

#include "../../gpuspectral_amd/csrc/pt_lightpick.h"

namespace {
// baked light records [+ pick table [+ trailing record]], back to back, 16-byte aligned: the layout of the table image
struct EstLightImage {
  std::vector<LightPickQuad> store;  // (alignas(16) elements: the allocation is aligned)
  gsp_triangle_light* lights() { return (gsp_triangle_light*)store.data(); }
  EstLightImage(const gsp_triangle_light* raw, uint32_t n, bool power, bool textbook) {
    static_assert(sizeof(gsp_triangle_light) % 16 == 0 && sizeof(LightPickQuad) == 16 && sizeof(gsp_light_pick) == 16, "layout");
    store.resize((size_t)n * (sizeof(gsp_triangle_light) / 16) + (power ? n : 0) + (power && textbook ? 1 : 0) + 1);
    if (n) std::memcpy(lights(), raw, sizeof(gsp_triangle_light) * (size_t)n);
    if (power && n) {
      gsp_light_pick* pick = (gsp_light_pick*)(lights() + n);
      build_light_pick(raw, n, pick);
      if (textbook) {
        const float inv = light_pick_inv_sum(raw, n);
        std::memcpy(pick + n, &inv, sizeof(float));
      }
    }
    for (uint32_t i = 0; i < n; ++i) bake_light(lights()[i]);
  }
};

template <bool TEX, bool MED, bool LSEL>
void shade_est(bool est, const SceneView& S, const RenderConstsBase& rc, const PathState& p, const HitRec& hit, ShadeOut& out, const gsp_medium* media) {
  if (est) shade_vertex<TEX, false, MED, LSEL, true>(S, rc, p, hit, out, media);
  else shade_vertex<TEX, false, MED, LSEL, false>(S, rc, p, hit, out, media);
}
template <bool TEX, bool MED>
void shade_lsel(bool power, bool est, const SceneView& S, const RenderConstsBase& rc, const PathState& p, const HitRec& hit, ShadeOut& out, const gsp_medium* media) {
  if (power) shade_est<TEX, MED, true>(est, S, rc, p, hit, out, media);
  else shade_est<TEX, MED, false>(est, S, rc, p, hit, out, media);
}
void shade_any(bool tex, bool med, bool power, bool est, const SceneView& S, const RenderConstsBase& rc, const PathState& p, const HitRec& hit, ShadeOut& out,
               const gsp_medium* media) {
  if (tex && med) shade_lsel<true, true>(power, est, S, rc, p, hit, out, media);
  else if (tex) shade_lsel<true, false>(power, est, S, rc, p, hit, out, media);
  else if (med) shade_lsel<false, true>(power, est, S, rc, p, hit, out, media);
  else shade_lsel<false, false>(power, est, S, rc, p, hit, out, media);
}
}  // namespace

extern "C" {

// the product's p_sel for light records hit as themselves: out[i] = light_hit_select_pmf(radiance_i, A_i, inv_sum_w, 1 / n) with A_i
// the float32 area of the record's vertices (light_hit_area) and inv_sum_w = light_pick_inv_sum(lights, n) (returned through *inv)
void estimator_emu_psel(const gsp_triangle_light* lights, uint32_t n, float* out, float* inv) {
  const float inv_sum_w = light_pick_inv_sum(lights, n);
  if (inv) *inv = inv_sum_w;
  for (uint32_t i = 0; i < n; ++i) {
    const f3 v0 = ld3(lights[i].positions[0]), v1 = ld3(lights[i].positions[1]), v2 = ld3(lights[i].positions[2]);
    out[i] = light_hit_select_pmf(ld3(lights[i].radiance), light_hit_area(v0, v1, v2), inv_sum_w, 1.0f / (float)n);
  }
}
// ... and the weight such a hit gets: power_heuristic(lastPdf, light_hit_pdf(t, d, N, A, p_sel))
float estimator_emu_hit_weight(float lastPdf, float t, const float* d, const float* N, float A, float p_sel) {
  return power_heuristic(lastPdf, light_hit_pdf(t, mk3(d[0], d[1], d[2]), mk3(N[0], N[1], N[2]), A, p_sel));
}
// bytes of light records + what follows them in the table image of a context in these two modes
uint64_t estimator_emu_light_image_bytes(uint32_t n, uint32_t light_mode, uint32_t estimator) {
  return sizeof(gsp_triangle_light) * (uint64_t)n + light_pick_table_bytes(n, light_mode) + light_pick_tail_bytes(n, light_mode, estimator);
}

// emu_render with the context's estimator, light selection mode and (optionally) media, dispatched as tex_ver_med_kernel
// (pt_render_pipeline.inc) does.  `lights` = the scene's light records as the caller gave them (the tables are built from those).
// counts (optional, 6) = {extension rays, shadow rays, shaded vertices, paths with an OCCLUDED shadow ray at vertex k that hit an emitter at
//   vertex k + 1 with NEE on, countEmitted == 0 and wasDelta == 0, such hits after an unoccluded shadow ray, emitter hits after a delta bounce}
// moments (optional, 6 doubles per pixel, added to) = per pixel sum and sum of squares of the samples' r, g, b
int estimator_emu_render(void* h, uint32_t width, uint32_t height, const uint32_t* pixel_ids, uint64_t num_pixels, const gsp_render_params* rp,
                         uint32_t estimator, uint32_t light_mode, const gsp_triangle_light* lights, const gsp_medium* media, uint32_t num_media,
                         float* accum, uint64_t* counts, double* moments) {
  Emu* e = (Emu*)h;
  if (light_mode != GSP_LIGHTS_UNIFORM && light_mode != GSP_LIGHTS_POWER) return 1;
  if (estimator != GSP_ESTIMATOR_REFERENCE && estimator != GSP_ESTIMATOR_TEXTBOOK) return 1;
  if (max_medium_number(e->instances.data(), e->instances.size()) > (media ? num_media : 0u)) return 4;
  const bool med = media != nullptr && num_media != 0u;
  const bool power = light_mode == GSP_LIGHTS_POWER;
  const bool est = estimator == GSP_ESTIMATOR_TEXTBOOK;
  RenderConsts rc;
  rc.width = width;
  rc.height = height;
  rc.max_depth = rp->max_depth;
  rc.rr_start_depth = rp->rr_start_depth;
  rc.clamp = rp->clamp;
  rc.nee = rp->disable_nee != 0 ? 0u : 1u;
  rc.zplane = (std::max((float)width, (float)height) / 2.0f) / tanf(e->sc.camera.fov / 2.0f);
  for (int i = 0; i < 16; ++i) rc.cam_to_world[i] = e->sc.camera.to_world[i];
  for (int i = 0; i < 3; ++i) rc.cam_origin[i] = e->sc.camera.to_world[12 + i];
  const uint64_t npix = pixel_ids ? num_pixels : (uint64_t)width * height;
  EstLightImage img(lights, e->view.num_lights, power, est);
  SceneView S = e->view;
  if (power) S.lights = img.lights();
  uint64_t n_ext = 0, n_sh = 0, n_vert = 0, n_occ_emit = 0, n_clear_emit = 0, n_delta_emit = 0;
  for (uint64_t lp = 0; lp < npix; ++lp) {
    const uint32_t gid = pixel_ids ? pixel_ids[lp] : (uint32_t)lp;
    q4 acc = mkq(accum[4 * lp], accum[4 * lp + 1], accum[4 * lp + 2], accum[4 * lp + 3]);
    for (uint32_t s = 0; s < rp->spp; ++s) {
      const uint32_t ts = rp->first_timestamp + s;
      PathState p;
      generate_path(rc, gid, ts, 0, p);
      q4 result = mkq(0, 0, 0, 0);
      bool alive = true;
      int prev_shadow = 0;  // the vertex that sent this ray: 0 = traced no shadow ray, 1 = unoccluded, 2 = occluded
      while (alive) {
        HitRec hit;
        uint32_t aux;
        trace1<false>(S, p.o, p.d, 0.0f, 1e10f, hit, aux);
        ++n_ext;
        if (hit.slot < 0 || e->sc.num_vertices == 0) {
          if (e->textured && S.tex.env_texels != nullptr) add_emitted(rc.clamp, miss_emitted(S, p), result);
          break;
        }
        {  // the path log: what kind of emitter hit is this?
          const q4* sp = S.tri_shade + 4ll * hit.slot;
          const bool emitter = sp[1].w != 0.0f || sp[2].w != 0.0f || sp[3].w != 0.0f;
          const uint32_t wasDelta = (p.flags >> 8) & 1u, countEmitted = (p.flags >> 9) & 1u;
          if (emitter && rc.nee != 0u && countEmitted == 0u) {
            if (wasDelta) ++n_delta_emit;
            else if (prev_shadow == 2) ++n_occ_emit;
            else if (prev_shadow == 1) ++n_clear_emit;
          }
        }
        ShadeOut out;
        shade_any(e->textured, med, power, est, S, rc, p, hit, out, media);
        ++n_vert;
        prev_shadow = 0;
        if (out.has_shadow) {
          HitRec sh;
          uint32_t aux2;
          const bool occ = trace1<true>(S, out.shadow.o, out.shadow.d, 0.01f, out.shadow.tmax, sh, aux2);
          ++n_sh;
          prev_shadow = occ ? 2 : 1;
          bool nee_done;
          connect_vertex(rc.clamp, out.shadow, occ, result, nee_done);
          // the commit: the reference's directWeight follows the verdict (rayhit.rchit:785-790); lastPdf does not
          if (!est && nee_done && out.alive) out.next.directWeight = out.shadow.dw_nee;
        } else {
          add_emitted(rc.clamp, out.emitted, result);
        }
        alive = out.alive;
        p = out.next;
      }
      if (moments) {
        double* m = moments + 6 * lp;
        m[0] += result.x, m[1] += result.y, m[2] += result.z;
        m[3] += (double)result.x * result.x, m[4] += (double)result.y * result.y, m[5] += (double)result.z * result.z;
      }
      resolve_sample(ts, result, acc);
    }
    accum[4 * lp] = acc.x;
    accum[4 * lp + 1] = acc.y;
    accum[4 * lp + 2] = acc.z;
    accum[4 * lp + 3] = acc.w;
  }
  if (counts) {
    counts[0] = n_ext;
    counts[1] = n_sh;
    counts[2] = n_vert;
    counts[3] = n_occ_emit;
    counts[4] = n_clear_emit;
    counts[5] = n_delta_emit;
  }
  return 0;
}
}
