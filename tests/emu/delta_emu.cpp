// tests/emu/delta_emu.cpp -- TEST HARNESS, NOT A PRODUCT PATH.
//
// The delta-light side of the host emulation (include/gpuspectral_pt.h, "Delta lights").  It includes pt_emu.cpp textually -- scene,
// BVH, per-ray traversal -- and adds the render loop of scatter_emu.cpp around the product's shade_vertex, dispatched as the library
// does: a context that holds delta lights runs <TEX, false, MED = true, LSEL, EST, SCT = true, DLT = true> whatever its media (null
// tables without media, a scattering table of zeros where the media only absorb), one without runs what scatter_emu.cpp runs.  The
// light table is the library's image: baked triangle lights, the accepted delta records behind them, then the pick table and its
// trailing record, built by the product's pt_lightpick.h.  Plus gsp_set_delta_lights' validation and the device functions of
// pt_deltalight.h one at a time.  Built into tests/emu/libdelta_emu.so by the tests that use it (tests/delta_util.py).
#include "pt_emu.cpp"

#include "../../gpuspectral_amd/csrc/pt_lightpick.h"
#include "../devfn/delta_bodies.h"

namespace {
// baked triangle lights, delta records [+ pick table [+ trailing record]], back to back, 16-byte aligned: the layout of the table image
struct DltLightImage {
  std::vector<LightPickQuad> store;
  uint32_t n, nd;
  gsp_triangle_light* lights() { return (gsp_triangle_light*)store.data(); }
  gsp_light_pick* pick() { return (gsp_light_pick*)(lights() + n + nd); }
  DltLightImage(const gsp_triangle_light* raw, uint32_t n_, const gsp_delta_light* delta, uint32_t nd_, bool power, bool textbook) : n(n_), nd(nd_) {
    const uint32_t all = n + nd;
    store.resize((size_t)all * (sizeof(gsp_triangle_light) / 16) + (power ? all : 0) + (power && textbook ? 1 : 0) + 1);
    if (n && raw) std::memcpy(lights(), raw, sizeof(gsp_triangle_light) * (size_t)n);
    if (nd) std::memcpy(lights() + n, delta, sizeof(gsp_delta_light) * (size_t)nd);
    if (power && all) {
      build_light_pick(raw, n, delta, nd, pick());
      if (textbook) {
        const float inv = light_pick_inv_sum(raw, n, delta, nd);
        std::memcpy(pick() + all, &inv, sizeof(float));
      }
    }
    for (uint32_t i = 0; i < n; ++i) bake_light(lights()[i]);
  }
};

struct Tables {
  const gsp_medium* media;
  const gsp_medium_scatter* scatter;  // null: the code of a context without scattering (no delta lights), zeros with them
  bool delta;
  uint32_t num_tri_lights;
  bool narrow;  // (delta only) not the library's dispatch: the <DLT> instantiation of the context's own media class, which the library does not build
  bool any_sct;
};

template <bool TEX, bool LSEL, bool EST>
void shade_dlt(const Tables& t, const SceneView& S, const RenderConstsBase& rc, const PathState& p, const HitRec& hit, ShadeOut& out) {
  if (t.delta && t.narrow && !t.media) shade_vertex<TEX, false, false, LSEL, EST, false, true>(S, rc, p, hit, out, nullptr, nullptr, t.num_tri_lights);
  else if (t.delta && t.narrow && !t.any_sct) shade_vertex<TEX, false, true, LSEL, EST, false, true>(S, rc, p, hit, out, t.media, nullptr, t.num_tri_lights);
  else if (t.delta) shade_vertex<TEX, false, true, LSEL, EST, true, true>(S, rc, p, hit, out, t.media, t.scatter, t.num_tri_lights);
  else if (t.scatter) shade_vertex<TEX, false, true, LSEL, EST, true>(S, rc, p, hit, out, t.media, t.scatter);
  else if (t.media) shade_vertex<TEX, false, true, LSEL, EST>(S, rc, p, hit, out, t.media);
  else shade_vertex<TEX, false, false, LSEL, EST>(S, rc, p, hit, out);
}
template <bool TEX>
void shade_modes(bool power, bool est, const Tables& t, const SceneView& S, const RenderConstsBase& rc, const PathState& p, const HitRec& hit, ShadeOut& out) {
  if (power && est) shade_dlt<TEX, true, true>(t, S, rc, p, hit, out);
  else if (power) shade_dlt<TEX, true, false>(t, S, rc, p, hit, out);
  else if (est) shade_dlt<TEX, false, true>(t, S, rc, p, hit, out);
  else shade_dlt<TEX, false, false>(t, S, rc, p, hit, out);
}
}  // namespace

extern "C" {

// gsp_set_delta_lights' validation.  Returns 0 and the accepted records in `accepted` (n of them; may be null), or 1 and the error
// text in err (cap bytes)
int delta_emu_check(const gsp_delta_light* lights, uint32_t n, gsp_delta_light* accepted, char* err, uint32_t cap) {
  const char* why = check_delta_lights(lights, n);
  if (why && err && cap) {
    std::strncpy(err, why, cap - 1);
    err[cap - 1] = 0;
  }
  if (!why && accepted && lights)
    for (uint32_t k = 0; k < n; ++k) accepted[k] = accept_delta_light(lights[k]);
  return why ? 1 : 0;
}

// ---- pt_deltalight.h, one function at a time, over n inputs: the bodies of tests/devfn/delta_bodies.h, which delta_devfn.hip runs on the GPU ----
void delta_emu_spot_falloff(uint64_t n, const float* c, const float* cos_cutoff, const float* cos_beam, float* out) {
  for (uint64_t i = 0; i < n; ++i) devfn::spot_falloff1(i, c, cos_cutoff, cos_beam, out);
}
void delta_emu_sample_delta_light(uint64_t n, const float* rec16, const float* pos, const float* pmf, float* out8) {
  for (uint64_t i = 0; i < n; ++i) devfn::sample_delta_light1(i, rec16, pos, pmf, out8);
}

// the pick table of GSP_LIGHTS_POWER over n triangle lights and nd ACCEPTED delta records: n + nd entries into `out`, 1 / sum(w) into *inv_sum
void delta_emu_light_pick(const gsp_triangle_light* lights, uint32_t n, const gsp_delta_light* delta, uint32_t nd, gsp_light_pick* out, float* inv_sum) {
  build_light_pick(lights, n, delta, nd, out);
  if (inv_sum) *inv_sum = light_pick_inv_sum(lights, n, delta, nd);
}

// scatter_emu_render with the context's delta-light table (`delta`: nd records as the CALLER gives them; validated and accepted here).
// counts (optional, 4) = {extension rays, shadow rays, shaded vertices, samples}
// narrow != 0: with delta lights, run the <DLT> instantiation of the context's own media class (none / absorbing only) where the library runs
//   the <MED, SCT, DLT> one: the two must agree bit for bit
// per_sample (optional, 4 floats per pixel and sample of the call, pixel-major): the sample's own value before the running mean
int delta_emu_render(void* h, uint32_t width, uint32_t height, const uint32_t* pixel_ids, uint64_t num_pixels, const gsp_render_params* rp,
                     uint32_t estimator, uint32_t light_mode, const gsp_triangle_light* lights, const gsp_delta_light* delta, uint32_t nd,
                     const gsp_medium* media, const gsp_medium_scatter* scatter, uint32_t num_media, float* accum, uint64_t* counts, float* per_sample, uint32_t narrow) {
  Emu* e = (Emu*)h;
  if (light_mode != GSP_LIGHTS_UNIFORM && light_mode != GSP_LIGHTS_POWER) return 1;
  if (estimator != GSP_ESTIMATOR_REFERENCE && estimator != GSP_ESTIMATOR_TEXTBOOK) return 1;
  if (max_medium_number(e->instances.data(), e->instances.size()) > (media ? num_media : 0u)) return 4;  // "BSDF handle out of range"
  const bool med = media != nullptr && num_media != 0u;
  if (scatter && check_media_scattering(scatter, num_media, med ? num_media : 0u)) return 1;
  if (check_delta_lights(delta, nd)) return 1;
  std::vector<gsp_delta_light> acc_d(delta ? nd : 0u);
  for (size_t k = 0; k < acc_d.size(); ++k) acc_d[k] = accept_delta_light(delta[k]);
  const bool power = light_mode == GSP_LIGHTS_POWER, est = estimator == GSP_ESTIMATOR_TEXTBOOK, dlt = !acc_d.empty();
  const std::vector<gsp_medium_scatter> zeros(med ? num_media : 0u, gsp_medium_scatter{{0.0f, 0.0f, 0.0f}, 0.0f});
  Tables tab{med ? media : nullptr, med && scatter && any_scattering(scatter, num_media) ? scatter : nullptr, dlt, e->view.num_lights, narrow != 0u,
             med && scatter && any_scattering(scatter, num_media)};
  if (dlt && med && !scatter) tab.scatter = zeros.data();
  else if (dlt && med) tab.scatter = scatter;
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
  DltLightImage img(lights, (power || dlt) ? e->view.num_lights : 0u, acc_d.data(), (uint32_t)acc_d.size(), power, est);
  SceneView S = e->view;
  if (power || dlt) {
    S.lights = img.lights();
    S.num_lights = e->view.num_lights + (uint32_t)acc_d.size();
    S.inv_num_lights = S.num_lights ? 1.0f / (float)S.num_lights : 0.0f;
  }
  uint64_t n_ext = 0, n_sh = 0, n_vert = 0, n_samples = 0;
  for (uint64_t lp = 0; lp < npix; ++lp) {
    const uint32_t gid = pixel_ids ? pixel_ids[lp] : (uint32_t)lp;
    q4 acc = mkq(accum[4 * lp], accum[4 * lp + 1], accum[4 * lp + 2], accum[4 * lp + 3]);
    for (uint32_t s = 0; s < rp->spp; ++s) {
      const uint32_t ts = rp->first_timestamp + s;
      PathState p;
      generate_path(rc, gid, ts, 0, p);
      q4 result = mkq(0, 0, 0, 0);
      bool alive = true;
      while (alive) {
        HitRec hit;
        uint32_t aux;
        trace1<false>(S, p.o, p.d, 0.0f, 1e10f, hit, aux);
        ++n_ext;
        if (hit.slot < 0 || e->sc.num_vertices == 0) {
          if (e->textured && S.tex.env_texels != nullptr) add_emitted(rc.clamp, miss_emitted(S, p), result);
          break;
        }
        ShadeOut out;
        if (e->textured) shade_modes<true>(power, est, tab, S, rc, p, hit, out);
        else shade_modes<false>(power, est, tab, S, rc, p, hit, out);
        ++n_vert;
        if (out.has_shadow) {
          HitRec sh;
          uint32_t aux2;
          const bool occ = trace1<true>(S, out.shadow.o, out.shadow.d, 0.01f, out.shadow.tmax, sh, aux2);
          ++n_sh;
          bool nee_done;
          connect_vertex(rc.clamp, out.shadow, occ, result, nee_done);
          if (!est && nee_done && out.alive) out.next.directWeight = out.shadow.dw_nee;
        } else {
          add_emitted(rc.clamp, out.emitted, result);
        }
        alive = out.alive;
        p = out.next;
      }
      if (per_sample) {
        float* o = per_sample + 4 * (lp * rp->spp + s);
        o[0] = result.x, o[1] = result.y, o[2] = result.z, o[3] = result.w;
      }
      ++n_samples;
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
    counts[3] = n_samples;
  }
  return 0;
}
}
