// tests/emu/scatter_emu.cpp -- TEST HARNESS, NOT A PRODUCT PATH.
//
// The scattering-media side of the host emulation (include/gpuspectral_pt.h, "Scattering media").  It includes pt_emu.cpp textually
// -- scene, BVH, per-ray traversal -- and adds the render loop of media_emu.cpp around the product's
// shade_vertex<TEX, false, true, LSEL, EST, SCT = true>, dispatched as the library does: the <SCT> instantiation exactly when the
// scattering table holds a nonzero sigma_s, else the code of a context without one.  Light selection and estimator as
// estimator_emu.cpp has them (the table image behind the light records, the commit rule of the textbook mode).  Plus a log: per
// pixel which back faces its paths met, per sample how many medium events it had -- the decision restated with the product's own
// medium_event on a copy of the stream, outside shade_vertex.  And gsp_set_media_scattering's validation, and the device functions
// of pt_medium.h one at a time.  Built into tests/emu/libscatter_emu.so by the tests that use it (tests/scatter_util.py).
#include "pt_emu.cpp"

#include "../../gpuspectral_amd/csrc/pt_lightpick.h"
#include "../devfn/medium_bodies.h"

namespace {
// baked light records [+ pick table [+ trailing record]], back to back, 16-byte aligned: the layout of the table image
struct SctLightImage {
  std::vector<LightPickQuad> store;
  gsp_triangle_light* lights() { return (gsp_triangle_light*)store.data(); }
  SctLightImage(const gsp_triangle_light* raw, uint32_t n, bool power, bool textbook) {
    store.resize((size_t)n * (sizeof(gsp_triangle_light) / 16) + (power ? n : 0) + (power && textbook ? 1 : 0) + 1);
    if (n && raw) std::memcpy(lights(), raw, sizeof(gsp_triangle_light) * (size_t)n);
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

struct Tables {
  const gsp_medium* media;
  const gsp_medium_scatter* scatter;  // null: the code of a context without scattering
};

template <bool TEX, bool LSEL, bool EST>
void shade_sct(const Tables& t, const SceneView& S, const RenderConstsBase& rc, const PathState& p, const HitRec& hit, ShadeOut& out) {
  if (t.scatter) shade_vertex<TEX, false, true, LSEL, EST, true>(S, rc, p, hit, out, t.media, t.scatter);
  else if (t.media) shade_vertex<TEX, false, true, LSEL, EST>(S, rc, p, hit, out, t.media);
  else shade_vertex<TEX, false, false, LSEL, EST>(S, rc, p, hit, out);
}
template <bool TEX>
void shade_modes(bool power, bool est, const Tables& t, const SceneView& S, const RenderConstsBase& rc, const PathState& p, const HitRec& hit, ShadeOut& out) {
  if (power && est) shade_sct<TEX, true, true>(t, S, rc, p, hit, out);
  else if (power) shade_sct<TEX, true, false>(t, S, rc, p, hit, out);
  else if (est) shade_sct<TEX, false, true>(t, S, rc, p, hit, out);
  else shade_sct<TEX, false, false>(t, S, rc, p, hit, out);
}
}  // namespace

extern "C" {

// gsp_set_media_scattering's validation against a context of `have` media.  Returns 0, or 1 and the error text in err (cap bytes)
int scatter_emu_check(const gsp_medium_scatter* scatter, uint32_t n, uint32_t have, char* err, uint32_t cap) {
  const char* why = check_media_scattering(scatter, n, have);
  if (why && err && cap) {
    std::strncpy(err, why, cap - 1);
    err[cap - 1] = 0;
  }
  return why ? 1 : 0;
}

// ---- pt_medium.h, one function at a time, over n inputs: the bodies of tests/devfn/medium_bodies.h, which medium_devfn.hip runs on the GPU ----
void scatter_emu_sample_hg(uint64_t n, const float* d, const float* g, const float* u1, const float* u2, float* out4) {
  for (uint64_t i = 0; i < n; ++i) devfn::sample_hg1(i, d, g, u1, u2, out4);
}
void scatter_emu_hg_pdf(uint64_t n, const float* g, const float* cos_theta, float* pdf) {
  for (uint64_t i = 0; i < n; ++i) devfn::hg_pdf1(i, g, cos_theta, pdf);
}
void scatter_emu_medium_event(uint64_t n, const float* sigma_a, const float* sigma_s, const float* t, const float* u_c, const float* u_d,
                              const float* weight, float* out6) {
  for (uint64_t i = 0; i < n; ++i) devfn::medium_event1(i, sigma_a, sigma_s, t, u_c, u_d, weight, out6);
}

// media_emu_render with the context's scattering table (null or num_media entries), estimator and light selection mode.
// `lights` = the scene's light records as the caller gave them (read under GSP_LIGHTS_POWER only).
// counts (optional, 5) = {extension rays, shadow rays, shaded vertices, medium events, samples}
// back_hits (optional, one byte per pixel of the call, OR-ed into): bit 0 = some vertex of the pixel's paths lay on a back face of a
//   triangle that names a medium, bit 1 = ... of a medium whose sigma_s has a nonzero channel
// events (optional, one uint32 per pixel and sample of the call, pixel-major): the medium events of that sample's path while it
//   carried weight (a path that met a black surface goes on with weight 0 and adds nothing: its later events are not counted)
int scatter_emu_render(void* h, uint32_t width, uint32_t height, const uint32_t* pixel_ids, uint64_t num_pixels, const gsp_render_params* rp,
                       uint32_t estimator, uint32_t light_mode, const gsp_triangle_light* lights, const gsp_medium* media,
                       const gsp_medium_scatter* scatter, uint32_t num_media, float* accum, uint64_t* counts, uint8_t* back_hits, uint32_t* events) {
  Emu* e = (Emu*)h;
  if (light_mode != GSP_LIGHTS_UNIFORM && light_mode != GSP_LIGHTS_POWER) return 1;
  if (estimator != GSP_ESTIMATOR_REFERENCE && estimator != GSP_ESTIMATOR_TEXTBOOK) return 1;
  if (max_medium_number(e->instances.data(), e->instances.size()) > (media ? num_media : 0u)) return 4;  // "BSDF handle out of range"
  const bool med = media != nullptr && num_media != 0u;
  if (scatter && check_media_scattering(scatter, num_media, med ? num_media : 0u)) return 1;
  const bool power = light_mode == GSP_LIGHTS_POWER, est = estimator == GSP_ESTIMATOR_TEXTBOOK;
  const Tables tab{med ? media : nullptr, med && scatter && any_scattering(scatter, num_media) ? scatter : nullptr};
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
  SctLightImage img(lights, power ? e->view.num_lights : 0u, power, est);
  SceneView S = e->view;
  if (power) S.lights = img.lights();
  uint64_t n_ext = 0, n_sh = 0, n_vert = 0, n_events = 0, n_samples = 0;
  for (uint64_t lp = 0; lp < npix; ++lp) {
    const uint32_t gid = pixel_ids ? pixel_ids[lp] : (uint32_t)lp;
    q4 acc = mkq(accum[4 * lp], accum[4 * lp + 1], accum[4 * lp + 2], accum[4 * lp + 3]);
    for (uint32_t s = 0; s < rp->spp; ++s) {
      const uint32_t ts = rp->first_timestamp + s;
      PathState p;
      generate_path(rc, gid, ts, 0, p);
      q4 result = mkq(0, 0, 0, 0);
      bool alive = true;
      uint32_t path_events = 0;
      while (alive) {
        HitRec hit;
        uint32_t aux;
        trace1<false>(S, p.o, p.d, 0.0f, 1e10f, hit, aux);
        ++n_ext;
        if (hit.slot < 0 || e->sc.num_vertices == 0) {
          if (e->textured && S.tex.env_texels != nullptr) add_emitted(rc.clamp, miss_emitted(S, p), result);
          break;
        }
        {  // the log, read off the packet here, outside the product's vertex
          const q4 s0 = S.tri_shade[4ll * hit.slot];
          const uint32_t k = (f2u(s0.w) >> 19) & 0xfffu;
          if (k != 0u && dot(mk3(s0.x, s0.y, s0.z), -p.d) < 0.0f) {
            if (back_hits) back_hits[lp] |= 1u;
            const gsp_medium_scatter* sc = scatter && med ? scatter + (k - 1u) : nullptr;
            if (sc && (sc->sigma_s[0] != 0.0f || sc->sigma_s[1] != 0.0f || sc->sigma_s[2] != 0.0f)) {
              if (back_hits) back_hits[lp] |= 2u;
              uint32_t rng = p.seed;
              const float u_c = rand_uniform(rng);
              const float u_d = rand_uniform(rng);
              const gsp_medium* m = media + (k - 1u);
              const MediumEvent ev = medium_event(mk3(m->sigma_a[0], m->sigma_a[1], m->sigma_a[2]), mk3(sc->sigma_s[0], sc->sigma_s[1], sc->sigma_s[2]), hit.t,
                                                  u_c, u_d, p.weight);
              if (ev.scatter && ev.valid && (p.weight.x != 0.0f || p.weight.y != 0.0f || p.weight.z != 0.0f)) ++path_events;
            }
          }
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
      if (events) events[lp * rp->spp + s] = path_events;
      n_events += path_events;
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
    counts[3] = n_events;
    counts[4] = n_samples;
  }
  return 0;
}
}
