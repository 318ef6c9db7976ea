// tests/emu/envlight_emu.cpp -- TEST HARNESS, NOT A PRODUCT PATH.
//
// The environment-light side of the host emulation (include/gpuspectral_pt.h, "Environment light").  It includes pt_emu.cpp
// textually -- scene, BVH, per-ray traversal -- and adds the render loop of delta_emu.cpp around the product's shade_vertex and
// miss_emitted_env, dispatched as the library does: a context whose switch is on under a scene with an envmap runs
// <TEX = true, false, MED = true, LSEL, EST = true, SCT = true, DLT = true, ENV = true> whatever its media and delta lights, every
// other context what delta_emu.cpp runs.  The light table is the library's image -- baked triangle lights, the accepted delta
// records, the environment record, then the pick table and its trailing record -- and the cell table the library's, both built by
// the product's pt_lightpick.h / pt_envlight.h.  Plus gsp_set_envmap_sampling's validation and the device functions of
// pt_envlight.h one at a time.  Built into tests/emu/libenvlight_emu.so by the tests that use it (tests/envlight_util.py).
#include "pt_emu.cpp"

#include "../../gpuspectral_amd/csrc/pt_lightpick.h"
#include "../devfn/envlight_bodies.h"

namespace {
// baked triangle lights, delta records, [environment record], [pick table [+ trailing record]], back to back, 16-byte aligned
struct EnvLightImage {
  std::vector<LightPickQuad> store;
  uint32_t n, nd, ne;
  gsp_triangle_light* lights() { return (gsp_triangle_light*)store.data(); }
  gsp_light_pick* pick() { return (gsp_light_pick*)(lights() + n + nd + ne); }
  EnvLightImage(const gsp_triangle_light* raw, uint32_t n_, const gsp_delta_light* delta, uint32_t nd_, const double* env_w, const float* to_local, uint32_t cw,
                uint32_t ch, bool power, bool textbook)
      : n(n_), nd(nd_), ne(env_w ? 1u : 0u) {
    const uint32_t all = n + nd + ne;
    store.resize((size_t)all * (sizeof(gsp_triangle_light) / 16) + (power ? all : 0) + (power && textbook ? 1 : 0) + 1);
    if (n && raw) std::memcpy(lights(), raw, sizeof(gsp_triangle_light) * (size_t)n);
    if (nd) std::memcpy(lights() + n, delta, sizeof(gsp_delta_light) * (size_t)nd);
    if (power && all) {
      build_light_pick(raw, n, delta, nd, pick(), env_w);
      if (textbook) {
        const float inv = light_pick_inv_sum(raw, n, delta, nd, env_w);
        std::memcpy(pick() + all, &inv, sizeof(float));
      }
    }
    if (ne) {
      const float p_sel = power ? pick()[all - 1u].pmf_self : 1.0f / (float)all;
      const EnvLightRecord rec = make_env_record(to_local, cw, ch, p_sel);
      std::memcpy(lights() + n + nd, &rec, sizeof(rec));
    }
    for (uint32_t i = 0; i < n; ++i) bake_light(lights()[i]);
  }
};

struct Tables {
  const gsp_medium* media;
  const gsp_medium_scatter* scatter;  // null: the code of a context without scattering (no delta lights, no environment light), zeros with them
  bool delta, env;
  uint32_t num_tri_lights;
  const gsp_light_pick* env_cells;
};

template <bool TEX, bool LSEL, bool EST>
void shade_env(const Tables& t, const SceneView& S, const RenderConstsBase& rc, const PathState& p, const HitRec& hit, ShadeOut& out) {
  if constexpr (TEX && EST) {
    if (t.env) {
      shade_vertex<true, false, true, LSEL, true, true, true, true>(S, rc, p, hit, out, t.media, t.scatter, t.num_tri_lights, t.env_cells);
      return;
    }
  }
  if (t.delta) shade_vertex<TEX, false, true, LSEL, EST, true, true>(S, rc, p, hit, out, t.media, t.scatter, t.num_tri_lights);
  else if (t.scatter) shade_vertex<TEX, false, true, LSEL, EST, true>(S, rc, p, hit, out, t.media, t.scatter);
  else if (t.media) shade_vertex<TEX, false, true, LSEL, EST>(S, rc, p, hit, out, t.media);
  else shade_vertex<TEX, false, false, LSEL, EST>(S, rc, p, hit, out);
}
template <bool TEX>
void shade_modes(bool power, bool est, const Tables& t, const SceneView& S, const RenderConstsBase& rc, const PathState& p, const HitRec& hit, ShadeOut& out) {
  if (power && est) shade_env<TEX, true, true>(t, S, rc, p, hit, out);
  else if (power) shade_env<TEX, true, false>(t, S, rc, p, hit, out);
  else if (est) shade_env<TEX, false, true>(t, S, rc, p, hit, out);
  else shade_env<TEX, false, false>(t, S, rc, p, hit, out);
}

TextureView map_view(const float* texels, uint32_t width, uint32_t height, const float* to_local) {
  TextureView T;
  T.env_texels = texels;
  T.env_width = width;
  T.env_height = height;
  for (int k = 0; k < 16; ++k) T.env_to_local[k] = to_local[k];
  return T;
}
}  // namespace

extern "C" {

// gsp_set_envmap_sampling's own validation: 0 = acceptable, 1 and the text in err otherwise
int envlight_emu_check(const gsp_envmap_sampling* s, char* err, uint32_t cap) {
  const char* why = check_envmap_sampling(s);
  if (why && err && cap) {
    std::strncpy(err, why, cap - 1);
    err[cap - 1] = 0;
  }
  return why ? 1 : 0;
}
int envlight_emu_is_rotation(const float* to_local) { return env_frame_is_rotation(to_local) ? 1 : 0; }

// The cell table of a map: dims[2] = {cw, ch}; cells (cw * ch entries; may be null to ask for the size) and weights (optional, cw * ch doubles)
void envlight_emu_cells(const float* texels, uint32_t width, uint32_t height, uint32_t* dims, gsp_light_pick* cells, double* weights) {
  uint32_t cw, ch;
  const std::vector<double> w = env_cell_weights(texels, width, height, cw, ch);
  dims[0] = cw;
  dims[1] = ch;
  if (cells) build_light_pick_from_weights(w.data(), (uint32_t)w.size(), cells);
  if (weights) std::memcpy(weights, w.data(), sizeof(double) * w.size());
}
// the power-pick weight of the record
double envlight_emu_power_weight(const float* texels, uint32_t width, uint32_t height, float extent) {
  return env_power_weight(env_radiant_sum(texels, width, height), extent);
}
// the record (16 words) for a frame, a cell grid and a p_sel
void envlight_emu_record(const float* to_local, uint32_t cw, uint32_t ch, float p_sel, float* rec16) {
  const EnvLightRecord rec = make_env_record(to_local, cw, ch, p_sel);
  std::memcpy(rec16, &rec, sizeof(rec));
}
// the light table's pick entries (n + nd + 1 of them) and the record's p_sel, as the library packs them
void envlight_emu_light_pick(const gsp_triangle_light* lights, uint32_t n, const gsp_delta_light* delta, uint32_t nd, double env_w, gsp_light_pick* out) {
  build_light_pick(lights, n, delta, nd, out, &env_w);
}

// ---- pt_envlight.h, one function at a time, over n inputs: the bodies of tests/devfn/envlight_bodies.h, which envlight_devfn.hip runs on the GPU ----
int envlight_emu_env_eval(uint64_t n, const float* texels, uint32_t width, uint32_t height, const float* to_local, const gsp_light_pick* cells, const float* rec16,
                          const float* dirs, float* out5) {
  const TextureView T = map_view(texels, width, height, to_local);
  for (uint64_t i = 0; i < n; ++i) devfn::env_eval1(i, T, cells, rec16, dirs, out5);
  return 0;
}
int envlight_emu_sample_env_light(uint64_t n, const float* texels, uint32_t width, uint32_t height, const float* to_local, const gsp_light_pick* cells, const float* rec16,
                                  const float* draws3, float* out9) {
  const TextureView T = map_view(texels, width, height, to_local);
  for (uint64_t i = 0; i < n; ++i) devfn::sample_env_light1(i, T, cells, rec16, draws3, out9);
  return 0;
}

// delta_emu_render with the context's environment switch (`env`: null or enabled == 0 = off).  Return codes: 1 = a call of the
// library would have returned GSP_ERR_INVALID (the switch under the reference estimator included), 2 = the frame is not a rotation.
// counts (optional, 4) = {extension rays, shadow rays, shaded vertices, samples}
int envlight_emu_render(void* h, uint32_t width, uint32_t height, const gsp_render_params* rp, uint32_t estimator, uint32_t light_mode,
                        const gsp_triangle_light* lights, const gsp_delta_light* delta, uint32_t nd, const gsp_medium* media, const gsp_medium_scatter* scatter,
                        uint32_t num_media, const gsp_envmap_sampling* env, float* accum, uint64_t* counts) {
  Emu* e = (Emu*)h;
  if (light_mode != GSP_LIGHTS_UNIFORM && light_mode != GSP_LIGHTS_POWER) return 1;
  if (estimator != GSP_ESTIMATOR_REFERENCE && estimator != GSP_ESTIMATOR_TEXTBOOK) return 1;
  if (max_medium_number(e->instances.data(), e->instances.size()) > (media ? num_media : 0u)) return 4;  // "BSDF handle out of range"
  const bool med = media != nullptr && num_media != 0u;
  if (scatter && check_media_scattering(scatter, num_media, med ? num_media : 0u)) return 1;
  if (check_delta_lights(delta, nd)) return 1;
  if (check_envmap_sampling(env)) return 1;
  const bool env_switch = env != nullptr && env->enabled != 0u;
  if (env_switch && estimator != GSP_ESTIMATOR_TEXTBOOK) return 1;
  const bool env_on = env_switch && e->textured && e->view.tex.env_texels != nullptr;
  if (env_on && !env_frame_is_rotation(e->view.tex.env_to_local)) return 2;
  std::vector<gsp_delta_light> acc_d(delta ? nd : 0u);
  for (size_t k = 0; k < acc_d.size(); ++k) acc_d[k] = accept_delta_light(delta[k]);
  const bool power = light_mode == GSP_LIGHTS_POWER, est = estimator == GSP_ESTIMATOR_TEXTBOOK, dlt = !acc_d.empty();
  const std::vector<gsp_medium_scatter> zeros(med ? num_media : 0u, gsp_medium_scatter{{0.0f, 0.0f, 0.0f}, 0.0f});
  Tables tab{med ? media : nullptr, med && scatter && any_scattering(scatter, num_media) ? scatter : nullptr, dlt, env_on, e->view.num_lights, nullptr};
  if ((dlt || env_on) && med && !scatter) tab.scatter = zeros.data();
  else if ((dlt || env_on) && med) tab.scatter = scatter;
  // the environment light's scene state
  std::vector<gsp_light_pick> cells;
  uint32_t cw = 0, ch = 0;
  double env_w = 0.0;
  if (env_on) {
    const std::vector<double> w = env_cell_weights(e->view.tex.env_texels, e->view.tex.env_width, e->view.tex.env_height, cw, ch);
    cells.assign(w.size(), gsp_light_pick{});
    build_light_pick_from_weights(w.data(), (uint32_t)w.size(), cells.data());
    env_w = env_power_weight(env_radiant_sum(e->view.tex.env_texels, e->view.tex.env_width, e->view.tex.env_height), env->extent);
    tab.env_cells = cells.data();
  }
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
  const uint64_t npix = (uint64_t)width * height;
  const bool image = power || dlt || env_on;
  EnvLightImage img(lights, image ? e->view.num_lights : 0u, acc_d.data(), (uint32_t)acc_d.size(), env_on ? &env_w : nullptr, e->view.tex.env_to_local, cw, ch, power, est);
  SceneView S = e->view;
  if (image) {
    S.lights = img.lights();
    S.num_lights = e->view.num_lights + (uint32_t)acc_d.size() + (env_on ? 1u : 0u);
    S.inv_num_lights = S.num_lights ? 1.0f / (float)S.num_lights : 0.0f;
  }
  uint64_t n_ext = 0, n_sh = 0, n_vert = 0, n_samples = 0;
  for (uint64_t lp = 0; lp < npix; ++lp) {
    const uint32_t gid = (uint32_t)lp;
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
          if (env_on) add_emitted(rc.clamp, miss_emitted_env<false>(S, rc, p, tab.env_cells), result);
          else if (e->textured && S.tex.env_texels != nullptr) add_emitted(rc.clamp, miss_emitted(S, p), result);
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
