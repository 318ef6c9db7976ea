// tests/emu/lightgrid_emu.cpp -- TEST HARNESS, NOT A PRODUCT PATH.
//
// The light-grid side of the host emulation (include/gpuspectral_pt.h, "Light grid").  It includes pt_emu.cpp textually -- scene,
// BVH, per-ray traversal -- and adds the render loop of delta_emu.cpp around the product's shade_vertex, dispatched as the library
// does: a context with a grid resident (the switch on under GSP_LIGHTS_POWER and GSP_ESTIMATOR_TEXTBOOK, a scene with lights) runs
// <TEX = true, false, MED = true, LSEL = true, EST = true, SCT = true, DLT = true, ENV = false, GRD = true> whatever its textures,
// media and delta lights, every other context what delta_emu.cpp runs.  The table image is the library's -- baked triangle lights,
// the accepted delta records, the pick table, its trailing record, the grid -- built by the product's pt_lightpick.h /
// pt_lightgrid.h.  Plus gsp_set_light_grid's validation, the builder on its own and the device functions of pt_lightgrid.h one at
// a time.  Built into tests/emu/liblightgrid_emu.so by the tests that use it (tests/lightgrid_util.py).
#include "pt_emu.cpp"

#include <chrono>

#include "../../gpuspectral_amd/csrc/pt_lightgrid.h"
#include "../../gpuspectral_amd/csrc/pt_lightpick.h"
#include "../devfn/lightgrid_bodies.h"

namespace {
// [baked triangle lights][delta records][pick table][tail][grid], 16-byte aligned: what pack_tables leaves behind the BSDF tables
struct GridImage {
  std::vector<LightPickQuad> store;
  uint32_t n, nd;
  size_t grid_off = 0;  // bytes from lights(); 0 = no grid
  uint8_t* base() { return (uint8_t*)store.data(); }
  gsp_triangle_light* lights() { return (gsp_triangle_light*)store.data(); }
  gsp_light_pick* pick() { return (gsp_light_pick*)(lights() + n + nd); }
  GridImage(const gsp_triangle_light* raw, uint32_t n_, const gsp_delta_light* delta, uint32_t nd_, bool power, bool textbook, const LightGridHeader* g)
      : n(n_), nd(nd_) {
    const uint32_t all = n + nd;
    size_t bytes = (size_t)all * sizeof(gsp_triangle_light) + (power ? (size_t)all * 16 : 0) + (power && textbook ? 16 : 0);
    if (g) grid_off = bytes, bytes += lightgrid_bytes(g->nx, g->ny, g->nz, all);
    store.assign(bytes / 16 + 1, LightPickQuad{});
    if (n && raw) std::memcpy(lights(), raw, sizeof(gsp_triangle_light) * (size_t)n);
    if (nd) std::memcpy(lights() + n, delta, sizeof(gsp_delta_light) * (size_t)nd);
    if (power && all) {
      build_light_pick(raw, n, delta, nd, pick());
      if (textbook) {
        const float inv = light_pick_inv_sum(raw, n, delta, nd);
        std::memcpy(pick() + all, &inv, sizeof(float));
      }
    }
    if (g) build_light_grid(*g, raw, n, delta, nd, pick(), base() + grid_off);
    for (uint32_t i = 0; i < n; ++i) bake_light(lights()[i]);
  }
};

struct Tables {
  const gsp_medium* media;
  const gsp_medium_scatter* scatter;
  bool delta, grid;
  uint32_t num_tri_lights;
  uint32_t grid_off;
};

template <bool TEX, bool LSEL, bool EST>
void shade_grid(const Tables& t, const SceneView& S, const RenderConstsBase& rc, const PathState& p, const HitRec& hit, ShadeOut& out) {
  if constexpr (LSEL && EST) {
    if (t.grid) {
      shade_vertex<true, false, true, true, true, true, true, false, true>(S, rc, p, hit, out, t.media, t.scatter, t.num_tri_lights, nullptr, t.grid_off);
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
  if (power && est) shade_grid<TEX, true, true>(t, S, rc, p, hit, out);
  else if (power) shade_grid<TEX, true, false>(t, S, rc, p, hit, out);
  else if (est) shade_grid<TEX, false, true>(t, S, rc, p, hit, out);
  else shade_grid<TEX, false, false>(t, S, rc, p, hit, out);
}

gsp_scene_desc desc_of(Emu* e) {
  gsp_scene_desc d = e->sc;
  d.instances = e->instances.data();
  d.positions = e->positions.data();
  return d;
}
}  // namespace

extern "C" {

// gsp_set_light_grid's own validation: 0 = acceptable, 1 and the text in err otherwise
int lightgrid_emu_check(const gsp_light_grid* s, char* err, uint32_t cap) {
  const char* why = check_light_grid(s);
  if (why && err && cap) {
    std::strncpy(err, why, cap - 1);
    err[cap - 1] = 0;
  }
  return why ? 1 : 0;
}
// the bounds of the emulation's scene as the library forms them at upload: bounds6 = {lo, hi}; 0 = the scene has no vertex
int lightgrid_emu_bounds(void* h, float* bounds6) {
  const gsp_scene_desc d = desc_of((Emu*)h);
  return lightgrid_scene_bounds(&d, bounds6, bounds6 + 3) ? 1 : 0;
}
// the resolution a grid over bounds6 is built with for num_lights lights: 0 = fine, 1 = beyond the cap
int lightgrid_emu_resolve(const gsp_light_grid* want, const float* bounds6, uint32_t num_lights, uint32_t* res3) {
  return lightgrid_resolve(*want, bounds6, bounds6 + 3, num_lights, res3);
}
// the header (16 words) of a grid over bounds6 at res3
void lightgrid_emu_header(const float* bounds6, const uint32_t* res3, void* head64) {
  const LightGridHeader g = make_lightgrid_header(bounds6, bounds6 + 3, res3);
  std::memcpy(head64, &g, sizeof(g));
}
// The builder: the fallback table (n + nd entries) + its tail (4 floats) and the grid image (lightgrid_bytes) of the UNBAKED records;
// weights (optional): cells * (n + nd) doubles.  Returns the host time of the grid build in milliseconds
double lightgrid_emu_build(const void* head64, const gsp_triangle_light* lights, uint32_t n, const gsp_delta_light* delta, uint32_t nd, gsp_light_pick* fallback,
                           float* fallback_tail4, uint8_t* grid, double* weights) {
  LightGridHeader g;
  std::memcpy(&g, head64, sizeof(g));
  std::vector<gsp_delta_light> acc(delta ? nd : 0u);
  for (size_t k = 0; k < acc.size(); ++k) acc[k] = accept_delta_light(delta[k]);
  build_light_pick(lights, n, acc.data(), (uint32_t)acc.size(), fallback);
  fallback_tail4[0] = light_pick_inv_sum(lights, n, acc.data(), (uint32_t)acc.size());
  fallback_tail4[1] = fallback_tail4[2] = fallback_tail4[3] = 0.0f;
  const auto t0 = std::chrono::steady_clock::now();
  build_light_grid(g, lights, n, acc.data(), (uint32_t)acc.size(), fallback, grid, weights);
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// ---- pt_lightgrid.h, one function at a time, over n inputs: the bodies of tests/devfn/lightgrid_bodies.h, which lightgrid_devfn.hip runs on the GPU ----
int lightgrid_emu_cell(uint64_t n, const uint8_t* grid, const float* pos3, uint32_t* out4) {
  for (uint64_t i = 0; i < n; ++i) devfn::lightgrid_cell1(i, grid, pos3, out4);
  return 0;
}
int lightgrid_emu_pick(uint64_t n, const uint8_t* grid, const gsp_light_pick* fallback, uint32_t num_lights, const float* pos3, const uint32_t* r, uint32_t* out2) {
  for (uint64_t i = 0; i < n; ++i) devfn::lightgrid_pick1(i, grid, fallback, num_lights, pos3, r, out2);
  return 0;
}
int lightgrid_emu_hit_pmf(uint64_t n, const uint8_t* grid, const gsp_light_pick* fallback, uint32_t num_lights, const float* pos3, const float* tri12, float* out1) {
  for (uint64_t i = 0; i < n; ++i) devfn::lightgrid_hit_pmf1(i, grid, fallback, num_lights, pos3, tri12, out1);
  return 0;
}

// delta_emu_render with the context's light grid (`grid`: null or enabled == 0 = off).  bounds6: the bounds of the scene AS UPLOADED
// (null = those of the emulation's own scene; a test that moves an instance after the upload hands the emulation the moved scene and
// the bounds of the first).  Return codes: 1 = a call of the library would have returned GSP_ERR_INVALID (the grid without the power
// pick or the textbook estimator included), 3 = GSP_ERR_NOMEM (the resolution is beyond the cap).
// counts (optional, 4) = {extension rays, shadow rays, shaded vertices, samples};  moments (optional): per pixel sum of the samples'
// r, g, b and of their squares, in double;  res3 (optional): the resolution the grid was built with (0, 0, 0: no grid)
int lightgrid_emu_render(void* h, uint32_t width, uint32_t height, const gsp_render_params* rp, uint32_t estimator, uint32_t light_mode,
                         const gsp_triangle_light* lights, const gsp_delta_light* delta, uint32_t nd, const gsp_medium* media, const gsp_medium_scatter* scatter,
                         uint32_t num_media, const gsp_light_grid* grid, const float* bounds6, float* accum, uint64_t* counts, double* moments, uint32_t* res3) {
  Emu* e = (Emu*)h;
  if (light_mode != GSP_LIGHTS_UNIFORM && light_mode != GSP_LIGHTS_POWER) return 1;
  if (estimator != GSP_ESTIMATOR_REFERENCE && estimator != GSP_ESTIMATOR_TEXTBOOK) return 1;
  if (max_medium_number(e->instances.data(), e->instances.size()) > (media ? num_media : 0u)) return 4;  // "BSDF handle out of range"
  const bool med = media != nullptr && num_media != 0u;
  if (scatter && check_media_scattering(scatter, num_media, med ? num_media : 0u)) return 1;
  if (check_delta_lights(delta, nd)) return 1;
  if (check_light_grid(grid)) return 1;
  const bool power = light_mode == GSP_LIGHTS_POWER, est = estimator == GSP_ESTIMATOR_TEXTBOOK;
  const bool grid_switch = grid != nullptr && grid->enabled != 0u;
  if (grid_switch && !(power && est)) return 1;
  std::vector<gsp_delta_light> acc_d(delta ? nd : 0u);
  for (size_t k = 0; k < acc_d.size(); ++k) acc_d[k] = accept_delta_light(delta[k]);
  const bool dlt = !acc_d.empty();
  const uint32_t all = e->view.num_lights + (uint32_t)acc_d.size();
  // the grid the library would hold resident
  float b6[6] = {0, 0, 0, 0, 0, 0};
  bool has_bounds = true;
  if (bounds6) std::memcpy(b6, bounds6, sizeof(b6));
  else has_bounds = lightgrid_emu_bounds(h, b6) != 0;
  const bool grid_on = grid_switch && all != 0u && has_bounds;
  LightGridHeader head{};
  uint32_t res[3] = {0, 0, 0};
  if (grid_on) {
    if (lightgrid_resolve(*grid, b6, b6 + 3, all, res) != 0) return 3;
    head = make_lightgrid_header(b6, b6 + 3, res);
  }
  if (res3) res3[0] = res[0], res3[1] = res[1], res3[2] = res[2];
  const std::vector<gsp_medium_scatter> zeros(med ? num_media : 0u, gsp_medium_scatter{{0.0f, 0.0f, 0.0f}, 0.0f});
  Tables tab{med ? media : nullptr, med && scatter && any_scattering(scatter, num_media) ? scatter : nullptr, dlt, grid_on, e->view.num_lights, 0u};
  if ((dlt || grid_switch) && med && !scatter) tab.scatter = zeros.data();
  else if ((dlt || grid_switch) && med) tab.scatter = scatter;
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
  const bool image = power || dlt;
  GridImage img(lights, image ? e->view.num_lights : 0u, acc_d.data(), (uint32_t)acc_d.size(), power, est, grid_on ? &head : nullptr);
  SceneView S = e->view;
  if (image) {
    S.lights = img.lights();
    S.num_lights = all;
    S.inv_num_lights = S.num_lights ? 1.0f / (float)S.num_lights : 0.0f;
    S.tables = img.base();  // (the grid's offset counts from here)
    tab.grid_off = (uint32_t)img.grid_off;
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
      ++n_samples;
      if (moments) {
        const double v[3] = {result.x, result.y, result.z};
        for (int c = 0; c < 3; ++c) moments[6 * lp + c] += v[c], moments[6 * lp + 3 + c] += v[c] * v[c];
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
    counts[3] = n_samples;
  }
  return 0;
}
}
