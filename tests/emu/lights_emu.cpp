// tests/emu/lights_emu.cpp -- TEST HARNESS, NOT A PRODUCT PATH.
//
// The light-selection side of the host emulation (include/gpuspectral_pt.h, "Light selection").  It includes pt_emu.cpp textually
// -- scene, BVH, per-ray traversal -- and adds: the product's table builder (pt_lightpick.h) as it is; the pick rule
// (light_pick_index, pt_shading.h) over chosen draws; the host twin of the device harness's sample_light_power vectors
// (tests/devfn/lights_bodies.h); and a render loop that is emu_render's around the product's shade_vertex<TEX, false, MED, LSEL>
// with the alias table straight behind a copy of the baked light records, as the resident table image has it.  Built into
// tests/emu/liblights_emu.so by the tests that use it (tests/lights_util.py).
#include "pt_emu.cpp"

#include "../../gpuspectral_amd/csrc/pt_lightpick.h"
#include "../devfn/lights_bodies.h"

namespace {
// baked light records + pick table, back to back, 16-byte aligned (the layout of the table image)
struct LightImage {
  std::vector<LightPickQuad> store;  // (alignas(16) elements: the allocation is aligned)
  gsp_triangle_light* lights() { return (gsp_triangle_light*)store.data(); }
  LightImage(const gsp_triangle_light* raw, uint32_t n) {
    static_assert(sizeof(gsp_triangle_light) % 16 == 0 && sizeof(LightPickQuad) == 16 && sizeof(gsp_light_pick) == 16, "layout");
    store.resize((size_t)n * (sizeof(gsp_triangle_light) / 16 + 1) + 1);
    if (n) std::memcpy(lights(), raw, sizeof(gsp_triangle_light) * (size_t)n);
    build_light_pick(raw, n, (gsp_light_pick*)(lights() + n));
    for (uint32_t i = 0; i < n; ++i) bake_light(lights()[i]);
  }
};
}  // namespace

extern "C" {

void lights_emu_build(const gsp_triangle_light* lights, uint32_t n, gsp_light_pick* out) { build_light_pick(lights, n, out); }
void lights_emu_build_weights(const double* w, uint32_t n, gsp_light_pick* out) { build_light_pick_from_weights(w, n, out); }
void lights_emu_weights(const gsp_triangle_light* lights, uint32_t n, double* out) {
  for (uint32_t i = 0; i < n; ++i) out[i] = light_pick_weight(lights[i]);
}

// light_pick_index over `count` draws r: counts[k] += 1 for the light picked; pmf_out (optional) = the pmf returned per draw
int lights_emu_pick(const gsp_light_pick* pick, uint32_t n, const uint32_t* r, uint64_t count, uint64_t* counts, float* pmf_out) {
  if (n == 0 || !devfn::ok_light_pick(pick, n)) return 1;
  std::vector<LightPickQuad> t(n);
  std::memcpy(t.data(), pick, sizeof(gsp_light_pick) * (size_t)n);
  for (uint64_t i = 0; i < count; ++i) {
    float pmf;
    const uint32_t k = light_pick_index((const gsp_light_pick*)t.data(), n, r[i], pmf);
    ++counts[k];
    if (pmf_out) pmf_out[i] = pmf;
  }
  return 0;
}

// host twin of lights_devfn_power (tests/devfn/lights_devfn.hip)
int lights_emu_devfn_power(const gsp_triangle_light* lights, uint32_t num_lights, const float* pos, const uint32_t* seeds, uint64_t n, float* out8,
                           gsp_light_pick* pick_out) {
  if (num_lights == 0 || num_lights > (1u << 20) || n > (1ull << 24)) return devfn::kBadIndex;
  LightImage img(lights, num_lights);
  const gsp_light_pick* pick = (const gsp_light_pick*)(img.lights() + num_lights);
  if (!devfn::ok_light_pick(pick, num_lights)) return devfn::kBadIndex;
  if (pick_out) std::memcpy(pick_out, pick, sizeof(gsp_light_pick) * (size_t)num_lights);
  for (uint64_t i = 0; i < n; ++i) devfn::light_power1(i, img.lights(), num_lights, pos, seeds, out8);
  return 0;
}

// emu_render with the context's light selection mode and (optionally) its media: mode == GSP_LIGHTS_POWER selects <LSEL = true>,
// num_media != 0 <MED = true>, as the dispatcher of pt_render_pipeline.inc does.  `lights` = the scene's light records as the
// caller gave them (the table is built from those).
// counts (optional) = {extension rays, shadow rays, shaded vertices, NEE terms added, NEE terms the firefly cut-off dropped}
// sums (optional, 6 doubles) = {NEE r, g, b, emission r, g, b} of what add_emitted / connect_vertex let through
// moments (optional, 6 doubles per pixel, added to) = per pixel sum and sum of squares of the samples' r, g, b
int lights_emu_render(void* h, uint32_t width, uint32_t height, const uint32_t* pixel_ids, uint64_t num_pixels, const gsp_render_params* rp,
                      uint32_t mode, const gsp_triangle_light* lights, const gsp_medium* media, uint32_t num_media, float* accum,
                      uint64_t* counts, double* sums, double* moments) {
  Emu* e = (Emu*)h;
  if (mode != GSP_LIGHTS_UNIFORM && mode != GSP_LIGHTS_POWER) return 1;
  if (max_medium_number(e->instances.data(), e->instances.size()) > (media ? num_media : 0u)) return 4;
  const bool med = media != nullptr && num_media != 0u;
  const bool power = mode == GSP_LIGHTS_POWER;
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
  LightImage img(lights, e->view.num_lights);
  SceneView S = e->view;
  if (power) S.lights = img.lights();
  uint64_t n_ext = 0, n_sh = 0, n_vert = 0, n_nee = 0, n_cut = 0;
  double sum[6] = {0, 0, 0, 0, 0, 0};
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
        if (power) {
          if (med) {
            if (e->textured) shade_vertex<true, false, true, true>(S, rc, p, hit, out, media);
            else shade_vertex<false, false, true, true>(S, rc, p, hit, out, media);
          } else {
            if (e->textured) shade_vertex<true, false, false, true>(S, rc, p, hit, out);
            else shade_vertex<false, false, false, true>(S, rc, p, hit, out);
          }
        } else {
          if (med) {
            if (e->textured) shade_vertex<true, false, true>(S, rc, p, hit, out, media);
            else shade_vertex<false, false, true>(S, rc, p, hit, out, media);
          } else {
            if (e->textured) shade_vertex<true>(S, rc, p, hit, out);
            else shade_vertex<false>(S, rc, p, hit, out);
          }
        }
        ++n_vert;
        if (out.has_shadow) {
          HitRec sh;
          uint32_t aux2;
          bool occ = trace1<true>(S, out.shadow.o, out.shadow.d, 0.01f, out.shadow.tmax, sh, aux2);
          ++n_sh;
          bool nee_done;
          const q4 before = result;
          connect_vertex(rc.clamp, out.shadow, occ, result, nee_done);
          if (!occ) {
            // (the sum the cut-off sees is nee + emis: a dropped sum takes both terms with it)
            const f3 t = out.shadow.nee + out.shadow.emis;
            const bool kept = t.x < rc.clamp && t.y < rc.clamp && t.z < rc.clamp;
            ++(kept ? n_nee : n_cut);
            if (kept) {
              sum[0] += out.shadow.nee.x, sum[1] += out.shadow.nee.y, sum[2] += out.shadow.nee.z;
              sum[3] += out.shadow.emis.x, sum[4] += out.shadow.emis.y, sum[5] += out.shadow.emis.z;
            }
          } else {
            sum[3] += (double)result.x - before.x, sum[4] += (double)result.y - before.y, sum[5] += (double)result.z - before.z;
          }
          if (nee_done && out.alive) out.next.directWeight = out.shadow.dw_nee;
        } else {
          const q4 before = result;
          add_emitted(rc.clamp, out.emitted, result);
          sum[3] += (double)result.x - before.x, sum[4] += (double)result.y - before.y, sum[5] += (double)result.z - before.z;
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
    counts[3] = n_nee;
    counts[4] = n_cut;
  }
  if (sums)
    for (int k = 0; k < 6; ++k) sums[k] = sum[k];
  return 0;
}
}
