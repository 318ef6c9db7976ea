// tests/emu/lens_emu.cpp -- TEST HARNESS, NOT A PRODUCT PATH.
//
// The thin-lens side of the host emulation (include/gpuspectral_pt.h, "Thin lens").  It includes filter_emu.cpp textually -- and
// through it pt_emu.cpp: scene, BVH, per-ray traversal, the filter's constants -- and adds entries that see a lens: the product's
// generate_path with RenderConstsLens, ray by ray; its lens sampler and lens ray on given inputs; gsp_set_lens's validation
// (resolve_lens, pt_hostmath.h); and a render loop that is filter_emu_render's with the lens in the constants.  Built into
// tests/emu/liblens_emu.so by the tests that use it.
#include "filter_emu.cpp"

namespace {

// the constants as render_consts (pt_render_pipeline.inc) forms them: the filter's, then set_lens_consts
RenderConstsLens lens_consts_for(uint32_t width, uint32_t height, float fov, const float* to_world, uint32_t filter, float param,
                                 const gsp_lens* lens) {
  RenderConstsLens rc;
  static_cast<RenderConsts&>(rc) = consts_for(width, height, fov, to_world, filter, param);
  gsp_lens l;
  if (resolve_lens(lens, l) == nullptr) set_lens_consts(rc, l);
  return rc;
}

}  // namespace

extern "C" {

// gsp_set_lens's validation.  Returns 0 and the stored lens in *out, or 1 and the error text in err (cap bytes)
int lens_emu_resolve(const gsp_lens* in, gsp_lens* out, char* err, uint32_t cap) {
  const char* why = resolve_lens(in, *out);
  if (why && err && cap) {
    std::strncpy(err, why, cap - 1);
    err[cap - 1] = 0;
  }
  return why ? 1 : 0;
}

// the resolved constants of a lens: out5 = {radius, focus, s, blades (as float), rotation}, out5[5] = zplane
void lens_emu_consts(uint32_t width, uint32_t height, float fov, const float* to_world, const gsp_lens* lens, float* out6) {
  const RenderConstsLens rc = lens_consts_for(width, height, fov, to_world, GSP_FILTER_NONE, 0.0f, lens);
  out6[0] = rc.lens_radius;
  out6[1] = rc.lens_focus;
  out6[2] = rc.lens_s;
  out6[3] = (float)rc.lens_blades;
  out6[4] = rc.lens_rotation;
  out6[5] = rc.zplane;
}

// n paths through generate_path(RenderConstsLens): out8 = n x {o.xyz, d.xyz, lens point xy}, seeds = n x prd.seed.  The lens point
// is drawn a second time with the product's filter_offset + lens_point from the same state; (0, 0) for a pinhole.
void lens_emu_generate(uint32_t width, uint32_t height, float fov, const float* to_world, uint32_t filter, float param,
                       const gsp_lens* lens, const uint32_t* gids, const uint32_t* timestamps, uint64_t n, float* out8, uint32_t* seeds) {
  const RenderConstsLens rc = lens_consts_for(width, height, fov, to_world, filter, param, lens);
  for (uint64_t i = 0; i < n; ++i) {
    PathState p;
    generate_path(rc, gids[i], timestamps[i], 0u, p);
    float lx = 0.0f, ly = 0.0f;
    if (rc.lens_radius > 0.0f) {
      uint32_t rng = pcg_hash(tea(width * (gids[i] / width) + gids[i] % width, timestamps[i]));
      float ox, oy;
      if (filter != GSP_FILTER_NONE) filter_offset(rc.pixel_filter, rc.pixel_filter_param, rng, ox, oy);
      lens_point(rc.lens_radius, rc.lens_blades, rc.lens_rotation, rng, lx, ly);
    }
    const float r[8] = {p.o.x, p.o.y, p.o.z, p.d.x, p.d.y, p.d.z, lx, ly};
    std::memcpy(out8 + 8 * i, r, sizeof(r));
    seeds[i] = p.seed;
  }
}

// the product's lens_point from GIVEN rng states: out2 = n x (lx, ly); states_out (optional) = the states after the two draws
void lens_emu_points(float radius, uint32_t blades, float rotation, const uint32_t* states, uint64_t n, float* out2, uint32_t* states_out) {
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t rng = states[i];
    lens_point(radius, blades, rotation, rng, out2[2 * i], out2[2 * i + 1]);
    if (states_out) states_out[i] = rng;
  }
}

// the product's camera_ray_lens for GIVEN fragCoords and lens points: out6 = n x {o.xyz, d.xyz}
void lens_emu_ray_through(uint32_t width, uint32_t height, float fov, const float* to_world, const gsp_lens* lens, const float* frag,
                          const float* lpts, uint64_t n, float* out6) {
  const RenderConstsLens rc = lens_consts_for(width, height, fov, to_world, GSP_FILTER_NONE, 0.0f, lens);
  for (uint64_t i = 0; i < n; ++i) {
    f3 o, d;
    camera_ray_lens(rc, frag[2 * i], frag[2 * i + 1], lpts[2 * i], lpts[2 * i + 1], o, d);
    const float r[6] = {o.x, o.y, o.z, d.x, d.y, d.z};
    std::memcpy(out6 + 6 * i, r, sizeof(r));
  }
}

// the pinhole ray of GIVEN fragCoords (camera_dir) and the float32 cosine gsp_focus_distance multiplies the hit distance with:
// out4 = n x {d.xyz, normalize(v).z}
void lens_emu_pinhole(uint32_t width, uint32_t height, float fov, const float* to_world, const float* frag, uint64_t n, float* out4) {
  const RenderConsts rc = consts_for(width, height, fov, to_world, GSP_FILTER_NONE, 0.0f);
  for (uint64_t i = 0; i < n; ++i) {
    const float fx = frag[2 * i], fy = frag[2 * i + 1];
    const f3 d = camera_dir(rc, fx, fy);
    const float cosz = normalize(mk3(-(fx - (float)width / 2.0f), fy - (float)height / 2.0f, rc.zplane)).z;
    const float r[4] = {d.x, d.y, d.z, cosz};
    std::memcpy(out4 + 4 * i, r, sizeof(r));
  }
}

// filter_emu_render with the lens in the constants; counts (optional) = {extension rays, shadow rays, shaded vertices}
int lens_emu_render(void* h, uint32_t width, uint32_t height, const uint32_t* pixel_ids, uint64_t num_pixels,
                    const gsp_render_params* rp, const gsp_lens* lens, float* accum, uint64_t* counts) {
  Emu* e = (Emu*)h;
  RenderConstsLens rc = lens_consts_for(width, height, e->sc.camera.fov, e->sc.camera.to_world, rp->pixel_filter, rp->pixel_filter_param, lens);
  rc.max_depth = rp->max_depth;
  rc.rr_start_depth = rp->rr_start_depth;
  rc.clamp = rp->clamp;
  rc.nee = rp->disable_nee != 0 ? 0u : 1u;
  const uint64_t npix = pixel_ids ? num_pixels : (uint64_t)width * height;
  const SceneView& S = e->view;
  uint64_t n_ext = 0, n_sh = 0, n_vert = 0;
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
        if (e->textured) shade_vertex<true>(S, rc, p, hit, out);
        else shade_vertex<false>(S, rc, p, hit, out);
        ++n_vert;
        if (out.has_shadow) {
          HitRec sh;
          uint32_t aux2;
          bool occ = trace1<true>(S, out.shadow.o, out.shadow.d, 0.01f, out.shadow.tmax, sh, aux2);
          ++n_sh;
          bool nee_done;
          connect_vertex(rc.clamp, out.shadow, occ, result, nee_done);
          if (nee_done && out.alive) out.next.directWeight = out.shadow.dw_nee;
        } else {
          add_emitted(rc.clamp, out.emitted, result);
        }
        alive = out.alive;
        p = out.next;
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
  }
  return 0;
}
}
