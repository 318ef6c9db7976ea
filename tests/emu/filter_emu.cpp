// tests/emu/filter_emu.cpp -- TEST HARNESS, NOT A PRODUCT PATH.
//
// The pixel-filter side of the host emulation (include/gpuspectral_pt.h, "Pixel filter").  pt_emu.cpp's emu_render fills
// RenderConsts field by field and so never sees a filter; this file includes it textually -- for its scene, BVH and per-ray
// traversal -- and adds entries that do: the product's generate_path with a filter in the constants, ray by ray, and a
// render loop that is emu_render's with the two filter fields set and ray counters.  Built into tests/emu/libfilter_emu.so by
// the tests that use it.
#include "pt_emu.cpp"

namespace {

RenderConsts consts_for(uint32_t width, uint32_t height, float fov, const float* to_world, uint32_t filter, float param) {
  RenderConsts rc;
  rc.width = width;
  rc.height = height;
  rc.max_depth = 50;
  rc.rr_start_depth = 10;
  rc.clamp = 20.0f;
  rc.nee = 1u;
  rc.zplane = (std::max((float)width, (float)height) / 2.0f) / tanf(fov / 2.0f);
  for (int i = 0; i < 16; ++i) rc.cam_to_world[i] = to_world[i];
  for (int i = 0; i < 3; ++i) rc.cam_origin[i] = to_world[12 + i];
  rc.pixel_filter = filter;
  // the parameter as render_consts (pt_render_pipeline.inc) resolves it: 0 = the filter's default
  rc.pixel_filter_param = filter == GSP_FILTER_TENT ? (param != 0.0f ? param : 1.0f) : filter == GSP_FILTER_GAUSSIAN ? (param != 0.0f ? param : 0.5f) : 0.0f;
  return rc;
}

}  // namespace

extern "C" {

// n paths: out8 = n x {o.xyz, d.xyz, offset.xy}, seeds = n x prd.seed.  The offset is drawn a second time from the same state
// with the product's filter_offset (generate_path does not hand it out); (0, 0) for GSP_FILTER_NONE.
void filter_emu_generate(uint32_t width, uint32_t height, float fov, const float* to_world, uint32_t filter, float param,
                         const uint32_t* gids, const uint32_t* timestamps, uint64_t n, float* out8, uint32_t* seeds) {
  const RenderConsts rc = consts_for(width, height, fov, to_world, filter, param);
  for (uint64_t i = 0; i < n; ++i) {
    PathState p;
    generate_path(rc, gids[i], timestamps[i], 0u, p);
    float ox = 0.0f, oy = 0.0f;
    if (filter != GSP_FILTER_NONE) {
      uint32_t rng = pcg_hash(tea(width * (gids[i] / width) + gids[i] % width, timestamps[i]));
      filter_offset(rc.pixel_filter, rc.pixel_filter_param, rng, ox, oy);
    }
    const float r[8] = {p.o.x, p.o.y, p.o.z, p.d.x, p.d.y, p.d.z, ox, oy};
    std::memcpy(out8 + 8 * i, r, sizeof(r));
    seeds[i] = p.seed;
  }
}

// TEST-ONLY entry: the camera ray through pixel + a GIVEN offset (the product's camera_dir, which generate_path calls with
// pixel + the drawn offset).  out3 = n x d.xyz
void filter_emu_ray_through(uint32_t width, uint32_t height, float fov, const float* to_world, const uint32_t* gids,
                            const float* offsets, uint64_t n, float* out3) {
  const RenderConsts rc = consts_for(width, height, fov, to_world, GSP_FILTER_NONE, 0.0f);
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t px = gids[i] % width, py = gids[i] / width;
    float fx = (float)px, fy = (float)py;
    fx = fx + offsets[2 * i];
    fy = fy + offsets[2 * i + 1];
    const f3 d = camera_dir(rc, fx, fy);
    out3[3 * i] = d.x;
    out3[3 * i + 1] = d.y;
    out3[3 * i + 2] = d.z;
  }
}

// emu_render with the pixel filter of rp in the constants; counts (optional) = {extension rays, shadow rays, shaded vertices}
int filter_emu_render(void* h, uint32_t width, uint32_t height, const uint32_t* pixel_ids, uint64_t num_pixels,
                      const gsp_render_params* rp, float* accum, uint64_t* counts) {
  Emu* e = (Emu*)h;
  RenderConsts rc = consts_for(width, height, e->sc.camera.fov, e->sc.camera.to_world, rp->pixel_filter, rp->pixel_filter_param);
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
