// tests/emu/media_emu.cpp -- TEST HARNESS, NOT A PRODUCT PATH.
//
// The interior-media side of the host emulation (include/gpuspectral_pt.h, "Interior media").  It includes pt_emu.cpp textually
// -- scene, BVH, per-ray traversal -- and adds a render loop that is emu_render's around the product's shade_vertex<TEX, false, MED>
// (pt_emu.cpp hard-codes the instantiations without media), with the counts of lens_emu_render and a per-pixel path log; and
// gsp_set_media's validation (check_media, pt_hostmath.h).  Built into tests/emu/libmedia_emu.so by the tests that use it.
#include "pt_emu.cpp"

extern "C" {

// gsp_set_media's validation.  Returns 0, or 1 and the error text in err (cap bytes)
int media_emu_check(const gsp_medium* media, uint32_t num_media, char* err, uint32_t cap) {
  const char* why = check_media(media, num_media);
  if (why && err && cap) {
    std::strncpy(err, why, cap - 1);
    err[cap - 1] = 0;
  }
  return why ? 1 : 0;
}

// the largest medium number the scene's instances name
uint32_t media_emu_max_number(void* h) {
  Emu* e = (Emu*)h;
  return max_medium_number(e->instances.data(), e->instances.size());
}

// emu_render with the context's media: num_media != 0 selects <MED = true>, as the dispatcher of pt_render_pipeline.inc does.
// counts (optional) = {extension rays, shadow rays, shaded vertices}.  back_hits (optional, one byte per pixel of the call, OR-ed
// into): bit 0 = some vertex of the pixel's paths lay on a back face (the test of rayhit.rchit:698 on the packet's geometric
// normal) of a triangle whose material word names a medium -- read off the packet here, outside the product's headers.
int media_emu_render(void* h, uint32_t width, uint32_t height, const uint32_t* pixel_ids, uint64_t num_pixels, const gsp_render_params* rp,
                     const gsp_medium* media, uint32_t num_media, float* accum, uint64_t* counts, uint8_t* back_hits) {
  Emu* e = (Emu*)h;
  if (max_medium_number(e->instances.data(), e->instances.size()) > (media ? num_media : 0u)) return 4;  // "BSDF handle out of range"
  const bool med = media != nullptr && num_media != 0u;
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
        if (back_hits) {
          const q4 s0 = S.tri_shade[4ll * hit.slot];
          const bool named = ((f2u(s0.w) >> 19) & 0xfffu) != 0u;
          if (named && dot(mk3(s0.x, s0.y, s0.z), -p.d) < 0.0f) back_hits[lp] |= 1u;
        }
        ShadeOut out;
        if (med) {
          if (e->textured) shade_vertex<true, false, true>(S, rc, p, hit, out, media);
          else shade_vertex<false, false, true>(S, rc, p, hit, out, media);
        } else {
          if (e->textured) shade_vertex<true>(S, rc, p, hit, out);
          else shade_vertex<false>(S, rc, p, hit, out);
        }
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
