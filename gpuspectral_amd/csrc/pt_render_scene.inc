// pt_render_scene.inc -- part of the translation unit pt_render.hip (included there; not compiled on its own).
// gsp_upload_scene, gsp_update_camera / _instances / _tables, gsp_frame_begin: validation, the resident tables (lazy version ring,
// pt_versions.h), the geometry ring, the split scene, bake + build / refit.  (Inside the extern "C" block pt_render.hip opens.)

// ---- scene upload and per-frame edits -----------------------------------------------------------------------------------
// gsp_upload_scene = validate -> tables (BSDF arrays + lights) -> resident geometry + instance table -> bake + BVH build;
// gsp_update_tables / gsp_update_instances / gsp_update_camera redo only their own part (PathTracer.cpp:58-93 re-reads all
// of it every frame; only the BLAS of a mesh is kept there, Renderer.cpp:122-131).

static int check_instances(gsp_context* ctx, const gsp_instance* inst, uint32_t n, const uint32_t* num_bsdfs, uint64_t num_vertices,
                           uint64_t* total_tris) {
  uint64_t total = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const gsp_instance& in = inst[i];
    if (in.vertex_count % 3 != 0 || (uint64_t)in.first_vertex + in.vertex_count > num_vertices) {
      ctx->err = "instance " + std::to_string(i) + ": vertex range outside the position/normal arrays";
      return GSP_ERR_SCENE;
    }
    // (bit 31 is not part of a handle: with it the type is out of range, as it was when the type was all of bits 16..31)
    const uint32_t type = (in.bsdf >> 16) & 7u, idx = in.bsdf & 0xffffu, medium = (in.bsdf >> 19) & 0xfffu;
    if ((in.bsdf >> 31) != 0u || idx >= num_bsdfs[type] || medium > ctx->num_media) {
      ctx->err = "instance " + std::to_string(i) + ": BSDF handle out of range";
      return GSP_ERR_SCENE;
    }
    total += in.vertex_count / 3;
  }
  if (total_tris) *total_tris = total;
  return GSP_OK;
}

// has_texture words against `num_textures` entries (0 textures: the words are ignored, as the reference's shaders ignore them)
static int check_texture_words(gsp_context* ctx, const gsp_scene_desc* sc, uint32_t num_textures) {
  if (num_textures == 0) return GSP_OK;
  auto bad = [&](int32_t h) { return h < 0 || (uint32_t)h > num_textures; };
  bool oob = false;
  for (uint32_t k = 0; k < sc->num_bsdfs[GSP_BSDF_DIFFUSE] && sc->diffuse_bsdfs; ++k) oob |= bad(sc->diffuse_bsdfs[k].has_texture);
  for (uint32_t k = 0; k < sc->num_bsdfs[GSP_BSDF_ROUGH_CONDUCTOR] && sc->rough_conductor_bsdfs; ++k)
    oob |= bad(sc->rough_conductor_bsdfs[k].has_texture);
  for (uint32_t k = 0; k < sc->num_bsdfs[GSP_BSDF_ROUGH_PLASTIC] && sc->rough_plastic_bsdfs; ++k)
    oob |= bad(sc->rough_plastic_bsdfs[k].has_texture);
  if (oob) {
    ctx->err = "has_texture must be 0 or 1 + the index of an entry of `textures`";
    return GSP_ERR_SCENE;
  }
  return GSP_OK;
}

// the primary-hit memos hold hits of the scene / camera / frame as it was: re-traced on the lane's stream before its next batch
static void invalidate_memos(gsp_context* ctx) {
  for (gsp_context::Lane& L : ctx->lanes) L.memo_valid = false;
}
// The one place an edit waits: the samples already queued belong to the scene as it was and finish first.  Counted in
// gsp_stats.scene_drains when there is something to wait for.
static int drain_for_edit(gsp_context* ctx) {
  if (!ctx->pipe_active) return GSP_OK;
  ++ctx->stats.scene_drains;
  return pipeline_drain(ctx);
}

// record sizes of the eight BSDF tables (in GSP_BSDF_* order), then of the lights
static constexpr size_t kRecordBytes[9] = {sizeof(gsp_diffuse_bsdf), sizeof(gsp_smooth_dielectric_bsdf), sizeof(gsp_smooth_conductor_bsdf),
                                           sizeof(gsp_smooth_plastic_bsdf), sizeof(gsp_rough_conductor_bsdf), sizeof(gsp_smooth_floor_bsdf),
                                           sizeof(gsp_rough_floor_bsdf), sizeof(gsp_rough_plastic_bsdf), sizeof(gsp_triangle_light)};
// The eight BSDF arrays + the lights (+ in GSP_LIGHTS_POWER mode their alias table) of `sc`, packed back to back (16-B aligned each) as they sit in the context's one table
// allocation; the counts ride in front of the image so that "equal images" means equal tables.  The context's delta lights
// (gsp_set_delta_lights) sit straight behind the triangle lights, 64 B each like them; count 8 stays the TRIANGLE lights, so an image
// unpacks into the scene it was packed from (repack_resident_tables) and a context without delta lights keeps its bytes.
struct TableImage {
  std::vector<uint8_t> bytes;  // [9 x uint64 count][tables ...]: the device holds bytes.data() + kHead onwards
  size_t off[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, total = 0;
  size_t pick_off = 0;         // the light pick table (GSP_LIGHTS_POWER only): == off[8] + 64 * num_lights
  size_t grid_off = 0;         // the light grid (gsp_set_light_grid; 0 = none): behind the pick table's trailing record
  size_t stage_total = 0;      // the bytes in front of the grid (== total without one): what LDS staging sees
  uint32_t grid_res[3] = {0, 0, 0};
  static constexpr size_t kHead = 9 * sizeof(uint64_t);
};
// the light grid is built for a table of n lights: the switch, both modes, lights, and a scene with vertices
static bool light_grid_applies(const gsp_context* ctx, uint32_t n) {
  return ctx->light_grid.enabled != 0u && ctx->light_mode == GSP_LIGHTS_POWER && ctx->estimator == GSP_ESTIMATOR_TEXTBOOK && n != 0u && ctx->scene_has_bounds;
}
static int pack_tables(gsp_context* ctx, const gsp_scene_desc* sc, TableImage& img) {
  const void* src[9] = {sc->diffuse_bsdfs, sc->smooth_dielectric_bsdfs, sc->smooth_conductor_bsdfs, sc->smooth_plastic_bsdfs,
                        sc->rough_conductor_bsdfs, sc->smooth_floor_bsdfs, sc->rough_floor_bsdfs, sc->rough_plastic_bsdfs, sc->lights};
  size_t bytes[9];
  uint64_t counts[9];
  // ... and the environment record (gsp_set_envmap_sampling with an envmap resident) behind those, the last of the light table
  const uint32_t num_delta = (uint32_t)ctx->h_delta.size(), num_env = ctx->env_light ? 1u : 0u, all_lights = sc->num_lights + num_delta + num_env;
  if (all_lights < num_delta + num_env || sc->num_lights + num_delta < num_delta) {
    ctx->err = "too many lights";
    return GSP_ERR_SCENE;
  }
  const size_t delta_bytes = sizeof(gsp_delta_light) * (size_t)num_delta, env_bytes = sizeof(EnvLightRecord) * (size_t)num_env;
  const double env_w = num_env ? env_power_weight(ctx->env_radiant, ctx->env_sampling.extent) : 0.0;
  const double* env_wp = num_env ? &env_w : nullptr;
  img.total = 0;
  for (int k = 0; k < 9; ++k) {
    counts[k] = k < 8 ? sc->num_bsdfs[k] : sc->num_lights;
    bytes[k] = kRecordBytes[k] * counts[k];
    if (bytes[k] && !src[k]) {
      ctx->err = "null array with non-zero count";
      return GSP_ERR_SCENE;
    }
    // a BSDF table is preceded by one derived quad per record (pt_shading.h derived_of / bake_bsdf; zero in the host image,
    // filled on the device by k_bake_tables): off[k] is the table's FIRST RECORD
    if (k < GSP_BSDF_TYPE_COUNT) img.total += 16 * (size_t)counts[k];
    img.off[k] = img.total;
    img.total += (bytes[k] + 15) & ~(size_t)15;
  }
  img.total += delta_bytes + env_bytes;  // (behind the triangle lights, the last of the nine: 64-B records, no padding)
  // GSP_LIGHTS_POWER: a tenth sub-table, the alias table of the lights (pt_lightpick.h), straight behind the light records (64 B
  // each: no padding in between), so that (const gsp_light_pick*)(lights + num_lights) finds it.  Absent in uniform mode: such a
  // context keeps the image size, and so the LDS staging decision, it always had
  const bool pick = light_pick_table_bytes(all_lights, ctx->light_mode) != 0;
  img.pick_off = img.total;
  img.total += light_pick_table_bytes(all_lights, ctx->light_mode);
  // ... and, with GSP_ESTIMATOR_TEXTBOOK on top, one trailing 16-byte record behind the table: {inv_sum_w, 0, 0, 0}, what
  // shade_vertex<.., LSEL, EST> multiplies the weight of a light that was HIT with.  Absent in every other combination
  const bool tail = light_pick_tail_bytes(all_lights, ctx->light_mode, ctx->estimator) != 0;
  const size_t tail_off = img.total;
  img.total += light_pick_tail_bytes(all_lights, ctx->light_mode, ctx->estimator);
  // the light grid (pt_lightgrid.h): behind everything a context without it holds, so that those bytes -- and the LDS staging
  // decision, which reads stage_total -- are what they were
  img.stage_total = img.total;
  img.grid_off = 0;
  LightGridHeader grid_head{};
  if (light_grid_applies(ctx, all_lights)) {
    if (lightgrid_resolve(ctx->light_grid, ctx->scene_lo, ctx->scene_hi, all_lights, img.grid_res) != 0) {
      ctx->err = "light grid: cells * lights is beyond 2^20 entries (a 16 MB table image)";
      return GSP_ERR_NOMEM;
    }
    grid_head = make_lightgrid_header(ctx->scene_lo, ctx->scene_hi, img.grid_res);
    img.grid_off = img.total;
    img.total += lightgrid_bytes(grid_head.nx, grid_head.ny, grid_head.nz, all_lights);
  }
  img.bytes.assign(TableImage::kHead + std::max<size_t>(img.total, 16), 0);
  std::memcpy(img.bytes.data(), counts, sizeof(counts));
  for (int k = 0; k < 9; ++k)
    if (bytes[k]) std::memcpy(img.bytes.data() + TableImage::kHead + img.off[k], src[k], bytes[k]);
  if (delta_bytes) std::memcpy(img.bytes.data() + TableImage::kHead + img.off[8] + bytes[8], ctx->h_delta.data(), delta_bytes);
  if (pick) build_light_pick(sc->lights, sc->num_lights, ctx->h_delta.data(), num_delta, (gsp_light_pick*)(img.bytes.data() + TableImage::kHead + img.pick_off), env_wp);
  if (tail) {
    const float inv_sum_w = light_pick_inv_sum(sc->lights, sc->num_lights, ctx->h_delta.data(), num_delta, env_wp);
    std::memcpy(img.bytes.data() + TableImage::kHead + tail_off, &inv_sum_w, sizeof(float));
  }
  if (img.grid_off)
    build_light_grid(grid_head, sc->lights, sc->num_lights, ctx->h_delta.data(), num_delta, (const gsp_light_pick*)(img.bytes.data() + TableImage::kHead + img.pick_off),
                     img.bytes.data() + TableImage::kHead + img.grid_off);
  if (num_env) {  // p_sel: what the table of the context's mode implies for the record -- 1 / n, or the mass of its entry of the alias table
    float p_sel = 1.0f / (float)all_lights;
    if (pick) p_sel = ((const gsp_light_pick*)(img.bytes.data() + TableImage::kHead + img.pick_off))[all_lights - 1u].pmf_self;
    const EnvLightRecord rec = make_env_record(ctx->env_light_to_local, ctx->env_cw, ctx->env_ch, p_sel);
    std::memcpy(img.bytes.data() + TableImage::kHead + img.off[8] + bytes[8] + delta_bytes, &rec, sizeof(rec));
  }
  return GSP_OK;
}
// image -> device, as the NEXT version of the tables (queued on the context's stream; the image becomes the context's host copy,
// so the source stays alive).  next_version == false: the pipeline is drained -- the ring is (re)allocated if the layout has
// changed and the image becomes version tab.ver; true (gsp_update_tables with samples in flight, same layout, a free slot): the
// image goes into the slot of tab.ver + 1, which no sample in flight reads, and becomes current.
static int upload_tables(gsp_context* ctx, const gsp_scene_desc* sc, TableImage& img, bool next_version = false) {
  const size_t slot = (std::max<size_t>(img.total, 16) + 255) & ~(size_t)255;
  uint32_t write_slot = 0;
  if (!next_version) {
    // behind a drain (or the first upload): ONE slot -- the ring is made by the first edit that arrives with samples in flight
    // (grow_table_ring), not at upload: 64 slots of a large light table are gigabytes (r05 review)
    if (ctx->tab.upload_behind_drain(slot) || !ctx->tables.p) {  // (another slot size starts with one slot again)
      ctx->bytes.sub(ctx->tables.count);
      ctx->tables.release();
      CTX_TRY(ctx, ctx->tables.ensure(ctx->tab.allocation_bytes(), &ctx->bytes));
    }
  } else {
    write_slot = ctx->tab.begin_next_version();
  }
  uint8_t* const base = ctx->tables.p + (size_t)write_slot * ctx->tab.slot_bytes;
  ctx->h_tables.swap(img.bytes);
  CTX_TRY(ctx, hipMemcpyAsync(base, ctx->h_tables.data() + TableImage::kHead, std::max<size_t>(img.total, 16), hipMemcpyHostToDevice, ctx->stream));
  for (int k = 0; k < 9; ++k) ctx->table_off[k] = img.off[k];
  ctx->tables_bytes = img.total;
  ctx->tables_stage_bytes = img.stage_total;
  ctx->grid_off = img.grid_off;
  ctx->grid_resident = img.grid_off != 0;
  for (int c = 0; c < 3; ++c) ctx->grid_res[c] = img.grid_res[c];
  ctx->num_tri_lights = sc->num_lights;
  ctx->num_lights = sc->num_lights + (uint32_t)ctx->h_delta.size() + (ctx->env_light ? 1u : 0u);  // (the delta and environment records need no bake: they are resident as packed)
  for (int k = 0; k < GSP_BSDF_TYPE_COUNT; ++k) ctx->num_bsdfs[k] = sc->num_bsdfs[k];
  // the resident light and diffuse records carry what a vertex would compute from them alone (pt_shading.h bake_light / bake_diffuse)
  uint32_t nb = sc->num_lights;
  BakeTables bt;
  for (uint32_t t = 0; t < GSP_BSDF_TYPE_COUNT; ++t) {
    bt.rec[t] = base + img.off[t];
    bt.rec_bytes[t] = (uint32_t)kRecordBytes[t];
    bt.num[t] = sc->num_bsdfs[t];
    nb = std::max(nb, sc->num_bsdfs[t]);
  }
  if (nb) {
    hipLaunchKernelGGL(k_bake_tables, dim3((nb + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream,
                       (gsp_triangle_light*)(base + img.off[8]), sc->num_lights,
                       (gsp_diffuse_bsdf*)(base + img.off[GSP_BSDF_DIFFUSE]), sc->num_bsdfs[GSP_BSDF_DIFFUSE], bt);
    CTX_TRY(ctx, hipGetLastError());
  }
  return GSP_OK;
}

// r06: the table ring is made when an edit first arrives with samples in flight.  The live version (the one-slot allocation,
// flags field 0) is copied into slot 0 of the new ring and the old allocation released: between two gsp_render calls no launch
// is queued (pipeline_run leaves every stream idle), so nothing reads it any more -- the samples in flight are records in the
// path pool, and the launches that pick them up next get the new pointer.  GSP_OK with tab.slots still 1 when the memory is not
// to be had (the edit then waits for the queued samples, as every edit did until r04).
static int grow_table_ring(gsp_context* ctx, uint32_t slots) {
  if (slots < 2 || ctx->tab.slots != 1 || !ctx->tables.p) return GSP_OK;
  DevBuf<uint8_t> ring;
  if (ring.ensure(ctx->tab.slot_bytes * slots, nullptr) != hipSuccess) {
    (void)hipGetLastError();
    return GSP_OK;
  }
  CTX_TRY(ctx, hipMemcpyAsync(ring.p, ctx->tables.p, ctx->tab.slot_bytes, hipMemcpyDeviceToDevice, ctx->stream));
  CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->bytes.sub(ctx->tables.count);
  ctx->tables.swap(ring);  // (`ring` now holds the one-slot allocation and frees it on return)
  ctx->bytes.add(ctx->tables.count);
  ctx->tab.on_grown(slots);
  return GSP_OK;
}

// ---- geometry ring (gsp_context::ring, a TreeArrays) ------------------------------------------------------------------------
// the tree gives back the three arrays it owns (as build_bvh counted them in DeviceBvh::bytes, which the context's ledger holds)
static void release_own_arrays(gsp_context* ctx, DeviceBvh& t) {
  const size_t freed = TreeArrays::bytes_owned_by(t);
  t.free_tree_arrays();
  t.bytes -= std::min(t.bytes, freed);
  ctx->bytes.sub(freed);
}
// the tree lets go of its slot of the ring (free_bvh would free what it points at)
static void detach_from_ring(DeviceBvh& t) {
  t.nodes = t.tri_isect = t.tri_shade = nullptr;
  t.arrays_external = false;
}
// the edited instances' tree of a split scene goes: its arrays were a slot of the ring, the rest was its own
static void drop_edited_tree(gsp_context* ctx) {
  detach_from_ring(ctx->dyn);
  ctx->bytes.sub(ctx->dyn.bytes);
  free_bvh(ctx->dyn);
}
// tree T := its slot of version v (T = ctx->dyn: behind the static tree of a split scene; T = ctx->bvh: a ring of whole trees)
static void point_tree_at(gsp_context* ctx, DeviceBvh& T, uint32_t v) {
  ctx->ring.point(T, (&T == &ctx->dyn ? (size_t)ctx->static_slots : 0) + (size_t)ctx->geo.phys(v) * ctx->geo.stride);
}

// drop_geo_ring and make_geo_ring need an idle pipeline: nothing queued may name the arrays that go away.
static void drop_geo_ring(gsp_context* ctx) {
  if (ctx->bvh.arrays_external) detach_from_ring(ctx->bvh);  // the tree's arrays were a slot of the ring
  if (ctx->split) {                                          // ... and so were the edited instances' tree's
    drop_edited_tree(ctx);
    ctx->split = false;
    ctx->static_slots = 0;
  }
  ctx->bytes.sub(ctx->ring.bytes());
  ctx->ring.release();
  ctx->geo.reset();
}
// Moves the tree's three arrays into slot 0 of a new ring of as many versions (a power of two, at most kGeoVersions) as 32-bit node
// offsets and a quarter of the free device memory allow: 176 B per triangle and version, 11 GB for 64 versions of a million
// triangles.  GSP_OK also when there is no ring to be had (fewer than four versions fit): gsp_update_instances then drains every
// time, as before.
static int make_geo_ring(gsp_context* ctx) {
  DeviceBvh& b = ctx->bvh;
  if (ctx->geo.stride != 0 || ctx->geo_ring_failed || !b.nodes || b.num_tris == 0 || b.arrays_external) return GSP_OK;
  size_t free_b = 0, total_b = 0;
  CTX_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
  // log2 of the slots: at most what the options allow (default kGeoVersions), 32-bit node offsets, a quarter of the free memory
  const GeoRingPlan plan = plan_geo_ring(0, 0, tree_slots(b), b.num_nodes, ctx->opt.geometry_versions, free_b, kNodeAllocMin / kNodeBytes, kGeoMaxStride, kNodeBytes);
  if (plan.log2 < 2) return GSP_OK;
  hipStream_t st = ctx->stream;
  const hipError_t e = ctx->ring.alloc_zeroed((size_t)plan.stride_ring << plan.log2, st);
  if (e == hipErrorOutOfMemory) {
    (void)hipGetLastError();
    ctx->ring.release();
    ctx->geo_ring_failed = true;
    return GSP_OK;
  }
  CTX_TRY(ctx, e);
  CTX_TRY(ctx, ctx->ring.copy_tree_in(0, b, st));
  CTX_TRY(ctx, hipStreamSynchronize(st));
  ctx->bytes.add(ctx->ring.bytes());
  release_own_arrays(ctx, b);
  ctx->ring.point(b, 0);
  ctx->geo.reset();
  ctx->geo.log2 = (uint32_t)plan.log2;
  ctx->geo.stride = (uint32_t)plan.stride_ring;
  return GSP_OK;
}

// ---- instance tables -> device ------------------------------------------------------------------------------------------------
// transformInvT per instance (PathTracer::prepareScene, PathTracer.cpp:58-93)
static void inverse_transposes(const std::vector<gsp_instance>& inst, std::vector<float>& inv_t) {
  inv_t.resize(16ull * inst.size());
  for (size_t i = 0; i < inst.size(); ++i) {
    float tr[16];
    transpose4(inst[i].transform, tr);
    inverse4(tr, &inv_t[16ull * i]);
  }
}
static BuildInput build_input(const gsp_context* ctx, const gsp_instance* inst, const float* inv_t, const uint32_t* tri_first, const uint32_t* tri_id_first,
                              size_t num_instances, uint32_t num_tris) {
  BuildInput bi{};
  bi.instances = inst;
  bi.inv_t = inv_t;
  bi.tri_first = tri_first;
  bi.tri_id_first = tri_id_first;
  bi.num_instances = (uint32_t)num_instances;
  bi.positions = ctx->d_pos.p;
  bi.normals = ctx->d_nrm.p;
  bi.num_tris = num_tris;
  bi.reinsert_rounds = (int)ctx->opt.reinsert_rounds - 1;
  return bi;
}
// the whole instance list (ctx->h_inst) for build_bvh / refit_bvh of the scene's one tree.  The copies are queued: their sources
// are the context's (h_inst, h_invt, h_tabs)
static int upload_scene_instances(gsp_context* ctx, BuildInput& bi) {
  hipStream_t st = ctx->stream;
  inverse_transposes(ctx->h_inst, ctx->h_invt);
  ctx->h_tabs = instance_tables(ctx->h_inst);
  CTX_TRY(ctx, ctx->d_inst.upload(ctx->h_inst.data(), ctx->h_inst.size(), st, &ctx->bytes));
  CTX_TRY(ctx, ctx->d_invt.upload(ctx->h_invt.data(), ctx->h_invt.size(), st, &ctx->bytes));
  CTX_TRY(ctx, ctx->d_first.upload(ctx->h_tabs.tri_first.data(), ctx->h_tabs.tri_first.size(), st, &ctx->bytes));
  bi = build_input(ctx, ctx->d_inst.p, ctx->d_invt.p, ctx->d_first.p, nullptr, ctx->h_inst.size(), (uint32_t)ctx->total_tris);
  return GSP_OK;
}
// ... and one subset of it (which = 0 static / 1 edited, ctx->sub_index) for the trees of a split scene
static int upload_subset(gsp_context* ctx, int which, BuildInput& bi) {
  const std::vector<uint32_t>& idx = ctx->sub_index[which];
  std::vector<gsp_instance> inst(idx.size());
  for (size_t k = 0; k < idx.size(); ++k) inst[k] = ctx->h_inst[idx[k]];
  std::vector<float> inv_t;
  inverse_transposes(inst, inv_t);
  const InstanceTables t = instance_tables(ctx->h_inst, &idx);
  hipStream_t st = ctx->stream;
  CTX_TRY(ctx, ctx->d_inst_sub[which].upload(inst.data(), inst.size(), st, &ctx->bytes));
  CTX_TRY(ctx, ctx->d_invt_sub[which].upload(inv_t.data(), inv_t.size(), st, &ctx->bytes));
  CTX_TRY(ctx, ctx->d_first_sub[which].upload(t.tri_first.data(), t.tri_first.size(), st, &ctx->bytes));
  CTX_TRY(ctx, ctx->d_idfirst_sub[which].upload(t.tri_id_first.data(), t.tri_id_first.size(), st, &ctx->bytes));
  CTX_TRY(ctx, hipStreamSynchronize(st));  // (the host vectors go out of scope)
  bi = build_input(ctx, ctx->d_inst_sub[which].p, ctx->d_invt_sub[which].p, ctx->d_first_sub[which].p, ctx->d_idfirst_sub[which].p, idx.size(), t.total);
  return GSP_OK;
}

// ---- split scene -----------------------------------------------------------------------------------------------------------
// The second half of make_split: the small tree D is built and owns its arrays; the new layout [static tree | ring of D] is
// allocated, filled and swapped in.  *made = false (and nothing changed; D is still the caller's) when there is no room for it.
static int lay_out_split(gsp_context* ctx, DeviceBvh& D, bool* made) {
  DeviceBvh& S = ctx->bvh;
  hipStream_t st = ctx->stream;
  size_t free_b = 0, total_b = 0;
  CTX_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
  const GeoRingPlan plan = plan_geo_ring(tree_slots(S), S.num_nodes, tree_slots(D), D.num_nodes, ctx->opt.geometry_versions, free_b, kNodeAllocMin / kNodeBytes, kGeoMaxStride, kNodeBytes);
  if (plan.log2 < 2) return GSP_OK;
  // ---- the new layout: [static | ring]; the static tree's arrays are copied into it, wherever they were ----
  TreeArrays next;  // (releases the old arrays on return, once they have been swapped into it)
  const hipError_t e = next.alloc_zeroed((size_t)plan.total_slots, st);
  if (e == hipErrorOutOfMemory) {
    (void)hipGetLastError();
    ctx->geo_ring_failed = true;
    return GSP_OK;  // (nothing has changed: the scene stays one tree)
  }
  CTX_TRY(ctx, e);
  CTX_TRY(ctx, next.copy_tree_in(0, S, st));
  CTX_TRY(ctx, next.copy_tree_in((size_t)plan.stride_static, D, st));
  {  // the edited instances' triangles leave the static tree
    const InstanceTables scene = instance_tables(ctx->h_inst);
    CTX_TRY(ctx, ctx->d_first.upload(scene.tri_first.data(), scene.tri_first.size(), st, &ctx->bytes));
    CTX_TRY(ctx, ctx->d_retired.upload(ctx->inst_dynamic.data(), ctx->inst_dynamic.size(), st, &ctx->bytes));
    hipLaunchKernelGGL(k_retire_triangles, dim3((uint32_t)((S.num_tris + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, S.num_tris, S.first_slot,
                       (const uint32_t*)S.slot_to_global, (const uint32_t*)ctx->d_first.p, (uint32_t)ctx->h_inst.size(),
                       (const uint8_t*)ctx->d_retired.p, next.isect.p);
    CTX_TRY(ctx, hipGetLastError());
    CTX_TRY(ctx, hipStreamSynchronize(st));  // (`scene` goes out of scope)
  }
  // ---- swap the new arrays in ----
  if (ctx->split) drop_edited_tree(ctx);               // a re-split: the old edited tree goes
  if (!S.arrays_external) release_own_arrays(ctx, S);  // the first split: the tree owned its arrays
  ctx->bytes.sub(ctx->ring.bytes());
  ctx->ring.swap(next);
  ctx->bytes.add(ctx->ring.bytes());
  ctx->ring.point(S, 0);
  ctx->bytes.add(D.bytes);  // the small tree becomes the context's: its arrays are a slot of the ring, the rest stays its own
  release_own_arrays(ctx, D);
  ctx->ring.point(D, (size_t)plan.stride_static);
  ctx->dyn = std::move(D);
  ctx->split = true;
  ctx->static_slots = (uint32_t)plan.stride_static;
  ctx->geo.reset();
  ctx->geo.stride = (uint32_t)plan.stride_ring;
  ctx->geo.log2 = (uint32_t)plan.log2;
  ctx->s2g_all_valid = false;  // (gsp_trace makes it when it needs it)
  *made = true;
  return ctx->ensure_spill();
}
// Makes (or re-makes, when an edit touches an instance not edited before) the two trees of a split scene and lays them out:
// [static tree | ring of the edited instances' tree].  The static tree IS the tree of the whole scene as it stands, minus the
// triangles of the edited instances (k_retire_triangles: their slots become all-zero triangles; the boxes above them keep what
// they enclosed): nothing is rebuilt but the small tree.  Needs an idle pipeline.  *made = false (and nothing changed) when the
// scene does not lend itself to a split: textures, nothing or too much edited (more than a quarter of the triangles), no room for
// at least four versions.
static int make_split(gsp_context* ctx, bool* made) {
  *made = false;
  // split_declined is passed as false: make_split has never looked at it, and it CAN be set on entry -- a re-split that is
  // declined sets it while the scene is still split, and if the drain that follows fails, the next edit of that split scene asks
  // again (edit_wants_split: is_split).  The callers' gate is edit_wants_split; a host that keeps touching new objects stops at
  // kMaxSceneSplits (a wait per edit is no bargain).
  if (!may_split(false, (uint32_t)ctx->stats.scene_splits, ctx->opt.refit_growth, ctx->opt.geometry_versions, ctx->num_textures, ctx->geo_ring_failed)) return GSP_OK;
  if (ctx->geo.stride != 0 && !ctx->split) return GSP_OK;  // (the scene lives in a ring of whole trees already)
  const DeviceBvh& S = ctx->bvh;
  if (!S.nodes || S.num_tris != ctx->total_tris || ctx->total_tris == 0) return GSP_OK;  // (the tree of the WHOLE scene: first split or a re-split)
  uint64_t tris[2] = {0, 0};
  ctx->sub_index[0].clear();
  ctx->sub_index[1].clear();
  for (size_t i = 0; i < ctx->h_inst.size(); ++i) {
    const int w = ctx->inst_dynamic[i] ? 1 : 0;
    ctx->sub_index[w].push_back((uint32_t)i);
    tris[w] += ctx->h_inst[i].vertex_count / 3;
  }
  if (!split_worthwhile(tris[0], tris[1])) return GSP_OK;
  // ---- the edited instances' tree: this function's until lay_out_split has moved it into ctx->dyn ----
  BuildInput bi;
  DeviceBvh D;
  int rc = upload_subset(ctx, 1, bi);
  if (rc == GSP_OK) rc = build_bvh(ctx->stream, bi, D, ctx->err);
  if (rc == GSP_OK) rc = lay_out_split(ctx, D, made);
  if (!*made) {
    if (rc != GSP_OK) (void)hipStreamSynchronize(ctx->stream);
    free_bvh(D);
  }
  return rc;
}

// slot counted through both trees -> scene triangle index, for gsp_trace on a split scene (made on first use)
static int make_split_s2g(gsp_context* ctx) {
  hipStream_t st = ctx->stream;
  std::vector<uint32_t> all((size_t)ctx->static_slots + ctx->geo.stride, 0xffffffffu);
  // the static tree is the tree of the whole scene: its slots name scene triangles already
  CTX_TRY(ctx, hipMemcpyAsync(all.data(), ctx->bvh.slot_to_global, tree_slots(ctx->bvh) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  CTX_TRY(ctx, hipStreamSynchronize(st));
  {  // the edited instances' tree counts the triangles of ITS instance list
    const DeviceBvh& D = ctx->dyn;
    std::vector<uint32_t> s2g(tree_slots(D));
    CTX_TRY(ctx, hipMemcpyAsync(s2g.data(), D.slot_to_global, s2g.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    CTX_TRY(ctx, hipStreamSynchronize(st));
    const InstanceTables t = instance_tables(ctx->h_inst, &ctx->sub_index[1]);
    for (uint64_t sl = D.first_slot; sl < (uint64_t)D.first_slot + D.num_tris; ++sl) all[(size_t)ctx->static_slots + sl] = scene_triangle_of(t, s2g[sl]);
  }
  CTX_TRY(ctx, ctx->s2g_all.upload(all.data(), all.size(), st, &ctx->bytes));
  CTX_TRY(ctx, hipStreamSynchronize(st));
  ctx->s2g_all_valid = true;
  return GSP_OK;
}

// A new tree of the whole scene from the instance tables of `bi` (upload_scene_instances): world-space bake + BVH build from the
// RESIDENT vertex arrays, per-slot uv gather of a textured scene, traversal spill region
static int build_whole_tree(gsp_context* ctx, const BuildInput& bi) {
  hipStream_t st = ctx->stream;
  // a new tree: its arrays are its own again, and whatever is in flight ends on the old ones first (the committed version's:
  // a refit into the next slot of the ring that grew too much is abandoned here)
  if (ctx->geo.stride && !ctx->split) point_tree_at(ctx, ctx->bvh, ctx->geo.ver);
  int rc = drain_for_edit(ctx);
  if (rc != GSP_OK) return rc;
  drop_geo_ring(ctx);
  ctx->bytes.sub(ctx->bvh.bytes);
  ctx->bytes.sub((ctx->node_hist.count + ctx->tri_hist.count) * sizeof(uint32_t));
  ctx->node_hist.release();
  ctx->tri_hist.release();
  rc = build_bvh(st, bi, ctx->bvh, ctx->err);  // (synchronises the stream)
  if (rc != GSP_OK) {
    (void)hipStreamSynchronize(st);  // ... also on a failed build: the uploads before it are queued
    free_bvh(ctx->bvh);              // whatever the failed build had allocated: nothing of it is counted in ctx->bytes (ADVICE r04)
    return rc;
  }
  ctx->bytes.add(ctx->bvh.bytes);
  if (ctx->num_textures) {  // the collapse defines the slot order: the per-slot uv follow it
    CTX_TRY(ctx, ctx->tri_uv.ensure(8ull * (tree_slots(ctx->bvh) + 1), &ctx->bytes));
    if (ctx->total_tris) {
      hipLaunchKernelGGL(k_gather_uv, dim3((uint32_t)((ctx->total_tris + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, (uint32_t)ctx->total_tris,
                         ctx->bvh.first_slot, ctx->bvh.slot_to_global, ctx->d_first.p, bi.num_instances, ctx->d_inst.p, ctx->d_uv.p, ctx->tri_uv.p);
      CTX_TRY(ctx, hipGetLastError());
    }
  }
  CTX_TRY(ctx, hipStreamSynchronize(st));
  return ctx->ensure_spill();
}
// instance table (ctx->h_inst) -> device, transformInvT per instance, then the tree of the whole scene
static int bake_and_build(gsp_context* ctx) {
  BuildInput bi;
  int rc = upload_scene_instances(ctx, bi);
  return rc == GSP_OK ? build_whole_tree(ctx, bi) : rc;
}

// null arrays, instance ranges and handles, the triangle limit, texture / environment-map sizes: before any device work
static int check_scene(gsp_context* ctx, const gsp_scene_desc* sc, uint64_t* total_tris) {
  if ((sc->num_instances && !sc->instances) || (sc->num_vertices && (!sc->positions || !sc->normals)) ||
      (sc->num_lights && !sc->lights)) {
    ctx->err = "null array with non-zero count";
    return GSP_ERR_SCENE;
  }
  int rc = check_instances(ctx, sc->instances, sc->num_instances, sc->num_bsdfs, sc->num_vertices, total_tris);
  if (rc != GSP_OK) return rc;
  // the wide tree of n triangles has fewer than n nodes and the traversal's stack entry holds node indices below kMaxNodes
  // (pt_trace.h)
  if (*total_tris >= (uint64_t)kMaxNodes) {
    ctx->err = "too many triangles: " + std::to_string(*total_tris) + " (limit 2^25 - 1 = 33 554 431)";
    return GSP_ERR_SCENE;
  }
  // dormant-feature extension: textures / environment map
  if (sc->num_textures != 0) {
    if (!sc->textures || !sc->texels || (sc->num_vertices && !sc->uvs)) {
      ctx->err = "textures need the textures, texels and uvs arrays";
      return GSP_ERR_SCENE;
    }
    for (uint32_t k = 0; k < sc->num_textures; ++k) {
      const gsp_texture& t = sc->textures[k];
      if (t.width == 0 || t.height == 0 || t.width > (1u << 15) || t.height > (1u << 15) ||
          t.first_texel + (uint64_t)t.width * t.height > sc->num_texels) {
        ctx->err = "texture " + std::to_string(k) + ": size 0, above 32768 or outside the texel array";
        return GSP_ERR_SCENE;
      }
    }
    rc = check_texture_words(ctx, sc, sc->num_textures);
    if (rc != GSP_OK) return rc;
  }
  if (sc->envmap.texels && (sc->envmap.width == 0 || sc->envmap.height == 0 || sc->envmap.width > (1u << 15) || sc->envmap.height > (1u << 15))) {
    ctx->err = "environment map: size 0 or above 32768";
    return GSP_ERR_SCENE;
  }
  return GSP_OK;
}
// dormant-feature extension: texel arrays, uv, environment map
static int upload_textures(gsp_context* ctx, const gsp_scene_desc* sc) {
  hipStream_t st = ctx->stream;
  const bool want_tex = sc->num_textures != 0, want_env = sc->envmap.texels != nullptr;
  ctx->textured = want_tex || want_env;
  ctx->num_textures = want_tex ? sc->num_textures : 0;
  ctx->env_width = want_env ? sc->envmap.width : 0;
  ctx->env_height = want_env ? sc->envmap.height : 0;
  if (want_tex) {
    float decode[256];
    for (int b = 0; b < 256; ++b) decode[b] = sc->texel_decode ? sc->texel_decode[b] : (float)b / 255.0f;
    CTX_TRY(ctx, ctx->texel_decode.upload(decode, 256, st, &ctx->bytes));
    CTX_TRY(ctx, ctx->textures.upload(sc->textures, sc->num_textures, st, &ctx->bytes));
    CTX_TRY(ctx, ctx->texels.upload(sc->texels, sc->num_texels, st, &ctx->bytes));
    CTX_TRY(ctx, ctx->d_uv.upload(sc->uvs, 2ull * sc->num_vertices, st, &ctx->bytes));
    CTX_TRY(ctx, hipStreamSynchronize(st));  // `decode` is a stack array
  }
  if (want_env) {
    CTX_TRY(ctx, ctx->env_texels.upload(sc->envmap.texels, 4ull * sc->envmap.width * sc->envmap.height, st, &ctx->bytes));
    for (int k = 0; k < 16; ++k) ctx->env_to_local[k] = sc->envmap.to_local[k];
  }
  return GSP_OK;
}

// The environment light's scene state (include/gpuspectral_pt.h, "Environment light") from the map's texels on the host: the cell
// table (host copy and device), the radiant sum of the power weight, the frame.  The caller has checked the frame
static int build_env_light(gsp_context* ctx, const float* texels, uint32_t width, uint32_t height, const float* to_local) {
  const std::vector<double> w = env_cell_weights(texels, width, height, ctx->env_cw, ctx->env_ch);
  ctx->h_env_cells.assign(w.size(), gsp_light_pick{});
  build_light_pick_from_weights(w.data(), (uint32_t)w.size(), ctx->h_env_cells.data());
  ctx->env_radiant = env_radiant_sum(texels, width, height);
  for (int k = 0; k < 16; ++k) ctx->env_light_to_local[k] = to_local[k];
  CTX_TRY(ctx, ctx->env_cells.upload(ctx->h_env_cells.data(), ctx->h_env_cells.size(), ctx->stream, &ctx->bytes));  // (h_env_cells stays alive)
  return GSP_OK;
}

int gsp_upload_scene(gsp_context* ctx, const gsp_scene_desc* sc) {
  if (!ctx || !sc) return GSP_ERR_INVALID;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  int rc = pipeline_drain(ctx);
  if (rc != GSP_OK) return rc;
  ctx->have_scene = false;
  ctx->tp_valid = false;  // (temporal accumulation: a new scene has no history)
  ctx->tp_xforms.clear();
  invalidate_memos(ctx);
  ctx->geo_ring_failed = false;
  ctx->inst_dynamic.clear();
  ctx->split_declined = false;
  uint64_t total_tris = 0;
  rc = check_scene(ctx, sc, &total_tris);
  if (rc != GSP_OK) return rc;
  auto t0 = std::chrono::steady_clock::now();
  // the bounds the light grid covers: the geometry as uploaded.  Formed at every upload (one pass over the vertices on the host,
  // small against the BVH build): gsp_set_light_grid may come later, when the positions are resident on the device only
  ctx->scene_has_bounds = lightgrid_scene_bounds(sc, ctx->scene_lo, ctx->scene_hi);
  // the environment light: on for this scene when the switch is and the scene has a map; its record goes into the tables below
  ctx->env_light = false;
  ctx->h_env_cells.clear();
  if (ctx->env_sampling.enabled != 0u && sc->envmap.texels != nullptr) {
    if (!env_frame_is_rotation(sc->envmap.to_local)) {
      ctx->err = "environment map: envmap sampling is on and the upper 3x3 of to_local is not orthonormal within 1e-4";
      return GSP_ERR_SCENE;
    }
    rc = build_env_light(ctx, sc->envmap.texels, sc->envmap.width, sc->envmap.height, sc->envmap.to_local);
    if (rc != GSP_OK) return rc;
    ctx->env_light = true;
  }
  {
    TableImage img;
    rc = pack_tables(ctx, sc, img);
    if (rc == GSP_OK) rc = upload_tables(ctx, sc, img);
    if (rc != GSP_OK) return rc;
  }
  ctx->camera = sc->camera;
  // ---- resident geometry (the "BLAS inputs": object-space vertices; Mesh.cpp:7-51) ----
  CTX_TRY(ctx, ctx->d_pos.upload(sc->positions, 3ull * sc->num_vertices, ctx->stream, &ctx->bytes));
  CTX_TRY(ctx, ctx->d_nrm.upload(sc->normals, 3ull * sc->num_vertices, ctx->stream, &ctx->bytes));
  ctx->num_vertices = sc->num_vertices;
  ctx->total_tris = total_tris;
  ctx->h_inst.assign(sc->instances, sc->instances + sc->num_instances);
  rc = upload_textures(ctx, sc);
  if (rc == GSP_OK) rc = bake_and_build(ctx);
  if (rc != GSP_OK) return rc;
  ctx->bvh_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  ctx->stats.scene_updates = 0;
  ctx->stats.scene_refits = 0;
  ctx->stats.scene_drains = 0;
  ctx->stats.scene_splits = 0;
  ctx->have_scene = true;
  return GSP_OK;
}

// common head of the gsp_update_* calls.  (The drain -- the samples already queued belong to the scene as it was -- comes only
// once the call has found something to change: a host that mirrors the reference calls all three every frame.)
static int begin_update(gsp_context* ctx, const char* what) {
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->have_scene) {
    ctx->err = std::string(what) + " needs gsp_upload_scene first";
    return GSP_ERR_INVALID;
  }
  return GSP_OK;
}

// No drain: a path in flight left the camera behind when its primary ray was generated (k_generate / the memo are the only
// readers of it, and gsp_render returns only after every sample of the call has been generated), so the samples queued so far
// finish as what they are -- samples through the old camera -- while the next gsp_render generates through the new one; they
// are folded in timestamp order either way.  A viewer that moves its camera every frame keeps the path pool full
// (profiles/r04_update_latency.txt: 500x500, one sample per frame).
int gsp_update_camera(gsp_context* ctx, const gsp_camera* camera) {
  if (!ctx || !camera) return GSP_ERR_INVALID;
  int rc = begin_update(ctx, "gsp_update_camera");
  if (rc != GSP_OK) return rc;
  if (std::memcmp(&ctx->camera, camera, sizeof(gsp_camera)) == 0) return GSP_OK;
  ctx->camera = *camera;  // (render_consts reads it at the next gsp_render)
  invalidate_memos(ctx);  // the memo holds the hits of the OLD camera rays
  ++ctx->stats.scene_updates;
  return GSP_OK;
}

// ---- gsp_update_instances ---------------------------------------------------------------------------------------------------
// An edit that changes something is offered to three arms in the order pt_versions.h documents -- (1) refit of the edited tree,
// (2) split / re-split, (3) the whole tree -- each of which waits for what it must (drain_for_edit), opens the edit (begin_edit),
// and either commits (*committed = true) or leaves it to the next arm.
struct InstanceEdit {
  const gsp_instance* instances;
  uint32_t n;
  bool only_edited;  // it touches only instances that already live in the edited instances' tree of a split scene
  std::chrono::steady_clock::time_point t0;
  bool changes(const gsp_context* ctx, uint32_t i) const { return std::memcmp(&instances[i], &ctx->h_inst[i], sizeof(gsp_instance)) != 0; }
};
// From here until gsp_update_instances commits, the context has no scene (a failed rebuild leaves no half-built tree in use), the
// memos are stale and the clock of bvh_build_ms runs (the wait before it is not build time).  adopt: the new table becomes h_inst.
static void begin_edit(gsp_context* ctx, InstanceEdit& e, bool adopt = true) {
  e.t0 = std::chrono::steady_clock::now();
  ctx->have_scene = false;
  invalidate_memos(ctx);
  if (adopt) ctx->h_inst.assign(e.instances, e.instances + e.n);
}

// Refit tree T (the edited instances' tree of a split scene, or the whole tree) to the instance tables of `bi` as version v.
// v == geo.ver: in place (nothing in flight reads it).  v == geo.ver + 1: into the next slot of the ring -- the topology (child
// links, triangle ranges) of the current version is copied there and refit_bvh rewrites every box and packet.  T points at v
// afterwards: the CALLER commits (geo.ver = v) or, when *growth says the tree has degraded, points T back.  On failure T points
// at the committed version again.
static int refit_tree_into(gsp_context* ctx, DeviceBvh& T, const BuildInput& bi, uint32_t v, double* growth) {
  hipStream_t st = ctx->stream;
  hipError_t e = hipSuccess;
  if (v != ctx->geo.ver) {
    const q4* from = T.nodes;
    point_tree_at(ctx, T, v);
    e = hipMemcpyAsync(T.nodes, from, (size_t)T.num_nodes * kNodeBytes, hipMemcpyDeviceToDevice, st);
  }
  int rc = GSP_ERR_DEVICE;
  if (e == hipSuccess) {
    const size_t held = T.bytes;
    rc = refit_bvh(st, bi, T, growth, ctx->err);  // (synchronises the stream)
    ctx->bytes.add(T.bytes - held);               // (the first refit of a tree allocates its scratch)
  }
  if (rc != GSP_OK) {
    (void)hipStreamSynchronize(st);
    if (v != ctx->geo.ver) point_tree_at(ctx, T, ctx->geo.ver);
    if (e != hipSuccess) CTX_TRY(ctx, e);
  }
  return rc;
}

// (1) r05, split scene.  The host that edits while samples are in flight (a viewer) usually moves a few objects of many: the first
// such edit -- and every later one that touches an instance not edited before -- builds TWO trees, one over the instances that
// have never changed and one over the edited ones (make_split: behind a drain, two builds); from then on an edit of those
// instances refits the small tree only, into the next slot of its ring, and the versions in flight share the large one.
static int refit_edited_tree(gsp_context* ctx, InstanceEdit& e, bool* committed) {
  if (!ctx->split || !e.only_edited) return GSP_OK;
  const bool in_slot = edited_tree_refit_needs_no_wait(ctx->pipe_active, ctx->caps_allow_versions(), ctx->geo, ctx->oldest_live_geo());
  int rc = in_slot ? GSP_OK : drain_for_edit(ctx);
  if (rc != GSP_OK) return rc;
  begin_edit(ctx, e);
  BuildInput bi;
  rc = upload_subset(ctx, 1, bi);
  if (rc != GSP_OK) return rc;
  double growth = 0.0;
  rc = refit_tree_into(ctx, ctx->dyn, bi, ctx->geo.ver + (in_slot ? 1 : 0), &growth);
  if (rc != GSP_OK) return rc;
  if (growth > ctx->opt.refit_growth) {  // the edited tree has degraded: both trees are built again by (2), behind a drain
    point_tree_at(ctx, ctx->dyn, ctx->geo.ver);
    return GSP_OK;
  }
  if (in_slot) ++ctx->geo.ver;
  ++ctx->stats.scene_refits;
  *committed = true;
  return GSP_OK;
}

// (2) the edit asks for a split: a first one, or a re-split because it touches an instance not edited before (or because the
// edited tree has degraded).
static int split_scene(gsp_context* ctx, InstanceEdit& e, bool* committed) {
  if (!edit_wants_split(ctx->split, ctx->split_declined, ctx->pipe_active, ctx->opt.refit_growth, ctx->opt.geometry_versions, ctx->num_textures)) return GSP_OK;
  // The FIRST split needs no wait: the edited instances' tree is built where they WERE (version 0: with the static tree it is,
  // triangle for triangle, the scene the samples in flight were generated under -- they carry stamp 0 -- and the hit records
  // the memo has handed out name slots of the static tree whose shading packets stay), and the edit itself is version 1, a
  // refit into the next slot like every later one.  Nothing is queued between two gsp_render calls, so the arrays can change hands.
  const bool no_wait = first_split_needs_no_wait(ctx->split, ctx->pipe_active, ctx->caps_allow_versions(), ctx->geo);
  int rc = no_wait ? GSP_OK : drain_for_edit(ctx);
  if (rc != GSP_OK) return rc;
  // (the instances count as edited from the edit that is OFFERED a split: one that arrives with nothing in flight on a scene in
  // one tree goes to (3) and marks nothing)
  for (uint32_t i = 0; i < e.n; ++i)
    if (e.changes(ctx, i)) ctx->inst_dynamic[i] = 1;
  begin_edit(ctx, e, !no_wait);
  bool made = false;
  rc = make_split(ctx, &made);
  if (rc != GSP_OK && rc != GSP_ERR_NOMEM) return rc;
  if (made && no_wait) {
    ctx->h_inst.assign(e.instances, e.instances + e.n);
    BuildInput bi;
    rc = upload_subset(ctx, 1, bi);
    if (rc != GSP_OK) return rc;
    double growth = 0.0;
    rc = refit_tree_into(ctx, ctx->dyn, bi, 1, &growth);
    if (rc != GSP_OK) return rc;
    if (growth <= ctx->opt.refit_growth) {
      ctx->geo.ver = 1;
    } else {  // the object has moved far in one step: the small tree is built where it IS, behind a wait after all
      point_tree_at(ctx, ctx->dyn, 0);
      rc = drain_for_edit(ctx);
      if (rc != GSP_OK) return rc;
      rc = make_split(ctx, &made);
      if (rc != GSP_OK && rc != GSP_ERR_NOMEM) return rc;
    }
  }
  if (!made) {
    // no split to be had (too much of the scene is being edited, textures, no memory): the scene stays / becomes ONE tree with the
    // ring of whole trees -- (3), with the pipeline idle now -- and the question is not asked again for this scene
    ctx->split_declined = true;
    ctx->have_scene = true;
    return GSP_OK;
  }
  ++ctx->stats.scene_splits;
  *committed = true;
  return GSP_OK;
}

// (3) the whole tree.  r05: NO DRAIN when the tree has its geometry ring and a slot of it is free: the refit -- re-bake of every
// packet, node boxes bottom-up in the existing topology -- goes into the NEXT slot, on the context's stream, while the lanes'
// streams finish the samples in flight in the slots they were generated under (a path carries its slot in its flags word,
// pt_stages.h); the next gsp_render stamps its samples with the new one.  Otherwise -- first edit of this tree (the ring is made
// then), as many edits as the ring has slots within the life of one sample, a tree that degrades and is rebuilt -- the queued
// samples finish first, as until r04.  The tree keeps its topology if its boxes stay within gsp_ctx_options.refit_growth of what
// they were after the last full build (a split scene goes back to one tree by a build).
static int edit_whole_tree(gsp_context* ctx, InstanceEdit& e, bool* committed) {
  const bool in_ring = whole_tree_refit_needs_no_wait(ctx->pipe_active, ctx->caps_allow_versions(), ctx->opt.refit_growth, ctx->geo, ctx->oldest_live_geo());
  int rc = in_ring ? GSP_OK : drain_for_edit(ctx);
  if (rc != GSP_OK) return rc;
  // (the ring of WHOLE trees only where a split scene is not to be had: an edit that arrives with nothing in flight refits in
  // place, and the first one that arrives with samples in flight asks for the split first, (2))
  if (!in_ring && ctx->opt.refit_growth > 1.0 && !scene_may_still_split(ctx->split_declined, ctx->opt.geometry_versions, ctx->num_textures)) {
    rc = make_geo_ring(ctx);
    if (rc != GSP_OK) return rc;
  }
  begin_edit(ctx, e);
  BuildInput bi;
  rc = upload_scene_instances(ctx, bi);
  if (rc != GSP_OK) return rc;
  bool refitted = false;
  if (!ctx->split && ctx->opt.refit_growth > 1.0 && ctx->bvh.nodes && ctx->bvh.num_tris == bi.num_tris && bi.num_tris > 0) {
    double growth = 0.0;
    rc = refit_tree_into(ctx, ctx->bvh, bi, ctx->geo.ver + (in_ring ? 1 : 0), &growth);
    if (rc != GSP_OK) return rc;
    refitted = growth <= ctx->opt.refit_growth;  // (per-slot uv of a textured scene: the slot order has not changed)
  }
  if (refitted) {
    if (in_ring) ++ctx->geo.ver;
    ++ctx->stats.scene_refits;
  } else {  // (the tree is rebuilt behind a drain and owns its arrays again)
    rc = build_whole_tree(ctx, bi);
    if (rc != GSP_OK) return rc;
  }
  *committed = true;
  return GSP_OK;
}

int gsp_update_instances(gsp_context* ctx, const gsp_instance* instances, uint32_t num_instances) {
  if (!ctx || (!instances && num_instances)) return GSP_ERR_INVALID;
  int rc = begin_update(ctx, "gsp_update_instances");
  if (rc != GSP_OK) return rc;
  if (num_instances != ctx->h_inst.size()) {
    ctx->err = "gsp_update_instances: " + std::to_string(num_instances) + " instances, the uploaded scene has " +
               std::to_string(ctx->h_inst.size()) + " (a different object list needs gsp_upload_scene)";
    return GSP_ERR_SCENE;
  }
  for (uint32_t i = 0; i < num_instances; ++i)
    if (instances[i].first_vertex != ctx->h_inst[i].first_vertex || instances[i].vertex_count != ctx->h_inst[i].vertex_count) {
      ctx->err = "gsp_update_instances: instance " + std::to_string(i) + " names another vertex range than the uploaded one (a different mesh needs gsp_upload_scene)";
      return GSP_ERR_SCENE;
    }
  rc = check_instances(ctx, instances, num_instances, ctx->num_bsdfs, ctx->num_vertices, nullptr);
  if (rc != GSP_OK) return rc;
  if (num_instances == 0 || std::memcmp(ctx->h_inst.data(), instances, num_instances * sizeof(gsp_instance)) == 0) return GSP_OK;
  ++ctx->inst_edits;  // (gsp_temporal_follow_instances: the frame's features belong to the transforms before this edit)
  if (ctx->inst_dynamic.size() != num_instances) ctx->inst_dynamic.assign(num_instances, 0);
  InstanceEdit e{instances, num_instances, ctx->split, {}};
  for (uint32_t i = 0; i < num_instances; ++i)
    if (e.changes(ctx, i) && !ctx->inst_dynamic[i]) e.only_edited = false;
  bool committed = false;
  rc = refit_edited_tree(ctx, e, &committed);
  if (rc == GSP_OK && !committed) rc = split_scene(ctx, e, &committed);
  if (rc == GSP_OK && !committed) rc = edit_whole_tree(ctx, e, &committed);
  if (rc != GSP_OK) return rc;
  ctx->bvh_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - e.t0).count();
  ctx->have_scene = true;
  ++ctx->stats.scene_updates;
  return GSP_OK;
}

int gsp_update_tables(gsp_context* ctx, const gsp_scene_desc* sc) {
  if (!ctx || !sc) return GSP_ERR_INVALID;
  int rc = begin_update(ctx, "gsp_update_tables");
  if (rc != GSP_OK) return rc;
  if (sc->num_lights && !sc->lights) {
    ctx->err = "null array with non-zero count";
    return GSP_ERR_SCENE;
  }
  rc = check_instances(ctx, ctx->h_inst.data(), (uint32_t)ctx->h_inst.size(), sc->num_bsdfs, ctx->num_vertices, nullptr);
  if (rc != GSP_OK) {
    ctx->err = "gsp_update_tables: the new tables leave a resident " + ctx->err;
    return rc;
  }
  rc = check_texture_words(ctx, sc, ctx->num_textures);
  if (rc != GSP_OK) return rc;
  TableImage img;
  rc = pack_tables(ctx, sc, img);
  if (rc != GSP_OK) return rc;
  if (img.bytes == ctx->h_tables) return GSP_OK;  // same counts, same bytes: nothing to do, nothing to wait for
  // r05: NO DRAIN when the new tables have the layout of the resident ones (same record counts: an edited colour, IOR, radiance
  // -- what a per-frame edit is) and the version ring has a free slot: the samples in flight carry their version in the path
  // flags and finish on the tables they started with, the next gsp_render generates under the new version.  (PathTracer.cpp:74-87
  // re-reads the tables every frame; a host that edits a material every frame keeps the path pool full now,
  // profiles/r05_update_latency.txt.)  Otherwise -- another layout, or kTableVersions edits within the life of one sample --
  // the queued samples finish first, as until r04.
  bool same_layout = ctx->pipe_active && sc->num_lights == ctx->num_tri_lights && sc->num_lights + ctx->h_delta.size() + (ctx->env_light ? 1u : 0u) == ctx->num_lights && img.total == ctx->tables_bytes && ctx->tables.p != nullptr;
  for (int k = 0; k < GSP_BSDF_TYPE_COUNT && same_layout; ++k) same_layout = sc->num_bsdfs[k] == ctx->num_bsdfs[k];
  size_t free_b = 0, total_b = 0;
  if (same_layout && ctx->tab.slots == 1) CTX_TRY(ctx, hipMemGetInfo(&free_b, &total_b));  // (only the decision to grow asks)
  TableRing::Update how = ctx->tab.decide(ctx->pipe_active, same_layout, ctx->caps_allow_versions(), ctx->oldest_live_version(), free_b);
  if (how == TableRing::Update::kGrowThenInPlace) {
    rc = grow_table_ring(ctx, TableRing::slots_for(ctx->tab.slot_bytes, TableRing::budget_for(free_b)));
    if (rc != GSP_OK) return rc;
    how = ctx->tab.slots > 1 ? TableRing::Update::kInPlace : TableRing::Update::kDrain;  // (no memory for it: wait, as until r04)
  }
  const bool in_place = how == TableRing::Update::kInPlace;
  if (!in_place) {
    rc = drain_for_edit(ctx);
    if (rc != GSP_OK) return rc;
  }
  rc = upload_tables(ctx, sc, img, in_place);  // (k_shade stages the tables per launch: nothing else holds a copy)
  if (rc != GSP_OK) {
    ctx->have_scene = false;
    return rc;
  }
  CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ++ctx->stats.scene_updates;
  return GSP_OK;
}

int gsp_frame_begin(gsp_context* ctx, uint32_t width, uint32_t height, const uint32_t* pixel_ids,
                    uint64_t num_pixels) {
  if (!ctx || width == 0 || height == 0) return GSP_ERR_INVALID;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  {
    int rc_ = pipeline_drain(ctx);
    if (rc_ != GSP_OK) return rc_;
  }
  const uint64_t frame = (uint64_t)width * height;
  if (frame >= (1ull << 32)) {
    ctx->err = "frame too large";
    return GSP_ERR_INVALID;
  }
  ctx->have_frame = false;
  invalidate_memos(ctx);
  for (gsp_context::Lane& L : ctx->lanes) {
    L.adaptive = false;  // (the next gsp_render decides whether the new frame is adaptive)
    L.num_active = 0;
  }
  ctx->frame_mode = gsp_context::kFrameUndecided;
  ctx->adaptive_n = 0;
  ctx->features_rendered = false;
  ctx->tp_done = false;
  if (width != ctx->tp_width || height != ctx->tp_height) ctx->tp_valid = false;  // (the history is of another size)
  ctx->features_ready = false;  // (the feature planes, where a frame has asked for them, start from zero again)
  ctx->subset = pixel_ids != nullptr;
  if (pixel_ids) {
    for (uint64_t i = 0; i < num_pixels; ++i) {
      if (pixel_ids[i] >= frame || (i && pixel_ids[i] <= pixel_ids[i - 1])) {
        ctx->err = "pixel_ids must be strictly increasing and inside the frame";
        return GSP_ERR_INVALID;
      }
    }
    ctx->pixel_ids_host.assign(pixel_ids, pixel_ids + num_pixels);
    CTX_TRY(ctx, ctx->pixel_ids.upload(pixel_ids, num_pixels, ctx->stream, &ctx->bytes));
  } else {
    num_pixels = frame;
    ctx->pixel_ids_host.clear();
  }
  ctx->width = width;
  ctx->height = height;
  ctx->num_pixels = num_pixels;
  for (uint32_t l = 0; l < ctx->num_lanes; ++l)
    ctx->lanes[l].num_pixels = (num_pixels + ctx->num_lanes - 1 - l) / ctx->num_lanes;  // owned pixels lp with lp % lanes == l
  CTX_TRY(ctx, ctx->accum.ensure(num_pixels, &ctx->bytes));
  if (num_pixels * sizeof(q4) > gsp_context::kStageBytes / 4) {
    int rc_ = ensure_read_back_stage(ctx);
    if (rc_ != GSP_OK) return rc_;
  }
  CTX_TRY(ctx, hipMemsetAsync(ctx->accum.p, 0, std::max<uint64_t>(num_pixels, 1) * sizeof(q4), ctx->stream));
  CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->h_stage[0] && !ctx->stage_warm) {
    // the first device-to-host copy into a new pinned buffer and the host's first read of it cost ~8 ms (measured: 9-10 ms for the
    // first gsp_download of a context, 1.3 ms for every later one); paid here, with the frame's other one-time set-up
    const size_t nb = std::min<size_t>(gsp_context::kStageBytes, num_pixels * sizeof(q4));
    for (int k = 0; k < 2; ++k) CTX_TRY(ctx, hipMemcpyAsync(ctx->h_stage[k], ctx->accum.p, nb, hipMemcpyDeviceToHost, ctx->stream));
    CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));
    unsigned sum = 0;
    for (int k = 0; k < 2; ++k)
      for (size_t b = 0; b < nb; b += 4096) sum += ((volatile uint8_t*)ctx->h_stage[k])[b];
    (void)sum;
    ctx->stage_warm = true;
  }
  ctx->folded_idle = 0;
  ctx->sample_base = 0;
  ctx->have_frame = true;
  return GSP_OK;
}
