// pt_render_pipeline.inc -- part of the translation unit pt_render.hip (included there; not compiled on its own).
// The streaming path pool: ensure_pool, one launcher per kernel family, lane_enqueue / lane_collect (one iteration = extend, shade,
// connect over the queues), pipeline_run; gsp_render, gsp_sync, the read-back calls, statistics, gsp_trace.  (Continues the extern "C" block.)  The LDR film,
// the denoiser, temporal accumulation and its filters are in pt_render_post.inc, included in front of gsp_debug_visit_histograms.

static int ensure_pool(gsp_context* ctx, gsp_context::Lane& L, uint64_t cap, uint64_t result_entries) {
  if (result_entries > L.result_cap) {
    CTX_TRY(ctx, L.result.ensure(result_entries, &ctx->bytes));
    L.result_cap = result_entries;
  }
  if (!L.counters.p) {
    CTX_TRY(ctx, L.counters.ensure(C_COUNT, &ctx->bytes));
    CTX_TRY(ctx, hipMemsetAsync(L.counters.p, 0, C_COUNT * sizeof(uint32_t), L.stream));
  }
  if (!ctx->dstats.p) {
    CTX_TRY(ctx, ctx->dstats.ensure(1, &ctx->bytes));
    CTX_TRY(ctx, hipMemsetAsync(ctx->dstats.p, 0, sizeof(DevStats), ctx->stream));
    CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (cap <= L.pool_cap) return GSP_OK;
  for (int k = 0; k < 2; ++k) {
    CTX_TRY(ctx, L.P0[k].ensure(cap, &ctx->bytes));
    CTX_TRY(ctx, L.P1[k].ensure(cap, &ctx->bytes));
    CTX_TRY(ctx, L.P2[k].ensure(cap, &ctx->bytes));
    CTX_TRY(ctx, L.P3[k].ensure(cap, &ctx->bytes));
  }
  CTX_TRY(ctx, L.hits[0].ensure(cap, &ctx->bytes));
  CTX_TRY(ctx, L.hits[1].ensure(cap, &ctx->bytes));
  CTX_TRY(ctx, L.S0.ensure(cap, &ctx->bytes));
  CTX_TRY(ctx, L.S1.ensure(cap, &ctx->bytes));
  CTX_TRY(ctx, L.S3.ensure(cap, &ctx->bytes));
  L.pool_cap = cap;
  return GSP_OK;
}

static RenderConstsLens render_consts(const gsp_context* ctx, const gsp_render_params* rp) {
  RenderConstsLens rcst;
  rcst.width = ctx->width;
  rcst.height = ctx->height;
  rcst.max_depth = rp->max_depth;
  rcst.rr_start_depth = rp->rr_start_depth;
  rcst.clamp = rp->clamp;
  rcst.nee = rp->disable_nee != 0 ? 0u : 1u;
  // raygen.rgen:22, tan() evaluated once on the host
  rcst.zplane = (std::max((float)ctx->width, (float)ctx->height) / 2.0f) / tanf(ctx->camera.fov / 2.0f);
  for (int i = 0; i < 16; ++i) rcst.cam_to_world[i] = ctx->camera.to_world[i];
  rcst.cam_origin[0] = ctx->camera.to_world[12];  // Camera::getPosition, Camera.cpp:41-45
  rcst.cam_origin[1] = ctx->camera.to_world[13];
  rcst.cam_origin[2] = ctx->camera.to_world[14];
  // pixel filter: the id and the parameter with its default resolved (include/gpuspectral_pt.h)
  rcst.pixel_filter = rp->pixel_filter;
  rcst.pixel_filter_param = rp->pixel_filter == GSP_FILTER_TENT       ? (rp->pixel_filter_param != 0.0f ? rp->pixel_filter_param : 1.0f)
                            : rp->pixel_filter == GSP_FILTER_GAUSSIAN ? (rp->pixel_filter_param != 0.0f ? rp->pixel_filter_param : 0.5f)
                                                                      : 0.0f;
  set_lens_consts(rcst, ctx->lens);  // thin lens (gsp_set_lens)
  return rcst;
}
static RenderConstsLens render_consts(const gsp_context* ctx) { return render_consts(ctx, &ctx->pipe_params); }  // the running pipeline's

#ifndef GSP_PIPE_DEPTH
#define GSP_PIPE_DEPTH 2  // iterations queued ahead of the host's view of the counters (1 = wait for every read-back)
#endif
constexpr uint32_t kPipeDepth = GSP_PIPE_DEPTH;
static_assert(kPipeDepth >= 1 && kPipeDepth <= 2, "two tail sets / read-back buffers");
#ifndef GSP_ROOM_CHUNK
#define GSP_ROOM_CHUNK 1024  // the largest chunk k_shade takes its room in the output queues in (shade_room_chunk)
#endif

// ---- the launchers: one per kernel family, each with the rule that picks the instantiation ------------------------------------
extern "C++" {
struct LiveVersions {  // what an iteration settles about the versions in flight before it queues anything (settle_versions)
  bool multi_version;     // the <VER> kernels run: samples of several table or geometry versions are in flight, or the scene is split
  SceneView vview;        // ... and this is the view they read: slot 0 of the rings + the strides.  The plain view otherwise
  GeoRing gring;          // the geometry ring as the Split / Ver records of k_trace carry it
  uint32_t gen_ver_bits;  // version fields in the flags word of the paths generated now (0 unless an edit is in flight)
  uint32_t gen_stamp;     // geometry stamp of the newest version: the rays of the memo and of gsp_trace belong to it
};

// The ray sources of k_trace.  kHit: the closest hit, any hit, or whichever the caller of gsp_trace asked for (TestIO::any_hit).  Split / Ver:
// the record the kernel takes in place of the base IO on a split scene / while several geometry versions are in flight.  The rays of the memo and
// of gsp_trace are no paths in flight: all belong to the newest version, so no Ver record (void), its stamp in Split, no statistics pass.
enum class Hit { kClosest, kAny, kAsked };
template <class IO> struct TraceSource;
template <> struct TraceSource<ExtendIO> { static constexpr Hit kHit = Hit::kClosest; typedef ExtendSplitIO Split; typedef ExtendVerIO Ver; };
template <> struct TraceSource<ConnectIO> { static constexpr Hit kHit = Hit::kAny; typedef ConnectSplitIO Split; typedef ConnectVerIO Ver; };
template <> struct TraceSource<ConnectTextbookIO> { static constexpr Hit kHit = Hit::kAny; typedef ConnectTextbookVerIOT<true> Split; typedef ConnectTextbookVerIOT<false> Ver; };
template <> struct TraceSource<MemoIO> { static constexpr Hit kHit = Hit::kClosest; typedef MemoSplitIO Split; typedef void Ver; };
template <> struct TraceSource<TestIO> { static constexpr Hit kHit = Hit::kAsked; typedef TestSplitIO Split; typedef void Ver; };

// k_trace<ANY, STATS, record>, the one launch of every traversal.  The rule, in this order: a split scene takes the source's Split
// record; several versions in flight its Ver record; a statistics pass the plain record with STATS = true; everything else the
// plain record.  The first two walk V.vview with STATS = false whatever `stats` says: the statistics instantiations know ONE tree of
// ONE version, which is why render_enqueue joins a split scene and drains older versions before a statistics pass.  The rays: *n_ptr
// entries of a queue from entry `first` on (`bound`: what the host knows of that size, for the grid), or [0, n).
template <class IO>
static void launch_trace(const gsp_context* ctx, hipStream_t st, const SceneView& view, const LiveVersions& V, bool stats, const IO& io,
                         const uint32_t* n_ptr, uint32_t n, uint32_t first, uint64_t bound, uint32_t chunk, uint32_t* work, uint32_t* spill,
                         const TraceStatsOut& so) {
  // GSP_ESTIMATOR_TEXTBOOK: the shadow rays take the any-hit sources whose occluded commit leaves P2.w (lastPdf) alone
  if constexpr (std::is_same<IO, ConnectIO>::value) {
    if (ctx->estimator == GSP_ESTIMATOR_TEXTBOOK) {
      ConnectTextbookIO tio;
      static_cast<ConnectIO&>(tio) = io;
      return launch_trace(ctx, st, view, V, stats, tio, n_ptr, n, first, bound, chunk, work, spill, so);
    }
  }
  typedef TraceSource<IO> S;
  constexpr bool in_flight = !std::is_void<typename S::Ver>::value;  // the rays are paths in flight: each carries its own stamp
  const auto launch = [&](auto ANY, auto STATS, const SceneView& v, const auto& record) {
    hipLaunchKernelGGL((k_trace<decltype(ANY)::value, decltype(STATS)::value, typename std::decay<decltype(record)>::type>),
                       dim3(ctx->trace_grid(bound, chunk, decltype(ANY)::value)), dim3(kTraceBlock), 0, st, v.nodes, v.tri_isect, n_ptr, n, first, chunk,
                       record, work, spill, ctx->spill_stride, so);
  };
  const auto with_hit_rule = [&](auto STATS, const SceneView& v, const auto& record) {
    if constexpr (S::kHit != Hit::kAsked) launch(std::integral_constant<bool, S::kHit == Hit::kAny>{}, STATS, v, record);
    else if (io.any_hit) launch(std::true_type{}, STATS, v, record);
    else launch(std::false_type{}, STATS, v, record);
  };
  if constexpr (in_flight) {
    if (ctx->split) return with_hit_rule(std::false_type{}, V.vview, typename S::Split{io, V.gring});
    if (V.multi_version) return with_hit_rule(std::false_type{}, V.vview, typename S::Ver{io, V.gring});
    if (stats) return with_hit_rule(std::true_type{}, view, io);
  } else if (ctx->split) {
    return with_hit_rule(std::false_type{}, V.vview, typename S::Split{io, V.gring, V.gen_stamp});
  }
  with_hit_rule(std::false_type{}, view, io);
}

// k_shade / k_finish <TEX, VER, MED, LSEL, EST = false>: TEX = the scene has textures or an environment map, VER = V.multi_version, MED = the context
// holds interior media (gsp_set_media), LSEL = it picks its light by emitted power (gsp_set_light_sampling); launch(TEX, VER, MED, LSEL, view)
// gets them as std::integral_constant values (as atrous_level, pt_render_post.inc).  These kernels read V.vview -- the versioned view
// exactly when VER -- and the <MED> ones the table behind it.
template <class Launch>
static void tex_ver_med_kernel(const gsp_context* ctx, const LiveVersions& V, Launch&& launch) {
  const auto with_view = [&](auto TEX, auto VER, auto LSEL) {
    if (ctx->num_media != 0) {
      SceneViewMed mv;
      static_cast<SceneView&>(mv) = V.vview;
      mv.media = ctx->media.p;
      launch(TEX, VER, std::true_type{}, LSEL, mv);
    } else {
      launch(TEX, VER, std::false_type{}, LSEL, V.vview);
    }
  };
  const auto with_pick = [&](auto TEX, auto VER) {
    if (ctx->light_mode == GSP_LIGHTS_POWER) with_view(TEX, VER, std::true_type{});
    else with_view(TEX, VER, std::false_type{});
  };
  if (V.multi_version && ctx->textured) with_pick(std::true_type{}, std::true_type{});
  else if (V.multi_version) with_pick(std::false_type{}, std::true_type{});
  else if (ctx->textured) with_pick(std::true_type{}, std::false_type{});
  else with_pick(std::false_type{}, std::false_type{});
}
// ... and <.., EST = true>, the kernels of a context that runs the textbook estimator (gsp_set_estimator): the same four flags, handed to
// the translation unit that holds those instantiations (pt_render_textbook.hip, launch_shade_textbook / launch_finish_textbook)
static TextbookLaunch textbook_launch(const gsp_context* ctx, const LiveVersions& V, const RenderConstsBase& rc, hipStream_t st, uint32_t blocks,
                                      const PathQueue& cur, q4* result, uint32_t* tails, uint32_t* live, uint32_t slot_paths) {
  TextbookLaunch a{};
  a.tex = ctx->textured;
  a.ver = V.multi_version;
  a.lsel = ctx->light_mode == GSP_LIGHTS_POWER;
  a.media = ctx->num_media != 0 ? ctx->media.p : nullptr;
  a.view = &V.vview;
  a.rc = &rc;
  a.stream = st;
  a.blocks = blocks;
  a.cur[0] = cur.P0, a.cur[1] = cur.P1, a.cur[2] = cur.P2, a.cur[3] = cur.P3;
  a.result = result;
  a.tails = tails;
  a.live = live;
  a.slot_paths = slot_paths;
  a.stats = ctx->dstats.p;
  return a;
}
// ... and <.., MED = true, .., SCT = true>, the kernels of a context whose media scatter (gsp_set_media_scattering, some sigma_s != 0):
// the same record + the scattering table and the estimator, handed to pt_render_scatter.hip
static ScatterLaunch scatter_launch(const gsp_context* ctx, const TextbookLaunch& t) {
  ScatterLaunch a{};
  static_cast<TextbookLaunch&>(a) = t;
  a.scatter = ctx->scatter.p;
  a.est = ctx->estimator == GSP_ESTIMATOR_TEXTBOOK;
  return a;
}
// ... and <.., DLT = true>, the kernels of a context that holds delta lights (gsp_set_delta_lights), handed to pt_render_delta.hip: the
// scattering record (the media tables null without media, the scattering table zeros where the media only absorb:
// sync_absorbing_scatter_table) + the number of triangle lights in front of the delta records
static DeltaLaunch delta_launch(const gsp_context* ctx, const TextbookLaunch& t) {
  DeltaLaunch a{};
  static_cast<ScatterLaunch&>(a) = scatter_launch(ctx, t);
  if (ctx->num_media == 0) a.scatter = nullptr;
  a.num_tri_lights = ctx->num_tri_lights;
  return a;
}
// ... and <.., ENV = true>, the kernels of a context that samples its environment map as a light (gsp_set_envmap_sampling with an envmap
// resident; always textured, always the textbook estimator), handed to pt_render_envlight.hip: the delta record + the cell table
static EnvLaunch env_launch(const gsp_context* ctx, const TextbookLaunch& t) {
  EnvLaunch a{};
  static_cast<DeltaLaunch&>(a) = delta_launch(ctx, t);
  a.env_cells = ctx->env_cells.p;
  return a;
}
// ... and <.., GRD = true>, the kernels of a context with a light grid resident (gsp_set_light_grid under the power pick and the textbook
// estimator, a scene with lights), handed to pt_render_lightgrid.hip: the delta record + where the grid sits inside a table version
static GridLaunch grid_launch(const gsp_context* ctx, const TextbookLaunch& t) {
  GridLaunch a{};
  static_cast<DeltaLaunch&>(a) = delta_launch(ctx, t);
  a.grid_off = (uint32_t)ctx->grid_off;
  return a;
}
}  // extern "C++"

// The blocks of k_shade a device holds at once: the largest grid (a block loops over tiles), each may leave one room chunk of fillers.
static uint64_t shade_resident_blocks(const gsp_context* ctx) { return (uint64_t)ctx->num_cus * GSP_SHADE_GRID_MULT * (GSP_SHADE_MINWAVES * 256 / kShadeBlock); }

// The six generate kernels: kb timestamps of the pixels the lane samples, appended to queue `q` at `offset`.  The rule: through a
// lens, else with a pixel filter, else the reference's pinhole ray; each over the lane's npix owned pixels or, in an adaptive frame,
// the wpix of its active list.  Only the two pinhole kernels copy the primary-hit memo: a filtered or lens sample's camera ray is its own.
static void launch_generate(const gsp_context* ctx, const gsp_context::Lane& L, const RenderConstsLens& rcst, uint32_t kb, uint32_t first_ts,
                            const PathQueue& q, q4* hits, uint32_t offset, uint32_t sid_base, bool use_memo, uint32_t ver_bits) {
  const bool filtered = rcst.pixel_filter != GSP_FILTER_NONE, lens = rcst.lens_radius > 0.0f;
  const uint32_t npix = (uint32_t)L.num_pixels, wpix = (uint32_t)L.work_pixels(), lane = L.index, lanes = ctx->num_lanes;
  const dim3 grid(ctx->grid_for((uint64_t)kb * wpix)), block(kBlock);
  const uint32_t *ids = ctx->subset ? ctx->pixel_ids.p : nullptr, *active = L.active[L.act].p;
  const q4 *const none = nullptr, *const memo = use_memo ? L.memo.p : none;
  hipStream_t st = L.stream;
  if (L.adaptive && lens)
    hipLaunchKernelGGL(k_generate_active_lens, grid, block, 0, st, rcst, wpix, kb, first_ts, ids, active, q, offset, sid_base, none, hits, lane, lanes, ver_bits);
  else if (lens)
    hipLaunchKernelGGL(k_generate_lens, grid, block, 0, st, rcst, npix, kb, first_ts, ids, q, offset, sid_base, none, hits, lane, lanes, ver_bits);
  else if (L.adaptive && filtered)
    hipLaunchKernelGGL(k_generate_active_filtered, grid, block, 0, st, rcst, wpix, kb, first_ts, ids, active, q, offset, sid_base, none, hits, lane, lanes, ver_bits);
  else if (filtered)
    hipLaunchKernelGGL(k_generate_filtered, grid, block, 0, st, rcst, npix, kb, first_ts, ids, q, offset, sid_base, none, hits, lane, lanes, ver_bits);
  else if (L.adaptive)
    hipLaunchKernelGGL(k_generate_active, grid, block, 0, st, rcst, wpix, kb, first_ts, ids, active, q, offset, sid_base, memo, hits, lane, lanes, ver_bits);
  else
    hipLaunchKernelGGL(k_generate, grid, block, 0, st, rcst, npix, kb, first_ts, ids, q, offset, sid_base, memo, hits, lane, lanes, ver_bits);
}

// k_resolve / k_resolve_active: folds a finished batch into the accumulate buffer; an adaptive frame its active pixels, m2 and counts too.
static void launch_resolve(const gsp_context* ctx, const gsp_context::Lane& L, const gsp_context::Batch& b) {
  const uint32_t npix = (uint32_t)L.num_pixels, wpix = (uint32_t)L.work_pixels();
  const q4* result = L.result.p + (uint64_t)b.slot * L.pipe.batch_paths;
  if (L.adaptive)
    hipLaunchKernelGGL(k_resolve_active, dim3(ctx->grid_for(wpix)), dim3(kBlock), 0, L.stream, wpix, b.kb, b.t0, (const uint32_t*)L.active[L.act].p, result,
                       ctx->accum.p, ctx->pix_m2.p, ctx->pix_spp.p, L.index, ctx->num_lanes);
  else  // (the fold counts the frame's samples from its sample base -- 0 unless gsp_frame_sample_base moved it; the seeds do not)
    hipLaunchKernelGGL(k_resolve, dim3(ctx->grid_for(npix)), dim3(kBlock), 0, L.stream, npix, b.kb, b.t0 - ctx->sample_base, result, ctx->accum.p, L.index,
                       ctx->num_lanes);
}

// ---- one iteration of a lane, step by step (lane_enqueue).  The lane's path queue k; the tail set iteration i writes (i - 1: reads) ----
static PathQueue lane_queue(const gsp_context::Lane& L, int k) { return PathQueue{L.P0[k].p, L.P1[k].p, L.P2[k].p, L.P3[k].p}; }
static uint32_t* lane_tails(const gsp_context::Lane& L, uint32_t i) { return L.counters.p + kTailSet * (i & 1u); }
// where the closest-hit launches (memo, extend) of a statistics pass add their counts
static TraceStatsOut extend_stats_out(const gsp_context* ctx) {
  DevStats* d = ctx->dstats.p;
  // per-record visit counts of the closest-hit rays (measurement hook; gsp_render allocates and zeroes the two histograms before any lane runs)
  const bool hist = ctx->pipe_params.collect_traversal_stats >= 2;
  return TraceStatsOut{&d->nodes, &d->tris, &d->stat_rays, nullptr, nullptr, &d->lds_nodes, nullptr, hist ? ctx->node_hist.p : nullptr, hist ? ctx->tri_hist.p : nullptr};
}

// Step 1, version settling: do the samples in flight belong to more than one version of the BSDF / light tables?  (only after a
// gsp_update_tables that did not drain: then k_shade / k_finish read every vertex's tables through the version its path carries)
// ... or to more than one version of the geometry (gsp_update_instances without a drain: then the traversal kernels too take
// every ray's geometry from the slot its path names)
static int settle_versions(gsp_context* ctx, const SceneView& view, LiveVersions& V) {
  V.multi_version = ctx->oldest_live_version() != ctx->tab.ver || ctx->oldest_live_geo() != ctx->geo.ver ||
                    ctx->split;  // (a split scene is always walked by the <VER> kernels: there is no whole tree in one place)
  if (!V.multi_version) ctx->geo.base = ctx->geo.phys(ctx->geo.ver);  // stamp 0 = the one live version (no copy: the kernels get its slot's pointers)
  if (!V.multi_version && ctx->tab.rot != ctx->tab.ver) {
    // the edits are over and the samples of the older versions have ended: the one live version moves into slot 0 and the
    // version field of the paths goes back to 0 (the <VER = false> kernels write 0).  Nothing reads slot 0 any more -- it held a
    // version whose last sample the host has seen end -- and nothing but the launches queued from here on reads the new copy.
    const uint32_t from = ctx->tab.collapse();
    if (from != 0) {
      CTX_TRY(ctx, hipMemcpyAsync(ctx->tables.p, ctx->tables.p + (size_t)from * ctx->tab.slot_bytes, ctx->tab.slot_bytes, hipMemcpyDeviceToDevice, ctx->stream));
      CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
  }
  V.vview = V.multi_version ? ctx->view(true) : view;
  V.gen_stamp = ctx->geo.phys(ctx->geo.ver + ctx->geo.slots() - ctx->geo.base);
  V.gen_ver_bits = (ctx->tab.slot_of(ctx->tab.ver) << kVerShift) | (V.gen_stamp << kGeoShift);
  // (split scene: the static tree's top goes into LDS -- every ray walks it, whatever its version)
  V.gring = GeoRing{V.vview.geo, ctx->split ? 0u : (uint32_t)((size_t)ctx->geo.phys(ctx->geo.ver) * ctx->geo.stride * kNodeBytes),
                    ctx->split ? ctx->static_slots : 0u};
  return GSP_OK;
}

// Step 2, the memo build, once per scene / camera / frame: the camera rays of the lane's owned pixels, traced into L.memo.
static int build_memo(gsp_context* ctx, gsp_context::Lane& L, const RenderConstsLens& rcst, const SceneView& view, const LiveVersions& V) {
  const uint64_t npix = L.num_pixels;
  uint32_t* work = L.counters.p + C_WORK_EXT;
  CTX_TRY(ctx, L.memo.ensure(npix, &ctx->bytes));
  CTX_TRY(ctx, hipMemsetAsync(work, 0, kWorkShards * kWorkStride * sizeof(uint32_t), L.stream));
  const MemoIO io{rcst, ctx->subset ? ctx->pixel_ids.p : nullptr, L.index, ctx->num_lanes, L.memo.p};
  const uint32_t chunk = npix >= (1u << 20) ? kChunkLarge : kChunkSmall;
  launch_trace(ctx, L.stream, view, V, false, io, nullptr, (uint32_t)npix, 0u, npix, chunk, work, L.spill.p, extend_stats_out(ctx));
  CTX_TRY(ctx, hipGetLastError());
  ctx->stats.memo_build_rays += npix;
  L.memo_valid = true;
  return GSP_OK;
}

// Step 3, the k_finish shortcut: the caller waits for the image, nothing is left to inject and few paths are alive, so every path
// runs to its end on its own lane (not when gsp_render merely queues work: those paths ride along with the next call's).  -> taken
static int finish_few_paths(gsp_context* ctx, gsp_context::Lane& L, const RenderConstsLens& rcst, const LiveVersions& V, bool drain, bool& taken) {
  const gsp_context::Pipeline& P = L.pipe;
  if (!(drain && L.queued == 0 && P.remaining == 0 && P.n > 0 && P.n <= ctx->finish_paths && ctx->pipe_params.collect_traversal_stats == 0 &&
        std::max(ctx->bvh.depth, ctx->split ? ctx->dyn.depth : 0u) + 2 <= kFinishLevels))
    return GSP_OK;
  if (ctx->estimator == GSP_ESTIMATOR_TEXTBOOK || ctx->scatter_on || !ctx->h_delta.empty() || ctx->env_light || ctx->grid_resident) {
    TextbookLaunch a = textbook_launch(ctx, V, rcst, L.stream, (uint32_t)((P.n + kBlock - 1) / kBlock), lane_queue(L, P.cur), L.result.p, lane_tails(L, L.enq),
                                       L.counters.p + C_LIVE, (uint32_t)P.batch_paths);
    a.n = (uint32_t)P.n;
    if (ctx->grid_resident) launch_finish_lightgrid(grid_launch(ctx, a));
    else if (ctx->env_light) launch_finish_envlight(env_launch(ctx, a));
    else if (!ctx->h_delta.empty()) launch_finish_delta(delta_launch(ctx, a));
    else if (ctx->scatter_on) launch_finish_scatter(scatter_launch(ctx, a));
    else launch_finish_textbook(a);
  } else
  tex_ver_med_kernel(ctx, V, [&](auto TEX, auto VER, auto MED, auto LSEL, const auto& sview) {
    hipLaunchKernelGGL((k_finish<decltype(TEX)::value, decltype(VER)::value, decltype(MED)::value, decltype(LSEL)::value, false>), dim3((uint32_t)((P.n + kBlock - 1) / kBlock)), dim3(kBlock), 0, L.stream, sview, rcst,
                       (uint32_t)P.n, lane_queue(L, P.cur), L.result.p, lane_tails(L, L.enq), L.counters.p + C_LIVE, (uint32_t)P.batch_paths, ctx->dstats.p);
  });
  CTX_TRY(ctx, hipGetLastError());
  taken = true;
  return GSP_OK;
}

// k_shade's room in the output queues, taken in chunks when every resident block shades many tiles (see the kernel): the chunk is
// sized for ~1 % of filler records, and the queues must hold them.  0 = one tile's room at a time.
static uint32_t shade_room_chunk(const gsp_context* ctx, const gsp_context::Pipeline& P, double n_guess) {
  if (ctx->pipe_params.collect_traversal_stats != 0 || GSP_ROOM_CHUNK < kShadeBlock) return 0;
  const uint64_t blocks = shade_resident_blocks(ctx);
  uint32_t room_chunk = GSP_ROOM_CHUNK;
  while (room_chunk >= (uint32_t)kShadeBlock && (double)room_chunk > 0.036 * n_guess / (double)blocks) room_chunk >>= 1;
  return (room_chunk < (uint32_t)kShadeBlock || P.n + blocks * room_chunk > P.cap) ? 0 : room_chunk;
}

// Step 4, injection: new batches while there is room, into the next queue, in front of this iteration's survivors.  The next iteration traces
// both: their sum is aimed at the pool target with the survivors `expect`ed, the buffers are checked against the bound P.n + `slack`.
static int inject_batches(gsp_context* ctx, gsp_context::Lane& L, const RenderConstsLens& rcst, const LiveVersions& V, bool use_memo, double expect,
                          uint64_t slack, uint64_t& injected) {
  gsp_context::Pipeline& P = L.pipe;
  injected = 0;
  while (P.remaining > 0 && expect + (double)injected < (double)P.pool_target) {
    const uint32_t kb = (uint32_t)std::min<uint64_t>(P.Kb, P.remaining);
    const uint32_t slot = (uint32_t)(std::find(P.slot_used.begin(), P.slot_used.end(), 0) - P.slot_used.begin());  // the first free ring slot
    const uint64_t paths = (uint64_t)kb * L.work_pixels();
    if (slot == P.num_slots || P.n + injected + paths + slack > P.cap) break;
    launch_generate(ctx, L, rcst, kb, P.next_ts, lane_queue(L, P.cur ^ 1), L.hits[P.cur ^ 1].p, (uint32_t)injected, (uint32_t)(slot * P.batch_paths), use_memo,
                    V.gen_ver_bits);
    CTX_TRY(ctx, hipGetLastError());
    CTX_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)(L.counters.p + C_LIVE + slot), (int)paths, 1, L.stream));
    L.h_live[slot] = (uint32_t)paths;
    L.live_since[slot] = L.enq;  // read-backs of earlier iterations still show the slot's previous state
    P.slot_used[slot] = 1;
    P.inflight.push_back(gsp_context::Batch{P.next_ts, kb, slot, ctx->tab.ver, ctx->geo.ver});
    injected += paths;
    P.next_ts += kb;
    P.remaining -= kb;
  }
  if (injected) CTX_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)(lane_tails(L, L.enq) + T_NEXT), (int)injected, 1, L.stream));
  return GSP_OK;
}

// Step 5, the trio over the current queue: k_trace<Extend> from entry `front` on (the entries before it have their hits from the
// memo), k_shade, k_trace<Connect> over the shadow queue k_shade has just filled.  `ev`: four events around the three, or null.
static int trace_shade_connect(gsp_context* ctx, gsp_context::Lane& L, const RenderConstsLens& rcst, const SceneView& view, const LiveVersions& V,
                               uint64_t front, uint32_t room_chunk, hipEvent_t* ev) {
  hipStream_t st = L.stream;
  const bool stats = ctx->pipe_params.collect_traversal_stats != 0;
  const uint64_t bound = std::max<uint64_t>(L.pipe.n, 1);
  const uint32_t chunk = L.pipe.n >= (1u << 20) ? kChunkLarge : kChunkSmall;
  const PathQueue cur = lane_queue(L, L.pipe.cur), next = lane_queue(L, L.pipe.cur ^ 1);
  q4* hits = L.hits[L.pipe.cur].p;
  const ShadowQueue sq{L.S0.p, L.S1.p, L.S3.p};
  const uint32_t* n_ptr = lane_tails(L, L.enq ^ 1u) + T_NEXT;
  uint32_t *tails_out = lane_tails(L, L.enq), *work = L.counters.p + C_WORK_EXT;
  DevStats* d = ctx->dstats.p;
  const TraceStatsOut so_sh{&d->sh_nodes, &d->sh_tris, &d->sh_rays, &d->sh_occluded, &d->sh_occluded_nodes, &d->sh_lds_nodes, &d->sh_no_tri};
  CTX_TRY(ctx, hipMemsetAsync(work, 0, (C_COUNT - C_WORK_EXT) * sizeof(uint32_t), st));
  if (ev) CTX_TRY(ctx, hipEventRecord(ev[0], st));
  launch_trace(ctx, st, view, V, stats, ExtendIO{cur, hits}, n_ptr, 0u, (uint32_t)front, bound, chunk, work, L.spill.p, extend_stats_out(ctx));
  CTX_TRY(ctx, hipGetLastError());
  if (ev) CTX_TRY(ctx, hipEventRecord(ev[1], st));
  const dim3 grid((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((bound + kShadeBlock - 1) / kShadeBlock, shade_resident_blocks(ctx))));
  if (ctx->estimator == GSP_ESTIMATOR_TEXTBOOK || ctx->scatter_on || !ctx->h_delta.empty() || ctx->env_light || ctx->grid_resident) {
    TextbookLaunch a = textbook_launch(ctx, V, rcst, st, grid.x, cur, L.result.p, tails_out, L.counters.p + C_LIVE, (uint32_t)L.pipe.batch_paths);
    a.n_ptr = n_ptr;
    a.hits = hits;
    a.next[0] = next.P0, a.next[1] = next.P1, a.next[2] = next.P2, a.next[3] = next.P3;
    a.shadow[0] = sq.S0, a.shadow[1] = sq.S1, a.shadow[2] = sq.S3;
    a.chunk = room_chunk;
    if (ctx->grid_resident) launch_shade_lightgrid(grid_launch(ctx, a));
    else if (ctx->env_light) launch_shade_envlight(env_launch(ctx, a));
    else if (!ctx->h_delta.empty()) launch_shade_delta(delta_launch(ctx, a));
    else if (ctx->scatter_on) launch_shade_scatter(scatter_launch(ctx, a));
    else launch_shade_textbook(a);
  } else
  tex_ver_med_kernel(ctx, V, [&](auto TEX, auto VER, auto MED, auto LSEL, const auto& sview) {
    hipLaunchKernelGGL((k_shade<decltype(TEX)::value, decltype(VER)::value, decltype(MED)::value, decltype(LSEL)::value, false>), grid, dim3(kShadeBlock), 0, st, sview, rcst, n_ptr, cur, hits, next, sq,
                       L.result.p, tails_out, L.counters.p + C_LIVE, (uint32_t)L.pipe.batch_paths, room_chunk, ctx->dstats.p);
  });
  CTX_TRY(ctx, hipGetLastError());
  if (ev) CTX_TRY(ctx, hipEventRecord(ev[2], st));
  launch_trace(ctx, st, view, V, stats, ConnectIO{sq, next.P2, next.P3, L.result.p, rcst.clamp}, tails_out + T_SHADOW, 0u, 0u, bound, chunk,
               L.counters.p + C_WORK_SH, L.spill.p, so_sh);
  CTX_TRY(ctx, hipGetLastError());
  if (ev) CTX_TRY(ctx, hipEventRecord(ev[3], st));
  return GSP_OK;
}

// Queues one iteration of a lane on its stream without waiting.  Iteration i: steps 1 and 2 above, between them
//   tails[i & 1] := {next-queue size = paths injected now, shadow-queue size = 0}
// then step 3 or steps 4 and 5 (new batches at the FRONT of the next queue; the trio reads the size of the current queue from
// tails[(i - 1) & 1] on the device and appends its survivors behind the injected paths), then
//   copy of the counter words to the host buffer of this parity + an event
static int lane_enqueue(gsp_context* ctx, gsp_context::Lane& L, const RenderConstsLens& rcst, const SceneView& view, bool drain) {
  gsp_context::Pipeline& P = L.pipe;
  const bool timing = ctx->pipe_params.collect_kernel_times != 0;  // per-kernel HIP event timing (bench)
  while (timing && L.ev.size() < 8) {
    hipEvent_t e;
    CTX_TRY(ctx, hipEventCreate(&e));
    L.ev.push_back(e);
  }
  const uint32_t t = L.enq & 1u;
  const uint64_t n = P.n;           // exact, or an upper bound of what this iteration traces
  const bool exact = L.queued == 0;  // no iteration is in flight, so n is the true queue size (and 0 means there is nothing to trace)
  const double n_guess = exact ? (double)n : std::min((double)n, P.n_est);
  gsp_context::Lane::Iter& I = L.it[t] = gsp_context::Lane::Iter{};
  LiveVersions V;
  if (int rc = settle_versions(ctx, view, V)) return rc;
  CTX_TRY(ctx, hipMemsetAsync(lane_tails(L, t), 0, kTailSet * sizeof(uint32_t), L.stream));
  // (a filtered sample's camera ray is its own: nothing to memoise, and so is a sample's through a lens.  L.memo / L.memo_valid are
  // left as they are -- the memo holds the UNJITTERED camera rays' hits and stays true for a later unfiltered call as long as scene,
  // camera and frame do)
  const bool use_memo = ctx->primary_memo && ctx->pipe_params.collect_traversal_stats == 0 && rcst.pixel_filter == GSP_FILTER_NONE && !(rcst.lens_radius > 0.0f);
  if (use_memo && !L.memo_valid && P.remaining > 0)
    if (int rc = build_memo(ctx, L, rcst, view, V)) return rc;
  I.front = use_memo ? P.front : 0;  // (a stats pass traces everything: its counters describe all rays)
  if (int rc = finish_few_paths(ctx, L, rcst, V, drain, I.finish)) return rc;
  if (!I.finish) {
    const uint32_t room_chunk = shade_room_chunk(ctx, P, n_guess);
    I.slack = shade_resident_blocks(ctx) * room_chunk;
    if (int rc = inject_batches(ctx, L, rcst, V, use_memo, n_guess * P.survive, I.slack, I.injected)) return rc;
    if (!(exact && n == 0)) {
      if (int rc = trace_shade_connect(ctx, L, rcst, view, V, I.front, room_chunk, timing ? &L.ev[4 * t] : nullptr)) return rc;
      I.traced = true;
      I.timing = timing;
    }
  }
  CTX_TRY(ctx, hipMemcpyAsync(L.h_counters + (size_t)t * C_READBACK, L.counters.p, C_READBACK * sizeof(uint32_t), hipMemcpyDeviceToHost, L.stream));
  CTX_TRY(ctx, hipEventRecord(L.done[t], L.stream));
  ++L.queued;
  ++L.enq;
  P.cur ^= 1;
  P.front = use_memo && !I.finish ? I.injected : 0;
  P.n = (I.finish ? 0 : n + I.slack) + I.injected;  // survivors <= n: an upper bound of the next iteration's input until the read-back says more
  P.n_est = (I.finish ? 0.0 : n_guess * P.survive) + (double)I.injected;
  return GSP_OK;
}

// Waits for the lane's oldest queued iteration, reads its counters and folds finished batches into the
// accumulate buffer, strictly in timestamp order.
static int lane_collect(gsp_context* ctx, gsp_context::Lane& L) {
  gsp_context::Pipeline& P = L.pipe;
  if (L.queued) {
    const uint32_t t = L.col & 1u;
    CTX_TRY(ctx, hipEventSynchronize(L.done[t]));
    CTX_TRY(ctx, hipGetLastError());
    const uint32_t* rb = L.h_counters + (size_t)t * C_READBACK;
    const uint32_t* tails = rb + kTailSet * t;
    const gsp_context::Lane::Iter I = L.it[t];
    const uint64_t n_traced = L.n_in;
    if (I.finish) {
      ctx->stats.extension_rays += (uint64_t)tails[T_FIN_EXT] | ((uint64_t)tails[T_FIN_EXT + 1] << 32);
      ctx->stats.shadow_rays += (uint64_t)tails[T_FIN_SH] | ((uint64_t)tails[T_FIN_SH + 1] << 32);
    } else if (I.traced) {
      ctx->stats.extension_rays += n_traced - L.holes_in;  // path segments; I.front of them were answered from the memo
      ctx->stats.memoised_rays += I.front;
      ctx->stats.shadow_rays += tails[T_SHADOW] - tails[T_HOLES_SHADOW];
    }
    const uint32_t bounce = P.iteration++;
    if (I.timing) {
      float ms = 0.0f, e_ms = 0.0f, s_ms = 0.0f;
      hipEvent_t* ev = &L.ev[4 * t];
      CTX_TRY(ctx, hipEventElapsedTime(&e_ms, ev[0], ev[1]));
      ctx->stats.extend_kernel_ms += e_ms;
      ctx->stats.extend_launches += 1;
      CTX_TRY(ctx, hipEventElapsedTime(&s_ms, ev[1], ev[2]));
      ctx->stats.shade_kernel_ms += s_ms;
      CTX_TRY(ctx, hipEventElapsedTime(&ms, ev[2], ev[3]));
      ctx->stats.connect_kernel_ms += ms;
      if (ctx->pipe_params.collect_kernel_times >= 2)  // (test tools: one line per iteration)
        fprintf(stderr, "lane %u iter %3u: n %9llu shadow %9u injected %9llu inflight %2zu | extend %8.3f ms shade %8.3f ms connect %8.3f ms\n",
                L.index, bounce, (unsigned long long)n_traced, tails[T_SHADOW], (unsigned long long)I.injected, P.inflight.size(), e_ms, s_ms, ms);
    }
    // the input size of the next iteration, exactly: injected paths + survivors
    if (I.traced && n_traced > L.holes_in) {
      const double r = ((double)tails[T_NEXT] - (double)tails[T_HOLES_NEXT] - (double)I.injected) / (double)(n_traced - L.holes_in);
      P.survive = 0.5 * P.survive + 0.5 * std::min(1.0, std::max(0.0, r));
    }
    L.n_in = tails[T_NEXT];
    L.holes_in = I.traced ? tails[T_HOLES_NEXT] : 0;
    for (const gsp_context::Batch& b : P.inflight)
      if (L.live_since[b.slot] <= L.col) L.h_live[b.slot] = rb[C_LIVE + b.slot];
    ++L.col;
    --L.queued;
    // what the next iteration to be QUEUED will trace: exact if nothing is in flight, else bounded through the one that is
    P.n = L.queued ? L.n_in + L.it[L.col & 1u].slack + L.it[L.col & 1u].injected : L.n_in;
    P.n_est = L.queued ? (double)L.n_in * P.survive + (double)L.it[L.col & 1u].injected : (double)L.n_in;
  }
  while (!P.inflight.empty() && L.h_live[P.inflight.front().slot] == 0) {
    const gsp_context::Batch b = P.inflight.front();
    P.inflight.pop_front();
    launch_resolve(ctx, L, b);
    CTX_TRY(ctx, hipGetLastError());
    P.slot_used[b.slot] = 0;
    P.folded_end = b.t0 + b.kb;
    ctx->stats.samples += (uint64_t)b.kb * L.work_pixels();
  }
  if (L.queued == 0 && P.n == 0 && P.remaining == 0 && !P.inflight.empty()) {
    ctx->err = "internal error: paths exhausted with unresolved sample batches";
    return GSP_ERR_DEVICE;
  }
  return GSP_OK;
}

// Runs the streaming pipelines.  drain == false: returns as soon as every queued sample has been
// injected (stragglers of the last batches stay in flight and ride along with the next call's
// launches); drain == true: runs until nothing is in flight and every batch has been folded into the
// accumulate buffer.  While samples remain to be injected each lane keeps kPipeDepth iterations queued, so the GPU
// never waits for the host; the tail of a drain (exact path counts decide k_finish and the end) runs one at a time.
static int pipeline_run(gsp_context* ctx, bool drain) {
  if (!ctx->pipe_active) return GSP_OK;
  const auto t_begin = std::chrono::steady_clock::now();
  const RenderConstsLens rcst = render_consts(ctx);
  const SceneView view = ctx->view();
  auto has_work = [&](const gsp_context::Lane& L) {
    const gsp_context::Pipeline& P = L.pipe;
    return P.active && (P.remaining > 0 || (drain && (P.n > 0 || !P.inflight.empty())));
  };
  auto depth_for = [&](const gsp_context::Lane& L) { return L.pipe.remaining > 0 && !ctx->pipe_params.collect_traversal_stats ? kPipeDepth : 1u; };
  for (;;) {
    bool any = false;
    for (uint32_t l = 0; l < ctx->num_lanes; ++l) {
      gsp_context::Lane& L = ctx->lanes[l];
      if (!L.pipe.active) continue;
      while (has_work(L) && L.queued < depth_for(L)) {
        if (L.queued == 0 && L.pipe.n == 0 && L.pipe.remaining == 0) break;  // nothing to trace: only batches to fold
        int rc = lane_enqueue(ctx, L, rcst, view, drain);
        if (rc != GSP_OK) return rc;
      }
    }
    for (uint32_t l = 0; l < ctx->num_lanes; ++l) {
      gsp_context::Lane& L = ctx->lanes[l];
      if (!L.pipe.active) continue;
      if (L.queued) {
        int rc = lane_collect(ctx, L);
        if (rc != GSP_OK) return rc;
        any = true;
      } else if (has_work(L)) {  // only batches to fold
        int rc = lane_collect(ctx, L);
        if (rc != GSP_OK) return rc;
        any = any || has_work(L);
      }
    }
    bool more = false;
    for (uint32_t l = 0; l < ctx->num_lanes; ++l) more = more || has_work(ctx->lanes[l]) || (drain && ctx->lanes[l].queued);
    if (!more) break;
    if (!any) break;
  }
  // leave with nothing in flight: the host's view of every lane is exact again
  for (uint32_t l = 0; l < ctx->num_lanes; ++l) {
    gsp_context::Lane& L = ctx->lanes[l];
    while (L.pipe.active && L.queued) {
      int rc = lane_collect(ctx, L);
      if (rc != GSP_OK) return rc;
    }
  }
  for (uint32_t l = 0; l < ctx->num_lanes; ++l) CTX_TRY(ctx, hipStreamSynchronize(ctx->lanes[l].stream));
  if (drain) {
    for (uint32_t l = 0; l < ctx->num_lanes; ++l)
      if (ctx->lanes[l].pipe.active) ctx->folded_idle = ctx->lanes[l].pipe.folded_end;
    ctx->pipe_active = false;
    for (uint32_t l = 0; l < ctx->num_lanes; ++l) ctx->lanes[l].pipe.active = false;
  }
  ctx->stats.render_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
  return GSP_OK;
}

// Completes everything gsp_render has queued.
static int pipeline_drain(gsp_context* ctx) { return pipeline_run(ctx, true); }

static int render_enqueue(gsp_context* ctx, const gsp_render_params* rp);
static int render_adaptive(gsp_context* ctx, const gsp_render_params* rp);

int gsp_render(gsp_context* ctx, const gsp_render_params* rp_host) {
  if (!ctx || !rp_host) return GSP_ERR_INVALID;
  // ABI 8: the host's struct may be shorter than this library's (an older header of ABI >= 8): the fields it does not have are 0,
  // which is the reference's behaviour for every field; struct_size 0 = the layout of ABI 8 (a zero-initialised struct)
  gsp_render_params rp_copy;
  std::memset(&rp_copy, 0, sizeof(rp_copy));
  {
    const size_t abi8 = offsetof(gsp_render_params, disable_nee) + sizeof(uint32_t);
    const size_t n = rp_host->struct_size ? std::min<size_t>(rp_host->struct_size, sizeof(rp_copy)) : abi8;
    if (n < abi8) {
      ctx->err = "gsp_render_params.struct_size " + std::to_string(rp_host->struct_size) + " is smaller than the ABI-8 struct (" + std::to_string(abi8) +
                 " bytes): set it with gsp_default_render_params or sizeof(gsp_render_params)";
      return GSP_ERR_INVALID;
    }
    std::memcpy(&rp_copy, rp_host, n);
  }
  const gsp_render_params* const rp = &rp_copy;
  if (!ctx->have_scene || !ctx->have_frame) {
    ctx->err = "gsp_render needs gsp_upload_scene and gsp_frame_begin first";
    return GSP_ERR_INVALID;
  }
  if (rp->max_depth > 250) {
    ctx->err = "max_depth > 250 unsupported";
    return GSP_ERR_INVALID;
  }
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  if (rp->spp == 0 || ctx->num_pixels == 0) return GSP_OK;
  if (!(rp->adaptive_threshold >= 0.0f) || std::isinf(rp->adaptive_threshold)) {
    ctx->err = "adaptive_threshold must be 0 (off) or a finite positive value";
    return GSP_ERR_INVALID;
  }
  if (rp->pixel_filter > GSP_FILTER_GAUSSIAN) {
    ctx->err = "pixel_filter " + std::to_string(rp->pixel_filter) + " is not a GSP_FILTER_* value";
    return GSP_ERR_INVALID;
  }
  if (!(rp->pixel_filter_param >= 0.0f) || std::isinf(rp->pixel_filter_param)) {
    ctx->err = "pixel_filter_param must be 0 (the filter's default) or a finite positive value";
    return GSP_ERR_INVALID;
  }
  // the first render of a frame decides whether it is adaptive (include/gpuspectral_pt.h, "Adaptive sampling")
  const bool adaptive = rp->adaptive_threshold > 0.0f;
  if (ctx->frame_mode != gsp_context::kFrameUndecided && (ctx->frame_mode == gsp_context::kFrameAdaptive) != adaptive) {
    ctx->err = adaptive ? "adaptive_threshold > 0 in a frame that began uniform: call gsp_frame_begin first"
                        : "adaptive_threshold == 0 in an adaptive frame: call gsp_frame_begin first";
    return GSP_ERR_INVALID;
  }
  if (ctx->sample_base != 0) {  // gsp_frame_sample_base
    if (adaptive) {
      ctx->err = "adaptive_threshold > 0 in a frame with a sample base (gsp_frame_sample_base): adaptive frames count from timestamp 0";
      return GSP_ERR_INVALID;
    }
    if (rp->first_timestamp < ctx->sample_base) {
      ctx->err = "first_timestamp " + std::to_string(rp->first_timestamp) + " lies before the frame's sample base " + std::to_string(ctx->sample_base);
      return GSP_ERR_INVALID;
    }
  }
  if (adaptive) return render_adaptive(ctx, rp);
  ctx->frame_mode = gsp_context::kFrameUniform;
  return render_enqueue(ctx, rp);
}

int gsp_frame_sample_base(gsp_context* ctx, uint32_t base) {
  if (!ctx) return GSP_ERR_INVALID;
  if (!ctx->have_frame || ctx->frame_mode != gsp_context::kFrameUndecided) {
    ctx->err = "gsp_frame_sample_base belongs between gsp_frame_begin and the frame's first gsp_render";
    return GSP_ERR_INVALID;
  }
  ctx->sample_base = base;
  return GSP_OK;
}

// Queues rp->spp samples of every pixel the lanes sample (all owned pixels, or an adaptive frame's active lists) without waiting
// for them (pipeline_run(ctx, false)).
static int render_enqueue(gsp_context* ctx, const gsp_render_params* rp) {
  // A running pipeline is continued when the integrator constants and the batch size are unchanged
  // (paths in flight carry no copy of them); otherwise it is drained first.
  if (ctx->pipe_active &&
      (ctx->pipe_params.max_depth != rp->max_depth || ctx->pipe_params.rr_start_depth != rp->rr_start_depth ||
       ctx->pipe_params.clamp != rp->clamp || ctx->pipe_params.timestamps_in_flight != rp->timestamps_in_flight ||
       (ctx->pipe_params.disable_nee != 0) != (rp->disable_nee != 0))) {
    int rc = pipeline_drain(ctx);
    if (rc != GSP_OK) return rc;
  }
  if (rp->collect_traversal_stats != 0 && ctx->split) {
    // the statistics instantiations of k_trace walk ONE tree: the queued samples finish, the two trees are built as one again
    int rc_ = pipeline_drain(ctx);
    if (rc_ == GSP_OK) {
      ctx->have_scene = false;
      rc_ = bake_and_build(ctx);
      ctx->have_scene = rc_ == GSP_OK;
      ctx->split_declined = true;  // (a host that asks for statistics gets the scene in one piece from here on)
    }
    if (rc_ != GSP_OK) return rc_;
  }
  if (rp->collect_traversal_stats != 0 && ctx->pipe_active &&
      (ctx->oldest_live_version() != ctx->tab.ver || ctx->oldest_live_geo() != ctx->geo.ver)) {
    // the statistics instantiations of k_trace know one version of the scene: samples of older ones finish first
    int rc_ = pipeline_drain(ctx);
    if (rc_ != GSP_OK) return rc_;
  }
  if (!ctx->pipe_active) {
    if (ctx->split) ctx->geo.base = ctx->geo.phys(ctx->geo.ver);  // (nothing in flight: stamp 0 = the current version again)
    // Streaming path pool, per lane.  Samples enter in batches of Kb timestamps (>= ~1M paths); a new batch
    // is injected whenever the pool has room, so every launch works on millions of paths even though 95 %
    // of a batch dies at the Russian-roulette depth and a few stragglers live for 52 bounces.  Each batch
    // owns a slot of the sample-result ring and is folded into the accumulate buffer, in timestamp
    // order, once its live count has dropped to zero.
    // paths in flight over all lanes: per-launch fixed costs (drained wave tails, launch gaps) amortise over the pool
    // size -- r01 bench scan: 8 M 5.35, 12 M 5.76, 24 M 6.11, 48 M 6.16, 96 M 6.25 Grays/s; r02 (final kernels): 32 M 7.48,
    // 48 M 7.63, 64 M 7.64 (profiles/r02_ab_pool_size.txt); r03 (faster kernels, so the fixed cost per launch weighs more): 32 M 7.84,
    // 48 M 7.98, 64 M 8.09, 96 M 8.24, 128 M 8.21 (profiles/r03_ab_pool_size.txt).  96 M paths: 43 GB of queues (capacity 2 x the target)
    const uint64_t total_target = ctx->opt.pool_paths;  // (default 96 Mi)
    for (uint32_t l = 0; l < ctx->num_lanes; ++l) {
      gsp_context::Lane& L = ctx->lanes[l];
      gsp_context::Pipeline& P = L.pipe;
      P = gsp_context::Pipeline{};
      P.folded_end = ctx->folded_idle;
      const uint64_t npix = L.work_pixels();
      if (npix == 0) continue;  // fewer pixels than lanes (or, adaptive, no pixel of this lane left)
      uint64_t Kb = rp->timestamps_in_flight;
      if (Kb == 0) Kb = std::max<uint64_t>(1, (1ull << 20) / npix);
      while (Kb > 1 && Kb * npix >= (1ull << 30)) --Kb;
      P.Kb = Kb;
      P.batch_paths = Kb * npix;
      // (at most 192 samples per pixel in flight for a whole frame: tiny frames do not allocate gigabytes and gsp_peek does not
      // lag far behind; 384 for a pixel SUBSET -- a tile share of a multi-GPU frame: the 1/8 share of a 1080p frame, 259 k
      // pixels, must still fill the 96 Mi-path pool, else every GPU of an 8-GPU job runs launches half the size of the
      // single-GPU run's, profiles/r04_share_probe.txt)
#ifndef GSP_SHARE_SPP
#define GSP_SHARE_SPP 384
#endif
      const uint64_t per_pixel = ctx->subset ? GSP_SHARE_SPP : 192;
      P.pool_target = std::max<uint64_t>(std::min<uint64_t>(total_target / ctx->num_lanes, per_pixel * npix), 2 * P.batch_paths);
      uint64_t ring_bytes = ctx->opt.ring_bytes;  // (default 16 GiB)
      {
        // Several contexts may share one GPU (the shares of gsp_multi on a test box, two viewers, ...): this pipeline
        // takes at most gsp_ctx_options.memory_share (default 40 %) of the device's memory (plus what the lane already holds).  208 B of queues per
        // path of capacity (2 x 64-B path records, 2 x 16-B hit, 48-B shadow record), capacity = 2 x the pool target.
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
          const uint64_t have = L.pool_cap * 208ull + L.result_cap * sizeof(q4);
          // r05: the share is of the device's TOTAL memory (two contexts created one after the other get the same budget --
          // until r04 it was a share of what was FREE at that moment, so the second one sized itself by the first), and never
          // more than 90 % of what is free now
          const uint64_t budget = std::min((uint64_t)((double)total_b * ctx->memory_share), (uint64_t)((double)free_b * 0.9)) + have;
          const uint64_t queues = (2 * P.pool_target + P.batch_paths) * 208ull;
          if (queues > budget / 2) {
            const uint64_t fit = budget / 2 / 208ull;  // paths of capacity that fit
            P.pool_target = std::max<uint64_t>(2 * P.batch_paths, fit > P.batch_paths ? (fit - P.batch_paths) / 2 : 0);
          }
          ring_bytes = std::min<uint64_t>(ring_bytes, std::max<uint64_t>(budget / 2, 4 * P.batch_paths * sizeof(q4)));
        }
      }
      P.cap = 2 * P.pool_target + P.batch_paths;  // survivors (<= the previous queue) + a pool target's worth of new paths
      // Slots of the sample-result ring: a batch holds its slot until its last path has ended, so with paths of
      // ~3 bounces on average and a tail of 52 the alive share of the batches in flight is only a few percent and
      // the ring must hold ~24 x the pool for the pool to fill (coffee: 4.2 rays per sample).  16 B per entry, most
      // of it never touched on scenes with long paths; bounded by gsp_ctx_options.ring_bytes (default 16 GiB of the 288).
      const uint64_t want_slots = 24 * ((P.pool_target + P.batch_paths - 1) / P.batch_paths);
      const uint64_t fit_slots = ring_bytes / ctx->num_lanes / (P.batch_paths * sizeof(q4));
      P.num_slots = (uint32_t)std::min<uint64_t>(kMaxSlots, std::max<uint64_t>(4, std::min(want_slots, fit_slots)));
      if (L.adaptive) {
        // an adaptive round re-derives the batch from a shrinking pixel count: it works in the pool and the ring the frame's first
        // round allocated rather than re-allocating them (a 16-GB ring freed and allocated again: 0.45-0.88 s per call in the first probe run)
        if (P.cap > L.pool_cap && L.pool_cap >= 3 * P.batch_paths) {
          P.pool_target = (L.pool_cap - P.batch_paths) / 2;
          P.cap = L.pool_cap;
        }
        if ((uint64_t)P.num_slots * P.batch_paths > L.result_cap && L.result_cap >= 4 * P.batch_paths)
          P.num_slots = (uint32_t)std::min<uint64_t>(kMaxSlots, L.result_cap / P.batch_paths);
      }
      if (P.cap >= (1ull << 32) || (uint64_t)P.num_slots * P.batch_paths >= (1ull << 32)) {
        ctx->err = "frame too large for 32-bit path indices";
        return GSP_ERR_INVALID;
      }
      int rc = ensure_pool(ctx, L, P.cap, (uint64_t)P.num_slots * P.batch_paths);
      if (rc != GSP_OK) return rc;
      P.slot_used.assign(P.num_slots, 0);
      P.active = true;
    }
    ctx->pipe_active = true;
  }
  ctx->pipe_params = *rp;  // (stats / timing flags may change from call to call)
  if (rp->collect_traversal_stats >= 2) {
    // the visit histograms belong to the context, every lane's k_trace adds to them on its own stream: allocate and zero them
    // here, on the context's stream, and wait -- not on the stream of whichever lane happens to enqueue first (ADVICE r04)
    const size_t nn = std::max<size_t>(ctx->bvh.num_nodes, 1), ns = (size_t)ctx->bvh.num_tris + ctx->bvh.first_slot + kWide;
    if (ctx->node_hist.count < nn || ctx->tri_hist.count < ns) {
      CTX_TRY(ctx, ctx->node_hist.ensure(nn, &ctx->bytes));
      CTX_TRY(ctx, ctx->tri_hist.ensure(ns, &ctx->bytes));
      CTX_TRY(ctx, hipMemsetAsync(ctx->node_hist.p, 0, ctx->node_hist.count * sizeof(uint32_t), ctx->stream));
      CTX_TRY(ctx, hipMemsetAsync(ctx->tri_hist.p, 0, ctx->tri_hist.count * sizeof(uint32_t), ctx->stream));
      CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
  }
  for (uint32_t l = 0; l < ctx->num_lanes; ++l) {
    gsp_context::Pipeline& P = ctx->lanes[l].pipe;
    if (!P.active) continue;
    P.next_ts = rp->first_timestamp;
    P.remaining += rp->spp;
  }
  return pipeline_run(ctx, false);
}

// ---- adaptive sampling (ABI 9) ----------------------------------------------------------------------------------------------
// The first adaptive gsp_render of a frame: m2 and the per-pixel counts (zero), every lane's active list = all its owned pixels.
static int adaptive_begin(gsp_context* ctx) {
  CTX_TRY(ctx, ctx->pix_m2.ensure(ctx->num_pixels, &ctx->bytes));
  CTX_TRY(ctx, ctx->pix_spp.ensure(ctx->num_pixels, &ctx->bytes));
  CTX_TRY(ctx, hipMemsetAsync(ctx->pix_m2.p, 0, ctx->num_pixels * sizeof(float), ctx->stream));
  CTX_TRY(ctx, hipMemsetAsync(ctx->pix_spp.p, 0, ctx->num_pixels * sizeof(uint32_t), ctx->stream));
  for (uint32_t l = 0; l < ctx->num_lanes; ++l) {
    gsp_context::Lane& L = ctx->lanes[l];
    const uint64_t n = L.num_pixels, nb = (n + kBlock - 1) / kBlock;
    CTX_TRY(ctx, L.active[0].ensure(n, &ctx->bytes));
    CTX_TRY(ctx, L.active[1].ensure(n, &ctx->bytes));
    CTX_TRY(ctx, L.conv_masks.ensure(nb * (kBlock / 64), &ctx->bytes));
    CTX_TRY(ctx, L.conv_blocks.ensure(nb + 1, &ctx->bytes));
    if (n) {
      hipLaunchKernelGGL(k_iota, dim3(ctx->grid_for(n)), dim3(kBlock), 0, ctx->stream, (uint32_t)n, L.active[0].p);
      CTX_TRY(ctx, hipGetLastError());
    }
    L.act = 0;
    L.num_active = n;
    L.adaptive = true;
  }
  CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->adaptive_n = 0;
  ctx->frame_mode = gsp_context::kFrameAdaptive;
  return GSP_OK;
}

// At a checkpoint (nothing in flight): every lane's active list loses the pixels the rule stops, order kept (k_converge).  One
// 4-byte read-back per lane.
static int adaptive_converge(gsp_context* ctx, float threshold) {
  for (uint32_t l = 0; l < ctx->num_lanes; ++l) {
    gsp_context::Lane& L = ctx->lanes[l];
    if (!L.adaptive || L.num_active == 0) continue;
    const uint32_t n = (uint32_t)L.num_active, nb = (n + kBlock - 1) / kBlock;
    const ConvergeIO io{ctx->accum.p, ctx->pix_m2.p, ctx->pix_spp.p, (double)threshold, L.index, ctx->num_lanes};
    hipLaunchKernelGGL(k_converge, dim3(nb), dim3(kBlock), 0, L.stream, n, (const uint32_t*)L.active[L.act].p, io, L.conv_masks.p,
                       L.conv_blocks.p);
    hipLaunchKernelGGL(k_converge_scan, dim3(1), dim3(kScanBlock), 0, L.stream, nb, L.conv_blocks.p);
    hipLaunchKernelGGL(k_converge_compact, dim3(nb), dim3(kBlock), 0, L.stream, n, (const uint32_t*)L.active[L.act].p,
                       (const uint64_t*)L.conv_masks.p, (const uint32_t*)L.conv_blocks.p, L.active[L.act ^ 1].p);
    CTX_TRY(ctx, hipGetLastError());
    CTX_TRY(ctx, hipMemcpyAsync(&L.h_num_active, L.conv_blocks.p + nb, sizeof(uint32_t), hipMemcpyDeviceToHost, L.stream));
  }
  for (uint32_t l = 0; l < ctx->num_lanes; ++l) {
    gsp_context::Lane& L = ctx->lanes[l];
    if (!L.adaptive || L.num_active == 0) continue;
    CTX_TRY(ctx, hipStreamSynchronize(L.stream));
    L.act ^= 1;
    L.num_active = L.h_num_active;
  }
  return GSP_OK;
}

// An adaptive gsp_render: rounds that end at the checkpoints and at the end of the call, each drained; k_converge at every
// checkpoint.  Decisions happen only at checkpoints, so the split of the samples over calls does not change the result.
static int render_adaptive(gsp_context* ctx, const gsp_render_params* rp) {
  if (ctx->frame_mode != gsp_context::kFrameAdaptive) {
    int rc = pipeline_drain(ctx);  // (nothing of this frame is in flight; a pipeline of an earlier frame would have been drained)
    if (rc == GSP_OK) rc = adaptive_begin(ctx);
    if (rc != GSP_OK) return rc;
  }
  if (ctx->active_pixels() == 0) return GSP_OK;  // every pixel has stopped: nothing to add
  if (rp->first_timestamp != ctx->adaptive_n) {
    ctx->err = "adaptive frame: first_timestamp " + std::to_string(rp->first_timestamp) + " must equal the samples the pixels still sampled hold (" +
               std::to_string(ctx->adaptive_n) + ")";
    return GSP_ERR_INVALID;
  }
  const uint64_t min_spp = rp->adaptive_min_spp ? rp->adaptive_min_spp : 16u, step = rp->adaptive_step ? rp->adaptive_step : 16u;
  uint32_t remaining = rp->spp;
  while (remaining > 0 && ctx->active_pixels() > 0) {
    const uint64_t n = ctx->adaptive_n;
    const uint64_t next = n < min_spp ? min_spp : min_spp + ((n - min_spp) / step + 1) * step;  // the next checkpoint
    const uint32_t k = (uint32_t)std::min<uint64_t>(remaining, next - n);
    gsp_render_params r = *rp;
    r.spp = k;
    r.first_timestamp = (uint32_t)n;
    int rc = render_enqueue(ctx, &r);
    if (rc == GSP_OK) rc = pipeline_drain(ctx);
    if (rc != GSP_OK) return rc;
    ctx->adaptive_n = (uint32_t)(n + k);
    remaining -= k;
    ++ctx->stats.adaptive_rounds;
    if (n + k == next) {
      const auto t0 = std::chrono::steady_clock::now();
      rc = adaptive_converge(ctx, rp->adaptive_threshold);
      if (rc != GSP_OK) return rc;
      ctx->stats.render_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
  }
  return GSP_OK;
}

int gsp_download_pixel_stats(gsp_context* ctx, float* second_moment, uint32_t* spp) {
  if (!ctx || !ctx->have_frame) return GSP_ERR_INVALID;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  {
    int rc_ = pipeline_drain(ctx);
    if (rc_ != GSP_OK) return rc_;
  }
  if (ctx->frame_mode != gsp_context::kFrameAdaptive) {
    ctx->err = "gsp_download_pixel_stats: the frame is not adaptive (no gsp_render with adaptive_threshold > 0 since gsp_frame_begin)";
    return GSP_ERR_INVALID;
  }
  if (second_moment) CTX_TRY(ctx, hipMemcpy(second_moment, ctx->pix_m2.p, ctx->num_pixels * sizeof(float), hipMemcpyDeviceToHost));
  if (spp) CTX_TRY(ctx, hipMemcpy(spp, ctx->pix_spp.p, ctx->num_pixels * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return GSP_OK;
}

#ifdef GSP_SHADE_PROFILE
// measurement build only (scripts/shade_lane_profile.py): read and clear the lane profile of k_shade
extern "C" void gsp_debug_shade_profile(unsigned long long* out) {
  (void)hipDeviceSynchronize();
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(gsp::g_shade_profile), PR_COUNT * 4 * sizeof(unsigned long long));
  static const unsigned long long zero[PR_COUNT * 4] = {};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(gsp::g_shade_profile), zero, sizeof(zero));
}
#endif
#ifdef GSP_WAVE_PROFILE
// measurement build only (scripts/trace_phase_budget.py): read and clear the 2 x 24 counters of pt_wavetrace.h
extern "C" void gsp_debug_wave_profile(unsigned long long* out) {
  (void)hipDeviceSynchronize();
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(gsp::g_wave_profile), 48 * sizeof(unsigned long long));
  static const unsigned long long zero[48] = {};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(gsp::g_wave_profile), zero, sizeof(zero));
}
#endif

int gsp_sync(gsp_context* ctx) {
  if (!ctx) return GSP_ERR_INVALID;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  {
    int rc = pipeline_drain(ctx);
    if (rc != GSP_OK) return rc;
  }
  CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return GSP_OK;
}

// the two pinned staging buffers of the frame read-back (12 ms the first time: gsp_frame_begin makes them with the frame's other buffers)
static int ensure_read_back_stage(gsp_context* ctx) {
  for (int k = 0; k < 2; ++k) {
    if (!ctx->h_stage[k]) CTX_TRY(ctx, hipHostMalloc((void**)&ctx->h_stage[k], gsp_context::kStageBytes, hipHostMallocDefault));
    if (!ctx->stage_ev[k]) CTX_TRY(ctx, hipEventCreateWithFlags(&ctx->stage_ev[k], hipEventDisableTiming));
  }
  return GSP_OK;
}
// the accumulate buffer -> caller's host memory, through the two pinned staging buffers (gsp_context::h_stage)
static int read_back_bytes(gsp_context* ctx, const void* device_src, size_t total, void* out);
static int read_back_frame(gsp_context* ctx, float* out) { return read_back_bytes(ctx, ctx->accum.p, ctx->num_pixels * sizeof(q4), out); }
// (the same for any device buffer of the context: the RGBA8 frame of the LDR film goes through the same two staging buffers)
static int read_back_bytes(gsp_context* ctx, const void* device_src, size_t total, void* out) {
  if (total <= gsp_context::kStageBytes / 4) {  // small frames: one plain copy
    CTX_TRY(ctx, hipMemcpyAsync(out, device_src, total, hipMemcpyDeviceToHost, ctx->stream));
    CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GSP_OK;
  }
  {
    int rc_ = ensure_read_back_stage(ctx);
    if (rc_ != GSP_OK) return rc_;
  }
  const size_t chunks = (total + gsp_context::kStageBytes - 1) / gsp_context::kStageBytes;
  const uint8_t* src = (const uint8_t*)device_src;
  auto bytes_of = [&](size_t c) { return std::min(gsp_context::kStageBytes, total - c * gsp_context::kStageBytes); };
  CTX_TRY(ctx, hipMemcpyAsync(ctx->h_stage[0], src, bytes_of(0), hipMemcpyDeviceToHost, ctx->stream));
  CTX_TRY(ctx, hipEventRecord(ctx->stage_ev[0], ctx->stream));
  for (size_t c = 0; c < chunks; ++c) {
    if (c + 1 < chunks) {  // (buffer (c + 1) & 1 was drained by the memcpy of chunk c - 1, below, before this point)
      CTX_TRY(ctx, hipMemcpyAsync(ctx->h_stage[(c + 1) & 1], src + (c + 1) * gsp_context::kStageBytes, bytes_of(c + 1), hipMemcpyDeviceToHost, ctx->stream));
      CTX_TRY(ctx, hipEventRecord(ctx->stage_ev[(c + 1) & 1], ctx->stream));
    }
    CTX_TRY(ctx, hipEventSynchronize(ctx->stage_ev[c & 1]));
    std::memcpy((uint8_t*)out + c * gsp_context::kStageBytes, ctx->h_stage[c & 1], bytes_of(c));
  }
  return GSP_OK;
}

int gsp_download_compact(gsp_context* ctx, float* out) {
  if (!ctx || !out || !ctx->have_frame) return GSP_ERR_INVALID;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  {
    int rc_ = pipeline_drain(ctx);
    if (rc_ != GSP_OK) return rc_;
  }
  return read_back_frame(ctx, out);
}

int gsp_peek(gsp_context* ctx, float* out, uint32_t* samples_folded) {
  if (!ctx || !out || !ctx->have_frame) return GSP_ERR_INVALID;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  // no drain: the folds queued so far finish, the paths in flight keep their state
  uint32_t folded = 0xffffffffu;
  for (uint32_t l = 0; l < ctx->num_lanes; ++l) {
    gsp_context::Lane& L = ctx->lanes[l];
    if (L.num_pixels == 0) continue;
    CTX_TRY(ctx, hipStreamSynchronize(L.stream));
    folded = std::min(folded, ctx->pipe_active && L.pipe.active ? L.pipe.folded_end : ctx->folded_idle);
  }
  {
    int rc_ = read_back_frame(ctx, out);
    if (rc_ != GSP_OK) return rc_;
  }
  if (samples_folded) *samples_folded = folded == 0xffffffffu ? 0u : (folded >= ctx->sample_base ? folded - ctx->sample_base : folded);
  return GSP_OK;
}

int gsp_peek_to_device(gsp_context* ctx, void* dst, uint64_t bytes, uint32_t* samples_folded) {
  if (!ctx || !dst || !ctx->have_frame) return GSP_ERR_INVALID;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  if (bytes < ctx->num_pixels * sizeof(q4)) {
    ctx->err = "destination too small";
    return GSP_ERR_INVALID;
  }
  uint32_t folded = 0xffffffffu;
  for (uint32_t l = 0; l < ctx->num_lanes; ++l) {  // (as gsp_peek: the folds queued so far finish, the paths in flight stay)
    gsp_context::Lane& L = ctx->lanes[l];
    if (L.num_pixels == 0) continue;
    CTX_TRY(ctx, hipStreamSynchronize(L.stream));
    folded = std::min(folded, ctx->pipe_active && L.pipe.active ? L.pipe.folded_end : ctx->folded_idle);
  }
  CTX_TRY(ctx, hipMemcpyAsync(dst, ctx->accum.p, ctx->num_pixels * sizeof(q4), hipMemcpyDeviceToDevice, ctx->stream));
  CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (samples_folded) *samples_folded = folded == 0xffffffffu ? 0u : (folded >= ctx->sample_base ? folded - ctx->sample_base : folded);
  return GSP_OK;
}

int gsp_download(gsp_context* ctx, float* out) {
  if (!ctx || !out || !ctx->have_frame) return GSP_ERR_INVALID;
  if (!ctx->subset) return gsp_download_compact(ctx, out);
  std::vector<float> tmp(4ull * ctx->num_pixels);
  int rc = gsp_download_compact(ctx, tmp.data());
  if (rc != GSP_OK) return rc;
  std::memset(out, 0, sizeof(float) * 4ull * ctx->width * ctx->height);
  for (uint64_t i = 0; i < ctx->num_pixels; ++i)
    std::memcpy(out + 4ull * ctx->pixel_ids_host[i], tmp.data() + 4ull * i, 4 * sizeof(float));
  return GSP_OK;
}

int gsp_copy_accum_to_device(gsp_context* ctx, void* dst, uint64_t bytes) {
  if (!ctx || !dst || !ctx->have_frame) return GSP_ERR_INVALID;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  {
    int rc_ = pipeline_drain(ctx);
    if (rc_ != GSP_OK) return rc_;
  }
  if (bytes < ctx->num_pixels * sizeof(q4)) {
    ctx->err = "destination too small";
    return GSP_ERR_INVALID;
  }
  CTX_TRY(ctx, hipMemcpyAsync(dst, ctx->accum.p, ctx->num_pixels * sizeof(q4), hipMemcpyDeviceToDevice, ctx->stream));
  CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return GSP_OK;
}

// ---- first-hit feature buffers (include/gpuspectral_pt.h, "Feature buffers"; per-hit code: pt_features.h) ----
// the three planes of the current frame: made by the first call that asks for them, zeroed once per frame
static int ensure_features(gsp_context* ctx) {
  if (ctx->features_ready) return GSP_OK;
  const size_t n = std::max<uint64_t>(ctx->num_pixels, 1);
  for (DevBuf<q4>* b : {&ctx->feat_albedo, &ctx->feat_geom, &ctx->feat_ids}) {
    CTX_TRY(ctx, b->ensure(n, &ctx->bytes));
    CTX_TRY(ctx, hipMemsetAsync(b->p, 0, n * sizeof(q4), ctx->stream));
  }
  ctx->features_ready = true;
  return GSP_OK;
}

}  // extern "C"

template <bool TEX, int CAMERA>
static void launch_features(gsp_context* ctx, const SceneView& view, const RenderConstsLens& rc, const FeatureGeo& geo, const gsp_render_params* rp) {
  const uint32_t n = (uint32_t)ctx->num_pixels;
  hipLaunchKernelGGL((k_features<TEX, CAMERA>), dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, view,
                     static_cast<const typename FeatureConsts<CAMERA>::type&>(rc), geo, n, rp->spp, rp->first_timestamp,
                     ctx->subset ? (const uint32_t*)ctx->pixel_ids.p : (const uint32_t*)nullptr, ctx->feat_albedo.p, ctx->feat_geom.p,
                     (v4w*)ctx->feat_ids.p);
}

extern "C" {

int gsp_render_features(gsp_context* ctx, const gsp_render_params* rp_host) {
  if (!ctx || !rp_host) return GSP_ERR_INVALID;
  gsp_render_params rp_copy;  // struct_size: the rule of gsp_render (fields beyond the host's struct are 0)
  std::memset(&rp_copy, 0, sizeof(rp_copy));
  {
    const size_t abi8 = offsetof(gsp_render_params, disable_nee) + sizeof(uint32_t);
    const size_t n = rp_host->struct_size ? std::min<size_t>(rp_host->struct_size, sizeof(rp_copy)) : abi8;
    if (n < abi8) {
      ctx->err = "gsp_render_params.struct_size " + std::to_string(rp_host->struct_size) + " is smaller than the ABI-8 struct (" + std::to_string(abi8) +
                 " bytes): set it with gsp_default_render_params or sizeof(gsp_render_params)";
      return GSP_ERR_INVALID;
    }
    std::memcpy(&rp_copy, rp_host, n);
  }
  const gsp_render_params* const rp = &rp_copy;
  if (!ctx->have_scene || !ctx->have_frame) {
    ctx->err = "gsp_render_features needs gsp_upload_scene and gsp_frame_begin first";
    return GSP_ERR_INVALID;
  }
  if (rp->spp == 0) {
    ctx->err = "gsp_render_features: spp must be at least 1";
    return GSP_ERR_INVALID;
  }
  if (rp->pixel_filter > GSP_FILTER_GAUSSIAN) {
    ctx->err = "pixel_filter " + std::to_string(rp->pixel_filter) + " is not a GSP_FILTER_* value";
    return GSP_ERR_INVALID;
  }
  if (!(rp->pixel_filter_param >= 0.0f) || std::isinf(rp->pixel_filter_param)) {
    ctx->err = "pixel_filter_param must be 0 (the filter's default) or a finite positive value";
    return GSP_ERR_INVALID;
  }
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  // NO DRAIN: the samples gsp_render has left in flight stay where they are (between two calls nothing of them runs: every lane's
  // stream is idle) and finish with the next gsp_render / gsp_download, exactly as without this call -- the pipeline, the accumulate
  // buffer, the memo, the pixel statistics and every counter of gsp_stats are not touched.  The pass reads ONE version of the
  // scene, the newest: the context's own tree pointers and the newest slot of the table ring, as gsp_trace does.
  if (std::max(ctx->bvh.depth, ctx->split ? ctx->dyn.depth : 0u) + 2 > kFinishLevels) {
    ctx->err = "gsp_render_features: the scene's BVH has " + std::to_string(std::max(ctx->bvh.depth, ctx->split ? ctx->dyn.depth : 0u)) +
               " levels, the per-lane traversal stack holds " + std::to_string(kFinishLevels - 2);
    return GSP_ERR_INVALID;
  }
  {
    int rc_ = ensure_features(ctx);
    if (rc_ != GSP_OK) return rc_;
  }
  if (!ctx->features_rendered) ctx->feat_inst_edits = ctx->inst_edits;  // (the frame's first call: whose transforms its planes show)
  if (ctx->num_pixels == 0) {
    ctx->features_rendered = true;
    return GSP_OK;
  }
  if (ctx->split && !ctx->s2g_all_valid) {
    int rc_ = make_split_s2g(ctx);
    if (rc_ != GSP_OK) return rc_;
  }
  // the newest version of everything: the tables from wherever their ring holds it, the tree(s) from the context's own pointers
  // (a split scene: `bvh` is the static tree at the front of the ring, `dyn` the newest slot of the edited instances' tree)
  SceneView view = ctx->view(true, true);
  view.nodes = ctx->bvh.nodes;
  view.tri_isect = ctx->bvh.tri_isect;
  view.tri_shade = ctx->bvh.tri_shade;
  FeatureGeo geo{};
  if (ctx->split) {
    geo.dyn_nodes = ctx->dyn.nodes;
    geo.dyn_isect = ctx->dyn.tri_isect;
    geo.dyn_shade = ctx->dyn.tri_shade;
    geo.static_slots = ctx->static_slots;
  }
  geo.num_tris = (uint32_t)ctx->total_tris;
  geo.slot_to_global = ctx->split ? ctx->s2g_all.p : ctx->bvh.slot_to_global;
  geo.tri_first = ctx->d_first.p;
  geo.num_instances = (uint32_t)ctx->h_inst.size();
  const RenderConstsLens rc = render_consts(ctx, rp);
  const int camera = rc.lens_radius > 0.0f ? 2 : (rc.pixel_filter != GSP_FILTER_NONE ? 1 : 0);
  if (ctx->textured) {
    if (camera == 2) launch_features<true, 2>(ctx, view, rc, geo, rp);
    else if (camera == 1) launch_features<true, 1>(ctx, view, rc, geo, rp);
    else launch_features<true, 0>(ctx, view, rc, geo, rp);
  } else {
    if (camera == 2) launch_features<false, 2>(ctx, view, rc, geo, rp);
    else if (camera == 1) launch_features<false, 1>(ctx, view, rc, geo, rp);
    else launch_features<false, 0>(ctx, view, rc, geo, rp);
  }
  CTX_TRY(ctx, hipGetLastError());
  CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the pass is complete when the call returns: a scene edit may follow at once)
  ctx->features_rendered = true;
  return GSP_OK;
}

// one compact plane -> `out` in the full-frame layout (unowned pixels 0), through read_back_bytes
static int download_feature_plane(gsp_context* ctx, const q4* plane, void* out) {
  if (!out) return GSP_OK;
  if (!ctx->subset) return read_back_bytes(ctx, plane, ctx->num_pixels * sizeof(q4), out);
  std::vector<q4> tmp(ctx->num_pixels);
  int rc = read_back_bytes(ctx, plane, ctx->num_pixels * sizeof(q4), tmp.data());
  if (rc != GSP_OK) return rc;
  std::memset(out, 0, sizeof(q4) * (size_t)ctx->width * ctx->height);
  for (uint64_t i = 0; i < ctx->num_pixels; ++i) std::memcpy((uint8_t*)out + sizeof(q4) * ctx->pixel_ids_host[i], &tmp[i], sizeof(q4));
  return GSP_OK;
}

int gsp_download_features(gsp_context* ctx, float* albedo, float* geom, uint32_t* ids) {
  if (!ctx || !ctx->have_frame) return GSP_ERR_INVALID;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  int rc = ensure_features(ctx);
  if (rc == GSP_OK && ctx->num_pixels == 0) {
    const size_t bytes = sizeof(q4) * (size_t)ctx->width * ctx->height;
    for (void* o : {(void*)albedo, (void*)geom, (void*)ids})
      if (o) std::memset(o, 0, bytes);
    return GSP_OK;
  }
  if (rc == GSP_OK) rc = download_feature_plane(ctx, ctx->feat_albedo.p, albedo);
  if (rc == GSP_OK) rc = download_feature_plane(ctx, ctx->feat_geom.p, geom);
  if (rc == GSP_OK) rc = download_feature_plane(ctx, ctx->feat_ids.p, ids);
  return rc;
}

int gsp_copy_features_to_device(gsp_context* ctx, void* albedo, void* geom, void* ids, uint64_t bytes_each) {
  if (!ctx || !ctx->have_frame) return GSP_ERR_INVALID;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  if (bytes_each < ctx->num_pixels * sizeof(q4)) {
    ctx->err = "destination too small";
    return GSP_ERR_INVALID;
  }
  int rc = ensure_features(ctx);
  if (rc != GSP_OK) return rc;
  const size_t n = ctx->num_pixels * sizeof(q4);
  if (albedo && n) CTX_TRY(ctx, hipMemcpyAsync(albedo, ctx->feat_albedo.p, n, hipMemcpyDeviceToDevice, ctx->stream));
  if (geom && n) CTX_TRY(ctx, hipMemcpyAsync(geom, ctx->feat_geom.p, n, hipMemcpyDeviceToDevice, ctx->stream));
  if (ids && n) CTX_TRY(ctx, hipMemcpyAsync(ids, ctx->feat_ids.p, n, hipMemcpyDeviceToDevice, ctx->stream));
  CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return GSP_OK;
}

}  // extern "C"

// gsp_multi_*: the three compact feature planes of a share (device pointers; complete: gsp_render_features returns synchronised)
int gsp::gsp_internal_features(gsp_context* ctx, void** albedo, void** geom, void** ids, uint64_t* num_pixels) {
  if (!ctx || !ctx->have_frame) return GSP_ERR_INVALID;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  int rc = ensure_features(ctx);
  if (rc != GSP_OK) return rc;
  CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *albedo = ctx->feat_albedo.p;
  *geom = ctx->feat_geom.p;
  *ids = ctx->feat_ids.p;
  *num_pixels = ctx->num_pixels;
  return GSP_OK;
}

int gsp::gsp_internal_features_rendered(const gsp_context* ctx) { return ctx && ctx->have_frame && ctx->features_rendered ? 1 : 0; }

int gsp::gsp_internal_accum(gsp_context* ctx, void** accum, uint64_t* num_pixels, hipStream_t* stream) {
  if (!ctx || !ctx->have_frame) return GSP_ERR_INVALID;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  int rc = pipeline_drain(ctx);
  if (rc != GSP_OK) return rc;
  CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (accum) *accum = ctx->accum.p;
  if (num_pixels) *num_pixels = ctx->num_pixels;
  if (stream) *stream = ctx->stream;
  return GSP_OK;
}

extern "C" {

int gsp_upload_accum(gsp_context* ctx, const float* rgba, uint64_t num_pixels) {
  if (!ctx || !rgba || !ctx->have_frame || num_pixels != ctx->num_pixels) return GSP_ERR_INVALID;
  if (ctx->frame_mode == gsp_context::kFrameAdaptive) {
    ctx->err = "gsp_upload_accum: not available in an adaptive frame (its per-pixel m2 and counts cannot be restored)";
    return GSP_ERR_INVALID;
  }
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  {
    int rc_ = pipeline_drain(ctx);
    if (rc_ != GSP_OK) return rc_;
  }
  CTX_TRY(ctx, hipMemcpyAsync(ctx->accum.p, rgba, num_pixels * sizeof(q4), hipMemcpyHostToDevice, ctx->stream));
  CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return GSP_OK;
}

int gsp_get_stats(gsp_context* ctx, gsp_stats* out) {
  if (!ctx || !out) return GSP_ERR_INVALID;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  {
    int rc_ = pipeline_drain(ctx);
    if (rc_ != GSP_OK) return rc_;
  }
  if (ctx->dstats.p) {
    DevStats d;
    CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));
    CTX_TRY(ctx, hipMemcpy(&d, ctx->dstats.p, sizeof(d), hipMemcpyDeviceToHost));
    ctx->stats.shaded_vertices = d.shaded;
    ctx->stats.nodes_visited = d.nodes;
    ctx->stats.tris_tested = d.tris;
    ctx->stats.stat_rays = d.stat_rays;
    ctx->stats.shadow_nodes_visited = d.sh_nodes;
    ctx->stats.shadow_tris_tested = d.sh_tris;
    ctx->stats.shadow_stat_rays = d.sh_rays;
    ctx->stats.nodes_from_lds = d.lds_nodes;
    ctx->stats.shadow_nodes_from_lds = d.sh_lds_nodes;
    ctx->stats.shadow_stat_occluded = d.sh_occluded;
    ctx->stats.shadow_stat_occluded_nodes = d.sh_occluded_nodes;
    ctx->stats.shadow_stat_no_triangle = d.sh_no_tri;
  }
  ctx->stats.bvh_build_ms = ctx->bvh_build_ms;
  ctx->stats.num_triangles = ctx->bvh.num_tris;  // (a split scene: the static tree keeps a slot for every triangle of the scene)
  ctx->stats.num_bvh_nodes = ctx->bvh.num_nodes + (ctx->split ? ctx->dyn.num_nodes : 0u);
  ctx->stats.bvh_depth = std::max(ctx->bvh.depth, ctx->split ? ctx->dyn.depth : 0u);
  ctx->stats.device_bytes = ctx->bytes.bytes;
  ctx->stats.adaptive_active_pixels = ctx->frame_mode == gsp_context::kFrameAdaptive ? ctx->active_pixels() : 0u;
  ctx->stats.algorithmic_bytes = 48ull * ctx->stats.stat_rays + (uint64_t)kNodeBytes * ctx->stats.nodes_visited + 48ull * ctx->stats.tris_tested +
                                 32ull * ctx->stats.shadow_stat_rays + 36ull * ctx->stats.shadow_stat_occluded +
                                 (uint64_t)kNodeBytes * ctx->stats.shadow_nodes_visited + 48ull * ctx->stats.shadow_tris_tested;
  *out = ctx->stats;
  return GSP_OK;
}

int gsp_reset_stats(gsp_context* ctx) {
  if (!ctx) return GSP_ERR_INVALID;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  {
    int rc_ = pipeline_drain(ctx);
    if (rc_ != GSP_OK) return rc_;
  }
  const uint64_t updates = ctx->stats.scene_updates, refits = ctx->stats.scene_refits, drains = ctx->stats.scene_drains,
                 splits = ctx->stats.scene_splits;  // (counts since the last gsp_upload_scene, not since the last reset)
  ctx->stats = gsp_stats{};
  ctx->stats.scene_updates = updates;
  ctx->stats.scene_refits = refits;
  ctx->stats.scene_drains = drains;
  ctx->stats.scene_splits = splits;
  if (ctx->dstats.p) {
    CTX_TRY(ctx, hipMemsetAsync(ctx->dstats.p, 0, sizeof(DevStats), ctx->stream));
    CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  return GSP_OK;
}

// ---- thin lens (include/gpuspectral_pt.h, "Thin lens") ----
int gsp_set_lens(gsp_context* ctx, const gsp_lens* lens_host) {
  if (!ctx) return GSP_ERR_INVALID;
  gsp_lens l;
  if (const char* why = resolve_lens(lens_host, l)) {
    ctx->err = why;
    return GSP_ERR_INVALID;
  }
  ctx->lens = l;  // no drain, and the memo stays: it holds the pinhole rays' hits, which a lens call does not read
  return GSP_OK;
}

// A context with delta lights (or the environment light or the light grid switched on) runs the <MED, SCT, DLT> kernels whatever its media (pt_render_delta.hip, pt_render_envlight.hip).  Where it holds media but
// no scattering table, those kernels read one of zeros from the table's device buffer: every medium then takes the deterministic
// line of the absorbing kernels.  Called behind every change of the three tables, under a drained pipeline.
static int sync_absorbing_scatter_table(gsp_context* ctx) {
  if ((ctx->h_delta.empty() && ctx->env_sampling.enabled == 0u && ctx->light_grid.enabled == 0u) || ctx->num_media == 0 || !ctx->h_scatter.empty()) return GSP_OK;
  const std::vector<gsp_medium_scatter> zeros(ctx->num_media, gsp_medium_scatter{{0.0f, 0.0f, 0.0f}, 0.0f});
  CTX_TRY(ctx, ctx->scatter.upload(zeros.data(), zeros.size(), ctx->stream, &ctx->bytes));
  CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (`zeros` goes out of scope; the lanes' streams read the table)
  return GSP_OK;
}

// ---- interior media (include/gpuspectral_pt.h, "Interior media") ----
int gsp_set_media(gsp_context* ctx, const gsp_medium* media, uint32_t num_media) {
  if (!ctx) return GSP_ERR_INVALID;
  if (const char* why = check_media(media, num_media)) {
    ctx->err = why;
    return GSP_ERR_INVALID;
  }
  const uint32_t n = media ? num_media : 0u;
  if (ctx->have_scene && max_medium_number(ctx->h_inst.data(), ctx->h_inst.size()) > n) {
    ctx->err = "gsp_set_media: the resident scene names a medium number above the new count";
    return GSP_ERR_INVALID;
  }
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  int rc = drain_for_edit(ctx);  // the samples in flight read the table as it was
  if (rc != GSP_OK) return rc;
  ctx->h_media.assign(media, media + n);
  for (gsp_medium& m : ctx->h_media) m.reserved = 0.0f;
  if (n != 0) {
    CTX_TRY(ctx, ctx->media.upload(ctx->h_media.data(), n, ctx->stream, &ctx->bytes));
    CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the lanes' streams read it)
  }
  if (n != ctx->num_media) {  // the scattering table is parallel to this one: another count drops it
    ctx->h_scatter.clear();
    ctx->scatter_on = false;
  }
  ctx->num_media = n;
  return sync_absorbing_scatter_table(ctx);
}

// ---- scattering media (include/gpuspectral_pt.h, "Scattering media") ----
int gsp_set_media_scattering(gsp_context* ctx, const gsp_medium_scatter* scatter, uint32_t num_media) {
  if (!ctx) return GSP_ERR_INVALID;
  if (const char* why = check_media_scattering(scatter, num_media, ctx->num_media)) {
    ctx->err = why;
    return GSP_ERR_INVALID;
  }
  const uint32_t n = scatter ? num_media : 0u;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  int rc = drain_for_edit(ctx);  // the samples in flight read the table as it was
  if (rc != GSP_OK) return rc;
  ctx->h_scatter.assign(scatter, scatter + n);
  if (n != 0) {
    CTX_TRY(ctx, ctx->scatter.upload(ctx->h_scatter.data(), n, ctx->stream, &ctx->bytes));
    CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the lanes' streams read it)
  }
  ctx->scatter_on = any_scattering(ctx->h_scatter.data(), n);
  return sync_absorbing_scatter_table(ctx);
}

// ---- light selection (include/gpuspectral_pt.h, "Light selection") ----
static_assert(sizeof(gsp_light_pick) == 16 && sizeof(gsp_triangle_light) % 16 == 0, "the pick table starts straight behind the light records, on a 16-byte boundary");
// A resident scene under a drained pipeline: its tables are packed again from the context's host copy (the caller's records, as
// they came) and uploaded, in the layout of the context's light mode and estimator as they are NOW.  No scene: nothing to do.
static int repack_resident_tables(gsp_context* ctx) {
  if (!ctx->have_scene || ctx->h_tables.size() < TableImage::kHead) return GSP_OK;
  gsp_scene_desc sc{};
  uint64_t counts[9];
  std::memcpy(counts, ctx->h_tables.data(), sizeof(counts));
  const uint8_t* tb = ctx->h_tables.data() + TableImage::kHead;
  for (int k = 0; k < GSP_BSDF_TYPE_COUNT; ++k) sc.num_bsdfs[k] = (uint32_t)counts[k];
  sc.diffuse_bsdfs = (const gsp_diffuse_bsdf*)(tb + ctx->table_off[0]);
  sc.smooth_dielectric_bsdfs = (const gsp_smooth_dielectric_bsdf*)(tb + ctx->table_off[1]);
  sc.smooth_conductor_bsdfs = (const gsp_smooth_conductor_bsdf*)(tb + ctx->table_off[2]);
  sc.smooth_plastic_bsdfs = (const gsp_smooth_plastic_bsdf*)(tb + ctx->table_off[3]);
  sc.rough_conductor_bsdfs = (const gsp_rough_conductor_bsdf*)(tb + ctx->table_off[4]);
  sc.smooth_floor_bsdfs = (const gsp_smooth_floor_bsdf*)(tb + ctx->table_off[5]);
  sc.rough_floor_bsdfs = (const gsp_rough_floor_bsdf*)(tb + ctx->table_off[6]);
  sc.rough_plastic_bsdfs = (const gsp_rough_plastic_bsdf*)(tb + ctx->table_off[7]);
  sc.lights = (const gsp_triangle_light*)(tb + ctx->table_off[8]);
  sc.num_lights = (uint32_t)counts[8];
  TableImage img;
  int rc = pack_tables(ctx, &sc, img);  // (copies out of h_tables into the new image; upload_tables then swaps the two)
  if (rc == GSP_OK) rc = upload_tables(ctx, &sc, img);
  if (rc != GSP_OK) {
    ctx->have_scene = false;
    return rc;
  }
  CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return GSP_OK;
}

int gsp_set_light_sampling(gsp_context* ctx, uint32_t mode) {
  if (!ctx) return GSP_ERR_INVALID;
  if (mode != GSP_LIGHTS_UNIFORM && mode != GSP_LIGHTS_POWER) {
    ctx->err = "gsp_set_light_sampling: unknown mode";
    return GSP_ERR_INVALID;
  }
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  int rc = drain_for_edit(ctx);  // the samples in flight were generated under the mode as it was
  if (rc != GSP_OK) return rc;
  if (mode == ctx->light_mode) return GSP_OK;
  if (mode != GSP_LIGHTS_POWER && ctx->light_grid.enabled != 0u) {
    ctx->err = "gsp_set_light_sampling: the light grid is on, and it exists under GSP_LIGHTS_POWER only";
    return GSP_ERR_INVALID;
  }
  const uint32_t old_mode = ctx->light_mode;
  ctx->light_mode = mode;
  rc = repack_resident_tables(ctx);
  if (rc != GSP_OK) ctx->light_mode = old_mode;
  return rc;
}

// ---- estimator (include/gpuspectral_pt.h, "Estimator") ----
int gsp_set_estimator(gsp_context* ctx, uint32_t mode) {
  if (!ctx) return GSP_ERR_INVALID;
  if (mode != GSP_ESTIMATOR_REFERENCE && mode != GSP_ESTIMATOR_TEXTBOOK) {
    ctx->err = "gsp_set_estimator: unknown mode";
    return GSP_ERR_INVALID;
  }
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  int rc = drain_for_edit(ctx);  // the samples in flight carry the directWeight / lastPdf of the mode as it was
  if (rc != GSP_OK) return rc;
  if (mode == ctx->estimator) return GSP_OK;
  if (mode == GSP_ESTIMATOR_REFERENCE && ctx->env_sampling.enabled != 0u) {
    ctx->err = "gsp_set_estimator: envmap sampling is on, and the environment light exists under GSP_ESTIMATOR_TEXTBOOK only";
    return GSP_ERR_INVALID;
  }
  if (mode == GSP_ESTIMATOR_REFERENCE && ctx->light_grid.enabled != 0u) {
    ctx->err = "gsp_set_estimator: the light grid is on, and it exists under GSP_ESTIMATOR_TEXTBOOK only";
    return GSP_ERR_INVALID;
  }
  const uint32_t old_mode = ctx->estimator;
  ctx->estimator = mode;
  if (ctx->light_mode != GSP_LIGHTS_POWER) return GSP_OK;  // (the tables of a uniform-pick context are the same in both modes)
  rc = repack_resident_tables(ctx);  // with or without the trailing record behind the pick table
  if (rc != GSP_OK) ctx->estimator = old_mode;
  return rc;
}

// ---- delta lights (include/gpuspectral_pt.h, "Delta lights") ----
int gsp_set_delta_lights(gsp_context* ctx, const gsp_delta_light* lights, uint32_t count) {
  if (!ctx) return GSP_ERR_INVALID;
  if (const char* why = check_delta_lights(lights, count)) {
    ctx->err = why;
    return GSP_ERR_INVALID;
  }
  std::vector<gsp_delta_light> accepted(lights ? count : 0u);
  for (size_t k = 0; k < accepted.size(); ++k) accepted[k] = accept_delta_light(lights[k]);
  if ((uint64_t)ctx->num_tri_lights + accepted.size() > 0xffffffffull) {
    ctx->err = "gsp_set_delta_lights: too many lights";
    return GSP_ERR_INVALID;
  }
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  int rc = drain_for_edit(ctx);  // the samples in flight read the light table as it was
  if (rc != GSP_OK) return rc;
  if (accepted.size() == ctx->h_delta.size() && (accepted.empty() || std::memcmp(accepted.data(), ctx->h_delta.data(), sizeof(gsp_delta_light) * accepted.size()) == 0))
    return GSP_OK;
  ctx->h_delta.swap(accepted);
  rc = repack_resident_tables(ctx);  // the records ride behind the triangle lights of the table image
  if (rc != GSP_OK) {
    ctx->h_delta.swap(accepted);
    return rc;
  }
  return sync_absorbing_scatter_table(ctx);
}

// ---- environment light (include/gpuspectral_pt.h, "Environment light") ----
int gsp_set_envmap_sampling(gsp_context* ctx, const gsp_envmap_sampling* sampling) {
  if (!ctx) return GSP_ERR_INVALID;
  if (const char* why = check_envmap_sampling(sampling)) {
    ctx->err = why;
    return GSP_ERR_INVALID;
  }
  gsp_envmap_sampling want{};
  if (sampling && sampling->enabled != 0u) want.enabled = 1u, want.extent = sampling->extent;
  if (want.enabled != 0u && ctx->estimator != GSP_ESTIMATOR_TEXTBOOK) {
    ctx->err = "gsp_set_envmap_sampling: the environment light exists under GSP_ESTIMATOR_TEXTBOOK only (gsp_set_estimator first)";
    return GSP_ERR_INVALID;
  }
  if (want.enabled != 0u && ctx->light_grid.enabled != 0u) {
    ctx->err = "gsp_set_envmap_sampling: the light grid is on, and the environment record has no selection probability per cell (gsp_set_light_grid(NULL) first)";
    return GSP_ERR_INVALID;
  }
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  int rc = drain_for_edit(ctx);  // the samples in flight read the light table as it was
  if (rc != GSP_OK) return rc;
  if (std::memcmp(&want, &ctx->env_sampling, sizeof(want)) == 0) return GSP_OK;
  const bool with_map = ctx->have_scene && ctx->env_width != 0u;
  const bool on = want.enabled != 0u && with_map;
  if (on && !env_frame_is_rotation(ctx->env_to_local)) {
    ctx->err = "gsp_set_envmap_sampling: the upper 3x3 of the resident envmap's to_local is not orthonormal within 1e-4";
    return GSP_ERR_INVALID;
  }
  if (on && ctx->h_env_cells.empty()) {  // the scene came before the switch: its texels come back from the device once
    std::vector<float> texels(4ull * ctx->env_width * ctx->env_height);
    CTX_TRY(ctx, hipMemcpyAsync(texels.data(), ctx->env_texels.p, texels.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));
    rc = build_env_light(ctx, texels.data(), ctx->env_width, ctx->env_height, ctx->env_to_local);
    if (rc != GSP_OK) return rc;
    CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  const gsp_envmap_sampling old = ctx->env_sampling;
  const bool old_on = ctx->env_light;
  ctx->env_sampling = want;
  ctx->env_light = on;
  if (on || old_on) {
    rc = repack_resident_tables(ctx);  // with or without the record behind the delta records
    if (rc != GSP_OK) {
      ctx->env_sampling = old;
      ctx->env_light = old_on;
      return rc;
    }
  }
  return sync_absorbing_scatter_table(ctx);
}

// ---- light grid (include/gpuspectral_pt.h, "Light grid") ----
int gsp_set_light_grid(gsp_context* ctx, const gsp_light_grid* grid) {
  if (!ctx) return GSP_ERR_INVALID;
  if (const char* why = check_light_grid(grid)) {
    ctx->err = why;
    return GSP_ERR_INVALID;
  }
  gsp_light_grid want{};
  if (grid && grid->enabled != 0u) {
    want.enabled = 1u;
    for (int c = 0; c < 3; ++c) want.resolution[c] = grid->resolution[c];
  }
  if (want.enabled != 0u && ctx->light_mode != GSP_LIGHTS_POWER) {
    ctx->err = "gsp_set_light_grid: the light grid exists under GSP_LIGHTS_POWER only (gsp_set_light_sampling first)";
    return GSP_ERR_INVALID;
  }
  if (want.enabled != 0u && ctx->estimator != GSP_ESTIMATOR_TEXTBOOK) {
    ctx->err = "gsp_set_light_grid: the light grid exists under GSP_ESTIMATOR_TEXTBOOK only (gsp_set_estimator first)";
    return GSP_ERR_INVALID;
  }
  if (want.enabled != 0u && ctx->env_sampling.enabled != 0u) {
    ctx->err = "gsp_set_light_grid: envmap sampling is on, and the environment record has no selection probability per cell (gsp_set_envmap_sampling(NULL) first)";
    return GSP_ERR_INVALID;
  }
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  int rc = drain_for_edit(ctx);  // the samples in flight read the light table as it was
  if (rc != GSP_OK) return rc;
  if (std::memcmp(&want, &ctx->light_grid, sizeof(want)) == 0) return GSP_OK;
  if (want.enabled != 0u && ctx->have_scene) {  // (checked before anything changes: a refused resolution leaves the resident tables alone)
    uint32_t res[3];
    if (light_grid_applies(ctx, ctx->num_lights) && lightgrid_resolve(want, ctx->scene_lo, ctx->scene_hi, ctx->num_lights, res) != 0) {
      ctx->err = "gsp_set_light_grid: cells * lights is beyond 2^20 entries (a 16 MB table image)";
      return GSP_ERR_NOMEM;
    }
  }
  const gsp_light_grid old = ctx->light_grid;
  ctx->light_grid = want;
  rc = repack_resident_tables(ctx);  // with or without the grid behind the pick table
  if (rc != GSP_OK) {
    ctx->light_grid = old;
    return rc;
  }
  return sync_absorbing_scatter_table(ctx);
}

int gsp_get_light_grid(gsp_context* ctx, gsp_light_grid* resolved, float bounds[6]) {
  if (!ctx) return GSP_ERR_INVALID;
  if (resolved) {
    *resolved = gsp_light_grid{};
    resolved->enabled = ctx->grid_resident ? 1u : 0u;
    for (int c = 0; c < 3; ++c) resolved->resolution[c] = ctx->grid_resident ? ctx->grid_res[c] : 0u;
  }
  if (bounds)
    for (int c = 0; c < 3; ++c) {
      bounds[c] = ctx->grid_resident ? ctx->scene_lo[c] : 0.0f;
      bounds[3 + c] = ctx->grid_resident ? ctx->scene_hi[c] : 0.0f;
    }
  return GSP_OK;
}

int gsp_download_light_pick(gsp_context* ctx, gsp_light_pick* out, uint32_t capacity, uint32_t* count) {
  if (!ctx) return GSP_ERR_INVALID;
  if (count) *count = ctx->have_scene ? ctx->num_lights : 0u;
  if (ctx->light_mode != GSP_LIGHTS_POWER) {
    ctx->err = "gsp_download_light_pick: the context is in GSP_LIGHTS_UNIFORM mode (no table)";
    return GSP_ERR_INVALID;
  }
  if (!ctx->have_scene) {
    ctx->err = "gsp_download_light_pick: no scene";
    return GSP_ERR_INVALID;
  }
  if (capacity < ctx->num_lights || (!out && ctx->num_lights)) {
    ctx->err = "gsp_download_light_pick: capacity below the number of lights";
    return GSP_ERR_INVALID;
  }
  if (ctx->num_lights == 0) return GSP_OK;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  // the resident table of the CURRENT table version (samples in flight may still read older ones)
  const uint8_t* base = ctx->tables.p + (size_t)ctx->tab.slot_of(ctx->tab.ver) * ctx->tab.slot_bytes;
  const size_t off = ctx->table_off[8] + sizeof(gsp_triangle_light) * (size_t)ctx->num_lights;
  CTX_TRY(ctx, hipMemcpyAsync(out, base + off, sizeof(gsp_light_pick) * (size_t)ctx->num_lights, hipMemcpyDeviceToHost, ctx->stream));
  CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return GSP_OK;
}

int gsp_focus_distance(gsp_context* ctx, uint32_t width, uint32_t height, float fx, float fy, float* out) {
  if (!ctx || !out) return GSP_ERR_INVALID;
  if (!ctx->have_scene) {
    ctx->err = "gsp_focus_distance needs gsp_upload_scene first";
    return GSP_ERR_INVALID;
  }
  if (width == 0 || height == 0 || !std::isfinite(fx) || !std::isfinite(fy)) {
    ctx->err = "gsp_focus_distance: width and height must be positive, fx and fy finite";
    return GSP_ERR_INVALID;
  }
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  {  // (a one-off query: the samples already queued finish first, so the traversal below has the device to itself)
    int rc_ = pipeline_drain(ctx);
    if (rc_ != GSP_OK) return rc_;
  }
  // the pinhole ray of fragCoord (fx, fy), as generate_path forms it (camera_dir), and the cosine of its angle to the local z
  RenderConstsBase rc{};
  rc.width = width;
  rc.height = height;
  rc.zplane = (std::max((float)width, (float)height) / 2.0f) / tanf(ctx->camera.fov / 2.0f);
  for (int i = 0; i < 16; ++i) rc.cam_to_world[i] = ctx->camera.to_world[i];
  const f3 d = camera_dir(rc, fx, fy);
  const float cosz = normalize(mk3(-(fx - (float)width / 2.0f), fy - (float)height / 2.0f, rc.zplane)).z;
  const float ray[8] = {ctx->camera.to_world[12], ctx->camera.to_world[13], ctx->camera.to_world[14], 0.0f, d.x, d.y, d.z, 1e10f};
  struct {
    float t, u, v;
    int32_t prim;
  } hit;
  int rc_ = gsp_trace(ctx, ray, 1, 0, &hit);
  if (rc_ != GSP_OK) return rc_;
  *out = hit.prim < 0 ? 0.0f : hit.t * cosz;
  return GSP_OK;
}

}  // extern "C"

// The stages behind the path tracer.  Included here and not behind this file: kernel templates are instantiated in the order of
// their first use (those a launcher template names: where it is first called, in the order of its body), and the k_trace<.., TestIO> of
// gsp_trace below stay the last of the device code.
#include "pt_render_post.inc"

extern "C" {

int gsp_debug_visit_histograms(gsp_context* ctx, uint32_t* node_counts, uint64_t num_nodes, uint32_t* slot_counts, uint64_t num_slots) {
  if (!ctx) return GSP_ERR_INVALID;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  {
    int rc_ = pipeline_drain(ctx);
    if (rc_ != GSP_OK) return rc_;
  }
  if (!ctx->node_hist.p || !ctx->tri_hist.p) {
    ctx->err = "gsp_debug_visit_histograms: no render with collect_traversal_stats = 2 since the last call";
    return GSP_ERR_INVALID;
  }
  if (node_counts) CTX_TRY(ctx, hipMemcpy(node_counts, ctx->node_hist.p, std::min<uint64_t>(num_nodes, ctx->node_hist.count) * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (slot_counts) CTX_TRY(ctx, hipMemcpy(slot_counts, ctx->tri_hist.p, std::min<uint64_t>(num_slots, ctx->tri_hist.count) * sizeof(uint32_t), hipMemcpyDeviceToHost));
  ctx->bytes.sub((ctx->node_hist.count + ctx->tri_hist.count) * sizeof(uint32_t));
  ctx->node_hist.release();
  ctx->tri_hist.release();
  return GSP_OK;
}

int gsp_trace(gsp_context* ctx, const float* rays, uint64_t n, int any_hit, void* hits) {
  if (!ctx || (!rays && n) || (!hits && n)) return GSP_ERR_INVALID;
  if (!ctx->have_scene) {
    ctx->err = "gsp_trace needs gsp_upload_scene first";
    return GSP_ERR_INVALID;
  }
  if (n == 0) return GSP_OK;
  if (n >= (1ull << 31)) return GSP_ERR_INVALID;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  DevBuf<float>& d_rays = ctx->trace_rays;
  DevBuf<q4>& d_hits = ctx->trace_hits;
  DevBuf<uint32_t>& d_work = ctx->trace_work;
  CTX_TRY(ctx, d_rays.upload(rays, 8 * n, ctx->stream, nullptr));
  CTX_TRY(ctx, d_hits.ensure(n, nullptr));
  CTX_TRY(ctx, d_work.ensure(kWorkShards * kWorkStride, nullptr));
  CTX_TRY(ctx, hipMemsetAsync(d_work.p, 0, kWorkShards * kWorkStride * sizeof(uint32_t), ctx->stream));
  if (ctx->split && !ctx->s2g_all_valid) {
    int rc_ = make_split_s2g(ctx);
    if (rc_ != GSP_OK) return rc_;
  }
  const SceneView view = ctx->view();
  const TestIO io{d_rays.p, d_hits.p, ctx->split ? ctx->s2g_all.p : ctx->bvh.slot_to_global, any_hit,
                  ctx->bvh.num_tris};
  const TraceStatsOut none{nullptr, nullptr, nullptr};
  // one version of the scene, the newest (a split scene: both trees, the newest version of the edited one), whatever is in flight
  const LiveVersions V{false, view, GeoRing{view.geo, 0u, ctx->static_slots}, 0u, ctx->geo.phys(ctx->geo.ver + ctx->geo.slots() - ctx->geo.base)};
  launch_trace(ctx, ctx->stream, view, V, false, io, nullptr, (uint32_t)n, 0u, n, kChunkSmall, d_work.p, ctx->lanes[0].spill.p, none);
  CTX_TRY(ctx, hipGetLastError());
  CTX_TRY(ctx, hipMemcpyAsync(hits, d_hits.p, n * sizeof(q4), hipMemcpyDeviceToHost, ctx->stream));
  CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (n > (8u << 20)) {  // a one-off large query does not pin half a gigabyte for the life of the context
    d_rays.release();
    d_hits.release();
  }
  return GSP_OK;
}

}  // extern "C"
