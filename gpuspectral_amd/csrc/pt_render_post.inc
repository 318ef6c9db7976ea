// pt_render_post.inc -- part of the translation unit pt_render.hip (through pt_render_pipeline.inc; not compiled on its
// own).  The host side of the stages behind the path tracer: the LDR film, the denoiser, temporal accumulation, the
// variance-guided filter, the illumination history, the temporal anti-lag and temporal anti-aliasing -- their launchers, guards,
// read-out tails and exports.

// ---- what the stages share: launch shapes, guards with one text, the tails of the *_to_device exports ----
// a grid-stride launch over `n` items: enough blocks for them, at most `per_cu` per compute unit
static uint32_t pointwise_grid(uint64_t n, uint32_t num_cus, uint32_t per_cu) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + kBlock - 1) / kBlock, (uint64_t)num_cus * per_cu));
}

// one block per kDnTileW x kDnTileH tile of a full frame
static dim3 tile_grid(uint32_t width, uint32_t height) { return dim3((width + kDnTileW - 1) / kDnTileW, (height + kDnTileH - 1) / kDnTileH); }

static int refuse_null_output(gsp_context* ctx, const char* who, const void* out_ptr) {
  if (out_ptr) return GSP_OK;
  ctx->err = std::string(who) + ": null output pointer";
  return GSP_ERR_INVALID;
}

// (tp_valid: the history has the size of the frame -- gsp_frame_begin invalidates any other -- and the frame is a full one)
static int refuse_without_full_frame_features(gsp_context* ctx, const char* who) {
  if (ctx->have_frame && !ctx->subset && ctx->features_rendered) return GSP_OK;
  ctx->err = std::string(who) + " needs a full frame (no pixel_ids) and a gsp_render_features call since gsp_frame_begin";
  return GSP_ERR_INVALID;
}

static int refuse_too_small(gsp_context* ctx, uint64_t bytes, uint64_t need) {
  if (bytes >= need) return GSP_OK;
  ctx->err = "destination too small";
  return GSP_ERR_INVALID;
}

// the four 16-byte planes of the filters (denoiser, variance-guided filter): made by the first call that filters
static int ensure_filter_scratch(gsp_context* ctx) {
  const size_t n = std::max<uint64_t>(ctx->num_pixels, 1);
  for (DevBuf<q4>* b : {&ctx->dn_e0, &ctx->dn_e1, &ctx->dn_a, &ctx->dn_out}) CTX_TRY(ctx, b->ensure(n, &ctx->bytes));
  return GSP_OK;
}

// The tail of a *_to_device export whose kernels store 16 bytes at a time: `stage(target)` queues the result into `target` where
// `dst` is aligned so, and else (target == nullptr) into the context's own buffer `own`, of which `dst` then gets a copy of `need`
// bytes.  dst == nullptr (a call that may do without an output): no copy.  Complete when it returns.
template <class T, class Stage>
static int to_device_tail(gsp_context* ctx, void* dst, uint64_t need, const DevBuf<T>& own, Stage&& stage) {
  const bool direct = dst && ((uintptr_t)dst & 15u) == 0;
  int rc = stage(direct ? dst : nullptr);
  if (rc != GSP_OK) return rc;
  if (dst && !direct) CTX_TRY(ctx, hipMemcpyAsync(dst, own.p, need, hipMemcpyDeviceToDevice, ctx->stream));
  CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return GSP_OK;
}

// The tail of a *_to_device export of a history-sized plane as it is: a copy (any alignment), complete when it returns
static int plane_to_device(gsp_context* ctx, void* dst, uint64_t bytes, const void* plane) {
  const uint64_t need = (uint64_t)ctx->tp_width * ctx->tp_height * sizeof(q4);
  int rc = refuse_too_small(ctx, bytes, need);
  if (rc != GSP_OK) return rc;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  CTX_TRY(ctx, hipMemcpyAsync(dst, plane, need, hipMemcpyDeviceToDevice, ctx->stream));
  CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return GSP_OK;
}

// ---- LDR film (include/gpuspectral_pt.h, "LDR film"; per-pixel code: pt_display.h) ----
hipError_t gsp::display_measure(hipStream_t stream, uint32_t num_cus, const void* src, uint64_t n, DisplayStatsRec* d_rec, DisplayStatsRec* h_rec,
                                gsp_luminance* out) {
  hipError_t e = hipMemsetAsync(d_rec, 0, sizeof(DisplayStatsRec), stream);
  if (e != hipSuccess) return e;
  if (n) {
    hipLaunchKernelGGL(k_display_stats, dim3(pointwise_grid(n, num_cus, 4)), dim3(kBlock), 0, stream, (const v4f*)src, n, d_rec);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if ((e = hipMemcpyAsync(h_rec, d_rec, sizeof(DisplayStatsRec), hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
  *out = display_luminance(*h_rec);
  return hipSuccess;
}

hipError_t gsp::display_map(hipStream_t stream, uint32_t num_cus, const void* src, uint64_t n, const DisplayConsts& k, uint32_t* dst) {
  if (n == 0) return hipSuccess;
  const dim3 grid(pointwise_grid((n + 3) / 4, num_cus, 8)), block(kBlock);  // (a lane converts four pixels)
  const v4f* s = (const v4f*)src;
#define GSP_DISPLAY_LAUNCH(T, S) hipLaunchKernelGGL((k_display_map<T, S>), grid, block, 0, stream, s, n, k, dst)
  if (k.srgb) {
    if (k.tonemap == GSP_TONEMAP_ACES) GSP_DISPLAY_LAUNCH(GSP_TONEMAP_ACES, true);
    else if (k.tonemap == GSP_TONEMAP_REINHARD) GSP_DISPLAY_LAUNCH(GSP_TONEMAP_REINHARD, true);
    else GSP_DISPLAY_LAUNCH(GSP_TONEMAP_CLAMP, true);
  } else {
    if (k.tonemap == GSP_TONEMAP_ACES) GSP_DISPLAY_LAUNCH(GSP_TONEMAP_ACES, false);
    else if (k.tonemap == GSP_TONEMAP_REINHARD) GSP_DISPLAY_LAUNCH(GSP_TONEMAP_REINHARD, false);
    else GSP_DISPLAY_LAUNCH(GSP_TONEMAP_CLAMP, false);
  }
#undef GSP_DISPLAY_LAUNCH
  return hipGetLastError();
}

// gsp_peek's ordering: the folds queued so far finish, the paths in flight keep their state
static int display_peek_sync(gsp_context* ctx, uint32_t* samples_folded) {
  uint32_t folded = 0xffffffffu;
  for (uint32_t l = 0; l < ctx->num_lanes; ++l) {
    gsp_context::Lane& L = ctx->lanes[l];
    if (L.num_pixels == 0) continue;
    CTX_TRY(ctx, hipStreamSynchronize(L.stream));
    folded = std::min(folded, ctx->pipe_active && L.pipe.active ? L.pipe.folded_end : ctx->folded_idle);
  }
  if (samples_folded) *samples_folded = folded == 0xffffffffu ? 0u : (folded >= ctx->sample_base ? folded - ctx->sample_base : folded);
  return GSP_OK;
}

static int display_measure_ctx(gsp_context* ctx, gsp_luminance* out, const void* src = nullptr) {
  CTX_TRY(ctx, ctx->display_rec.ensure(1, &ctx->bytes));
  if (!ctx->h_display_rec) CTX_TRY(ctx, hipHostMalloc((void**)&ctx->h_display_rec, sizeof(DisplayStatsRec), hipHostMallocDefault));
  CTX_TRY(ctx, display_measure(ctx->stream, (uint32_t)ctx->num_cus, src ? src : ctx->accum.p, ctx->num_pixels, ctx->display_rec.p, ctx->h_display_rec, out));
  return GSP_OK;
}

// validates `display_host`, measures the frame where the display asks for it and queues the map of the compact accumulate
// buffer (or of `src`: the denoised frame) into `dst` (device, 16-byte aligned; nullptr = the context's own RGBA8 buffer) on
// ctx->stream
static int display_run(gsp_context* ctx, const gsp_display* display_host, uint32_t* dst, const void* src = nullptr) {
  gsp_display d;
  if (const char* why = resolve_display(display_host, d)) {
    ctx->err = why;
    return GSP_ERR_INVALID;
  }
  gsp_luminance lum{};
  if (display_needs_stats(d)) {
    int rc = display_measure_ctx(ctx, &lum, src);
    if (rc != GSP_OK) return rc;
  }
  if (!dst) {
    CTX_TRY(ctx, ctx->display_out.ensure((ctx->num_pixels + 3) / 4 * 4, &ctx->bytes));
    dst = ctx->display_out.p;
  }
  CTX_TRY(ctx, display_map(ctx->stream, (uint32_t)ctx->num_cus, src ? src : ctx->accum.p, ctx->num_pixels, display_consts(d, lum), dst));
  return GSP_OK;
}

// The tail of a gsp_download_*_display export: `stage()` validates and queues a filter that leaves its frame in dn_out; the map
// of that frame is read back into `out`.
template <class Stage>
static int filtered_display_tail(gsp_context* ctx, const gsp_display* display, uint32_t* out, Stage&& stage) {
  {  // (an invalid display is refused before anything is queued)
    gsp_display d;
    if (const char* why = resolve_display(display, d)) {
      ctx->err = why;
      return GSP_ERR_INVALID;
    }
  }
  int rc = stage();
  if (rc == GSP_OK) rc = display_run(ctx, display, nullptr, ctx->dn_out.p);
  if (rc != GSP_OK) return rc;
  return read_back_bytes(ctx, ctx->display_out.p, ctx->num_pixels * sizeof(uint32_t), out);
}

// ---- denoiser (include/gpuspectral_pt.h, "Denoiser"; per-pixel code: pt_denoise.h) ----
// queues the demodulation of `colour` (a frame, or with `illum` a demodulated history: pt_illum.h) into the planes `e` and `a`
static hipError_t prepare_run(hipStream_t stream, uint32_t num_cus, bool illum, const void* colour, const void* albedo, uint64_t n, void* e, void* a) {
  const dim3 grid(pointwise_grid(n, num_cus, 8)), block(kBlock);
  if (illum) hipLaunchKernelGGL(k_illum_prepare, grid, block, 0, stream, (const v4f*)colour, (const v4f*)albedo, n, (v4f*)e, (v4f*)a);
  else hipLaunchKernelGGL(k_denoise_prepare, grid, block, 0, stream, (const v4f*)colour, (const v4f*)albedo, n, (v4f*)e, (v4f*)a);
  return hipGetLastError();
}

// The instantiation of an à-trous kernel (k_denoise_atrous, k_svgf_atrous, k_svgf_atrous_feedback) for level `level` of a filter
// whose last level is `last`: launch(S, LAST) is called with the template arguments as std::integral_constant values.  Levels 0 and
// 1 (steps S = 1 and 2) stage tile + halo in LDS, the wider steps (S = 0) read their taps from global memory.
template <class Launch>
static void atrous_level(uint32_t level, bool last, Launch&& launch) {
  const auto step = [&](auto S) {
    if (last) launch(S, std::true_type{});
    else launch(S, std::false_type{});
  };
  if (level == 0) step(std::integral_constant<int, 1>{});
  else if (level == 1) step(std::integral_constant<int, 2>{});
  else step(std::integral_constant<int, 0>{});
}

hipError_t gsp::denoise_run(hipStream_t stream, uint32_t num_cus, const void* accum, const void* albedo, const void* geom, uint32_t width, uint32_t height,
                            const DenoiseConsts& k, void* e0, void* e1, void* a, void* out, bool illum) {
  const uint64_t n = (uint64_t)width * height;
  if (n == 0) return hipSuccess;
  hipError_t e = prepare_run(stream, num_cus, illum, accum, albedo, n, e0, a);
  if (e != hipSuccess) return e;
  const dim3 grid = tile_grid(width, height), block(kBlock);
  v4f* E[2] = {(v4f*)e0, (v4f*)e1};
  for (uint32_t i = 0; i < k.iterations; ++i) {
    const bool last = i + 1 == k.iterations;
    const v4f* in = E[i & 1u];
    v4f* dst = last ? (v4f*)out : E[(i + 1u) & 1u];
    atrous_level(i, last, [&](auto S, auto LAST) {
      hipLaunchKernelGGL((k_denoise_atrous<decltype(S)::value, decltype(LAST)::value>), grid, block, 0, stream, in, (const v4f*)a, (const v4f*)geom,
                         (const v4f*)accum, dst, k, i, (int)width, (int)height);
    });
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

// Validates, completes the queued samples and queues the filter of the frame into `dst` (device, 16-byte aligned; nullptr = the
// context's own buffer) on ctx->stream.  `out_ptr` is the caller's output pointer (checked for NULL only).
static int denoise_ctx(gsp_context* ctx, const gsp_denoise* denoise_host, const char* who, const void* out_ptr, void* dst) {
  int rc = refuse_null_output(ctx, who, out_ptr);
  if (rc != GSP_OK) return rc;
  if (!ctx->have_frame) {
    ctx->err = std::string(who) + " needs gsp_frame_begin first";
    return GSP_ERR_INVALID;
  }
  if (ctx->subset) {
    ctx->err = std::string(who) + ": the frame was begun with pixel_ids; a share has no neighbours (use gsp_multi_download_denoised)";
    return GSP_ERR_INVALID;
  }
  if (!ctx->features_rendered) {
    ctx->err = std::string(who) + " needs a gsp_render_features call since gsp_frame_begin";
    return GSP_ERR_INVALID;
  }
  DenoiseConsts k;
  if (const char* why = resolve_denoise(denoise_host, k)) {
    ctx->err = why;
    return GSP_ERR_INVALID;
  }
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  rc = pipeline_drain(ctx);
  if (rc == GSP_OK) rc = ensure_filter_scratch(ctx);
  if (rc != GSP_OK) return rc;
  CTX_TRY(ctx, denoise_run(ctx->stream, (uint32_t)ctx->num_cus, ctx->accum.p, ctx->feat_albedo.p, ctx->feat_geom.p, ctx->width, ctx->height, k,
                           ctx->dn_e0.p, ctx->dn_e1.p, ctx->dn_a.p, dst ? dst : (void*)ctx->dn_out.p));
  return GSP_OK;
}

extern "C" {

int gsp_download_denoised(gsp_context* ctx, const gsp_denoise* denoise, float* out) {
  if (!ctx) return GSP_ERR_INVALID;
  int rc = denoise_ctx(ctx, denoise, "gsp_download_denoised", out, nullptr);
  if (rc != GSP_OK) return rc;
  return read_back_bytes(ctx, ctx->dn_out.p, ctx->num_pixels * sizeof(q4), out);
}

int gsp_denoise_to_device(gsp_context* ctx, const gsp_denoise* denoise, void* dst, uint64_t bytes) {
  if (!ctx) return GSP_ERR_INVALID;
  const uint64_t need = ctx->num_pixels * sizeof(q4);
  if (dst && ctx->have_frame && refuse_too_small(ctx, bytes, need) != GSP_OK) return GSP_ERR_INVALID;
  return to_device_tail(ctx, dst, need, ctx->dn_out, [&](void* target) { return denoise_ctx(ctx, denoise, "gsp_denoise_to_device", dst, target); });
}

int gsp_download_denoised_display(gsp_context* ctx, const gsp_denoise* denoise, const gsp_display* display, uint32_t* out) {
  if (!ctx) return GSP_ERR_INVALID;
  return filtered_display_tail(ctx, display, out, [&] { return denoise_ctx(ctx, denoise, "gsp_download_denoised_display", out, nullptr); });
}

}  // extern "C"

// ---- temporal accumulation (include/gpuspectral_pt.h, "Temporal accumulation"; per-pixel code: pt_temporal.h) ----
// the planes of a full frame that an accumulate reads, 16 bytes per pixel each
struct TemporalFrame {
  const v4f *accum, *albedo, *geom;
  const v4u* ids;
};

// one history set: H and G (16 bytes per pixel), I (4) and, while the moments are tracked, M (16; not touched otherwise)
struct TemporalSet {
  v4f *h, *g;
  uint32_t* i;
  v4f* m;
};

struct TemporalFlags {
  bool moments, follow, demod;  // gsp_temporal_track_moments, gsp_temporal_follow_instances, gsp_temporal_demodulate
};

// Queues the one launch of an accumulate on `stream`: `frame` and the set `prev` (not read when k.history_valid == 0) into the set
// `out`; does not synchronise.  Every combination of the flags has a kernel of its own, so that a context which does not use a
// feature runs the instruction stream it ran before: k_temporal_reproject, k_temporal_reproject_moments (pt_svgf.h),
// k_temporal_reproject_follow<M> (pt_motion.h) and, with the frame demodulated, k_temporal_reproject_illum<M, F> (pt_illum.h).
// table, num_records (the instances' motion records) and `motion` (the motion plane written) belong to `follow` alone.
static hipError_t temporal_run(hipStream_t stream, TemporalFlags f, const TemporalFrame& frame, const TemporalSet& prev, const TemporalSet& out,
                               const v4f* table, uint32_t num_records, v4f* motion, const TemporalConsts& k) {
  if (k.cur.width == 0 || k.cur.height == 0) return hipSuccess;
  const dim3 grid = tile_grid(k.cur.width, k.cur.height), block(kBlock);
#define GSP_TEMPORAL_LAUNCH(KERNEL)                                                                                                             \
  hipLaunchKernelGGL((KERNEL), grid, block, 0, stream, frame.accum, frame.albedo, frame.geom, frame.ids, prev.h, prev.g, prev.i, prev.m, table, \
                     num_records, out.h, out.g, out.i, out.m, motion, k)
  if (!f.demod) {
    if (f.follow) {
      if (f.moments) GSP_TEMPORAL_LAUNCH(k_temporal_reproject_follow<true>);
      else GSP_TEMPORAL_LAUNCH(k_temporal_reproject_follow<false>);
    } else if (f.moments) {
      hipLaunchKernelGGL(k_temporal_reproject_moments, grid, block, 0, stream, frame.accum, frame.albedo, frame.geom, frame.ids, prev.h, prev.g, prev.i,
                         prev.m, out.h, out.g, out.i, out.m, k);
    } else {
      hipLaunchKernelGGL(k_temporal_reproject, grid, block, 0, stream, frame.accum, frame.albedo, frame.geom, frame.ids, prev.h, prev.g, prev.i, out.h,
                         out.g, out.i, k);
    }
  } else if (f.follow) {
    if (f.moments) GSP_TEMPORAL_LAUNCH((k_temporal_reproject_illum<true, true>));
    else GSP_TEMPORAL_LAUNCH((k_temporal_reproject_illum<false, true>));
  } else {
    if (f.moments) GSP_TEMPORAL_LAUNCH((k_temporal_reproject_illum<true, false>));
    else GSP_TEMPORAL_LAUNCH((k_temporal_reproject_illum<false, false>));
  }
#undef GSP_TEMPORAL_LAUNCH
  return hipGetLastError();
}

// set `s` of the context's two
static TemporalSet temporal_set(gsp_context* ctx, int s) {
  return TemporalSet{(v4f*)ctx->tp_h[s].p, (v4f*)ctx->tp_g[s].p, ctx->tp_i[s].p, (v4f*)ctx->tp_m[s].p};
}

// what every temporal read-out asks first (null_ok: the call may do without an output)
static int temporal_have_history(gsp_context* ctx, const char* who, const void* out_ptr, bool null_ok = false) {
  if (!null_ok) {
    int rc = refuse_null_output(ctx, who, out_ptr);
    if (rc != GSP_OK) return rc;
  }
  if (!ctx->tp_valid) {
    ctx->err = std::string(who) + " needs a gsp_temporal_accumulate call since the history was last invalidated";
    return GSP_ERR_INVALID;
  }
  return GSP_OK;
}

// Validates and queues the denoiser with the newest history as its colour source into the context's own buffer
static int temporal_denoise_ctx(gsp_context* ctx, const gsp_denoise* denoise_host, const char* who, const void* out_ptr) {
  int rc = temporal_have_history(ctx, who, out_ptr);
  if (rc == GSP_OK) rc = refuse_without_full_frame_features(ctx, who);
  if (rc != GSP_OK) return rc;
  DenoiseConsts k;
  if (const char* why = resolve_denoise(denoise_host, k)) {
    ctx->err = why;
    return GSP_ERR_INVALID;
  }
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  rc = ensure_filter_scratch(ctx);
  if (rc != GSP_OK) return rc;
  CTX_TRY(ctx, denoise_run(ctx->stream, (uint32_t)ctx->num_cus, ctx->tp_h[ctx->tp_cur].p, ctx->feat_albedo.p, ctx->feat_geom.p, ctx->width, ctx->height, k,
                           ctx->dn_e0.p, ctx->dn_e1.p, ctx->dn_a.p, ctx->dn_out.p, ctx->tp_demod));
  return GSP_OK;
}

extern "C" {

int gsp_temporal_accumulate(gsp_context* ctx, const gsp_temporal* temporal) {
  if (!ctx) return GSP_ERR_INVALID;
  const char* who = "gsp_temporal_accumulate";
  if (!ctx->have_frame) {
    ctx->err = std::string(who) + " needs gsp_frame_begin first";
    return GSP_ERR_INVALID;
  }
  if (ctx->subset) {
    ctx->err = std::string(who) + ": the frame was begun with pixel_ids; a share has no neighbours and there is no multi-GPU variant";
    return GSP_ERR_INVALID;
  }
  if (!ctx->features_rendered) {
    ctx->err = std::string(who) + " needs a gsp_render_features call since gsp_frame_begin";
    return GSP_ERR_INVALID;
  }
  if (ctx->tp_done) {
    ctx->err = std::string(who) + ": the frame has been accumulated already (one call per gsp_frame_begin)";
    return GSP_ERR_INVALID;
  }
  if (ctx->tp_follow && ctx->inst_edits != ctx->feat_inst_edits) {
    ctx->err = std::string(who) + ": gsp_update_instances has changed the instances since the frame's gsp_render_features; with "
               "gsp_temporal_follow_instances on, an edit belongs before the frame's gsp_render_features";
    return GSP_ERR_INVALID;
  }
  TemporalParams tp;
  if (const char* why = resolve_temporal(temporal, tp)) {
    ctx->err = why;
    return GSP_ERR_INVALID;
  }
  // (gsp_frame_begin has invalidated a history of another size)
  TemporalConsts k;
  if (const char* why = temporal_consts(ctx->camera, &ctx->tp_camera, ctx->tp_valid, ctx->width, ctx->height, tp, k)) {
    ctx->err = std::string(who) + ": " + why;
    return GSP_ERR_INVALID;
  }
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  {
    int rc_ = pipeline_drain(ctx);
    if (rc_ != GSP_OK) return rc_;
  }
  const size_t n = std::max<uint64_t>(ctx->num_pixels, 1);
  for (int s = 0; s < 2; ++s) {
    CTX_TRY(ctx, ctx->tp_h[s].ensure(n, &ctx->bytes));
    CTX_TRY(ctx, ctx->tp_g[s].ensure(n, &ctx->bytes));
    CTX_TRY(ctx, ctx->tp_i[s].ensure(n, &ctx->bytes));
    if (ctx->tp_moments) CTX_TRY(ctx, ctx->tp_m[s].ensure(n, &ctx->bytes));
  }
  const int from = ctx->tp_cur, to = from ^ 1;
  std::vector<float> cur;  // (following: the instances' transforms of this frame)
  uint32_t records = 0;
  if (ctx->tp_follow) {
    // the records of the instances between the history's frame and this one: formed in the pinned buffer, copied on the stream
    // in front of the launch.  Without a history (or without a snapshot of its transforms) the table is not read.
    const uint32_t ni = (uint32_t)ctx->h_inst.size();
    const bool have_prev = ctx->tp_valid && ctx->tp_xforms.size() == 16ull * ni;
    if (!have_prev) k.history_valid = 0;
    cur.resize(16ull * ni);
    for (uint32_t i = 0; i < ni; ++i) std::memcpy(&cur[16ull * i], ctx->h_inst[i].transform, 16 * sizeof(float));
    CTX_TRY(ctx, ctx->tp_v.ensure(n, &ctx->bytes));
    CTX_TRY(ctx, ctx->tp_table.ensure((size_t)std::max<uint32_t>(ni, 1) * kMotionRecordQuads, &ctx->bytes));
    if (ctx->h_motion_cap < std::max<uint32_t>(ni, 1)) {
      if (ctx->h_motion) (void)hipHostFree(ctx->h_motion);
      ctx->h_motion = nullptr;
      ctx->h_motion_cap = 0;
      CTX_TRY(ctx, hipHostMalloc((void**)&ctx->h_motion, (size_t)std::max<uint32_t>(ni, 1) * sizeof(MotionRecord), hipHostMallocDefault));
      ctx->h_motion_cap = std::max<uint32_t>(ni, 1);
    }
    if (k.history_valid && ni) {
      motion_table(ctx->tp_xforms.data(), cur.data(), ni, ctx->h_motion);
      CTX_TRY(ctx, hipMemcpyAsync(ctx->tp_table.p, ctx->h_motion, (size_t)ni * sizeof(MotionRecord), hipMemcpyHostToDevice, ctx->stream));
      records = ni;
    }
  }
  const TemporalFrame frame{(const v4f*)ctx->accum.p, (const v4f*)ctx->feat_albedo.p, (const v4f*)ctx->feat_geom.p, (const v4u*)ctx->feat_ids.p};
  CTX_TRY(ctx, temporal_run(ctx->stream, TemporalFlags{ctx->tp_moments, ctx->tp_follow, ctx->tp_demod}, frame, temporal_set(ctx, from), temporal_set(ctx, to),
                            ctx->tp_follow ? (const v4f*)ctx->tp_table.p : nullptr, records, ctx->tp_follow ? (v4f*)ctx->tp_v.p : nullptr, k));
  CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (complete when the call returns: a camera or scene edit may follow at once)
  ctx->tp_cur = to;
  ctx->tp_camera = ctx->camera;
  if (ctx->tp_follow) ctx->tp_xforms.swap(cur);
  ctx->tp_width = ctx->width;
  ctx->tp_height = ctx->height;
  ctx->tp_valid = true;
  ctx->tp_done = true;
  ctx->tp_fed = false;  // (gsp_temporal_svgf_feedback: at most one per accumulate)
  ctx->tp_acc = {k, records, ctx->tp_follow, ctx->tp_demod, ctx->tp_acc.serial + 1};  // (gsp_temporal_antilag: what this accumulate ran with)
  if (!k.history_valid) ctx->tp_epoch = ctx->tp_acc.serial;  // (gsp_temporal_taa: a history begins here)
  return GSP_OK;
}

int gsp_temporal_reset(gsp_context* ctx) {
  if (!ctx) return GSP_ERR_INVALID;
  ctx->tp_valid = false;
  return GSP_OK;
}

int gsp_download_temporal(gsp_context* ctx, float* out) {
  if (!ctx) return GSP_ERR_INVALID;
  int rc = temporal_have_history(ctx, "gsp_download_temporal", out);
  if (rc != GSP_OK) return rc;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  return read_back_bytes(ctx, ctx->tp_h[ctx->tp_cur].p, (size_t)ctx->tp_width * ctx->tp_height * sizeof(q4), out);
}

int gsp_temporal_to_device(gsp_context* ctx, void* dst, uint64_t bytes) {
  if (!ctx) return GSP_ERR_INVALID;
  int rc = temporal_have_history(ctx, "gsp_temporal_to_device", dst);
  if (rc != GSP_OK) return rc;
  return plane_to_device(ctx, dst, bytes, ctx->tp_h[ctx->tp_cur].p);
}

int gsp_download_temporal_denoised(gsp_context* ctx, const gsp_denoise* denoise, float* out) {
  if (!ctx) return GSP_ERR_INVALID;
  int rc = temporal_denoise_ctx(ctx, denoise, "gsp_download_temporal_denoised", out);
  if (rc != GSP_OK) return rc;
  return read_back_bytes(ctx, ctx->dn_out.p, ctx->num_pixels * sizeof(q4), out);
}

int gsp_download_temporal_denoised_display(gsp_context* ctx, const gsp_denoise* denoise, const gsp_display* display, uint32_t* out) {
  if (!ctx) return GSP_ERR_INVALID;
  return filtered_display_tail(ctx, display, out, [&] { return temporal_denoise_ctx(ctx, denoise, "gsp_download_temporal_denoised_display", out); });
}

}  // extern "C"

// ---- variance-guided filter (include/gpuspectral_pt.h, "Variance-guided filter"; per-pixel code: pt_svgf.h) ----
// The filter of the history `hist` with moments `moments` on a full frame: k_denoise_prepare, k_svgf_variance and k.iterations
// launches of k_svgf_atrous on `stream`; does not synchronise.  e0, e1, a, out: 16 bytes per pixel; v0, v1: 4 bytes per pixel.
// illum: hist is a demodulated history (k_illum_prepare for k_denoise_prepare).  fb_levels > 0 (gsp_temporal_svgf_feedback): level
// fb_levels - 1 is k_svgf_atrous_feedback and writes its colour into `hist`; with !want_out the levels after it are not run.
static hipError_t svgf_run(hipStream_t stream, uint32_t num_cus, void* hist, const void* moments, const void* albedo, const void* geom, uint32_t width,
                           uint32_t height, const SvgfConsts& k, void* e0, void* e1, void* a, void* v0, void* v1, void* out, bool illum = false,
                           uint32_t fb_levels = 0, bool want_out = true) {
  const uint64_t n = (uint64_t)width * height;
  if (n == 0) return hipSuccess;
  hipError_t e = prepare_run(stream, num_cus, illum, hist, albedo, n, e0, a);
  if (e != hipSuccess) return e;
  const dim3 grid = tile_grid(width, height), block(kBlock);
  hipLaunchKernelGGL(k_svgf_variance, grid, block, 0, stream, (const v4f*)e0, (const v4f*)a, (const v4f*)geom, (const v4f*)hist, (const v4f*)moments,
                     (float*)v0, k, (int)width, (int)height);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  v4f* E[2] = {(v4f*)e0, (v4f*)e1};
  float* V[2] = {(float*)v0, (float*)v1};
  const uint32_t run_levels = fb_levels && !want_out ? fb_levels : k.iterations;
  for (uint32_t i = 0; i < run_levels; ++i) {
    const bool last = i + 1 == k.iterations;
    v4f* dst = last ? (v4f*)out : E[(i + 1u) & 1u];
#define GSP_SVGF_LAUNCH(KERNEL)                                                                                                                      \
  hipLaunchKernelGGL((KERNEL), grid, block, 0, stream, (const v4f*)E[i & 1u], (const v4f*)a, (const v4f*)geom, (const float*)V[i & 1u], (v4f*)hist, dst, \
                     V[(i + 1u) & 1u], k, i, (int)width, (int)height)
    if (fb_levels && i + 1 == fb_levels)
      atrous_level(i, last, [&](auto S, auto LAST) {
        if (illum) GSP_SVGF_LAUNCH((k_svgf_atrous_feedback<decltype(S)::value, decltype(LAST)::value, true>));
        else GSP_SVGF_LAUNCH((k_svgf_atrous_feedback<decltype(S)::value, decltype(LAST)::value, false>));
      });
    else
      atrous_level(i, last, [&](auto S, auto LAST) { GSP_SVGF_LAUNCH((k_svgf_atrous<decltype(S)::value, decltype(LAST)::value>)); });
#undef GSP_SVGF_LAUNCH
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

// Validates and queues the filter into `dst` (device, 16-byte aligned; nullptr = the context's own buffer) on ctx->stream
// fb: the call is a gsp_temporal_svgf_feedback of `fb_levels` levels -- out_ptr may be NULL (then nothing is written to dst), the
// frame must have been accumulated and not fed back yet, and the newest history takes the colour of level fb_levels - 1
static int svgf_ctx(gsp_context* ctx, const gsp_denoise* denoise_host, const gsp_svgf* svgf_host, const char* who, const void* out_ptr, void* dst,
                    bool fb = false, uint32_t fb_levels = 0) {
  int rc = temporal_have_history(ctx, who, out_ptr, fb);
  if (rc != GSP_OK) return rc;
  if (!ctx->tp_moments) {
    ctx->err = std::string(who) + " needs gsp_temporal_track_moments(ctx, 1) before the history was accumulated";
    return GSP_ERR_INVALID;
  }
  rc = refuse_without_full_frame_features(ctx, who);
  if (rc != GSP_OK) return rc;
  SvgfConsts k;
  if (const char* why = resolve_svgf(denoise_host, svgf_host, k)) {
    ctx->err = why;
    return GSP_ERR_INVALID;
  }
  if (fb) {
    if (fb_levels < 1 || fb_levels > k.iterations) {
      ctx->err = std::string(who) + ": levels must be within 1 .. " + std::to_string(k.iterations) + " (the filter's iterations)";
      return GSP_ERR_INVALID;
    }
    if (!ctx->tp_done) {
      ctx->err = std::string(who) + " needs a gsp_temporal_accumulate call since gsp_frame_begin";
      return GSP_ERR_INVALID;
    }
    if (ctx->tp_fed) {
      ctx->err = std::string(who) + ": the history has been fed back already (one call per gsp_temporal_accumulate)";
      return GSP_ERR_INVALID;
    }
  }
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  rc = ensure_filter_scratch(ctx);
  if (rc != GSP_OK) return rc;
  for (DevBuf<float>& b : ctx->sv_v) CTX_TRY(ctx, b.ensure(std::max<uint64_t>(ctx->num_pixels, 1), &ctx->bytes));
  CTX_TRY(ctx, svgf_run(ctx->stream, (uint32_t)ctx->num_cus, ctx->tp_h[ctx->tp_cur].p, ctx->tp_m[ctx->tp_cur].p, ctx->feat_albedo.p, ctx->feat_geom.p,
                        ctx->width, ctx->height, k, ctx->dn_e0.p, ctx->dn_e1.p, ctx->dn_a.p, ctx->sv_v[0].p, ctx->sv_v[1].p,
                        dst ? dst : (void*)ctx->dn_out.p, ctx->tp_demod, fb ? fb_levels : 0u, !fb || out_ptr != nullptr));
  if (fb) ctx->tp_fed = true;
  return GSP_OK;
}

extern "C" {

int gsp_temporal_track_moments(gsp_context* ctx, int on) {
  if (!ctx) return GSP_ERR_INVALID;
  const bool want = on != 0;
  if (want == ctx->tp_moments) return GSP_OK;
  ctx->tp_moments = want;
  ctx->tp_valid = false;  // (moments and history have the same age)
  return GSP_OK;
}

int gsp_temporal_follow_instances(gsp_context* ctx, int on) {
  if (!ctx) return GSP_ERR_INVALID;
  const bool want = on != 0;
  if (want == ctx->tp_follow) return GSP_OK;
  ctx->tp_follow = want;
  ctx->tp_valid = false;  // (the transforms the history belongs to are recorded only while following is on)
  ctx->tp_xforms.clear();
  return GSP_OK;
}

// what the two read-outs of the motion plane ask first
static int temporal_have_motion(gsp_context* ctx, const char* who, const void* out_ptr) {
  int rc = temporal_have_history(ctx, who, out_ptr);
  if (rc != GSP_OK) return rc;
  if (!ctx->tp_follow) {
    ctx->err = std::string(who) + " needs gsp_temporal_follow_instances(ctx, 1) before the history was accumulated";
    return GSP_ERR_INVALID;
  }
  return GSP_OK;
}

int gsp_download_temporal_motion(gsp_context* ctx, float* out) {
  if (!ctx) return GSP_ERR_INVALID;
  int rc = temporal_have_motion(ctx, "gsp_download_temporal_motion", out);
  if (rc != GSP_OK) return rc;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  return read_back_bytes(ctx, ctx->tp_v.p, (size_t)ctx->tp_width * ctx->tp_height * sizeof(q4), out);
}

int gsp_temporal_motion_to_device(gsp_context* ctx, void* dst, uint64_t bytes) {
  if (!ctx) return GSP_ERR_INVALID;
  int rc = temporal_have_motion(ctx, "gsp_temporal_motion_to_device", dst);
  if (rc != GSP_OK) return rc;
  return plane_to_device(ctx, dst, bytes, ctx->tp_v.p);
}

int gsp_download_temporal_moments(gsp_context* ctx, float* out) {
  if (!ctx) return GSP_ERR_INVALID;
  int rc = temporal_have_history(ctx, "gsp_download_temporal_moments", out);
  if (rc != GSP_OK) return rc;
  if (!ctx->tp_moments) {
    ctx->err = "gsp_download_temporal_moments needs gsp_temporal_track_moments(ctx, 1) before the history was accumulated";
    return GSP_ERR_INVALID;
  }
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  return read_back_bytes(ctx, ctx->tp_m[ctx->tp_cur].p, (size_t)ctx->tp_width * ctx->tp_height * sizeof(q4), out);
}

int gsp_download_temporal_svgf(gsp_context* ctx, const gsp_denoise* denoise, const gsp_svgf* svgf, float* out) {
  if (!ctx) return GSP_ERR_INVALID;
  int rc = svgf_ctx(ctx, denoise, svgf, "gsp_download_temporal_svgf", out, nullptr);
  if (rc != GSP_OK) return rc;
  return read_back_bytes(ctx, ctx->dn_out.p, ctx->num_pixels * sizeof(q4), out);
}

int gsp_temporal_svgf_to_device(gsp_context* ctx, const gsp_denoise* denoise, const gsp_svgf* svgf, void* dst, uint64_t bytes) {
  if (!ctx) return GSP_ERR_INVALID;
  const uint64_t need = ctx->num_pixels * sizeof(q4);
  if (dst && ctx->have_frame && refuse_too_small(ctx, bytes, need) != GSP_OK) return GSP_ERR_INVALID;
  return to_device_tail(ctx, dst, need, ctx->dn_out,
                        [&](void* target) { return svgf_ctx(ctx, denoise, svgf, "gsp_temporal_svgf_to_device", dst, target); });
}

int gsp_download_temporal_svgf_display(gsp_context* ctx, const gsp_denoise* denoise, const gsp_svgf* svgf, const gsp_display* display, uint32_t* out) {
  if (!ctx) return GSP_ERR_INVALID;
  return filtered_display_tail(ctx, display, out, [&] { return svgf_ctx(ctx, denoise, svgf, "gsp_download_temporal_svgf_display", out, nullptr); });
}

}  // extern "C"

// ---- illumination history (include/gpuspectral_pt.h, "Illumination history"; per-pixel code: pt_illum.h) ----
// what the two image read-outs ask first
static int temporal_have_image(gsp_context* ctx, const char* who, const void* out_ptr) {
  int rc = temporal_have_history(ctx, who, out_ptr);
  if (rc != GSP_OK) return rc;
  if (!ctx->tp_done) {
    ctx->err = std::string(who) + " needs a gsp_temporal_accumulate call since gsp_frame_begin";
    return GSP_ERR_INVALID;
  }
  return GSP_OK;
}

// queues the re-modulated newest history into `dst` (device, 16-byte aligned; nullptr = the context's own buffer) on ctx->stream
static int temporal_image_run(gsp_context* ctx, void* dst) {
  if (!dst) {
    CTX_TRY(ctx, ctx->dn_out.ensure(std::max<uint64_t>(ctx->num_pixels, 1), &ctx->bytes));
    dst = ctx->dn_out.p;
  }
  const uint64_t n = (uint64_t)ctx->tp_width * ctx->tp_height;
  if (n == 0) return GSP_OK;
  hipLaunchKernelGGL(k_illum_image, dim3(pointwise_grid(n, (uint32_t)ctx->num_cus, 8)), dim3(kBlock), 0, ctx->stream,
                     (const v4f*)ctx->tp_h[ctx->tp_cur].p, (const v4f*)ctx->feat_albedo.p, n, (v4f*)dst);
  CTX_TRY(ctx, hipGetLastError());
  return GSP_OK;
}

extern "C" {

int gsp_temporal_demodulate(gsp_context* ctx, int on) {
  if (!ctx) return GSP_ERR_INVALID;
  const bool want = on != 0;
  if (want == ctx->tp_demod) return GSP_OK;
  ctx->tp_demod = want;
  ctx->tp_valid = false;  // (a history of colour is no history of illumination)
  return GSP_OK;
}

int gsp_download_temporal_image(gsp_context* ctx, float* out) {
  if (!ctx) return GSP_ERR_INVALID;
  int rc = temporal_have_image(ctx, "gsp_download_temporal_image", out);
  if (rc != GSP_OK) return rc;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  const size_t bytes = (size_t)ctx->tp_width * ctx->tp_height * sizeof(q4);
  if (!ctx->tp_demod) return read_back_bytes(ctx, ctx->tp_h[ctx->tp_cur].p, bytes, out);
  rc = temporal_image_run(ctx, nullptr);
  if (rc != GSP_OK) return rc;
  return read_back_bytes(ctx, ctx->dn_out.p, bytes, out);
}

int gsp_temporal_image_to_device(gsp_context* ctx, void* dst, uint64_t bytes) {
  if (!ctx) return GSP_ERR_INVALID;
  int rc = temporal_have_image(ctx, "gsp_temporal_image_to_device", dst);
  if (rc != GSP_OK) return rc;
  if (!ctx->tp_demod) return plane_to_device(ctx, dst, bytes, ctx->tp_h[ctx->tp_cur].p);  // (the history is the image)
  const uint64_t need = (uint64_t)ctx->tp_width * ctx->tp_height * sizeof(q4);
  rc = refuse_too_small(ctx, bytes, need);
  if (rc != GSP_OK) return rc;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  return to_device_tail(ctx, dst, need, ctx->dn_out, [&](void* target) { return temporal_image_run(ctx, target); });
}

int gsp_temporal_svgf_feedback(gsp_context* ctx, const gsp_denoise* denoise, const gsp_svgf* svgf, uint32_t levels, float* out) {
  if (!ctx) return GSP_ERR_INVALID;
  int rc = svgf_ctx(ctx, denoise, svgf, "gsp_temporal_svgf_feedback", out, nullptr, true, levels);
  if (rc != GSP_OK) return rc;
  if (out) return read_back_bytes(ctx, ctx->dn_out.p, ctx->num_pixels * sizeof(q4), out);
  CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return GSP_OK;
}

int gsp_temporal_svgf_feedback_to_device(gsp_context* ctx, const gsp_denoise* denoise, const gsp_svgf* svgf, uint32_t levels, void* dst, uint64_t bytes) {
  if (!ctx) return GSP_ERR_INVALID;
  const uint64_t need = ctx->num_pixels * sizeof(q4);
  if (dst && ctx->have_frame && refuse_too_small(ctx, bytes, need) != GSP_OK) return GSP_ERR_INVALID;
  return to_device_tail(ctx, dst, need, ctx->dn_out,
                        [&](void* target) { return svgf_ctx(ctx, denoise, svgf, "gsp_temporal_svgf_feedback_to_device", dst, target, true, levels); });
}

}  // extern "C"

// ---- temporal anti-lag (include/gpuspectral_pt.h, "Temporal anti-lag"; per-pixel code: pt_antilag.h) ----
// Queues the two launches of a gsp_temporal_antilag on `stream`: Step A -- `frame`, F of `fprev` and G, I of the older set `prev`
// (none of the three read when k.history_valid == 0) into `fout` under the accumulate's flags -- and Step B, the clamp of out.h
// into the box of `fout` with out.g and out.i; does not synchronise.  k = antilag_fast_consts of the accumulate's constants;
// table, num_records: the accumulate's motion records (`follow` alone).
static hipError_t antilag_run(hipStream_t stream, TemporalFlags f, const TemporalFrame& frame, const v4f* fprev, const TemporalSet& prev, const TemporalSet& out,
                              const v4f* table, uint32_t num_records, v4f* fout, const TemporalConsts& k, const AntilagParams& a) {
  if (k.cur.width == 0 || k.cur.height == 0) return hipSuccess;
  const dim3 grid = tile_grid(k.cur.width, k.cur.height), block(kBlock);
#define GSP_ANTILAG_LAUNCH(FOLLOW, DEMOD)                                                                                                       \
  hipLaunchKernelGGL((k_antilag_fast<FOLLOW, DEMOD>), grid, block, 0, stream, frame.accum, frame.albedo, frame.geom, frame.ids, fprev, prev.g, prev.i, \
                     table, num_records, fout, k)
  if (f.demod) {
    if (f.follow) GSP_ANTILAG_LAUNCH(true, true);
    else GSP_ANTILAG_LAUNCH(false, true);
  } else {
    if (f.follow) GSP_ANTILAG_LAUNCH(true, false);
    else GSP_ANTILAG_LAUNCH(false, false);
  }
#undef GSP_ANTILAG_LAUNCH
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
#define GSP_ANTILAG_LAUNCH(R) \
  hipLaunchKernelGGL((k_antilag_clamp<R>), grid, block, 0, stream, (const v4f*)fout, (const v4f*)out.g, (const uint32_t*)out.i, out.h, a, k.p.normal_min, \
                     (int)k.cur.width, (int)k.cur.height)
  if (a.radius == 1) GSP_ANTILAG_LAUNCH(1);
  else if (a.radius == 2) GSP_ANTILAG_LAUNCH(2);
  else GSP_ANTILAG_LAUNCH(3);
#undef GSP_ANTILAG_LAUNCH
  return hipGetLastError();
}

// what the two read-outs of the fast history ask first
static int temporal_have_fast(gsp_context* ctx, const char* who, const void* out_ptr) {
  int rc = temporal_have_history(ctx, who, out_ptr);
  if (rc != GSP_OK) return rc;
  if (ctx->al_serial != ctx->tp_acc.serial) {
    ctx->err = std::string(who) + " needs a gsp_temporal_antilag call since the newest gsp_temporal_accumulate";
    return GSP_ERR_INVALID;
  }
  return GSP_OK;
}

extern "C" {

int gsp_temporal_antilag(gsp_context* ctx, const gsp_antilag* antilag) {
  if (!ctx) return GSP_ERR_INVALID;
  const char* who = "gsp_temporal_antilag";
  int rc = temporal_have_history(ctx, who, nullptr, true);
  if (rc != GSP_OK) return rc;
  AntilagParams a;
  if (const char* why = resolve_antilag(antilag, a)) {
    ctx->err = why;
    return GSP_ERR_INVALID;
  }
  if (!ctx->tp_done) {
    ctx->err = std::string(who) + " needs a gsp_temporal_accumulate call since gsp_frame_begin";
    return GSP_ERR_INVALID;
  }
  if (ctx->al_serial == ctx->tp_acc.serial) {
    ctx->err = std::string(who) + ": the history has been clamped already (one call per gsp_temporal_accumulate)";
    return GSP_ERR_INVALID;
  }
  if (ctx->tp_fed) {
    ctx->err = std::string(who) + ": the history has been fed back already (the call belongs before gsp_temporal_svgf_feedback)";
    return GSP_ERR_INVALID;
  }
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  rc = pipeline_drain(ctx);
  if (rc != GSP_OK) return rc;
  const size_t n = std::max<uint64_t>(ctx->num_pixels, 1);
  for (DevBuf<q4>& b : ctx->al_f) CTX_TRY(ctx, b.ensure(n, &ctx->bytes));
  const gsp_context::AccumulateRecord& acc = ctx->tp_acc;
  const bool fast_valid = ctx->al_serial != 0 && ctx->al_serial + 1 == acc.serial;
  const TemporalConsts k = antilag_fast_consts(acc.k, a, fast_valid);
  const int from = ctx->al_cur, to = from ^ 1;
  const TemporalFrame frame{(const v4f*)ctx->accum.p, (const v4f*)ctx->feat_albedo.p, (const v4f*)ctx->feat_geom.p, (const v4u*)ctx->feat_ids.p};
  CTX_TRY(ctx, antilag_run(ctx->stream, TemporalFlags{false, acc.follow, acc.demod}, frame, (const v4f*)ctx->al_f[from].p, temporal_set(ctx, ctx->tp_cur ^ 1),
                           temporal_set(ctx, ctx->tp_cur), acc.follow ? (const v4f*)ctx->tp_table.p : nullptr, acc.records, (v4f*)ctx->al_f[to].p, k, a));
  CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (complete when the call returns, like the accumulate)
  ctx->al_cur = to;
  ctx->al_serial = acc.serial;
  return GSP_OK;
}

int gsp_download_temporal_fast(gsp_context* ctx, float* out) {
  if (!ctx) return GSP_ERR_INVALID;
  int rc = temporal_have_fast(ctx, "gsp_download_temporal_fast", out);
  if (rc != GSP_OK) return rc;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  return read_back_bytes(ctx, ctx->al_f[ctx->al_cur].p, (size_t)ctx->tp_width * ctx->tp_height * sizeof(q4), out);
}

int gsp_temporal_fast_to_device(gsp_context* ctx, void* dst, uint64_t bytes) {
  if (!ctx) return GSP_ERR_INVALID;
  int rc = temporal_have_fast(ctx, "gsp_temporal_fast_to_device", dst);
  if (rc != GSP_OK) return rc;
  return plane_to_device(ctx, dst, bytes, ctx->al_f[ctx->al_cur].p);
}

}  // extern "C"

// ---- temporal anti-aliasing (include/gpuspectral_pt.h, "Temporal anti-aliasing"; per-pixel code: pt_taa.h) ----
// Queues the one launch of a resolve on `stream`: the source plane `src`, the motion plane `motion` and the older plane `dprev`
// (not read when !taa_valid) into `dout`; does not synchronise.
static hipError_t taa_run(hipStream_t stream, const v4f* src, const v4f* motion, const v4f* dprev, v4f* dout, const TaaParams& a, const DisplayConsts& k,
                          bool taa_valid, uint32_t width, uint32_t height) {
  if (width == 0 || height == 0) return hipSuccess;
  const dim3 grid = tile_grid(width, height), block(kBlock);
#define GSP_TAA_LAUNCH(T) hipLaunchKernelGGL((k_taa_resolve<T>), grid, block, 0, stream, src, motion, dprev, dout, a, k, taa_valid ? 1 : 0, (int)width, (int)height)
  if (k.tonemap == GSP_TONEMAP_ACES) GSP_TAA_LAUNCH(GSP_TONEMAP_ACES);
  else if (k.tonemap == GSP_TONEMAP_REINHARD) GSP_TAA_LAUNCH(GSP_TONEMAP_REINHARD);
  else GSP_TAA_LAUNCH(GSP_TONEMAP_CLAMP);
#undef GSP_TAA_LAUNCH
  return hipGetLastError();
}

// A resolve with its source in host memory (host_src), in the caller's device memory (device_src, `bytes`) or, with both NULL, the
// image of the newest history.  A source the kernel cannot read where it lies -- host memory, a device address that is not
// 16-byte aligned, the image of a demodulated history -- passes through the filters' output plane dn_out.
static int taa_ctx(gsp_context* ctx, const char* who, const gsp_taa* taa_host, const gsp_display* display_host, const float* host_src, const void* device_src,
                   uint64_t bytes) {
  if (!ctx->have_frame) {
    ctx->err = std::string(who) + " needs gsp_frame_begin first";
    return GSP_ERR_INVALID;
  }
  if (ctx->subset) {
    ctx->err = std::string(who) + ": the frame was begun with pixel_ids; a share has no neighbours and there is no multi-GPU variant";
    return GSP_ERR_INVALID;
  }
  int rc = temporal_have_history(ctx, who, nullptr, true);
  if (rc != GSP_OK) return rc;
  if (!ctx->tp_done) {
    ctx->err = std::string(who) + " needs a gsp_temporal_accumulate call since gsp_frame_begin";
    return GSP_ERR_INVALID;
  }
  const gsp_context::AccumulateRecord& acc = ctx->tp_acc;
  if (!acc.follow || !ctx->tp_follow) {
    ctx->err = std::string(who) + " needs gsp_temporal_follow_instances(ctx, 1) before the frame was accumulated: the motion plane is made only then";
    return GSP_ERR_INVALID;
  }
  if (ctx->ta_serial == acc.serial) {
    ctx->err = std::string(who) + ": the frame has been resolved already (one call per gsp_temporal_accumulate)";
    return GSP_ERR_INVALID;
  }
  TaaParams a;
  if (const char* why = resolve_taa(taa_host, a)) {
    ctx->err = why;
    return GSP_ERR_INVALID;
  }
  gsp_display d;
  if (const char* why = resolve_display(display_host, d)) {
    ctx->err = why;
    return GSP_ERR_INVALID;
  }
  const uint64_t need = (uint64_t)ctx->tp_width * ctx->tp_height * sizeof(q4);
  if (device_src && bytes < need) {
    ctx->err = std::string(who) + ": source too small";
    return GSP_ERR_INVALID;
  }
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  const size_t n = std::max<uint64_t>(ctx->num_pixels, 1);
  for (DevBuf<q4>& b : ctx->ta_d) CTX_TRY(ctx, b.ensure(n, &ctx->bytes));
  const void* src = nullptr;
  if (host_src || (device_src && ((uintptr_t)device_src & 15u) != 0)) {
    CTX_TRY(ctx, ctx->dn_out.ensure(n, &ctx->bytes));
    if (need) CTX_TRY(ctx, hipMemcpyAsync(ctx->dn_out.p, host_src ? (const void*)host_src : device_src, need, host_src ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, ctx->stream));
    src = ctx->dn_out.p;
  } else if (device_src) {
    src = device_src;
  } else if (ctx->tp_demod) {
    rc = temporal_image_run(ctx, nullptr);
    if (rc != GSP_OK) return rc;
    src = ctx->dn_out.p;
  } else {
    src = ctx->tp_h[ctx->tp_cur].p;  // (the history is the image)
  }
  gsp_luminance lum{};
  if (display_needs_stats(d)) {
    rc = display_measure_ctx(ctx, &lum, src);
    if (rc != GSP_OK) return rc;
  }
  const bool taa_valid = ctx->ta_serial != 0 && ctx->ta_serial + 1 == acc.serial && acc.k.history_valid != 0;
  const int from = ctx->ta_cur, to = from ^ 1;
  CTX_TRY(ctx, taa_run(ctx->stream, (const v4f*)src, (const v4f*)ctx->tp_v.p, (const v4f*)ctx->ta_d[from].p, (v4f*)ctx->ta_d[to].p, a, display_consts(d, lum), taa_valid,
                       ctx->tp_width, ctx->tp_height));
  CTX_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (complete when the call returns, like the accumulate)
  ctx->ta_cur = to;
  ctx->ta_serial = acc.serial;
  ctx->ta_display = d;
  return GSP_OK;
}

// what the three read-outs of D ask first
static int temporal_have_taa(gsp_context* ctx, const char* who, const void* out_ptr) {
  int rc = temporal_have_history(ctx, who, out_ptr);
  if (rc != GSP_OK) return rc;
  if (ctx->ta_serial == 0 || ctx->ta_serial < ctx->tp_epoch) {
    ctx->err = std::string(who) + " needs a gsp_temporal_taa call since the history was last invalidated";
    return GSP_ERR_INVALID;
  }
  return GSP_OK;
}

// queues the encode of the newest D under the stored display into `dst` (device, 16-byte aligned; nullptr = the context's own RGBA8
// buffer) on ctx->stream: k_display_map's CLAMP instantiation at exposure 0, whose tone half leaves a value of [0, 1] as it is --
// display_channel(v) * 1.0f and display_clamp01 of it are v -- so that the word is the encode half of D' and no kernel is added
static int taa_display_run(gsp_context* ctx, uint32_t* dst) {
  const uint64_t n = (uint64_t)ctx->tp_width * ctx->tp_height;
  if (!dst) {
    CTX_TRY(ctx, ctx->display_out.ensure((std::max<uint64_t>(n, 1) + 3) / 4 * 4, &ctx->bytes));
    dst = ctx->display_out.p;
  }
  gsp_display d = ctx->ta_display;
  d.tonemap = GSP_TONEMAP_CLAMP;
  d.exposure = 0.0f;
  CTX_TRY(ctx, display_map(ctx->stream, (uint32_t)ctx->num_cus, ctx->ta_d[ctx->ta_cur].p, n, display_consts(d, gsp_luminance{}), dst));
  return GSP_OK;
}

extern "C" {

int gsp_temporal_taa(gsp_context* ctx, const gsp_taa* taa, const gsp_display* display, const float* src) {
  if (!ctx) return GSP_ERR_INVALID;
  return taa_ctx(ctx, "gsp_temporal_taa", taa, display, src, nullptr, 0);
}

int gsp_temporal_taa_from_device(gsp_context* ctx, const gsp_taa* taa, const gsp_display* display, const void* device_src, uint64_t bytes) {
  if (!ctx) return GSP_ERR_INVALID;
  return taa_ctx(ctx, "gsp_temporal_taa_from_device", taa, display, nullptr, device_src, bytes);
}

int gsp_download_taa(gsp_context* ctx, float* out) {
  if (!ctx) return GSP_ERR_INVALID;
  int rc = temporal_have_taa(ctx, "gsp_download_taa", out);
  if (rc != GSP_OK) return rc;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  return read_back_bytes(ctx, ctx->ta_d[ctx->ta_cur].p, (size_t)ctx->tp_width * ctx->tp_height * sizeof(q4), out);
}

int gsp_download_taa_display(gsp_context* ctx, uint32_t* out) {
  if (!ctx) return GSP_ERR_INVALID;
  int rc = temporal_have_taa(ctx, "gsp_download_taa_display", out);
  if (rc != GSP_OK) return rc;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  rc = taa_display_run(ctx, nullptr);
  if (rc != GSP_OK) return rc;
  return read_back_bytes(ctx, ctx->display_out.p, (size_t)ctx->tp_width * ctx->tp_height * sizeof(uint32_t), out);
}

int gsp_taa_display_to_device(gsp_context* ctx, void* dst, uint64_t bytes) {
  if (!ctx) return GSP_ERR_INVALID;
  int rc = temporal_have_taa(ctx, "gsp_taa_display_to_device", dst);
  if (rc != GSP_OK) return rc;
  const uint64_t need = (uint64_t)ctx->tp_width * ctx->tp_height * sizeof(uint32_t);
  rc = refuse_too_small(ctx, bytes, need);
  if (rc != GSP_OK) return rc;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  return to_device_tail(ctx, dst, need, ctx->display_out, [&](void* target) { return taa_display_run(ctx, (uint32_t*)target); });
}

}  // extern "C"

extern "C" {

int gsp_frame_luminance(gsp_context* ctx, int drain, gsp_luminance* out) {
  if (!ctx || !out || !ctx->have_frame) return GSP_ERR_INVALID;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  int rc = drain ? pipeline_drain(ctx) : display_peek_sync(ctx, nullptr);
  if (rc != GSP_OK) return rc;
  return display_measure_ctx(ctx, out);
}

int gsp_peek_display(gsp_context* ctx, const gsp_display* display, uint32_t* out, uint32_t* samples_folded) {
  if (!ctx || !out || !ctx->have_frame) return GSP_ERR_INVALID;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  int rc = display_peek_sync(ctx, samples_folded);
  if (rc == GSP_OK) rc = display_run(ctx, display, nullptr);
  if (rc != GSP_OK) return rc;
  return read_back_bytes(ctx, ctx->display_out.p, ctx->num_pixels * sizeof(uint32_t), out);
}

int gsp_peek_display_to_device(gsp_context* ctx, const gsp_display* display, void* dst, uint64_t bytes, uint32_t* samples_folded) {
  if (!ctx || !dst || !ctx->have_frame) return GSP_ERR_INVALID;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  const uint64_t need = ctx->num_pixels * sizeof(uint32_t);
  int rc = refuse_too_small(ctx, bytes, need);
  if (rc == GSP_OK) rc = display_peek_sync(ctx, samples_folded);
  if (rc != GSP_OK) return rc;
  return to_device_tail(ctx, dst, need, ctx->display_out, [&](void* target) { return display_run(ctx, display, (uint32_t*)target); });
}

int gsp_download_display(gsp_context* ctx, const gsp_display* display, uint32_t* out) {
  if (!ctx || !out || !ctx->have_frame) return GSP_ERR_INVALID;
  CTX_TRY(ctx, hipSetDevice(ctx->device));
  int rc = pipeline_drain(ctx);
  if (rc == GSP_OK) rc = display_run(ctx, display, nullptr);
  if (rc != GSP_OK) return rc;
  if (!ctx->subset) return read_back_bytes(ctx, ctx->display_out.p, ctx->num_pixels * sizeof(uint32_t), out);
  std::vector<uint32_t> tmp(ctx->num_pixels);
  rc = read_back_bytes(ctx, ctx->display_out.p, ctx->num_pixels * sizeof(uint32_t), tmp.data());
  if (rc != GSP_OK) return rc;
  std::memset(out, 0, sizeof(uint32_t) * (size_t)ctx->width * ctx->height);
  for (uint64_t i = 0; i < ctx->num_pixels; ++i) out[ctx->pixel_ids_host[i]] = tmp[i];
  return GSP_OK;
}

}  // extern "C"
