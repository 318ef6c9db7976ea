// pt_render_kernels.inc -- part of the translation unit pt_render.hip (included there; not compiled on its own).  Also included by
// pt_render_textbook.hip, the translation unit of the <EST = true> instantiations of k_shade / k_finish, with GSP_SHADE_KERNELS_ONLY
// defined: everything behind k_finish is left out there.
// The DEVICE side of the wavefront tracer: queue layouts, the ray sources / result sinks of k_trace (pt_wavetrace.h), k_generate,
// k_shade, k_finish, k_resolve, the table / uv bake kernels, and DevBuf.  Host code: pt_render.hip (context, options),
// pt_render_scene.inc (upload + per-frame edits), pt_render_pipeline.inc (the streaming pipeline + the rest of the C ABI),
// pt_render_post.inc (the stages behind the path tracer: LDR film, denoiser, temporal accumulation, filters).

namespace gsp {

namespace {

constexpr int kBlock = 256;

struct PathQueue {
  q4* P0;
  q4* P1;
  q4* P2;
  q4* P3;
};
struct ShadowQueue {
  q4* S0;
  q4* S1;
  q4* S3;  // (S2, the unoccluded outcome, left the record in r04: k_shade writes it where it belongs)
};

// Device counter words of a pipeline lane.  Two TAIL SETS of 32 words (one 128-B line each), used alternately by
// successive iterations: iteration i appends to the queues whose tails live in set i & 1 and reads its own input size from
// set (i - 1) & 1, so the host can queue iteration i + 1 before it has seen iteration i's counters.  Then the live-path
// counters of the sample slots, then the ray hand-out counters of the extend and connect launches (kWorkShards words each,
// on separate 128-B lines; one set: launches of one stream run in order).  Words [0, C_READBACK) travel to the host once
// per iteration.
// kMaxSlots: a slot of the sample-result ring is held from the injection of its batch until the batch's LAST path has
// ended (up to 52 bounces later) although ~95 % of its paths end within a few bounces, so the number of slots -- not
// the path pool -- bounds the paths in flight on scenes with short paths: with 64 slots the reference's coffee scene
// (4.2 rays per sample) ran 3 M-path launches in a 32 M-path pool (profiles/r02_scene_probe.txt).
constexpr int kMaxSlots = 1024;
constexpr int kTailSet = 32;  // words per tail set
constexpr uint32_t kFillerSid = 0xffffffffu;  // sample-id word of a queue record that is no path (k_shade's chunked reservation)
enum { T_NEXT = 0, T_SHADOW = 1, T_FIN_EXT = 2, T_FIN_SH = 4,  // within a tail set (the two 64-bit k_finish totals are 8-byte aligned)
       T_HOLES_NEXT = 6, T_HOLES_SHADOW = 7 };                   // filler records behind the blocks' last chunks (chunked reservation)
enum { C_LIVE = 2 * kTailSet, C_READBACK = C_LIVE + kMaxSlots,
       C_WORK_EXT = ((C_READBACK + 31) / 32) * 32, C_WORK_SH = C_WORK_EXT + kWorkShards * kWorkStride,
       C_COUNT = C_WORK_SH + kWorkShards * kWorkStride };
#ifdef GSP_SHADE_PROFILE
__device__ unsigned long long g_shade_profile[PR_COUNT * 4];
#endif
struct DevStats {
  unsigned long long shaded, nodes, tris, stat_rays, sh_nodes, sh_tris, sh_rays, sh_occluded, sh_occluded_nodes, lds_nodes, sh_lds_nodes, sh_no_tri;
};

__device__ __forceinline__ q4 mkq(float x, float y, float z, float w) {
  q4 r;
  r.x = x;
  r.y = y;
  r.z = z;
  r.w = w;
  return r;
}
// Queue records are written once and read once per iteration, ~7 GB per iteration through a 256-MiB Infinity Cache that
// would otherwise hold the BVH, the triangle packets and the shading packets (140 MB for a million triangles): the
// streaming accesses of k_generate and k_shade carry the non-temporal hint (A/B: k_shade -3.7 %, bench +1.1 %; on the
// ray loads / hit stores of k_trace the hint costs 1 %, so those stay plain; profiles/r02_ab_nt_queues.txt).
typedef float v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ q4 qld(const q4* p) {
  const v4f v = __builtin_nontemporal_load((const v4f*)p);
  q4 r;
  r.x = v.x;
  r.y = v.y;
  r.z = v.z;
  r.w = v.w;
  return r;
}
__device__ __forceinline__ void qst(q4* p, q4 a) {
  const v4f v = {a.x, a.y, a.z, a.w};
  __builtin_nontemporal_store(v, (v4f*)p);
}
__device__ __forceinline__ uint32_t qld(const uint32_t* p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ void qst(uint32_t* p, uint32_t a) { __builtin_nontemporal_store(a, p); }
__device__ __forceinline__ float ub(uint32_t u) { return __uint_as_float(u); }
__device__ __forceinline__ uint32_t fb(float f) { return __float_as_uint(f); }

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ---- generate ------------------------------------------------------------------
// Appends K timestamps x num_pixels new paths to the queue at `offset`; their sample slots start
// at `sid_base` in the result ring.
// MODE: 0 = the reference's pinhole ray, 1 = with a pixel filter, 2 = through a thin lens (the filter by a runtime branch)
template <int MODE, class RC>
__device__ __forceinline__ void generate_body(RC rc, uint32_t num_pixels, uint32_t K,
                                                      uint32_t first_timestamp,
                                                      const uint32_t* __restrict__ pixel_ids, PathQueue q,
                                                      uint32_t offset, uint32_t sid_base, const q4* __restrict__ memo,
                                                      q4* __restrict__ hits, uint32_t lane, uint32_t lanes, uint32_t ver_bits) {
  // num_pixels = pixels of this pipeline lane: owned pixel lp * lanes + lane for lp in [0, num_pixels)
  const uint64_t total = (uint64_t)num_pixels * K;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (uint64_t)gridDim.x * kBlock) {
    const uint32_t k = (uint32_t)(i / num_pixels), lp = (uint32_t)(i % num_pixels) * lanes + lane;
    const uint32_t gid = pixel_ids ? pixel_ids[lp] : lp;
    const uint32_t sid = sid_base + (uint32_t)i;
    PathState p;
    if constexpr (MODE == 2) generate_path_lens(rc, gid, first_timestamp + k, sid, p);
    else generate_path_t<MODE != 0>(rc, gid, first_timestamp + k, sid, p);
    p.flags |= ver_bits;  // the version of the BSDF / light tables this sample belongs to (pt_stages.h kVerMask)
    const uint64_t j = offset + i;
    qst(&q.P0[j], mkq(p.o.x, p.o.y, p.o.z, p.d.x));
    qst(&q.P1[j], mkq(p.d.y, p.d.z, ub(p.seed), ub(p.sid)));
    qst(&q.P2[j], mkq(p.weight.x, p.weight.y, p.weight.z, p.directWeight));
    qst(&q.P3[j], mkq(0.0f, 0.0f, 0.0f, ub(p.flags)));  // (the ring entry is written once, by the bounce that ends the path)
    // primary-hit memo: the camera ray of a pixel is the same for every sample (no jitter, raygen.rgen:31-38), so its
    // hit record is copied instead of traced again; the extend launch skips these leading entries of the queue
    if (memo) qst(&hits[j], memo[i % num_pixels]);
  }
}

__global__ __launch_bounds__(kBlock) void k_generate(RenderConstsBase rc, uint32_t num_pixels, uint32_t K,
                                                      uint32_t first_timestamp,
                                                      const uint32_t* __restrict__ pixel_ids, PathQueue q,
                                                      uint32_t offset, uint32_t sid_base, const q4* __restrict__ memo,
                                                      q4* __restrict__ hits, uint32_t lane, uint32_t lanes, uint32_t ver_bits) {
  generate_body<false>(rc, num_pixels, K, first_timestamp, pixel_ids, q, offset, sid_base, memo, hits, lane, lanes, ver_bits);
}
// ... with a pixel filter (include/gpuspectral_pt.h): every sample's camera ray goes through its own sub-pixel offset, so the
// launch gets memo = nullptr and the extend launch traces these entries like every other.  A kernel of its own so that the
// unfiltered launch runs the code it ran before.
__global__ __launch_bounds__(kBlock) void k_generate_filtered(RenderConsts rc, uint32_t num_pixels, uint32_t K,
                                                      uint32_t first_timestamp,
                                                      const uint32_t* __restrict__ pixel_ids, PathQueue q,
                                                      uint32_t offset, uint32_t sid_base, const q4* __restrict__ memo,
                                                      q4* __restrict__ hits, uint32_t lane, uint32_t lanes, uint32_t ver_bits) {
  generate_body<true>(rc, num_pixels, K, first_timestamp, pixel_ids, q, offset, sid_base, memo, hits, lane, lanes, ver_bits);
}
// ... through a thin lens (include/gpuspectral_pt.h, "Thin lens"): every sample leaves from its own point of the aperture, so this
// launch too gets memo = nullptr.  The queue stores are generate_body's, non-temporal hint included.
__global__ __launch_bounds__(kBlock) void k_generate_lens(RenderConstsLens rc, uint32_t num_pixels, uint32_t K,
                                                      uint32_t first_timestamp,
                                                      const uint32_t* __restrict__ pixel_ids, PathQueue q,
                                                      uint32_t offset, uint32_t sid_base, const q4* __restrict__ memo,
                                                      q4* __restrict__ hits, uint32_t lane, uint32_t lanes, uint32_t ver_bits) {
  generate_body<2>(rc, num_pixels, K, first_timestamp, pixel_ids, q, offset, sid_base, memo, hits, lane, lanes, ver_bits);
}

// ---- extend / connect / test hook: ray sources and result sinks of k_trace -----------------
struct ExtendIO {  // raygen.rgen:53-58: tmin 0, tmax 1e10, closest hit
  static constexpr float kTmin = 0.0f, kTmax = 1e10f;
  static constexpr bool kVersioned = false, kSplit = false;
  PathQueue q;
  q4* hits;
  __device__ __forceinline__ void load(uint32_t i, f3& o, f3& d, float& tmin, float& tmax, uint32_t& pay) const {
    const q4 p0 = q.P0[i], p1 = q.P1[i];
    o = mk3(p0.x, p0.y, p0.z);
    d = mk3(p0.w, p1.x, p1.y);
    tmin = 0.0f;
    tmax = 1e10f;
  }
  // hit word: slot in bits 0..27, BSDF type of the hit triangle in bits 28..30; miss = all ones
  __device__ __forceinline__ void store(uint32_t i, const HitRec& h, uint32_t aux, uint32_t) const {
    hits[i] = mkq(h.t, h.u, h.v, ub(h.slot < 0 ? 0xffffffffu : ((uint32_t)h.slot | ((aux & 7u) << 28))));
  }
};

// Primary-hit memo (r03): the reference shoots the SAME camera ray for every sample of a pixel -- the sub-pixel jitter is
// commented out, raygen.rgen:38, only the RNG seed depends on the timestamp -- so the depth-0 hit of each owned pixel is
// traced once per frame (this source: ray i = camera ray of owned pixel i, hit record in ExtendIO's format) and copied
// into the hit queue by k_generate for every later sample.  Bit-exact by construction: the closest-hit rule does not
// depend on the traversal.  gsp_stats.memoised_rays counts the path segments answered from the memo: they are not
// traced rays (bench.py's Mrays/s leaves them out).
struct MemoIO {
  static constexpr float kTmin = 0.0f, kTmax = 1e10f;
  static constexpr bool kVersioned = false, kSplit = false;
  RenderConstsBase rc;
  const uint32_t* pixel_ids;
  uint32_t lane, lanes;
  q4* memo;
  __device__ __forceinline__ void load(uint32_t i, f3& o, f3& d, float& tmin, float& tmax, uint32_t& pay) const {
    const uint32_t lp = i * lanes + lane;
    PathState p;
    generate_path_t<false>(rc, pixel_ids ? pixel_ids[lp] : lp, 0u, 0u, p);  // (a filtered frame never uses the memo)
    o = p.o;
    d = p.d;
    tmin = 0.0f;
    tmax = 1e10f;
  }
  __device__ __forceinline__ void store(uint32_t i, const HitRec& h, uint32_t aux, uint32_t) const {
    memo[i] = mkq(h.t, h.u, h.v, ub(h.slot < 0 ? 0xffffffffu : ((uint32_t)h.slot | ((aux & 7u) << 28))));
  }
};

struct ConnectIO {  // rayhit.rchit:737-757: tmin 0.01, tmax Ldist - 0.01, any hit
  static constexpr float kTmin = 0.01f, kTmax = -1.0f;
  static constexpr bool kVersioned = false, kSplit = false;
  ShadowQueue sq;
  q4* next_P2;
  q4* next_P3;
  q4* result;
  float clampv;
  __device__ __forceinline__ void load(uint32_t i, f3& o, f3& d, float& tmin, float& tmax, uint32_t& pay) const {
    const q4 s0 = sq.S0[i], s1 = sq.S1[i];
    o = mk3(s0.x, s0.y, s0.z);
    d = mk3(s1.x, s1.y, s1.z);
    tmin = 0.01f;
    tmax = s0.w;
    pay = fb(s1.w);  // index of the continuing path in the next queue, or none: the commit needs it
  }
  // k_shade has already written the outcome of the UNOCCLUDED verdict where it belongs -- the continuing path's P3 (sum | flags)
  // and P2.w (the MIS weight of rayhit.rchit:785-787), or the sample-result ring for a path that ended at this vertex -- because
  // that is what happens to 80-93 % of the shadow rays (profiles/r04_scene_probe_occlusion.txt).  Only an OCCLUDED ray has work
  // left: one 16-B load of the other outcome and the stores that overwrite the optimistic ones (same stream, later kernel).
  // The values are the ones connect_vertex computed in k_shade either way: nothing is recomputed here.
  __device__ __forceinline__ void store(uint32_t i, const HitRec& h, uint32_t, uint32_t nx) const {
    if (h.slot < 0) return;
    q4 res = sq.S3[i];  // {sum if occluded .rgb, flags of the continuing path | sample id of a path that ended}
    if (nx != 0xffffffffu) {
      next_P3[nx] = res;
      next_P2[nx].w = 1.0f;  // no NEE happened: directWeight stays 1 (rayhit.rchit:788-790)
    } else {
      const uint32_t sid = fb(res.w);
      res.w = 0.0f;
      result[sid] = res;
    }
  }
};

// The same two sources while samples of several GEOMETRY versions are in flight (gsp_update_instances without a drain,
// pt_stages.h): a path's stamp sits in its flags word; a shadow ray finds it in the flags of the continuing path (S3.w) or, when
// the path ended at the vertex, in the word that would have named it.  `nodes` / `tris` of the launch are slot 0 of the ring.
struct GeoRing {
  uint32_t geo;           // pt_stages.h pack_geo
  uint32_t top_off;       // node-record byte offset of the tree whose top the blocks stage into LDS
  uint32_t static_slots;  // split scene: slots of the static tree in front of the ring (0: the ring holds whole trees)
  __device__ __forceinline__ void offsets(uint32_t stamp, uint32_t& node_off, uint32_t& tri_base) const {
    tri_base = static_slots + geo_slot_offset(geo, stamp);
    node_off = tri_base * kNodeBytes;
  }
};
constexpr uint32_t kNoNextBit = 0x80000000u;  // <VER> shadow records: index of the continuing path, or this bit | the geometry stamp
// SPLIT: the ring holds the tree of the edited instances only, the static tree at offset 0 is walked second (pt_wavetrace.h)
template <bool SPLIT>
struct ExtendVerIOT : ExtendIO {
  static constexpr bool kVersioned = true, kSplit = SPLIT;
  GeoRing g;
  __device__ __forceinline__ uint32_t top_offset() const { return g.top_off; }
  __device__ __forceinline__ uint32_t static_slots() const { return g.static_slots; }
  __device__ __forceinline__ void geometry(uint32_t i, uint32_t, uint32_t& node_off, uint32_t& tri_base) const {
    g.offsets(geo_stamp(((const uint32_t*)&q.P3[i])[3]), node_off, tri_base);
  }
};
template <bool SPLIT>
struct ConnectVerIOT : ConnectIO {
  static constexpr bool kVersioned = true, kSplit = SPLIT;
  GeoRing g;
  __device__ __forceinline__ uint32_t top_offset() const { return g.top_off; }
  __device__ __forceinline__ uint32_t static_slots() const { return g.static_slots; }
  __device__ __forceinline__ void geometry(uint32_t i, uint32_t pay, uint32_t& node_off, uint32_t& tri_base) const {
    const uint32_t stamp = (pay & kNoNextBit) ? (pay & (kGeoVersions - 1u)) : geo_stamp(((const uint32_t*)&sq.S3[i])[3]);
    g.offsets(stamp, node_off, tri_base);
  }
  __device__ __forceinline__ void store(uint32_t i, const HitRec& h, uint32_t aux, uint32_t pay) const {
    ConnectIO::store(i, h, aux, (pay & kNoNextBit) ? 0xffffffffu : pay);
  }
};
typedef ExtendVerIOT<false> ExtendVerIO;
typedef ConnectVerIOT<false> ConnectVerIO;
typedef ExtendVerIOT<true> ExtendSplitIO;
typedef ConnectVerIOT<true> ConnectSplitIO;
// GSP_ESTIMATOR_TEXTBOOK (include/gpuspectral_pt.h, "Estimator"): P2.w of the continuing path is not the reference's directWeight
// but lastPdf, the same for both verdicts -- the occluded commit leaves it alone.  Sources of their own (plain, versioned, split):
// the any-hit kernels of a reference-mode context are the ones they were
struct ConnectTextbookIO : ConnectIO {
  __device__ __forceinline__ void store(uint32_t i, const HitRec& h, uint32_t, uint32_t nx) const {
    if (h.slot < 0) return;
    q4 res = sq.S3[i];
    if (nx != 0xffffffffu) {
      next_P3[nx] = res;
    } else {
      const uint32_t sid = fb(res.w);
      res.w = 0.0f;
      result[sid] = res;
    }
  }
};
template <bool SPLIT>
struct ConnectTextbookVerIOT : ConnectTextbookIO {
  static constexpr bool kVersioned = true, kSplit = SPLIT;
  GeoRing g;
  __device__ __forceinline__ uint32_t top_offset() const { return g.top_off; }
  __device__ __forceinline__ uint32_t static_slots() const { return g.static_slots; }
  __device__ __forceinline__ void geometry(uint32_t i, uint32_t pay, uint32_t& node_off, uint32_t& tri_base) const {
    const uint32_t stamp = (pay & kNoNextBit) ? (pay & (kGeoVersions - 1u)) : geo_stamp(((const uint32_t*)&sq.S3[i])[3]);
    g.offsets(stamp, node_off, tri_base);
  }
  __device__ __forceinline__ void store(uint32_t i, const HitRec& h, uint32_t aux, uint32_t pay) const {
    ConnectTextbookIO::store(i, h, aux, (pay & kNoNextBit) ? 0xffffffffu : pay);
  }
};
// the camera rays of the memo and the rays of gsp_trace on a split scene: every ray belongs to the newest version (`stamp`)
struct MemoSplitIO : MemoIO {
  static constexpr bool kVersioned = true, kSplit = true;
  GeoRing g;
  uint32_t stamp;
  __device__ __forceinline__ uint32_t top_offset() const { return g.top_off; }
  __device__ __forceinline__ uint32_t static_slots() const { return g.static_slots; }
  __device__ __forceinline__ void geometry(uint32_t, uint32_t, uint32_t& node_off, uint32_t& tri_base) const { g.offsets(stamp, node_off, tri_base); }
};

struct TestIO {  // gsp_trace
  static constexpr float kTmin = -1.0f, kTmax = -1.0f;
  static constexpr bool kVersioned = false, kSplit = false;
  const float* rays;
  q4* hits;
  const uint32_t* slot_to_global;
  int any_hit;
  uint32_t num_tris;
  __device__ __forceinline__ void load(uint32_t i, f3& o, f3& d, float& tmin, float& tmax, uint32_t& pay) const {
    const float* r = rays + 8ull * i;
    o = mk3(r[0], r[1], r[2]);
    d = mk3(r[4], r[5], r[6]);
    tmin = r[3];
    tmax = r[7];
  }
  __device__ __forceinline__ void store(uint32_t i, const HitRec& h, uint32_t, uint32_t) const {
    const bool hit = h.slot >= 0 && num_tris != 0;
    if (any_hit) hits[i] = mkq(0.0f, 0.0f, 0.0f, ub(hit ? 0u : 0xffffffffu));
    else hits[i] = hit ? mkq(h.t, h.u, h.v, ub(slot_to_global[h.slot])) : mkq(0.0f, 0.0f, 0.0f, ub(0xffffffffu));
  }
};

struct TestSplitIO : TestIO {  // gsp_trace on a split scene (slot_to_global is indexed by the slots counted through both trees)
  static constexpr bool kVersioned = true, kSplit = true;
  GeoRing g;
  uint32_t stamp;
  __device__ __forceinline__ uint32_t top_offset() const { return g.top_off; }
  __device__ __forceinline__ uint32_t static_slots() const { return g.static_slots; }
  __device__ __forceinline__ void geometry(uint32_t, uint32_t, uint32_t& node_off, uint32_t& tri_base) const { g.offsets(stamp, node_off, tri_base); }
};

// ---- shade ----------------------------------------------------------------------
// Four blocks of 256 threads per CU (4 waves per SIMD, <= 128 VGPRs).  The two queue tails (next queue,
// shadow queue) are single words: with one atomic pair per WAVE the ~130k same-address atomics of
// an 8M-path launch serialise at the ~88/us a single address sustains (MI355X_MICROARCH.md,
// "dequeue" row) and cost half the kernel.  So survivors are counted per block through LDS and the
// block reserves its ranges with ONE atomic pair per tile.  Tile = block = 256 paths (r01_j A/B with the
// register budget pinned at 128: 1024 threads 77.7 ms, 512 76.2, 256 72.2, 128 104 per 48 spp): the waves of a
// block cost differently after the BSDF-type sort and meet at five barriers per tile, so four small blocks per CU
// overlap better than one large one, until the atomics per tile take over.
#ifndef GSP_SHADE_BLOCK
#define GSP_SHADE_BLOCK 256
#endif
constexpr int kShadeBlock = GSP_SHADE_BLOCK;
#ifndef GSP_SHADE_TABLE_BYTES
#define GSP_SHADE_TABLE_BYTES 8192
#endif
constexpr int kShadeTableBytes = GSP_SHADE_TABLE_BYTES;  // BSDF + light tables up to this size are staged into LDS by k_shade
constexpr int kShadeWaves = kShadeBlock / 64;
#ifndef GSP_SHADE_GRID_MULT
#define GSP_SHADE_GRID_MULT 1  // grid = exactly the resident blocks, each loops over tiles
#endif
#ifndef GSP_SHADE_MINWAVES
#define GSP_SHADE_MINWAVES 4  // 128 VGPRs: 4 blocks of 256 threads per CU
#endif
// r04: a software-pipelined tile loop (the hit / P0 / P1 records of tile i + 1 brought into a second set of LDS buffers by
// LDS-DMA, global_load_lds_dwordx4, while tile i is shaded; P2 / P3 gathered at the sorted index) was built, is bit-exact
// and measured flat to 2 % SLOWER on five scenes (profiles/r04_ab_shade_pipeline_*.txt; the patch:
// scripts/experiments/r04_shade_pipeline_lds_dma.patch): what the prefetch hides, the two extra gathers cost.
// TEX: scene with textures / an environment map (dormant-feature extension): a second instantiation, so that the code
// of the reference's path (TEX = false) is what it was
// VER: tables of several versions are live (gsp_update_tables while samples were in flight): every vertex reads the version its
// path carries, from HBM / L2 (no LDS copy: it would have to hold every live version) -- unless the versions in flight differ only
// in their GEOMETRY (gsp_update_instances): then the one live version of the tables is staged as usual (SceneView::ver_stride == 0)
// MED: the context holds interior media (gsp_set_media): shade_vertex<.., MED = true> reads the medium number of the hit and the
// table behind SceneViewMed::media (16 B per medium, from L2: a handful of entries that only back-face vertices of glass read).
// Only these instantiations take the larger view: the kernels of a context without media keep their argument layout
// LSEL: the context picks its light by emitted power (gsp_set_light_sampling): shade_vertex<.., LSEL = true> reads the alias table
// behind the light records -- part of the table image, so it is staged into LDS with it and has a copy in every version
// EST: the context runs the textbook estimator (gsp_set_estimator): shade_vertex<.., EST = true>; P2.w carries lastPdf
// SCT (with MED): some medium scatters (gsp_set_media_scattering): shade_vertex<.., SCT = true> and the table behind
// SceneViewSct::scatter, read like the media table.  These instantiations live in pt_render_scatter.hip
// DLT: the context holds delta lights (gsp_set_delta_lights): shade_vertex<.., DLT = true> and SceneViewDlt::num_tri_lights; the
// records sit behind the triangle lights in the table image.  These instantiations live in pt_render_delta.hip
// ENV: the context samples its environment map as a light (gsp_set_envmap_sampling): shade_vertex<.., ENV = true>, miss_emitted_env
// and SceneViewEnv::env_cells; the record is the last of the light table.  These instantiations live in pt_render_envlight.hip
// GRD: the context selects its light through the light grid (gsp_set_light_grid): shade_vertex<.., GRD = true> and
// SceneViewGrd::grid_off; the grid sits behind the pick table of every table version and is read from global memory (tables_bytes
// of the view, and so the staged copy, ends in front of it).  These instantiations live in pt_render_lightgrid.hip
template <bool TEX, bool VER, bool MED, bool LSEL, bool EST, bool SCT = false, bool DLT = false, bool ENV = false, bool GRD = false>
__global__ __launch_bounds__(kShadeBlock, GSP_SHADE_MINWAVES) void k_shade(typename ShadeViewOf<MED, SCT, DLT, ENV, GRD>::type S, RenderConstsBase rc, const uint32_t* __restrict__ n_ptr, PathQueue cur,
                                                        const q4* __restrict__ hits, PathQueue nxt, ShadowQueue sq,
                                                        q4* __restrict__ result, uint32_t* __restrict__ tails,
                                                        uint32_t* __restrict__ live,
                                                        uint32_t slot_paths, uint32_t chunk, DevStats* __restrict__ stats) {
  const uint32_t n = *n_ptr;  // written by the previous iteration's k_shade / the host's memset (stream order)
#ifndef GSP_NO_LDS_TABLES
  // The BSDF and light tables of a scene are a few hundred bytes to a few KB, and every vertex makes two DEPENDENT
  // fetches into them (material record after the shading packet, light record after the RNG draw): staged into LDS
  // once per block those become ~64-cycle reads instead of L2 round trips in a kernel whose 4 waves per SIMD cannot
  // hide them.
  // (VER: only while ONE version of the tables is live -- ver_stride == 0: the versions in flight differ in their geometry)
  __shared__ uint4 s_tables[kShadeTableBytes / 16];
  if ((!VER || S.ver_stride == 0u) && S.tables_bytes <= (uint32_t)kShadeTableBytes) {
    const uint4* src = (const uint4*)S.tables;
    for (uint32_t k = threadIdx.x; k < S.tables_bytes / 16; k += kShadeBlock) s_tables[k] = src[k];
    const uint8_t* lb = (const uint8_t*)s_tables;
    const uint8_t* gb = S.tables;
    S.bsdf.diffuse = (const gsp_diffuse_bsdf*)(lb + ((const uint8_t*)S.bsdf.diffuse - gb));
    S.bsdf.smooth_dielectric = (const gsp_smooth_dielectric_bsdf*)(lb + ((const uint8_t*)S.bsdf.smooth_dielectric - gb));
    S.bsdf.smooth_conductor = (const gsp_smooth_conductor_bsdf*)(lb + ((const uint8_t*)S.bsdf.smooth_conductor - gb));
    S.bsdf.smooth_plastic = (const gsp_smooth_plastic_bsdf*)(lb + ((const uint8_t*)S.bsdf.smooth_plastic - gb));
    S.bsdf.rough_conductor = (const gsp_rough_conductor_bsdf*)(lb + ((const uint8_t*)S.bsdf.rough_conductor - gb));
    S.bsdf.smooth_floor = (const gsp_smooth_floor_bsdf*)(lb + ((const uint8_t*)S.bsdf.smooth_floor - gb));
    S.bsdf.rough_floor = (const gsp_rough_floor_bsdf*)(lb + ((const uint8_t*)S.bsdf.rough_floor - gb));
    S.bsdf.rough_plastic = (const gsp_rough_plastic_bsdf*)(lb + ((const uint8_t*)S.bsdf.rough_plastic - gb));
    S.lights = (const gsp_triangle_light*)(lb + ((const uint8_t*)S.lights - gb));
  }
  // (the barrier behind the s_dead initialisation below also publishes the staged tables)
#endif
  // textured scenes: the byte -> value table and the texture headers sit on the dependent chain packet -> BSDF record ->
  // header -> texels -> decode; from LDS the last and the third hop cost no memory round trip
  constexpr uint32_t kLdsTextures = 64;
  __shared__ float s_decode[TEX ? 256 : 1];
  __shared__ gsp_texture s_textures[TEX ? kLdsTextures : 1];
  if (TEX && S.tex.num_textures != 0) {
    for (uint32_t k = threadIdx.x; k < 256u; k += kShadeBlock) s_decode[k] = S.tex.decode[k];
    S.tex.decode = s_decode;
    if (S.tex.num_textures <= kLdsTextures) {
      for (uint32_t k = threadIdx.x; k < S.tex.num_textures; k += kShadeBlock) s_textures[k] = S.tex.textures[k];
      S.tex.textures = s_textures;
    }
  }
  __shared__ uint32_t s_dead[kMaxSlots];
  __shared__ uint32_t s_bin[12];               // counting sort of the tile by BSDF type: counts, then starts
  __shared__ uint16_t s_order[kShadeBlock];    // sorted position -> thread offset inside the tile
  __shared__ uint32_t s_cnt[2][kShadeWaves];   // per-wave survivor / shadow counts of this iteration
  __shared__ uint32_t s_base[2][kShadeWaves];  // per-wave first rank among the tile's survivors / shadow rays
  __shared__ uint32_t s_alloc[2][3];           // where those ranks go: rank r < R ? A + r : B + (r - R)   {A, R, B}
  __shared__ uint32_t s_room[2][2];            // the block's current chunk of each queue: {next free entry, end}
  if (threadIdx.x < 4) s_room[threadIdx.x >> 1][threadIdx.x & 1] = 0;
  __shared__ q4 s_hq[kShadeBlock], s_p0[kShadeBlock], s_p1[kShadeBlock], s_p2[kShadeBlock], s_p3[kShadeBlock];
  for (uint32_t k = threadIdx.x; k < (uint32_t)kMaxSlots; k += kShadeBlock) s_dead[k] = 0;
#ifdef GSP_SHADE_PROFILE
  for (uint32_t k = threadIdx.x; k < (uint32_t)PR_COUNT * 4; k += kShadeBlock) gsp_prof_table()[k] = 0;
#endif
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = threadIdx.x >> 6;
  const uint64_t lt_mask = (1ull << lane) - 1ull;
  // every thread of the block runs the same number of iterations (barriers inside the loop)
  const uint32_t stride = gridDim.x * kShadeBlock;
  const uint32_t iters = (n + stride - 1) / stride;
  unsigned long long shaded = 0;
  for (uint32_t it = 0; it < iters; ++it) {
    // ---- order the tile by the BSDF type of the hit (8 = miss, 9 = beyond the queue) so that the
    // lanes of a wave run the same branch of the 8-way BSDF switch (rayhit.rchit:630-654): LDS
    // counting sort of the tile's keys, laid out back to back.  (r05: on the bench scene that leaves three pure diffuse waves
    // and one wave with every other type of the tile, for which the others wait at the compaction barrier -- the lane profile,
    // profiles/r05_shade_lane_profile.txt; dealing the keys over the waves halves that wait and does not make the kernel
    // faster, profiles/r05_ab_shade_placement.txt, scripts/experiments/r05_shade_balanced_placement.patch)
    const uint32_t tile = it * stride + blockIdx.x * kShadeBlock;
    GSP_PROF_BEGIN(PR_TILE);
    GSP_PROF_BEGIN(PR_LOADSORT);
    {
      if (threadIdx.x < 12) s_bin[threadIdx.x] = 0;
      __syncthreads();
      const uint32_t i0 = tile + threadIdx.x;
      uint32_t key = 9;
      // the tile is read in queue order (fully coalesced) and handed to its sorted position through LDS
      if (i0 < n) {
        const q4 hq0 = qld(&hits[i0]);
        s_hq[threadIdx.x] = hq0;
        s_p0[threadIdx.x] = qld(&cur.P0[i0]);
        const q4 p1q = qld(&cur.P1[i0]);
        s_p1[threadIdx.x] = p1q;
        s_p2[threadIdx.x] = qld(&cur.P2[i0]);
        s_p3[threadIdx.x] = qld(&cur.P3[i0]);
        const uint32_t w = fb(hq0.w);
        key = (w == 0xffffffffu) ? 8u : ((w >> 28) & 7u);
        if (fb(p1q.w) == kFillerSid) key = 9u;  // a filler record behind some block's last chunk: not a path
      }
      const uint32_t rank = atomicAdd(&s_bin[key], 1u);
      __syncthreads();
      if (threadIdx.x == 0) {
        uint32_t acc = 0;
        for (int k = 0; k < 10; ++k) {
          const uint32_t c = s_bin[k];
          s_bin[k] = acc;
          acc += c;
        }
      }
      __syncthreads();
      s_order[s_bin[key] + rank] = (uint16_t)threadIdx.x;
      __syncthreads();
    }
    GSP_PROF_END(PR_LOADSORT);
    const uint32_t src = s_order[threadIdx.x];
    const uint32_t i = tile + src;
    bool alive = false, has_shadow = false;
    uint32_t my_sid = 0;
    ShadeOut out;
    q4 sum = mkq(0.0f, 0.0f, 0.0f, 0.0f);
#ifdef GSP_SHADE_PROFILE
    {  // how many sort keys (BSDF types, miss, beyond the queue) share this wave?
      const q4 hk = s_hq[src];
      const uint32_t wk = fb(hk.w), key2 = (i < n) ? ((wk == 0xffffffffu) ? 8u : ((wk >> 28) & 7u)) : 9u;
      int kinds = 0;
      for (uint32_t k = 0; k < 10; ++k) kinds += __ballot(key2 == k) != 0ull;
      if (lane == 0) atomicAdd(gsp_prof_table() + 4 * (PR_TYPES_IN_WAVE + kinds), 1ull);
    }
#endif
    const bool valid = i < n && fb(s_p1[src].w) != kFillerSid;
    if (valid) {
      GSP_PROF_BEGIN(PR_FETCH);
      const q4 hq = s_hq[src];
      const q4 p0 = s_p0[src], p1 = s_p1[src], p2 = s_p2[src];
      sum = s_p3[src];  // the sample's sum so far + the flags word
      const uint32_t fl = fb(sum.w);
      my_sid = fb(p1.w);
      HitRec h;
      h.t = hq.x;
      h.u = hq.y;
      h.v = hq.z;
      {
        const uint32_t w = fb(hq.w);
        h.slot = (w == 0xffffffffu) ? -1 : (int32_t)(w & 0x0fffffffu);
      }
      GSP_PROF_END(PR_FETCH);
      if (h.slot >= 0) {  // miss: miss.rmiss:15-18, the path ends and adds nothing
        GSP_PROF_BEGIN(PR_VERTEX);
        PathState in;
        in.o = mk3(p0.x, p0.y, p0.z);
        in.d = mk3(p0.w, p1.x, p1.y);
        in.seed = fb(p1.z);
        in.sid = my_sid;
        in.weight = mk3(p2.x, p2.y, p2.z);
        in.directWeight = p2.w;
        in.flags = fl;
        shade_vertex<TEX, VER, MED, LSEL, EST, SCT, DLT, ENV, GRD>(S, rc, in, h, out, view_media(S), view_scatter(S), view_tri_lights(S), view_env_cells(S), view_grid_off(S));
        alive = out.alive;
        has_shadow = out.has_shadow;
        ++shaded;
        if (!has_shadow) add_emitted(rc.clamp, out.emitted, sum);  // (else k_trace<ConnectIO> adds the bounce's terms)
        GSP_PROF_END(PR_VERTEX);
      } else if (TEX && S.tex.env_texels != nullptr) {  // escaped: environment radiance, then the path ends
        PathState in;
        in.d = mk3(p0.w, p1.x, p1.y);
        in.weight = mk3(p2.x, p2.y, p2.z);
        if constexpr (ENV) {
          in.directWeight = p2.w;
          in.flags = fl;
          add_emitted(rc.clamp, miss_emitted_env<VER>(S, rc, in, view_env_cells(S)), sum);
        } else
        add_emitted(rc.clamp, miss_emitted(S, in), sum);
      }
      // the path ends here and no shadow ray is pending: its sum is the sample
      if (!alive && !has_shadow) result[my_sid] = mkq(sum.x, sum.y, sum.z, 0.0f);
    }
    // paths that ended here leave their sample slot's live count (a slot is resolved when it
    // reaches 0): summed per block in LDS, flushed once at the end of the kernel
    GSP_PROF_BEGIN(PR_COMPACT);
    {
      const bool died = valid && !alive;
      uint64_t dm = __ballot(died);
      const uint32_t slot = my_sid / slot_paths;
      while (dm) {  // wave-uniform; lanes of a wave almost always share a slot
        const int first = __ffsll((unsigned long long)dm) - 1;
        const uint32_t s0 = (uint32_t)__shfl((int)slot, first);
        const uint64_t same = __ballot(died && slot == s0) & dm;
        if ((int)lane == first) atomicAdd(&s_dead[s0], (uint32_t)__popcll(same));
        dm &= ~same;
      }
    }
    // compaction: wave64 ballot + prefix popcount inside the wave, LDS scan over the 16 waves,
    // one atomic per queue per block
    const uint64_t am = __ballot(alive);
    const uint64_t sm = __ballot(has_shadow);
    if (lane == 0) {
      s_cnt[0][wave] = (uint32_t)__popcll(am);
      s_cnt[1][wave] = (uint32_t)__popcll(sm);
    }
    __syncthreads();
    // Room in the two output queues.  Every resident block asks once per tile and waits for the answer at the next barrier,
    // and one cache line takes 88 M atomic requests per second whatever they carry (scripts/microbench/atomic_rate.hip:
    // u32, u64, two lanes of one instruction alike; sixteen lines take sixteen times that).  r04: at 70 M tiles per second the
    // tail line was 79 % busy; r05: 80 M tiles per second, 91 %.  So a block of a large launch takes its room in CHUNKS of
    // `chunk` entries per queue -- one request per ~chunk / 150 tiles, a 64-bit add when both queues run out at once -- and
    // fills its chunks densely: a tile that does not fit uses up the old chunk and continues in the new one.  What a block has
    // left when the kernel ends is filled with records that are no paths (sid / next-path word all ones; rays that start 1e30
    // away and miss the root) and counted in T_HOLES_*: under 1 % of a queue.  chunk == 0 (small launches, statistics runs):
    // the tile's exact room, as before, with ONE 64-bit add for both queues.
    if (threadIdx.x == 0) {
      static_assert(T_NEXT == 0 && T_SHADOW == 1, "the two tails share one 64-bit word");
      uint32_t tot[2] = {0, 0};
      for (int w = 0; w < kShadeWaves; ++w) {
        s_base[0][w] = tot[0];
        s_base[1][w] = tot[1];
        tot[0] += s_cnt[0][w];
        tot[1] += s_cnt[1][w];
      }
      uint32_t rem[2], want[2];
      for (int q = 0; q < 2; ++q) {
        rem[q] = s_room[q][1] - s_room[q][0];
        want[q] = tot[q] > rem[q] ? (chunk ? chunk : tot[q]) : 0u;
      }
      unsigned long long got = 0;
      if (want[0] | want[1]) got = atomicAdd((unsigned long long*)tails, ((unsigned long long)want[1] << 32) | want[0]);
      for (int q = 0; q < 2; ++q) {
        const uint32_t b = q == 0 ? (uint32_t)got : (uint32_t)(got >> 32);
        s_alloc[q][0] = s_room[q][0];
        s_alloc[q][1] = want[q] ? rem[q] : 0xffffffffu;
        s_alloc[q][2] = b;
        if (want[q]) {
          s_room[q][0] = b + (tot[q] - rem[q]);
          s_room[q][1] = b + want[q];
        } else {
          s_room[q][0] += tot[q];
        }
      }
    }
    __syncthreads();
    uint32_t j = s_base[0][wave] + (uint32_t)__popcll(am & lt_mask);
    j = j < s_alloc[0][1] ? s_alloc[0][0] + j : s_alloc[0][2] + (j - s_alloc[0][1]);
    GSP_PROF_END(PR_COMPACT);
    GSP_PROF_BEGIN(PR_WRITE);
    // both outcomes of a bounce with a shadow ray, by the function k_finish and the host harness apply once the verdict is
    // known; the UNOCCLUDED one is written where it belongs right here, the occluded one travels with the shadow ray
    q4 clear = sum, occ = sum;
    if (has_shadow) {
      bool nee_done;
      connect_vertex(rc.clamp, out.shadow, false, clear, nee_done);
      connect_vertex(rc.clamp, out.shadow, true, occ, nee_done);
    }
    if (alive) {
      const PathState& p = out.next;
      qst(&nxt.P0[j], mkq(p.o.x, p.o.y, p.o.z, p.d.x));
      qst(&nxt.P1[j], mkq(p.d.y, p.d.z, ub(p.seed), ub(p.sid)));
      qst(&nxt.P2[j], mkq(p.weight.x, p.weight.y, p.weight.z, has_shadow ? out.shadow.dw_nee : p.directWeight));  // rayhit.rchit:785-787
      qst(&nxt.P3[j], mkq(clear.x, clear.y, clear.z, ub(p.flags)));  // (clear == sum without a shadow ray)
    }
    if (has_shadow) {
      uint32_t s = s_base[1][wave] + (uint32_t)__popcll(sm & lt_mask);
      s = s < s_alloc[1][1] ? s_alloc[1][0] + s : s_alloc[1][2] + (s - s_alloc[1][1]);
      const ShadowRay& r = out.shadow;
      if (!alive) result[my_sid] = mkq(clear.x, clear.y, clear.z, 0.0f);  // the path ended here: its sample, unless occluded
      qst(&sq.S0[s], mkq(r.o.x, r.o.y, r.o.z, r.tmax));
      if (VER) qst(&sq.S1[s], mkq(r.d.x, r.d.y, r.d.z, ub(alive ? j : (kNoNextBit | geo_stamp(fb(sum.w))))));  // (sum.w: the flags the vertex came with)
      else qst(&sq.S1[s], mkq(r.d.x, r.d.y, r.d.z, ub(alive ? j : 0xffffffffu)));
      qst(&sq.S3[s], mkq(occ.x, occ.y, occ.z, ub(alive ? out.next.flags : r.sid)));
    }
    GSP_PROF_END(PR_WRITE);
    GSP_PROF_END(PR_TILE);
  }
  __syncthreads();
  // what is left of the block's last chunks: records that are no paths (see the reservation above)
  {
    const uint32_t a0 = s_room[0][0], e0 = s_room[0][1], a1 = s_room[1][0], e1 = s_room[1][1];
    for (uint32_t k = a0 + threadIdx.x; k < e0; k += kShadeBlock) {
      qst(&nxt.P0[k], mkq(1e30f, 1e30f, 1e30f, 1.0f));
      qst(&nxt.P1[k], mkq(1.0f, 1.0f, 0.0f, ub(kFillerSid)));
      // the versioned ray sources read a record's geometry stamp from P3.w (ExtendVerIOT::geometry): a filler names stamp 0, not
      // whatever the slot held before (r05 ADVICE: it worked only because geo_slot_offset masks to the ring and the ring is zeroed)
      if (VER) qst(&nxt.P3[k], mkq(0.0f, 0.0f, 0.0f, ub(0u)));
    }
    for (uint32_t k = a1 + threadIdx.x; k < e1; k += kShadeBlock) {
      qst(&sq.S0[k], mkq(1e30f, 1e30f, 1e30f, -1.0f));  // tmax < tmin: the ray is over before the root
      qst(&sq.S1[k], mkq(1.0f, 1.0f, 1.0f, ub(VER ? kNoNextBit : 0xffffffffu)));  // (VER: "no next path", stamp 0 -- ConnectVerIOT::geometry)
    }
    if (threadIdx.x == 0 && e0 != a0) atomicAdd(&tails[T_HOLES_NEXT], e0 - a0);
    if (threadIdx.x == 0 && e1 != a1) atomicAdd(&tails[T_HOLES_SHADOW], e1 - a1);
  }
#ifdef GSP_SHADE_PROFILE
  for (uint32_t k = threadIdx.x; k < (uint32_t)PR_COUNT * 4; k += kShadeBlock)
    if (gsp_prof_table()[k]) atomicAdd(&g_shade_profile[k], gsp_prof_table()[k]);
#endif
  for (uint32_t k = threadIdx.x; k < (uint32_t)kMaxSlots; k += kShadeBlock)
    if (s_dead[k]) atomicSub(&live[k], s_dead[k]);
  shaded = wave_sum(shaded);
  if (lane == 0 && shaded) atomicAdd(&stats->shaded, shaded);
}

// ---- finish ----------------------------------------------------------------------
// The last few thousand paths of a drain, one path per lane from its current vertex to its end: extend, shade,
// shadow ray, next bounce, with no queues and no launches in between.  A wavefront iteration over a few hundred
// paths costs ~0.3 ms of launch, memset and read-back latency and a drain has ~45 of them; here every path pays
// only its own chain of dependent loads.  Same stage functions (shade_vertex, connect_vertex, add_emitted) and the
// same per-sample order of additions as k_shade / ConnectIO, so the arithmetic per path is unchanged.
constexpr uint32_t kFinishPaths = 262144;  // scan 0 / 64 k / 256 k / 1 M: 8-spp call 62 / 56 / 54 / 56 ms, 500x500 1-spp frames 88 / 138 / 182 / 184 per s
// the traversal stack of a k_finish lane: one node group per tree level, in LDS ([word][thread]; r02 kept 96 entries per
// lane in scratch memory, 400 B).  Trees deeper than this leave the tail of a drain to the wavefront kernels.
constexpr uint32_t kFinishLevels = 36;
struct FinishStack {
  lds_u32* col;  // this thread's column
  uint32_t top;  // words in use
  __device__ __forceinline__ void push(uint32_t v) { col[(top++) * kBlock] = v; }
  __device__ __forceinline__ uint32_t pop() { return col[(--top) * kBlock]; }
};

template <bool TEX, bool VER, bool MED, bool LSEL, bool EST, bool SCT = false, bool DLT = false, bool ENV = false, bool GRD = false>
__global__ __launch_bounds__(kBlock) void k_finish(typename ShadeViewOf<MED, SCT, DLT, ENV, GRD>::type S, RenderConstsBase rc, uint32_t n, PathQueue q,
                                                    q4* __restrict__ result, uint32_t* __restrict__ tails,
                                                    uint32_t* __restrict__ live,
                                                    uint32_t slot_paths, DevStats* __restrict__ stats) {
  __shared__ uint32_t s_stack[kFinishLevels * kStackWords * kBlock];
  __shared__ uint32_t s_table[kStepTableBytes / 4];
  stage_step_table(s_table, threadIdx.x, kBlock);
  __syncthreads();
  const LdsStepTable tab{(const __attribute__((address_space(3))) char*)s_table};
  FinishStack stk{(lds_u32*)s_stack + threadIdx.x, 0u};
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  unsigned long long ext = 0, sh = 0, shaded = 0;
  uint32_t done_slot = 0xffffffffu;  // sample slot of the path this lane has run to its end (none: beyond the queue)
  if (i < n && fb(q.P1[i].w) != kFillerSid) {  // (not a filler record of k_shade's chunked reservation)
    const q4 p0 = q.P0[i], p1 = q.P1[i], p2 = q.P2[i];
    PathState in;
    in.o = mk3(p0.x, p0.y, p0.z);
    in.d = mk3(p0.w, p1.x, p1.y);
    in.seed = fb(p1.z);
    in.sid = fb(p1.w);
    in.weight = mk3(p2.x, p2.y, p2.z);
    in.directWeight = p2.w;
    const q4 p3 = q.P3[i];
    in.flags = fb(p3.w);
    const uint32_t sid = in.sid;
    q4 res = mkq(p3.x, p3.y, p3.z, 0.0f);  // the sample's sum so far
    // VER: this path's version of the geometry (constant along the path).  Split scene (S.static_slots != 0): the versioned tree
    // holds the edited instances only and sits behind the static tree, which every version shares: a ray walks both, and the hit
    // is min (t, tie-break key) of the two -- the closest-hit rule does not care which tree a triangle lives in.
    const uint32_t goff = VER ? S.static_slots + geo_slot_offset(S.geo, geo_stamp(in.flags)) : 0u;
    const q4* nodes_v = VER ? (const q4*)((const char*)S.nodes + (size_t)goff * kNodeBytes) : S.nodes;
    const q4* isect_v = VER ? S.tri_isect + 3ull * goff : S.tri_isect;
    const bool split = VER && S.static_slots != 0u;
    for (;;) {
      HitRec h;
      uint32_t aux;
      ++ext;
      stk.top = 0;
      uint32_t key = 0xffffffffu;
      bool hit = trace_ray<false>(nodes_v, isect_v, in.o, in.d, 0.0f, 1e10f, h, aux, stk, tab, &key);
      if (split) {
        if (hit) h.slot += (int32_t)S.static_slots;  // (slots are counted through both trees, version-free)
        HitRec h2;
        uint32_t aux2, key2 = 0xffffffffu;
        stk.top = 0;
        if (trace_ray<false>(S.nodes, S.tri_isect, in.o, in.d, 0.0f, 1e10f, h2, aux2, stk, tab, &key2) &&
            (!hit || h2.t < h.t || (h2.t == h.t && key2 < key))) {
          h = h2;
          aux = aux2;
          hit = true;
        }
      }
      if (!hit) {  // miss.rmiss:15-18
        if constexpr (ENV) add_emitted(rc.clamp, miss_emitted_env<VER>(S, rc, in, view_env_cells(S)), res);
        else if (TEX && S.tex.env_texels != nullptr) add_emitted(rc.clamp, miss_emitted(S, in), res);
        break;
      }
      ShadeOut out;
      shade_vertex<TEX, VER, MED, LSEL, EST, SCT, DLT, ENV, GRD>(S, rc, in, h, out, view_media(S), view_scatter(S), view_tri_lights(S), view_env_cells(S), view_grid_off(S));
      ++shaded;
      if (!out.has_shadow) {
        add_emitted(rc.clamp, out.emitted, res);
      } else {
        HitRec hs;
        uint32_t aux2;
        ++sh;
        stk.top = 0;
        bool occluded = trace_ray<true>(nodes_v, isect_v, out.shadow.o, out.shadow.d, 0.01f, out.shadow.tmax, hs, aux2, stk, tab);
        if (split && !occluded) {
          stk.top = 0;
          occluded = trace_ray<true>(S.nodes, S.tri_isect, out.shadow.o, out.shadow.d, 0.01f, out.shadow.tmax, hs, aux2, stk, tab);
        }
        bool nee_done;
        connect_vertex(rc.clamp, out.shadow, occluded, res, nee_done);
        if (!EST && nee_done && out.alive) out.next.directWeight = out.shadow.dw_nee;  // rayhit.rchit:785-787 (EST: lastPdf is in place)
      }
      if (!out.alive) break;
      in = out.next;
    }
    result[sid] = res;
    done_slot = sid / slot_paths;
  }
  // every path of this launch leaves its sample slot's live count: one atomic per wave and slot (the lanes of a wave almost
  // always share a slot), not one per path -- 262 144 of them on one word are 3 ms at the 88 M requests/s a cache line takes
  // (profiles/r04_atomic_rate.txt), most of what this kernel took at the end of a drain
  {
    uint64_t dm = __ballot(done_slot != 0xffffffffu);
    while (dm) {  // wave-uniform
      const int first = __ffsll((unsigned long long)dm) - 1;
      const uint32_t s0 = (uint32_t)__shfl((int)done_slot, first);
      const uint64_t same = __ballot(done_slot == s0) & dm;
      if ((int)(threadIdx.x & 63) == first) atomicSub(&live[s0], (uint32_t)__popcll(same));
      dm &= ~same;
    }
  }
  ext = wave_sum(ext);
  sh = wave_sum(sh);
  shaded = wave_sum(shaded);
  if ((threadIdx.x & 63) == 0) {
    if (ext) atomicAdd((unsigned long long*)(tails + T_FIN_EXT), ext);
    if (sh) atomicAdd((unsigned long long*)(tails + T_FIN_SH), sh);
    if (shaded) atomicAdd(&stats->shaded, shaded);
  }
}

#ifndef GSP_SHADE_KERNELS_ONLY
// ---- resolve ----------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_resolve(uint32_t num_pixels, uint32_t K, uint32_t first_timestamp,
                                                     const q4* __restrict__ result, q4* __restrict__ accum,
                                                     uint32_t lane, uint32_t lanes) {
  for (uint32_t l = blockIdx.x * kBlock + threadIdx.x; l < num_pixels; l += gridDim.x * kBlock) {
    const uint64_t lp = (uint64_t)l * lanes + lane;
    q4 a = accum[lp];
    for (uint32_t k = 0; k < K; ++k) resolve_sample(first_timestamp + k, result[(uint64_t)k * num_pixels + l], a);
    accum[lp] = a;
  }
}

// ---- adaptive sampling (include/gpuspectral_pt.h, ABI 9) ----------------------------------------------------------------
// An adaptive frame samples only the pixels of each lane's ACTIVE LIST: lane-local owned indices l (owned pixel l * lanes + lane)
// in increasing order, so that the camera rays of a launch stay as coherent as the uniform frame's.  k_generate_active /
// k_resolve_active are k_generate / k_resolve with path i mapped to (timestamp k, active[a]) instead of (k, l); they are kernels
// of their own so that the uniform frame's launches -- their arguments and their code -- are exactly what they were.
template <int MODE, class RC>
__device__ __forceinline__ void generate_active_body(RC rc, uint32_t num_active, uint32_t K, uint32_t first_timestamp,
                                                            const uint32_t* __restrict__ pixel_ids, const uint32_t* __restrict__ active,
                                                            PathQueue q, uint32_t offset, uint32_t sid_base, const q4* __restrict__ memo,
                                                            q4* __restrict__ hits, uint32_t lane, uint32_t lanes, uint32_t ver_bits) {
  const uint64_t total = (uint64_t)num_active * K;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (uint64_t)gridDim.x * kBlock) {
    const uint32_t k = (uint32_t)(i / num_active), l = active[i % num_active];
    const uint32_t lp = l * lanes + lane;
    const uint32_t gid = pixel_ids ? pixel_ids[lp] : lp;
    const uint32_t sid = sid_base + (uint32_t)i;
    PathState p;
    if constexpr (MODE == 2) generate_path_lens(rc, gid, first_timestamp + k, sid, p);
    else generate_path_t<MODE != 0>(rc, gid, first_timestamp + k, sid, p);
    p.flags |= ver_bits;
    const uint64_t j = offset + i;
    qst(&q.P0[j], mkq(p.o.x, p.o.y, p.o.z, p.d.x));
    qst(&q.P1[j], mkq(p.d.y, p.d.z, ub(p.seed), ub(p.sid)));
    qst(&q.P2[j], mkq(p.weight.x, p.weight.y, p.weight.z, p.directWeight));
    qst(&q.P3[j], mkq(0.0f, 0.0f, 0.0f, ub(p.flags)));
    if (memo) qst(&hits[j], memo[l]);  // (the memo holds every owned pixel of the lane)
  }
}
__global__ __launch_bounds__(kBlock) void k_generate_active(RenderConstsBase rc, uint32_t num_active, uint32_t K, uint32_t first_timestamp,
                                                            const uint32_t* __restrict__ pixel_ids, const uint32_t* __restrict__ active,
                                                            PathQueue q, uint32_t offset, uint32_t sid_base, const q4* __restrict__ memo,
                                                            q4* __restrict__ hits, uint32_t lane, uint32_t lanes, uint32_t ver_bits) {
  generate_active_body<false>(rc, num_active, K, first_timestamp, pixel_ids, active, q, offset, sid_base, memo, hits, lane, lanes, ver_bits);
}
__global__ __launch_bounds__(kBlock) void k_generate_active_filtered(RenderConsts rc, uint32_t num_active, uint32_t K, uint32_t first_timestamp,
                                                            const uint32_t* __restrict__ pixel_ids, const uint32_t* __restrict__ active,
                                                            PathQueue q, uint32_t offset, uint32_t sid_base, const q4* __restrict__ memo,
                                                            q4* __restrict__ hits, uint32_t lane, uint32_t lanes, uint32_t ver_bits) {
  generate_active_body<true>(rc, num_active, K, first_timestamp, pixel_ids, active, q, offset, sid_base, memo, hits, lane, lanes, ver_bits);
}
__global__ __launch_bounds__(kBlock) void k_generate_active_lens(RenderConstsLens rc, uint32_t num_active, uint32_t K, uint32_t first_timestamp,
                                                            const uint32_t* __restrict__ pixel_ids, const uint32_t* __restrict__ active,
                                                            PathQueue q, uint32_t offset, uint32_t sid_base, const q4* __restrict__ memo,
                                                            q4* __restrict__ hits, uint32_t lane, uint32_t lanes, uint32_t ver_bits) {
  generate_active_body<2>(rc, num_active, K, first_timestamp, pixel_ids, active, q, offset, sid_base, memo, hits, lane, lanes, ver_bits);
}

// the second moment of an adaptive pixel: running mean of Y^2 over its samples, with the recurrence and the NaN rule of
// resolve_sample (a sample whose colour mix is NaN leaves the colour, and so m2, as they were).  Called BEFORE resolve_sample
// folds the same sample: the mix it tests is of the previous mean.
__device__ __forceinline__ void fold_second_moment(uint32_t timestamp, q4 sample, const q4& accum, float& m2) {
  f3 c = mk3(sample.x, sample.y, sample.z);
  const float a = 1.0f / (float)(timestamp + 1u);
  if (timestamp > 0) c = mk3(accum.x, accum.y, accum.z) * (1.0f - a) + c * a;
  if (gisnan(c.x) || gisnan(c.y) || gisnan(c.z)) return;
  const float y = 0.2126f * sample.x + 0.7152f * sample.y + 0.0722f * sample.z;
  m2 = timestamp > 0 ? m2 * (1.0f - a) + (y * y) * a : y * y;
}

__global__ __launch_bounds__(kBlock) void k_resolve_active(uint32_t num_active, uint32_t K, uint32_t first_timestamp,
                                                           const uint32_t* __restrict__ active, const q4* __restrict__ result,
                                                           q4* __restrict__ accum, float* __restrict__ m2, uint32_t* __restrict__ count,
                                                           uint32_t lane, uint32_t lanes) {
  for (uint32_t a = blockIdx.x * kBlock + threadIdx.x; a < num_active; a += gridDim.x * kBlock) {
    const uint64_t lp = (uint64_t)active[a] * lanes + lane;
    q4 acc = accum[lp];
    float m = m2[lp];
    for (uint32_t k = 0; k < K; ++k) {
      const q4 s = result[(uint64_t)k * num_active + a];
      fold_second_moment(first_timestamp + k, s, acc, m);
      resolve_sample(first_timestamp + k, s, acc);  // (the colour: the uniform frame's fold, unchanged)
    }
    accum[lp] = acc;
    m2[lp] = m;
    count[lp] = first_timestamp + K;
  }
}

// The stopping rule of include/gpuspectral_pt.h, in double from the float32 buffers.
struct ConvergeIO {
  const q4* accum;
  const float* m2;
  const uint32_t* count;
  double threshold;
  uint32_t lane, lanes;
};
__device__ __forceinline__ bool adaptive_stops(const ConvergeIO& io, uint64_t lp) {
  const uint32_t n = io.count[lp];
  if (n < 2) return false;
  const q4 mean = io.accum[lp];
  const double yb = 0.2126 * (double)mean.x + 0.7152 * (double)mean.y + 0.0722 * (double)mean.z;
  const double var = fmax((double)io.m2[lp] - yb * yb, 0.0) * (double)n / (double)(n - 1u);
  const double err = sqrt(var / (double)n);
  return err <= io.threshold * fmax(yb, (double)GSP_ADAPTIVE_LUMINANCE_FLOOR);
}

// k_converge, once per checkpoint and lane: a STABLE compaction of the active list to the pixels that go on, in three launches
// and no atomics.  (1) k_converge: the rule per pixel, one wave64 ballot of "keeps going" per wave -> masks, the block's count
// -> blocks[b]; (2) k_converge_scan: one block turns the counts into exclusive offsets and writes the total behind them;
// (3) k_converge_compact: every kept pixel goes to blocks[b] + the popcounts of the waves before it + its rank in its wave.
__global__ __launch_bounds__(kBlock) void k_converge(uint32_t num_active, const uint32_t* __restrict__ active, ConvergeIO io,
                                                     uint64_t* __restrict__ masks, uint32_t* __restrict__ blocks) {
  __shared__ uint32_t s_cnt[kBlock / 64];
  const uint32_t a = blockIdx.x * kBlock + threadIdx.x;
  const bool keep = a < num_active && !adaptive_stops(io, (uint64_t)active[a] * io.lanes + io.lane);
  const uint64_t m = __ballot(keep);
  if ((threadIdx.x & 63) == 0) {
    masks[a / 64] = m;
    s_cnt[threadIdx.x / 64] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t c = 0;
    for (int w = 0; w < kBlock / 64; ++w) c += s_cnt[w];
    blocks[blockIdx.x] = c;
  }
}

constexpr int kScanBlock = 1024;
__global__ __launch_bounds__(kScanBlock) void k_converge_scan(uint32_t num_blocks, uint32_t* __restrict__ blocks) {
  __shared__ uint32_t s[kScanBlock];
  const uint32_t per = (num_blocks + kScanBlock - 1) / kScanBlock;
  const uint32_t b0 = threadIdx.x * per, b1 = min(num_blocks, b0 + per);
  uint32_t sum = 0;
  for (uint32_t b = b0; b < b1; ++b) sum += blocks[b];
  s[threadIdx.x] = sum;
  __syncthreads();
  for (uint32_t off = 1; off < (uint32_t)kScanBlock; off <<= 1) {  // inclusive scan of the per-thread sums
    const uint32_t v = threadIdx.x >= off ? s[threadIdx.x - off] : 0u;
    __syncthreads();
    s[threadIdx.x] += v;
    __syncthreads();
  }
  uint32_t run = s[threadIdx.x] - sum;
  for (uint32_t b = b0; b < b1; ++b) {
    const uint32_t c = blocks[b];
    blocks[b] = run;
    run += c;
  }
  if (threadIdx.x == kScanBlock - 1) blocks[num_blocks] = s[kScanBlock - 1];  // the new active count
}

__global__ __launch_bounds__(kBlock) void k_converge_compact(uint32_t num_active, const uint32_t* __restrict__ active,
                                                             const uint64_t* __restrict__ masks, const uint32_t* __restrict__ blocks,
                                                             uint32_t* __restrict__ out) {
  const uint32_t a = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x / 64;
  const uint64_t m = masks[a / 64];
  if (a < num_active && ((m >> lane) & 1ull)) {
    uint32_t pos = blocks[blockIdx.x] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wave; ++w) pos += (uint32_t)__popcll(masks[blockIdx.x * (kBlock / 64) + w]);
    out[pos] = active[a];
  }
}

__global__ __launch_bounds__(kBlock) void k_iota(uint32_t n, uint32_t* __restrict__ out) {
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) out[i] = i;
}

// ---- resident table records ---------------------------------------------------------------------------------------------
// once per gsp_upload_scene / gsp_update_tables: what a vertex would compute from its light / diffuse record alone (pt_shading.h)
struct BakeTables {  // the resident BSDF tables: records of type t at rec[t] (stride rec_bytes[t]), their derived quads in front (derived_of)
  uint8_t* rec[GSP_BSDF_TYPE_COUNT];
  uint32_t rec_bytes[GSP_BSDF_TYPE_COUNT], num[GSP_BSDF_TYPE_COUNT];
};
__global__ __launch_bounds__(kBlock) void k_bake_tables(gsp_triangle_light* __restrict__ lights, uint32_t num_lights,
                                                        gsp_diffuse_bsdf* __restrict__ diffuse, uint32_t num_diffuse, BakeTables bt) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  for (uint32_t t = 0; t < GSP_BSDF_TYPE_COUNT; ++t)  // (before the diffuse record is rewritten: bake_bsdf reads records as uploaded)
    if (i < bt.num[t]) ((q4s*)bt.rec[t])[-1 - (int32_t)i] = bake_bsdf(t, bt.rec[t] + (size_t)i * bt.rec_bytes[t]);
  if (i < num_lights) {
    gsp_triangle_light L = lights[i];
    bake_light(L);
    lights[i] = L;
  }
  if (i < num_diffuse) {
    gsp_diffuse_bsdf b = diffuse[i];
    bake_diffuse(b);
    diffuse[i] = b;
  }
}

// ---- per-slot texture coordinates (dormant-feature extension) -----------------------------------------------------
// slot -> global triangle (BVH order) -> instance (tri_first is ascending) -> the instance's vertices in the uv array
__global__ __launch_bounds__(kBlock) void k_gather_uv(uint32_t num_tris, uint32_t first_slot, const uint32_t* __restrict__ slot_to_global,
                                                      const uint32_t* __restrict__ tri_first, uint32_t num_instances,
                                                      const gsp_instance* __restrict__ instances, const float* __restrict__ uvs,
                                                      float* __restrict__ tri_uv) {
  uint32_t s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= num_tris) return;
  s += first_slot;
  const uint32_t g = slot_to_global[s];
  uint32_t lo = 0, hi = num_instances;  // last instance with tri_first <= g
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (tri_first[mid] <= g) lo = mid;
    else hi = mid;
  }
  const float* src = uvs + 2ull * (instances[lo].first_vertex + 3ull * (g - tri_first[lo]));
  float* dst = tri_uv + 8ull * s;
  for (int k = 0; k < 6; ++k) dst[k] = src[k];
  dst[6] = dst[7] = 0.0f;
}

// split scene: the triangles of the instances that have moved into the edited instances' tree leave the static one -- their
// slots become all-zero triangles (det == 0: never hit, like the padding slots); the boxes above them stay as they were
__global__ __launch_bounds__(kBlock) void k_retire_triangles(uint32_t num_tris, uint32_t first_slot, const uint32_t* __restrict__ slot_to_global,
                                                             const uint32_t* __restrict__ tri_first, uint32_t num_instances,
                                                             const uint8_t* __restrict__ retired, q4* __restrict__ isect) {
  uint32_t s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= num_tris) return;
  s += first_slot;
  const uint32_t g = slot_to_global[s];
  uint32_t lo = 0, hi = num_instances;  // last instance with tri_first <= g
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (tri_first[mid] <= g) lo = mid;
    else hi = mid;
  }
  if (retired[lo]) {
    const q4 z = mkq(0.0f, 0.0f, 0.0f, 0.0f);
    isect[3ull * s + 0] = z;
    isect[3ull * s + 1] = z;
    isect[3ull * s + 2] = z;
  }
}

// ---- LDR film (pt_display.h; include/gpuspectral_pt.h "LDR film") ------------------------------------------------
// Frame statistics: grid-stride over the compact RGBA32F buffer, one 16-byte load per lane; (sum of q, count, max Y) are reduced
// over the wave and reach the 24-byte record with two 64-bit atomic adds and one 32-bit atomic max per wave.  The sum is an
// integer and the max is taken on non-negative float bit patterns, so the record does not depend on the launch shape.
__global__ __launch_bounds__(kBlock) void k_display_stats(const v4f* __restrict__ src, uint64_t n, DisplayStatsRec* __restrict__ rec) {
  long long s = 0;
  uint32_t c = 0, m = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const v4f v = src[i];
    long long q;
    float Y;
    if (display_stat(v.x, v.y, v.z, q, Y)) {
      s += q;
      c += 1u;
      m = max(m, fb(Y));  // Y >= 0 and finite: its bit pattern orders like its value
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o);
    c += __shfl_xor(c, o);
    m = max(m, (uint32_t)__shfl_xor((int)m, o));
  }
  if ((threadIdx.x & 63u) == 0u && c != 0u) {
    atomicAdd(&rec->sum, (unsigned long long)s);
    atomicAdd(&rec->count, (unsigned long long)c);
    atomicMax(&rec->max_bits, m);
  }
}

// Tone map + encode: each lane converts four consecutive pixels (four 16-byte loads, one 16-byte store); the last group of a
// buffer whose length is not a multiple of four stores its words one by one.  The curve and the encode are template parameters:
// the CLAMP + gamma instantiation carries no Reinhard registers.
typedef uint32_t v4u __attribute__((ext_vector_type(4)));
template <uint32_t TONEMAP, bool SRGB>
__global__ __launch_bounds__(kBlock) void k_display_map(const v4f* __restrict__ src, uint64_t n, DisplayConsts k, uint32_t* __restrict__ dst) {
  const uint64_t groups = (n + 3) / 4;
  for (uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x; g < groups; g += (uint64_t)gridDim.x * kBlock) {
    const uint64_t base = 4 * g;
    if (base + 4 <= n) {
      const v4f a = src[base], b = src[base + 1], c = src[base + 2], d = src[base + 3];
      v4u o;
      o.x = display_pixel_t<TONEMAP, SRGB>(a.x, a.y, a.z, k);
      o.y = display_pixel_t<TONEMAP, SRGB>(b.x, b.y, b.z, k);
      o.z = display_pixel_t<TONEMAP, SRGB>(c.x, c.y, c.z, k);
      o.w = display_pixel_t<TONEMAP, SRGB>(d.x, d.y, d.z, k);
      *(v4u*)(dst + base) = o;
    } else {
      for (uint64_t i = base; i < n; ++i) {
        const v4f a = src[i];
        dst[i] = display_pixel_t<TONEMAP, SRGB>(a.x, a.y, a.z, k);
      }
    }
  }
}

// ---- first-hit feature buffers (pt_features.h; include/gpuspectral_pt.h "Feature buffers") -------------------------------
// One lane owns one owned pixel for the whole call: it loads the pixel's three planes once (16 bytes each), loops over the call's
// timestamps -- the camera ray of the beauty sample (generate_path_t / generate_path_lens), k_finish's per-lane traversal with
// its stack and step table in LDS, the hit's features, the running mean in registers -- and stores the planes once.  No atomics:
// nothing is shared between lanes.  CAMERA as generate_body's MODE: 0 pinhole, 1 pixel filter, 2 thin lens.
// Split scene (G.dyn_nodes != nullptr): the ray walks the static tree and the newest version of the edited instances' tree and
// keeps min (t, tie-break key), as k_finish does.
struct FeatureGeo {
  const q4* dyn_nodes;   // split scene: the edited instances' tree, newest version (else nullptr)
  const q4* dyn_isect;
  const q4* dyn_shade;
  uint32_t static_slots;                // ... whose slots are counted behind these in slot_to_global
  uint32_t num_tris;                    // 0: an empty scene, every ray misses
  const uint32_t* slot_to_global;       // slot -> scene-wide triangle index, as gsp_trace reports it
  const uint32_t* tri_first;            // per instance: its first scene triangle (num_instances + 1 entries)
  uint32_t num_instances;
};
template <int CAMERA>
struct FeatureConsts {
  typedef RenderConstsBase type;
};
template <>
struct FeatureConsts<1> {
  typedef RenderConsts type;
};
template <>
struct FeatureConsts<2> {
  typedef RenderConstsLens type;
};
typedef uint32_t v4w __attribute__((ext_vector_type(4)));
template <bool TEX, int CAMERA>
__global__ __launch_bounds__(kBlock) void k_features(SceneView S, typename FeatureConsts<CAMERA>::type rc, FeatureGeo G, uint32_t num_pixels,
                                                      uint32_t K, uint32_t first_timestamp, const uint32_t* __restrict__ pixel_ids,
                                                      q4* __restrict__ albedo, q4* __restrict__ geom, v4w* __restrict__ ids) {
  __shared__ uint32_t s_stack[kFinishLevels * kStackWords * kBlock];
  __shared__ uint32_t s_table[kStepTableBytes / 4];
  stage_step_table(s_table, threadIdx.x, kBlock);
  __syncthreads();
  const LdsStepTable tab{(const __attribute__((address_space(3))) char*)s_table};
  FinishStack stk{(lds_u32*)s_stack + threadIdx.x, 0u};
  const uint32_t lp = blockIdx.x * kBlock + threadIdx.x;
  if (lp >= num_pixels) return;  // (no barrier below)
  const uint32_t gid = pixel_ids ? pixel_ids[lp] : lp;
  FeaturePixel px;
  px.albedo = qld(&albedo[lp]);
  px.geom = qld(&geom[lp]);
  {
    const v4w w = __builtin_nontemporal_load(&ids[lp]);
    px.tri = w.x;
    px.bsdf = w.y;
    px.inst = w.z;
    px.n = w.w;
  }
  for (uint32_t k = 0; k < K; ++k) {
    PathState p;
    if constexpr (CAMERA == 2) generate_path_lens(rc, gid, first_timestamp + k, 0u, p);
    else generate_path_t<CAMERA != 0>(rc, gid, first_timestamp + k, 0u, p);
    HitRec h;
    uint32_t aux, key = 0xffffffffu;
    stk.top = 0;
    bool hit = trace_ray<false>(S.nodes, S.tri_isect, p.o, p.d, 0.0f, 1e10f, h, aux, stk, tab, &key);
    const q4* shade = S.tri_shade;
    uint32_t slot_base = 0;
    if (G.dyn_nodes != nullptr) {
      HitRec h2;
      uint32_t aux2, key2 = 0xffffffffu;
      stk.top = 0;
      if (trace_ray<false>(G.dyn_nodes, G.dyn_isect, p.o, p.d, 0.0f, 1e10f, h2, aux2, stk, tab, &key2) &&
          (!hit || h2.t < h.t || (h2.t == h.t && key2 < key))) {
        h = h2;
        hit = true;
        shade = G.dyn_shade;
        slot_base = G.static_slots;
      }
    }
    if (hit && G.num_tris != 0u) {
      // (tri_uv is indexed by the slot within the tree that was hit: a textured scene never splits -- scene_may_still_split wants
      // num_textures == 0 -- so a hit that takes uv is a hit in the one tree and slot_base is 0)
      const q4* uv = (TEX && S.tex.tri_uv != nullptr) ? (const q4*)S.tex.tri_uv + 2ll * h.slot : nullptr;
      const FeatureSample f = feature_vertex<TEX>(S.bsdf, S.tex, shade + 4ll * h.slot, uv, p.d, h);
      uint32_t tri = 0u, inst = 0u;
      if (px.n == 0u) {  // (only the first sample of the frame names the pixel's ids)
        tri = G.slot_to_global[slot_base + (uint32_t)h.slot];
        inst = feature_instance(G.tri_first, G.num_instances, tri);
      }
      feature_fold(px, f, tri, inst);
    } else {
      feature_fold(px, feature_miss(), 0xffffffffu, 0xffffffffu);
    }
  }
  qst(&albedo[lp], px.albedo);
  qst(&geom[lp], px.geom);
  {
    const v4w w = {px.tri, px.bsdf, px.inst, px.n};
    __builtin_nontemporal_store(w, &ids[lp]);
  }
}

// ---- denoiser (pt_denoise.h; include/gpuspectral_pt.h "Denoiser") ---------------------------------------------------------
// Three planes of 16 bytes per pixel go through a level: E = {e.rgb, L}, A = {a'.rgb, valid}, G = {n.xyz, z}.
__device__ __forceinline__ dn4 dn_load(const v4f* p) {
  const v4f v = *p;
  return dn4{v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ void dn_store(v4f* p, const dn4& d) {
  v4f v;
  v.x = d.x;
  v.y = d.y;
  v.z = d.z;
  v.w = d.w;
  *p = v;
}

// Prepare: streaming, one pixel per lane and trip -- two 16-byte loads, two 16-byte stores, every access of a wave one 1-KiB run.
// (Records are 16 bytes on both sides, so several pixels per lane would widen nothing, unlike k_display_map's 4-byte words.)
__global__ __launch_bounds__(kBlock) void k_denoise_prepare(const v4f* __restrict__ accum, const v4f* __restrict__ albedo, uint64_t n,
                                                            v4f* __restrict__ E, v4f* __restrict__ A) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    dn4 e, a;
    denoise_prepare(dn_load(accum + i), dn_load(albedo + i), e, a);
    dn_store(E + i, e);
    dn_store(A + i, a);
  }
}

// One level.  A block of 256 lanes owns a tile of 32 x 8 pixels: a wave covers two rows of 32 pixels, i.e. 512-byte runs that
// start on a 16-byte boundary (every record does).
//   S = 1, 2 (levels 0 and 1): the three planes of tile + halo of 2 S pixels are staged in LDS -- (32 + 4 S) x (8 + 4 S) records
//     per plane, 20 736 bytes (S = 1) and 30 720 bytes (S = 2) per block -- by row-major 16-byte loads, and the 25 taps are
//     ds_read_b128 from there.  Out-of-frame records are zero and never read (denoise_pixel_level skips the tap first).
//   S = 0 (levels >= 2): the halo would be wider than the tile; the taps are 16-byte loads from global memory (L2).
// The per-pixel text is denoise_pixel_level either way, with the same taps in the same order: the fetch path cannot change a bit.
// LAST: the level's output goes through denoise_finish (remodulation; an invalid pixel = its accumulate record) into `out`.
constexpr int kDnTileW = 32, kDnTileH = 8;
static_assert(kDnTileW * kDnTileH == kBlock, "a lane per pixel of the tile");
template <int S, bool LAST>
__global__ __launch_bounds__(kBlock) void k_denoise_atrous(const v4f* __restrict__ Ein, const v4f* __restrict__ A, const v4f* __restrict__ G,
                                                           const v4f* __restrict__ accum, v4f* __restrict__ out, DenoiseConsts k, uint32_t level,
                                                           int width, int height) {
  const int px = (int)blockIdx.x * kDnTileW + (int)(threadIdx.x & (kDnTileW - 1));
  const int py = (int)blockIdx.y * kDnTileH + (int)(threadIdx.x / kDnTileW);
  dn4 r;
  if constexpr (S != 0) {
    constexpr int PW = kDnTileW + 4 * S, PH = kDnTileH + 4 * S;
    __shared__ v4f sE[PW * PH], sA[PW * PH], sG[PW * PH];
    const int x0 = (int)blockIdx.x * kDnTileW - 2 * S, y0 = (int)blockIdx.y * kDnTileH - 2 * S;
    for (int i = (int)threadIdx.x; i < PW * PH; i += kBlock) {
      const int ly = i / PW, lx = i - ly * PW;
      const int gx = x0 + lx, gy = y0 + ly;
      v4f e = {0.0f, 0.0f, 0.0f, 0.0f}, a = e, g = e;
      if (gx >= 0 && gx < width && gy >= 0 && gy < height) {
        const size_t idx = (size_t)gy * (size_t)width + (size_t)gx;
        e = Ein[idx];
        a = A[idx];
        g = G[idx];
      }
      sE[i] = e;
      sA[i] = a;
      sG[i] = g;
    }
    __syncthreads();
    if (px >= width || py >= height) return;  // (no barrier below)
    r = denoise_pixel_level(k, level, width, height, px, py, [&](int x, int y, dn4& E_, dn4& A_, dn4& G_) {
      const int i = (y - y0) * PW + (x - x0);  // |x - px| <= 2 S and |y - py| <= 2 S: inside the staged rectangle
      E_ = dn_load(&sE[i]);
      A_ = dn_load(&sA[i]);
      G_ = dn_load(&sG[i]);
    });
  } else {
    if (px >= width || py >= height) return;
    r = denoise_pixel_level(k, level, width, height, px, py, [&](int x, int y, dn4& E_, dn4& A_, dn4& G_) {
      const size_t idx = (size_t)y * (size_t)width + (size_t)x;  // denoise_pixel_level asks for pixels of the frame only
      E_ = dn_load(Ein + idx);
      A_ = dn_load(A + idx);
      G_ = dn_load(G + idx);
    });
  }
  const size_t p = (size_t)py * (size_t)width + (size_t)px;
  if constexpr (LAST) r = denoise_finish(r, dn_load(A + p), dn_load(accum + p));
  dn_store(out + p, r);
}

// ---- temporal accumulation (pt_temporal.h; include/gpuspectral_pt.h "Temporal accumulation") --------------------------------
// One launch per frame.  A block of 256 lanes owns a tile of 32 x 8 pixels like k_denoise_atrous: a wave's own loads (c, albedo,
// geom, ids: 16 bytes each) and stores (H', G': 16 bytes, I': 4 bytes) are 512-byte runs (128-byte for I'), and the four taps of
// neighbouring lanes fall into the same few rows of the previous planes.  A latency-bound gather: temporal_pixel fetches every
// in-frame tap (H, G 16 bytes, I 4 bytes) before it tests the first, so up to twelve independent loads per lane are in flight;
// no LDS, no atomics.  The new history is read again at once (next frame, the denoiser): plain stores.
__global__ __launch_bounds__(kBlock) void k_temporal_reproject(const v4f* __restrict__ accum, const v4f* __restrict__ albedo,
                                                               const v4f* __restrict__ geom, const v4u* __restrict__ ids,
                                                               const v4f* __restrict__ Hprev, const v4f* __restrict__ Gprev,
                                                               const uint32_t* __restrict__ Iprev, v4f* __restrict__ Hout,
                                                               v4f* __restrict__ Gout, uint32_t* __restrict__ Iout, TemporalConsts k) {
  const int px = (int)blockIdx.x * kDnTileW + (int)(threadIdx.x & (kDnTileW - 1));
  const int py = (int)blockIdx.y * kDnTileH + (int)(threadIdx.x / kDnTileW);
  const int width = (int)k.cur.width;
  if (px >= width || py >= (int)k.cur.height) return;
  const size_t p = (size_t)py * (size_t)width + (size_t)px;
  const TemporalOut o = temporal_pixel(k, px, py, dn_load(accum + p), dn_load(albedo + p), dn_load(geom + p), ids[p].z,
                                       [&](int x, int y, dn4& H_, dn4& G_, uint32_t& I_) {
                                         const size_t q = (size_t)y * (size_t)width + (size_t)x;  // temporal_pixel asks for pixels of the frame only
                                         H_ = dn_load(Hprev + q);
                                         G_ = dn_load(Gprev + q);
                                         I_ = Iprev[q];
                                       });
  dn_store(Hout + p, o.H);
  dn_store(Gout + p, o.G);
  Iout[p] = o.I;
}

// ---- variance-guided filter (pt_svgf.h; include/gpuspectral_pt.h "Variance-guided filter") ----------------------------------
// k_temporal_reproject with the moments plane M beside H: a kernel of its own, so that a context which does not track moments
// runs the instruction stream it ran before.  Four more 16-byte loads per lane in flight and one more 16-byte store.
__global__ __launch_bounds__(kBlock) void k_temporal_reproject_moments(const v4f* __restrict__ accum, const v4f* __restrict__ albedo,
                                                                       const v4f* __restrict__ geom, const v4u* __restrict__ ids,
                                                                       const v4f* __restrict__ Hprev, const v4f* __restrict__ Gprev,
                                                                       const uint32_t* __restrict__ Iprev, const v4f* __restrict__ Mprev,
                                                                       v4f* __restrict__ Hout, v4f* __restrict__ Gout, uint32_t* __restrict__ Iout,
                                                                       v4f* __restrict__ Mout, TemporalConsts k) {
  const int px = (int)blockIdx.x * kDnTileW + (int)(threadIdx.x & (kDnTileW - 1));
  const int py = (int)blockIdx.y * kDnTileH + (int)(threadIdx.x / kDnTileW);
  const int width = (int)k.cur.width;
  if (px >= width || py >= (int)k.cur.height) return;
  const size_t p = (size_t)py * (size_t)width + (size_t)px;
  const TemporalMomentsOut o = temporal_pixel_moments(k, px, py, dn_load(accum + p), dn_load(albedo + p), dn_load(geom + p), ids[p].z,
                                                      [&](int x, int y, dn4& H_, dn4& G_, uint32_t& I_, dn4& M_) {
                                                        const size_t q = (size_t)y * (size_t)width + (size_t)x;  // a pixel of the frame
                                                        H_ = dn_load(Hprev + q);
                                                        G_ = dn_load(Gprev + q);
                                                        I_ = Iprev[q];
                                                        M_ = dn_load(Mprev + q);
                                                      });
  dn_store(Hout + p, o.t.H);
  dn_store(Gout + p, o.t.G);
  Iout[p] = o.t.I;
  dn_store(Mout + p, o.M);
}

// ---- moved instances (pt_motion.h; include/gpuspectral_pt.h "Temporal accumulation: moved instances") -------------------------
// k_temporal_reproject / k_temporal_reproject_moments with the per-instance records: kernels of their own, so that a context which
// does not follow instances runs the instruction streams it ran before.  The same 32 x 8 tile.  The chain ids -> record ->
// projection -> taps is three dependent loads deep, so the ids word is asked for first and the six record quads (96 bytes, the
// same few cache lines for every lane of an instance) go out before c, albedo and geom are waited for; the taps are in flight
// together as in the kernels above.  The table is read from global memory: a tile sees a handful of instances, their records stay
// in the vector cache, and a copy to LDS would put a block-wide barrier in front of the first tap (not measured).  A wave none
// of whose lanes is of class 1 skips the record arithmetic (one ballot).  One more 16-byte store per lane: V.
template <bool MOMENTS>
__global__ __launch_bounds__(kBlock) void k_temporal_reproject_follow(const v4f* __restrict__ accum, const v4f* __restrict__ albedo,
                                                                      const v4f* __restrict__ geom, const v4u* __restrict__ ids,
                                                                      const v4f* __restrict__ Hprev, const v4f* __restrict__ Gprev,
                                                                      const uint32_t* __restrict__ Iprev, const v4f* __restrict__ Mprev,
                                                                      const v4f* __restrict__ table, uint32_t num_records, v4f* __restrict__ Hout,
                                                                      v4f* __restrict__ Gout, uint32_t* __restrict__ Iout, v4f* __restrict__ Mout,
                                                                      v4f* __restrict__ Vout, TemporalConsts k) {
  const int px = (int)blockIdx.x * kDnTileW + (int)(threadIdx.x & (kDnTileW - 1));
  const int py = (int)blockIdx.y * kDnTileH + (int)(threadIdx.x / kDnTileW);
  const int width = (int)k.cur.width;
  if (px >= width || py >= (int)k.cur.height) return;
  const size_t p = (size_t)py * (size_t)width + (size_t)px;
  const uint32_t inst = ids[p].z;
  const dn4 c = dn_load(accum + p), alb = dn_load(albedo + p), g = dn_load(geom + p);  // (in flight behind ids; consumed after the record)
  MotionRecord rec = motion_record_of_class(kMotionNoHistory);  // an index the table does not have (the background's among them)
  if (inst < num_records) {
    const v4f* r = table + (size_t)inst * kMotionRecordQuads;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      rec.b[i] = dn_load(r + i);
      rec.n[i] = dn_load(r + 3 + i);
    }
  }
  const bool wave_moved = __ballot(motion_class(rec) == kMotionMoved) != 0;
  const MotionOut o = temporal_pixel_follow<MOMENTS>(k, px, py, c, alb, g, inst, rec, wave_moved,
                                                     [&](int x, int y, dn4& H_, dn4& G_, uint32_t& I_, dn4& M_) {
                                                       const size_t q = (size_t)y * (size_t)width + (size_t)x;  // a pixel of the frame
                                                       H_ = dn_load(Hprev + q);
                                                       G_ = dn_load(Gprev + q);
                                                       I_ = Iprev[q];
                                                       if constexpr (MOMENTS) M_ = dn_load(Mprev + q);
                                                     });
  dn_store(Hout + p, o.t.H);
  dn_store(Gout + p, o.t.G);
  Iout[p] = o.t.I;
  if constexpr (MOMENTS) dn_store(Mout + p, o.M);
  dn_store(Vout + p, o.V);
}

// The initial variance.  A block owns a tile of 32 x 8 pixels and stages tile + halo of 3 -- 38 x 14 records -- in LDS by
// row-major 16-byte loads of E, A and G: G as it is and of E and A the two floats the pass reads, {L, valid}; 12 768 bytes per
// block.  H.len and M are read at the centre only.  Only a pixel whose history is too short walks the 49 taps.  Out-of-frame
// records are zero and never read (svgf_variance_pixel skips the tap first).
__global__ __launch_bounds__(kBlock) void k_svgf_variance(const v4f* __restrict__ E, const v4f* __restrict__ A, const v4f* __restrict__ G,
                                                          const v4f* __restrict__ H, const v4f* __restrict__ M, float* __restrict__ V, SvgfConsts k,
                                                          int width, int height) {
  constexpr int R = kSvgfVarianceRadius, PW = kDnTileW + 2 * R, PH = kDnTileH + 2 * R;
  __shared__ v4f sG[PW * PH];
  __shared__ float2 sLV[PW * PH];
  const int x0 = (int)blockIdx.x * kDnTileW - R, y0 = (int)blockIdx.y * kDnTileH - R;
  for (int i = (int)threadIdx.x; i < PW * PH; i += kBlock) {
    const int ly = i / PW, lx = i - ly * PW;
    const int gx = x0 + lx, gy = y0 + ly;
    v4f g = {0.0f, 0.0f, 0.0f, 0.0f};
    float2 lv = {0.0f, 0.0f};
    if (gx >= 0 && gx < width && gy >= 0 && gy < height) {
      const size_t idx = (size_t)gy * (size_t)width + (size_t)gx;
      g = G[idx];
      lv.x = E[idx].w;
      lv.y = A[idx].w;
    }
    sG[i] = g;
    sLV[i] = lv;
  }
  __syncthreads();
  const int px = (int)blockIdx.x * kDnTileW + (int)(threadIdx.x & (kDnTileW - 1));
  const int py = (int)blockIdx.y * kDnTileH + (int)(threadIdx.x / kDnTileW);
  if (px >= width || py >= height) return;  // (no barrier below)
  const size_t p = (size_t)py * (size_t)width + (size_t)px;
  V[p] = svgf_variance_pixel(k, width, height, px, py, H[p].w, dn_load(M + p), [&](int x, int y, float& L_, float& valid_, dn4& G_) {
    const int i = (y - y0) * PW + (x - x0);  // |x - px| <= 3 and |y - py| <= 3: inside the staged rectangle
    const float2 lv = sLV[i];
    L_ = lv.x;
    valid_ = lv.y;
    G_ = dn_load(&sG[i]);
  });
}

// One level, shaped like k_denoise_atrous: S = 1, 2 (levels 0 and 1) stage E, A, G and V -- 52 bytes per record -- of tile + halo
// of 2 S pixels in LDS, 22 464 bytes (S = 1) and 33 280 bytes (S = 2) per block; the 3 x 3 variance prefilter (step 1) lies
// inside the halo.  S = 0 (levels >= 2) reads its taps from global memory.  The per-pixel text is svgf_pixel_level either way.
// LAST: the colour goes through denoise_finish into `out` and V' is not stored.
template <int S, bool LAST>
__global__ __launch_bounds__(kBlock) void k_svgf_atrous(const v4f* __restrict__ Ein, const v4f* __restrict__ A, const v4f* __restrict__ G,
                                                        const float* __restrict__ Vin, const v4f* __restrict__ hist, v4f* __restrict__ out,
                                                        float* __restrict__ Vout, SvgfConsts k, uint32_t level, int width, int height) {
  const int px = (int)blockIdx.x * kDnTileW + (int)(threadIdx.x & (kDnTileW - 1));
  const int py = (int)blockIdx.y * kDnTileH + (int)(threadIdx.x / kDnTileW);
  SvgfLevelOut r;
  if constexpr (S != 0) {
    constexpr int PW = kDnTileW + 4 * S, PH = kDnTileH + 4 * S;
    __shared__ v4f sE[PW * PH], sA[PW * PH], sG[PW * PH];
    __shared__ float sV[PW * PH];
    const int x0 = (int)blockIdx.x * kDnTileW - 2 * S, y0 = (int)blockIdx.y * kDnTileH - 2 * S;
    for (int i = (int)threadIdx.x; i < PW * PH; i += kBlock) {
      const int ly = i / PW, lx = i - ly * PW;
      const int gx = x0 + lx, gy = y0 + ly;
      v4f e = {0.0f, 0.0f, 0.0f, 0.0f}, a = e, g = e;
      float v = 0.0f;
      if (gx >= 0 && gx < width && gy >= 0 && gy < height) {
        const size_t idx = (size_t)gy * (size_t)width + (size_t)gx;
        e = Ein[idx];
        a = A[idx];
        g = G[idx];
        v = Vin[idx];
      }
      sE[i] = e;
      sA[i] = a;
      sG[i] = g;
      sV[i] = v;
    }
    __syncthreads();
    if (px >= width || py >= height) return;  // (no barrier below)
    r = svgf_pixel_level(k, level, width, height, px, py, [&](int x, int y, dn4& E_, dn4& A_, dn4& G_, float& V_) {
      const int i = (y - y0) * PW + (x - x0);  // |x - px| <= 2 S and |y - py| <= 2 S: inside the staged rectangle
      E_ = dn_load(&sE[i]);
      A_ = dn_load(&sA[i]);
      G_ = dn_load(&sG[i]);
      V_ = sV[i];
    });
  } else {
    if (px >= width || py >= height) return;
    r = svgf_pixel_level(k, level, width, height, px, py, [&](int x, int y, dn4& E_, dn4& A_, dn4& G_, float& V_) {
      const size_t idx = (size_t)y * (size_t)width + (size_t)x;  // svgf_pixel_level asks for pixels of the frame only
      E_ = dn_load(Ein + idx);
      A_ = dn_load(A + idx);
      G_ = dn_load(G + idx);
      V_ = Vin[idx];
    });
  }
  const size_t p = (size_t)py * (size_t)width + (size_t)px;
  if constexpr (LAST) {
    dn_store(out + p, denoise_finish(r.E, dn_load(A + p), dn_load(hist + p)));
  } else {
    dn_store(out + p, r.E);
    Vout[p] = r.V;
  }
}

// ---- illumination history (pt_illum.h; include/gpuspectral_pt.h "Illumination history") ---------------------------------------
// The accumulate with the frame demodulated: k_temporal_reproject (MOMENTS, FOLLOW = false, false), k_temporal_reproject_moments
// (true, false) and k_temporal_reproject_follow<MOMENTS> (FOLLOW = true) with e = c / A blended in place of c.  Kernels of their
// own, launched only by a context with gsp_temporal_demodulate on: every other context runs the instruction streams it ran
// before.  Loads, stores and their order are those of the kernel each one stands for (!FOLLOW: no table read, no V store; the
// record is the constant of class 0 and folds away); the three quotients per lane are added to a kernel that
// waits for its taps.
template <bool MOMENTS, bool FOLLOW>
__global__ __launch_bounds__(kBlock) void k_temporal_reproject_illum(const v4f* __restrict__ accum, const v4f* __restrict__ albedo,
                                                                     const v4f* __restrict__ geom, const v4u* __restrict__ ids,
                                                                     const v4f* __restrict__ Hprev, const v4f* __restrict__ Gprev,
                                                                     const uint32_t* __restrict__ Iprev, const v4f* __restrict__ Mprev,
                                                                     const v4f* __restrict__ table, uint32_t num_records, v4f* __restrict__ Hout,
                                                                     v4f* __restrict__ Gout, uint32_t* __restrict__ Iout, v4f* __restrict__ Mout,
                                                                     v4f* __restrict__ Vout, TemporalConsts k) {
  const int px = (int)blockIdx.x * kDnTileW + (int)(threadIdx.x & (kDnTileW - 1));
  const int py = (int)blockIdx.y * kDnTileH + (int)(threadIdx.x / kDnTileW);
  const int width = (int)k.cur.width;
  if (px >= width || py >= (int)k.cur.height) return;
  const size_t p = (size_t)py * (size_t)width + (size_t)px;
  const uint32_t inst = ids[p].z;
  const dn4 c = dn_load(accum + p), alb = dn_load(albedo + p), g = dn_load(geom + p);
  MotionRecord rec = motion_record_of_class(FOLLOW ? kMotionNoHistory : kMotionStatic);
  bool wave_moved = false;
  if constexpr (FOLLOW) {
    if (inst < num_records) {
      const v4f* r = table + (size_t)inst * kMotionRecordQuads;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        rec.b[i] = dn_load(r + i);
        rec.n[i] = dn_load(r + 3 + i);
      }
    }
    wave_moved = __ballot(motion_class(rec) == kMotionMoved) != 0;
  }
  const MotionOut o = illum_pixel<MOMENTS>(k, px, py, c, alb, g, inst, rec, wave_moved, [&](int x, int y, dn4& H_, dn4& G_, uint32_t& I_, dn4& M_) {
    const size_t q = (size_t)y * (size_t)width + (size_t)x;  // a pixel of the frame
    H_ = dn_load(Hprev + q);
    G_ = dn_load(Gprev + q);
    I_ = Iprev[q];
    if constexpr (MOMENTS) M_ = dn_load(Mprev + q);
  });
  dn_store(Hout + p, o.t.H);
  dn_store(Gout + p, o.t.G);
  Iout[p] = o.t.I;
  if constexpr (MOMENTS) dn_store(Mout + p, o.M);
  if constexpr (FOLLOW) dn_store(Vout + p, o.V);
}

// Prepare of a demodulated history, and the re-modulation of the image read-out: streaming like k_denoise_prepare, one pixel per
// lane and trip, 16-byte loads and stores in 1-KiB runs per wave.
__global__ __launch_bounds__(kBlock) void k_illum_prepare(const v4f* __restrict__ hist, const v4f* __restrict__ albedo, uint64_t n, v4f* __restrict__ E,
                                                          v4f* __restrict__ A) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    dn4 e, a;
    illum_prepare(dn_load(hist + i), dn_load(albedo + i), e, a);
    dn_store(E + i, e);
    dn_store(A + i, a);
  }
}

__global__ __launch_bounds__(kBlock) void k_illum_image(const v4f* __restrict__ hist, const v4f* __restrict__ albedo, uint64_t n, v4f* __restrict__ out) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock)
    dn_store(out + i, illum_image(dn_load(hist + i), dn_load(albedo + i)));
}

// k_svgf_atrous with the feedback store in its epilogue: the one level of a gsp_temporal_svgf_feedback whose output goes into the
// history as well.  A kernel of its own, so that every other level -- and every call without feedback -- runs k_svgf_atrous as
// it stands.  A lane loads its own record of `hist` (16 bytes; the LAST form has it already), replaces the colour by the level's
// and stores it back: no level reads hist at another pixel, so there is no hazard, and the level needs no pass of its own.
// DEMOD: hist holds illumination and takes e; otherwise it takes e * A.
template <int S, bool LAST, bool DEMOD>
__global__ __launch_bounds__(kBlock) void k_svgf_atrous_feedback(const v4f* __restrict__ Ein, const v4f* __restrict__ A, const v4f* __restrict__ G,
                                                                 const float* __restrict__ Vin, v4f* __restrict__ hist, v4f* __restrict__ out,
                                                                 float* __restrict__ Vout, SvgfConsts k, uint32_t level, int width, int height) {
  const int px = (int)blockIdx.x * kDnTileW + (int)(threadIdx.x & (kDnTileW - 1));
  const int py = (int)blockIdx.y * kDnTileH + (int)(threadIdx.x / kDnTileW);
  SvgfLevelOut r;
  if constexpr (S != 0) {
    constexpr int PW = kDnTileW + 4 * S, PH = kDnTileH + 4 * S;
    __shared__ v4f sE[PW * PH], sA[PW * PH], sG[PW * PH];
    __shared__ float sV[PW * PH];
    const int x0 = (int)blockIdx.x * kDnTileW - 2 * S, y0 = (int)blockIdx.y * kDnTileH - 2 * S;
    for (int i = (int)threadIdx.x; i < PW * PH; i += kBlock) {
      const int ly = i / PW, lx = i - ly * PW;
      const int gx = x0 + lx, gy = y0 + ly;
      v4f e = {0.0f, 0.0f, 0.0f, 0.0f}, a = e, g = e;
      float v = 0.0f;
      if (gx >= 0 && gx < width && gy >= 0 && gy < height) {
        const size_t idx = (size_t)gy * (size_t)width + (size_t)gx;
        e = Ein[idx];
        a = A[idx];
        g = G[idx];
        v = Vin[idx];
      }
      sE[i] = e;
      sA[i] = a;
      sG[i] = g;
      sV[i] = v;
    }
    __syncthreads();
    if (px >= width || py >= height) return;  // (no barrier below)
    r = svgf_pixel_level(k, level, width, height, px, py, [&](int x, int y, dn4& E_, dn4& A_, dn4& G_, float& V_) {
      const int i = (y - y0) * PW + (x - x0);  // |x - px| <= 2 S and |y - py| <= 2 S: inside the staged rectangle
      E_ = dn_load(&sE[i]);
      A_ = dn_load(&sA[i]);
      G_ = dn_load(&sG[i]);
      V_ = sV[i];
    });
  } else {
    if (px >= width || py >= height) return;
    r = svgf_pixel_level(k, level, width, height, px, py, [&](int x, int y, dn4& E_, dn4& A_, dn4& G_, float& V_) {
      const size_t idx = (size_t)y * (size_t)width + (size_t)x;  // svgf_pixel_level asks for pixels of the frame only
      E_ = dn_load(Ein + idx);
      A_ = dn_load(A + idx);
      G_ = dn_load(G + idx);
      V_ = Vin[idx];
    });
  }
  const size_t p = (size_t)py * (size_t)width + (size_t)px;
  const dn4 a = dn_load(A + p), h = dn_load(hist + p);
  if constexpr (LAST) {
    dn_store(out + p, denoise_finish(r.E, a, h));
  } else {
    dn_store(out + p, r.E);
    Vout[p] = r.V;
  }
  dn_store(hist + p, illum_feedback<DEMOD>(r.E, a, h));
}

// ---- temporal anti-lag (pt_antilag.h; include/gpuspectral_pt.h "Temporal anti-lag") ---------------------------------------------
// Step A, the fast history: the frame's accumulate once more with F of the older fast plane in H's place and no plane but F'
// written -- k_temporal_reproject (FOLLOW, DEMOD = false, false), k_temporal_reproject_follow<false> (true, false) and
// k_temporal_reproject_illum<false, FOLLOW> (DEMOD) stand behind it, with their tile, their loads and their order.  G and I of
// the taps come from the older history set, which the accumulate left as it was.  Kernels of their own, launched only by
// gsp_temporal_antilag: the accumulate runs the instruction streams it ran before.
template <bool FOLLOW, bool DEMOD>
__global__ __launch_bounds__(kBlock) void k_antilag_fast(const v4f* __restrict__ accum, const v4f* __restrict__ albedo, const v4f* __restrict__ geom,
                                                         const v4u* __restrict__ ids, const v4f* __restrict__ Fprev, const v4f* __restrict__ Gprev,
                                                         const uint32_t* __restrict__ Iprev, const v4f* __restrict__ table, uint32_t num_records,
                                                         v4f* __restrict__ Fout, TemporalConsts k) {
  const int px = (int)blockIdx.x * kDnTileW + (int)(threadIdx.x & (kDnTileW - 1));
  const int py = (int)blockIdx.y * kDnTileH + (int)(threadIdx.x / kDnTileW);
  const int width = (int)k.cur.width;
  if (px >= width || py >= (int)k.cur.height) return;
  const size_t p = (size_t)py * (size_t)width + (size_t)px;
  const uint32_t inst = ids[p].z;
  const dn4 c = dn_load(accum + p), alb = dn_load(albedo + p), g = dn_load(geom + p);
  MotionRecord rec = motion_record_of_class(FOLLOW ? kMotionNoHistory : kMotionStatic);
  bool wave_moved = false;
  if constexpr (FOLLOW) {
    if (inst < num_records) {
      const v4f* r = table + (size_t)inst * kMotionRecordQuads;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        rec.b[i] = dn_load(r + i);
        rec.n[i] = dn_load(r + 3 + i);
      }
    }
    wave_moved = __ballot(motion_class(rec) == kMotionMoved) != 0;
  }
  dn_store(Fout + p, antilag_fast_pixel<FOLLOW, DEMOD>(k, px, py, c, alb, g, inst, rec, wave_moved, [&](int x, int y, dn4& F_, dn4& G_, uint32_t& I_) {
             const size_t q = (size_t)y * (size_t)width + (size_t)x;  // a pixel of the frame
             F_ = dn_load(Fprev + q);
             G_ = dn_load(Gprev + q);
             I_ = Iprev[q];
           }));
}

// Step B, the clamp of the newest history into the box of F's window statistics, in place.  A block owns a tile of 32 x 8 pixels
// and stages tile + apron of R -- (32 + 2 R) x (8 + 2 R) records, 38 x 14 at R = 3 -- in LDS by row-major 16-byte loads, one per
// lane and plane as k_svgf_variance does: F' as it is, and of G the normal with the instance word I in the place of the depth,
// which the window does not read -- two 16-byte records per pixel, 17 024 bytes per block at R = 3, and two ds_read_b128 per
// tap.  A tap of a wave is two rows of 32 consecutive records: the 16 lanes of a ds_read_b128 group lie in one row at 16
// distinct 16-byte slots of the 256-byte bank row, so the reads are free of bank conflicts at any row pitch, and no padding is
// needed.  Out-of-frame records are zero and never read (antilag_clamp_pixel skips the tap first).  H is read once per pixel
// and written only where it left its box.
template <int R>
__global__ __launch_bounds__(kBlock) void k_antilag_clamp(const v4f* __restrict__ F, const v4f* __restrict__ G, const uint32_t* __restrict__ I,
                                                          v4f* __restrict__ H, AntilagParams a, float normal_min, int width, int height) {
  constexpr int PW = kDnTileW + 2 * R, PH = kDnTileH + 2 * R;
  __shared__ v4f sF[PW * PH], sN[PW * PH];
  const int x0 = (int)blockIdx.x * kDnTileW - R, y0 = (int)blockIdx.y * kDnTileH - R;
  for (int i = (int)threadIdx.x; i < PW * PH; i += kBlock) {
    const int ly = i / PW, lx = i - ly * PW;
    const int gx = x0 + lx, gy = y0 + ly;
    v4f f = {0.0f, 0.0f, 0.0f, 0.0f}, n = f;
    if (gx >= 0 && gx < width && gy >= 0 && gy < height) {
      const size_t idx = (size_t)gy * (size_t)width + (size_t)gx;
      f = F[idx];
      n = G[idx];
      n.w = u2f(I[idx]);
    }
    sF[i] = f;
    sN[i] = n;
  }
  __syncthreads();
  const int px = (int)blockIdx.x * kDnTileW + (int)(threadIdx.x & (kDnTileW - 1));
  const int py = (int)blockIdx.y * kDnTileH + (int)(threadIdx.x / kDnTileW);
  if (px >= width || py >= height) return;  // (no barrier below)
  const size_t p = (size_t)py * (size_t)width + (size_t)px;
  a.radius = R;
  const AntilagClampOut o = antilag_clamp_pixel(a, normal_min, width, height, px, py, dn_load(H + p), [&](int x, int y, dn4& F_, dn4& G_, uint32_t& I_) {
    const int i = (y - y0) * PW + (x - x0);  // |x - px| <= R and |y - py| <= R: inside the staged rectangle
    F_ = dn_load(&sF[i]);
    G_ = dn_load(&sN[i]);
    I_ = f2u(G_.w);
  });
  if (o.changed) dn_store(H + p, o.H);
}

// ---- temporal anti-aliasing (pt_taa.h; include/gpuspectral_pt.h "Temporal anti-aliasing") ---------------------------------------
// One launch per resolve.  A block owns a tile of 32 x 8 pixels and stages X -- YCoCg of the toned source -- of tile + halo of 1,
// 34 x 10 records of 16 bytes (5440 bytes), in LDS: every source pixel is read once with a 16-byte load and toned once, and the
// nine taps of the box are ds_read_b128 of rows of 32 consecutive records, free of bank conflicts at any row pitch as in
// k_antilag_clamp.  A record outside the frame is marked by .w = 0 (inside: 1) and never read: taa_pixel skips the tap first, the
// definition counts only pixels inside the frame.  V is one 16-byte load, issued in front of the staging; the four history taps
// are 16-byte global loads of neighbouring records of the older D, served by L2; D' is one 16-byte store.  No atomics, one
// barrier.  The curve is a template parameter: the CLAMP instantiation carries no Reinhard registers.
template <uint32_t TONEMAP>
__global__ __launch_bounds__(kBlock) void k_taa_resolve(const v4f* __restrict__ src, const v4f* __restrict__ V, const v4f* __restrict__ Dprev,
                                                        v4f* __restrict__ Dout, TaaParams a, DisplayConsts k, int taa_valid, int width, int height) {
  constexpr int PW = kDnTileW + 2, PH = kDnTileH + 2;
  __shared__ v4f sX[PW * PH];
  const int x0 = (int)blockIdx.x * kDnTileW - 1, y0 = (int)blockIdx.y * kDnTileH - 1;
  const int px = (int)blockIdx.x * kDnTileW + (int)(threadIdx.x & (kDnTileW - 1));
  const int py = (int)blockIdx.y * kDnTileH + (int)(threadIdx.x / kDnTileW);
  const bool inside = px < width && py < height;
  const size_t p = (size_t)py * (size_t)width + (size_t)px;
  dn4 v = {0.0f, 0.0f, 0.0f, 0.0f};
  if (inside) v = dn_load(V + p);
  for (int i = (int)threadIdx.x; i < PW * PH; i += kBlock) {
    const int ly = i / PW, lx = i - ly * PW;
    const int gx = x0 + lx, gy = y0 + ly;
    v4f x = {0.0f, 0.0f, 0.0f, 0.0f};
    if (gx >= 0 && gx < width && gy >= 0 && gy < height) {
      const dn4 X = taa_source_t<TONEMAP>(dn_load(src + ((size_t)gy * (size_t)width + (size_t)gx)), k);
      x.x = X.x;
      x.y = X.y;
      x.z = X.z;
      x.w = 1.0f;
    }
    sX[i] = x;
  }
  __syncthreads();
  if (!inside) return;  // (no barrier below)
  dn_store(Dout + p, taa_pixel(
                         a, taa_valid != 0, width, height, px, py, v,
                         [&](int x, int y) { return dn_load(&sX[(y - y0) * PW + (x - x0)]); },  // |x - px| <= 1 and |y - py| <= 1: inside the staged rectangle
                         [&](int x, int y) { return dn_load(Dprev + ((size_t)y * (size_t)width + (size_t)x)); }));  // a pixel of the frame
}

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t count = 0;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    count = 0;
  }
  void swap(DevBuf& o) {
    std::swap(p, o.p);
    std::swap(count, o.count);
  }
  hipError_t ensure(size_t n, ByteLedger* tally) {
    if (n <= count && p) return hipSuccess;
    if (tally && p) tally->sub(count * sizeof(T));
    release();
    n = n ? n : 1;
    hipError_t e = hipMalloc((void**)&p, n * sizeof(T));
    if (e == hipSuccess) {
      count = n;
      if (tally) tally->add(n * sizeof(T));
    }
    return e;
  }
  hipError_t upload(const T* src, size_t n, hipStream_t s, ByteLedger* tally) {
    hipError_t e = ensure(n, tally);
    if (e != hipSuccess || n == 0 || !src) return e;
    return hipMemcpyAsync(p, src, n * sizeof(T), hipMemcpyHostToDevice, s);
  }
};

std::mutex g_err_mutex;
std::string g_create_error = "";

#endif  // GSP_SHADE_KERNELS_ONLY

}  // namespace

}  // namespace gsp
