// tests/emu/display_emu.cpp -- TEST HARNESS, NOT A PRODUCT PATH.
//
// The LDR film of the library (include/gpuspectral_pt.h, "LDR film") compiled for the host: the very text the kernels
// k_display_stats / k_display_map run (csrc/pt_display.h), driven by plain loops, plus gsp_*_display's validation and the
// resolution of a gsp_display into the kernels' constants.  Built into tests/emu/libdisplay_emu.so by the tests that use it.
#include "../../gpuspectral_amd/csrc/pt_display.h"

using namespace gsp;

extern "C" {

// the validation + struct_size rule.  Returns 0 and the stored display in *out, or 1 and the error text in err (cap bytes)
int display_emu_resolve(const gsp_display* in, gsp_display* out, char* err, uint32_t cap) {
  const char* why = resolve_display(in, *out);
  if (why && err && cap) {
    std::strncpy(err, why, cap - 1);
    err[cap - 1] = 0;
  }
  return why ? 1 : 0;
}

// the frame statistics of n RGBA32F records, by a plain loop
void display_emu_stats(const float* rgba, uint64_t n, gsp_luminance* out) {
  DisplayStatsRec rec{};
  long long sum = 0;
  for (uint64_t i = 0; i < n; ++i) {
    long long q;
    float Y;
    if (!display_stat(rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2], q, Y)) continue;
    sum += q;
    rec.count += 1;
    if (f2u(Y) > rec.max_bits) rec.max_bits = f2u(Y);
  }
  rec.sum = (unsigned long long)sum;
  *out = display_luminance(rec);
}

// the statistics record of given partial sums (a partition of a frame): S, n and the max bits -> the public record
void display_emu_combine(int64_t sum, uint64_t count, float max, gsp_luminance* out) {
  DisplayStatsRec rec{};
  rec.sum = (unsigned long long)sum;
  rec.count = count;
  rec.max_bits = f2u(max);
  *out = display_luminance(rec);
}

// out6 = {tonemap, srgb, bits(2^exposure), bits(1/gamma), bits(scale), bits(invWp2)} as gsp_*_display resolves them; the frame is
// measured (from rgba, n) only where the display asks for it.  Returns 1 on an invalid display
int display_emu_consts(const gsp_display* in, const float* rgba, uint64_t n, uint32_t* out6) {
  gsp_display d;
  if (resolve_display(in, d)) return 1;
  gsp_luminance lum{};
  if (display_needs_stats(d)) display_emu_stats(rgba, n, &lum);
  const DisplayConsts k = display_consts(d, lum);
  out6[0] = k.tonemap;
  out6[1] = k.srgb;
  out6[2] = f2u(k.exposure_scale);
  out6[3] = f2u(k.inv_gamma);
  out6[4] = f2u(k.scale);
  out6[5] = f2u(k.inv_wp2);
  return 0;
}

// gsp_download_display of a compact buffer: n RGBA8 words.  Returns 1 on an invalid display
int display_emu_map(const gsp_display* in, const float* rgba, uint64_t n, uint32_t* out) {
  gsp_display d;
  if (resolve_display(in, d)) return 1;
  gsp_luminance lum{};
  if (display_needs_stats(d)) display_emu_stats(rgba, n, &lum);
  const DisplayConsts k = display_consts(d, lum);
  for (uint64_t i = 0; i < n; ++i) out[i] = display_pixel(rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2], k);
  return 0;
}

// the linear value before step 4 of one pixel's luminance under REINHARD (a test hook for the white-point property): Y'
float display_emu_reinhard_luma(const gsp_display* in, const float* rgba, uint64_t n, float Y) {
  gsp_display d;
  if (resolve_display(in, d)) return -1.0f;
  gsp_luminance lum{};
  if (display_needs_stats(d)) display_emu_stats(rgba, n, &lum);
  const DisplayConsts k = display_consts(d, lum);
  const float Ye = Y * k.exposure_scale;
  const float Lp = Ye * k.scale;
  return (Lp * (1.0f + Lp * k.inv_wp2)) / (1.0f + Lp);
}

}  // extern "C"
