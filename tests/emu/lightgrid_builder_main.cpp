// tests/emu/lightgrid_builder_main.cpp -- TEST HARNESS, NOT A PRODUCT PATH.
//
// The host side of the light grid (gpuspectral_amd/csrc/pt_lightgrid.h: validation, resolution, header, the builder) and the device
// functions that read its image, as a stand-alone program for the sanitizers (tests/test_lightgrid_cpu.py builds it with
// -fsanitize=address,undefined): random light tables of 1 .. 300 triangles and 0 .. 3 delta records -- NaN, infinite, negative and
// degenerate ones among them -- over boxes with and without extent, at explicit and auto resolutions.  Every image is built into a
// buffer of exactly lightgrid_bytes(), every table is checked, and lookup, pick and hit pdf are run over it with positions inside,
// outside and not finite.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../gpuspectral_amd/csrc/pt_lightgrid.h"

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static double urand() {  // xorshift64*, [0, 1)
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return (double)((g_state * 0x2545f4914f6cdd1dull) >> 11) / 9007199254740992.0;
}

int main() {
  using namespace gsp;
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float boxes[][6] = {{0, 0, 0, 1, 1, 1}, {-3, 0, -2, 5, 0, 2}, {0, 0, 0, 0, 0, 0}, {-1e3f, -1, -1, 1e3f, 1, 1}};
  const uint32_t wants[][3] = {{0, 0, 0}, {1, 1, 1}, {8, 2, 8}, {64, 1, 3}, {5, 7, 3}};
  const uint32_t counts[] = {1, 2, 3, 40, 300};
  unsigned grids = 0;
  for (const auto& box : boxes)
    for (const auto& want3 : wants)
      for (uint32_t n : counts)
        for (uint32_t nd = 0; nd <= 3; nd += 3) {
          std::vector<gsp_triangle_light> lights(n);
          for (uint32_t i = 0; i < n; ++i) {
            for (int v = 0; v < 3; ++v)
              for (int c = 0; c < 3; ++c) lights[i].positions[v][c] = box[c] + (float)(urand() * 1.2 - 0.1) * (box[3 + c] - box[c] + 1.0f);
            for (int c = 0; c < 4; ++c) lights[i].radiance[c] = (float)(urand() * 10.0);
            if (i % 7 == 3) lights[i].radiance[1] = nan;
            if (i % 11 == 5) lights[i].radiance[0] = -50.0f;
            if (i % 13 == 6) lights[i].positions[1][0] = inf;
            if (i % 17 == 8)
              for (int c = 0; c < 3; ++c) lights[i].positions[2][c] = lights[i].positions[0][c];  // no area
          }
          std::vector<gsp_delta_light> delta(nd);
          for (uint32_t i = 0; i < nd; ++i) {
            delta[i] = gsp_delta_light{};
            delta[i].kind = GSP_LIGHT_POINT + i;
            delta[i].position[0] = box[0], delta[i].position[1] = box[4], delta[i].position[2] = box[2];
            delta[i].direction[1] = -1.0f;
            delta[i].intensity[0] = delta[i].intensity[1] = delta[i].intensity[2] = 2.0f;
            delta[i].cos_beam = 0.9f, delta[i].cos_cutoff = 0.5f, delta[i].extent = 3.0f;
          }
          if (check_delta_lights(delta.data(), nd)) return std::printf("the delta records were refused\n"), 1;
          gsp_light_grid want{1u, {want3[0], want3[1], want3[2]}, {0u, 0u, 0u, 0u}};
          if (check_light_grid(&want)) return std::printf("a resolution was refused\n"), 1;
          const uint32_t all = n + nd;
          uint32_t res[3];
          if (lightgrid_resolve(want, box, box + 3, all, res) != 0) return std::printf("a resolution within the cap was refused\n"), 1;
          const uint64_t cells = ((uint64_t)res[0] * res[1]) * res[2];
          if (cells == 0 || cells * all > kLightGridMaxEntries) return std::printf("the resolution breaks the cap\n"), 1;
          for (int c = 0; c < 3; ++c)
            if (!(box[3 + c] > box[c]) && res[c] != 1u) return std::printf("an axis without extent has %u cells\n", res[c]), 1;
          const LightGridHeader g = make_lightgrid_header(box, box + 3, res);
          std::vector<gsp_light_pick> fallback((size_t)all + 1u);
          build_light_pick(lights.data(), n, delta.data(), nd, fallback.data());
          const float inv = light_pick_inv_sum(lights.data(), n, delta.data(), nd);
          std::memcpy(&fallback[all], &inv, sizeof(float));
          std::vector<uint8_t> image(lightgrid_bytes(g.nx, g.ny, g.nz, all));  // exactly: a byte beyond it is the sanitizer's finding
          std::vector<double> weights(cells * all);
          build_light_grid(g, lights.data(), n, delta.data(), nd, fallback.data(), image.data(), weights.data());
          for (double w : weights)
            if (!(w >= 0.0) || !std::isfinite(w)) return std::printf("a weight is negative or not finite\n"), 1;
          for (uint64_t c = 0; c < cells; ++c) {
            const gsp_light_pick* t = (const gsp_light_pick*)(image.data() + sizeof(LightGridHeader) + c * lightgrid_cell_bytes(all));
            double sum = 0.0;
            for (uint32_t j = 0; j < all; ++j) {
              if (t[j].alias >= all) return std::printf("alias out of range\n"), 1;
              sum += (double)t[j].pmf_self;
            }
            if (std::fabs(sum - 1.0) > 1e-4) return std::printf("the pmfs of a cell sum to %.9g\n", sum), 1;
          }
          for (int s = 0; s < 400; ++s) {  // the device functions read nothing beyond the image and the fallback
            f3 p = mk3(box[0] + (float)(urand() * 1.4 - 0.2) * (box[3] - box[0] + 0.5f), box[1] + (float)(urand() * 1.4 - 0.2) * (box[4] - box[1] + 0.5f),
                       box[2] + (float)(urand() * 1.4 - 0.2) * (box[5] - box[2] + 0.5f));
            if (s % 9 == 0) p.x = nan;
            if (s % 9 == 1) p.y = inf;
            if (s % 9 == 2) p = mk3(box[3], box[4], box[5]);
            if (s % 9 == 3) p = mk3(box[0], box[1], box[2]);
            uint32_t ix, iy, iz;
            const uint32_t cell = lightgrid_cell(g, p, ix, iy, iz);
            if (cell != kLightGridNoCell && cell >= cells) return std::printf("cell out of range\n"), 1;
            float pmf;
            if (lightgrid_pick(image.data(), fallback.data(), all, p, (uint32_t)(urand() * 4294967296.0), pmf) >= all) return std::printf("pick out of range\n"), 1;
            const gsp_triangle_light& L = lights[(size_t)(urand() * n) % n];
            const f3 v0 = ld3(L.positions[0]), v1 = ld3(L.positions[1]), v2 = ld3(L.positions[2]);
            const float ps = lightgrid_hit_select_pmf(image.data(), fallback.data(), all, 1.0f / (float)all, p, v0, v1, v2, ld3(L.radiance), light_hit_area(v0, v1, v2));
            if (!(ps >= 0.0f)) return std::printf("a hit pmf is negative or NaN\n"), 1;
          }
          ++grids;
        }
  const gsp_light_grid bad[] = {{1u, {65u, 1u, 1u}, {0u, 0u, 0u, 0u}}, {1u, {4u, 0u, 4u}, {0u, 0u, 0u, 0u}}, {1u, {0u, 0u, 0u}, {0u, 1u, 0u, 0u}}};
  for (const gsp_light_grid& b : bad)
    if (!check_light_grid(&b)) return std::printf("a bad gsp_light_grid was accepted\n"), 1;
  const float cube[6] = {0, 0, 0, 1, 1, 1};
  uint32_t res[3];
  const gsp_light_grid big{1u, {64u, 64u, 64u}, {0u, 0u, 0u, 0u}};
  if (lightgrid_resolve(big, cube, cube + 3, 5u, res) == 0) return std::printf("64^3 cells x 5 lights passed the cap\n"), 1;
  std::printf("%u grids ok\n", grids);
  return 0;
}
