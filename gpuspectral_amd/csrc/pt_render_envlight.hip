// pt_render_envlight.hip -- the <ENV = true> instantiations of k_shade / k_finish (the environment map sampled as a light,
// include/gpuspectral_pt.h "Environment light") and their launches, in a translation unit of their own like pt_render_delta.hip: 4 more
// of each of the library's two largest kernels (VER x LSEL, all with TEX = MED = EST = SCT = DLT = true: DESIGN.md section 30).
// The kernels are the templates of pt_render_kernels.inc, nothing is defined here but the rule that picks the instantiation.
#include <cstddef>
#include <cstring>
#include <type_traits>
#include <vector>

#include "pt_hostmath.h"
#include "pt_internal.h"
#include "pt_versions.h"
#include "pt_wavetrace.h"
#include "pt_features.h"

#define GSP_SHADE_KERNELS_ONLY
#include "pt_render_kernels.inc"

namespace gsp {

namespace {
// launch(VER, LSEL, view) with the flags as std::integral_constant values; the view carries the media tables, the triangle count and the cell table
template <class Launch>
void envlight_kernel(const EnvLaunch& a, Launch&& launch) {
  SceneViewEnv sv;
  static_cast<SceneView&>(sv) = *a.view;
  sv.media = a.media;
  sv.scatter = a.scatter;
  sv.num_tri_lights = a.num_tri_lights;
  sv.env_cells = a.env_cells;
  const auto with_pick = [&](auto VER) {
    if (a.lsel) launch(VER, std::true_type{}, sv);
    else launch(VER, std::false_type{}, sv);
  };
  if (a.ver) with_pick(std::true_type{});
  else with_pick(std::false_type{});
}
}  // namespace

void launch_shade_envlight(const EnvLaunch& a) {
  const PathQueue cur{a.cur[0], a.cur[1], a.cur[2], a.cur[3]}, next{a.next[0], a.next[1], a.next[2], a.next[3]};
  const ShadowQueue sq{a.shadow[0], a.shadow[1], a.shadow[2]};
  envlight_kernel(a, [&](auto VER, auto LSEL, const SceneViewEnv& sview) {
    hipLaunchKernelGGL((k_shade<true, decltype(VER)::value, true, decltype(LSEL)::value, true, true, true, true>), dim3(a.blocks), dim3(kShadeBlock), 0,
                       a.stream, sview, *a.rc, a.n_ptr, cur, a.hits, next, sq, a.result, a.tails, a.live, a.slot_paths, a.chunk, (DevStats*)a.stats);
  });
}

void launch_finish_envlight(const EnvLaunch& a) {
  const PathQueue q{a.cur[0], a.cur[1], a.cur[2], a.cur[3]};
  envlight_kernel(a, [&](auto VER, auto LSEL, const SceneViewEnv& sview) {
    hipLaunchKernelGGL((k_finish<true, decltype(VER)::value, true, decltype(LSEL)::value, true, true, true, true>), dim3(a.blocks), dim3(kBlock), 0, a.stream,
                       sview, *a.rc, a.n, q, a.result, a.tails, a.live, a.slot_paths, (DevStats*)a.stats);
  });
}

}  // namespace gsp
