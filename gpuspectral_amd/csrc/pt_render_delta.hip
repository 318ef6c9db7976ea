// pt_render_delta.hip -- the <DLT = true> instantiations of k_shade / k_finish (point, spot and directional emitters,
// include/gpuspectral_pt.h "Delta lights") and their launches, in a translation unit of their own like pt_render_scatter.hip: 16 more
// of each of the library's two largest kernels (TEX x VER x LSEL x EST, all with MED = SCT = true: DESIGN.md section 29).
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
// launch(TEX, VER, LSEL, EST, view) with the flags as std::integral_constant values; the view carries both media tables and the triangle count
template <class Launch>
void delta_kernel(const DeltaLaunch& a, Launch&& launch) {
  SceneViewDlt sv;
  static_cast<SceneView&>(sv) = *a.view;
  sv.media = a.media;
  sv.scatter = a.scatter;
  sv.num_tri_lights = a.num_tri_lights;
  const auto with_est = [&](auto TEX, auto VER, auto LSEL) {
    if (a.est) launch(TEX, VER, LSEL, std::true_type{}, sv);
    else launch(TEX, VER, LSEL, std::false_type{}, sv);
  };
  const auto with_pick = [&](auto TEX, auto VER) {
    if (a.lsel) with_est(TEX, VER, std::true_type{});
    else with_est(TEX, VER, std::false_type{});
  };
  if (a.ver && a.tex) with_pick(std::true_type{}, std::true_type{});
  else if (a.ver) with_pick(std::false_type{}, std::true_type{});
  else if (a.tex) with_pick(std::true_type{}, std::false_type{});
  else with_pick(std::false_type{}, std::false_type{});
}
}  // namespace

void launch_shade_delta(const DeltaLaunch& a) {
  const PathQueue cur{a.cur[0], a.cur[1], a.cur[2], a.cur[3]}, next{a.next[0], a.next[1], a.next[2], a.next[3]};
  const ShadowQueue sq{a.shadow[0], a.shadow[1], a.shadow[2]};
  delta_kernel(a, [&](auto TEX, auto VER, auto LSEL, auto EST, const SceneViewDlt& sview) {
    hipLaunchKernelGGL((k_shade<decltype(TEX)::value, decltype(VER)::value, true, decltype(LSEL)::value, decltype(EST)::value, true, true>), dim3(a.blocks), dim3(kShadeBlock), 0,
                       a.stream, sview, *a.rc, a.n_ptr, cur, a.hits, next, sq, a.result, a.tails, a.live, a.slot_paths, a.chunk, (DevStats*)a.stats);
  });
}

void launch_finish_delta(const DeltaLaunch& a) {
  const PathQueue q{a.cur[0], a.cur[1], a.cur[2], a.cur[3]};
  delta_kernel(a, [&](auto TEX, auto VER, auto LSEL, auto EST, const SceneViewDlt& sview) {
    hipLaunchKernelGGL((k_finish<decltype(TEX)::value, decltype(VER)::value, true, decltype(LSEL)::value, decltype(EST)::value, true, true>), dim3(a.blocks), dim3(kBlock), 0, a.stream,
                       sview, *a.rc, a.n, q, a.result, a.tails, a.live, a.slot_paths, (DevStats*)a.stats);
  });
}

}  // namespace gsp
