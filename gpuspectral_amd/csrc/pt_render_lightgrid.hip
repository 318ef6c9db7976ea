// pt_render_lightgrid.hip -- the <GRD = true> instantiations of k_shade / k_finish (spatial light selection through the light grid,
// include/gpuspectral_pt.h "Light grid") and their launches, in a translation unit of their own like pt_render_envlight.hip: 2 more
// of each of the library's two largest kernels (VER, all with TEX = MED = LSEL = EST = SCT = DLT = true and ENV = false: DESIGN.md
// section 31).  The kernels are the templates of pt_render_kernels.inc, nothing is defined here but the rule that picks the
// instantiation.
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
// launch(VER, view) with the flag as a std::integral_constant value; the view carries the media tables, the triangle count and the grid's offset
template <class Launch>
void lightgrid_kernel(const GridLaunch& a, Launch&& launch) {
  SceneViewGrd sv;
  static_cast<SceneView&>(sv) = *a.view;
  sv.media = a.media;
  sv.scatter = a.scatter;
  sv.num_tri_lights = a.num_tri_lights;
  sv.grid_off = a.grid_off;
  if (a.ver) launch(std::true_type{}, sv);
  else launch(std::false_type{}, sv);
}
}  // namespace

void launch_shade_lightgrid(const GridLaunch& a) {
  const PathQueue cur{a.cur[0], a.cur[1], a.cur[2], a.cur[3]}, next{a.next[0], a.next[1], a.next[2], a.next[3]};
  const ShadowQueue sq{a.shadow[0], a.shadow[1], a.shadow[2]};
  lightgrid_kernel(a, [&](auto VER, const SceneViewGrd& sview) {
    hipLaunchKernelGGL((k_shade<true, decltype(VER)::value, true, true, true, true, true, false, true>), dim3(a.blocks), dim3(kShadeBlock), 0, a.stream, sview, *a.rc,
                       a.n_ptr, cur, a.hits, next, sq, a.result, a.tails, a.live, a.slot_paths, a.chunk, (DevStats*)a.stats);
  });
}

void launch_finish_lightgrid(const GridLaunch& a) {
  const PathQueue q{a.cur[0], a.cur[1], a.cur[2], a.cur[3]};
  lightgrid_kernel(a, [&](auto VER, const SceneViewGrd& sview) {
    hipLaunchKernelGGL((k_finish<true, decltype(VER)::value, true, true, true, true, true, false, true>), dim3(a.blocks), dim3(kBlock), 0, a.stream, sview, *a.rc,
                       a.n, q, a.result, a.tails, a.live, a.slot_paths, (DevStats*)a.stats);
  });
}

}  // namespace gsp
