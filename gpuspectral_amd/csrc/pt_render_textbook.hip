// pt_render_textbook.hip -- the <EST = true> instantiations of k_shade / k_finish (GSP_ESTIMATOR_TEXTBOOK, include/gpuspectral_pt.h
// "Estimator") and their launches, in a translation unit of their own.  The estimator flag doubles the instantiations of the two
// largest kernels of the library; compiled next to pt_render.hip instead of inside it, the parallel build stays where it was.
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
// launch(TEX, VER, MED, LSEL, view) with the flags as std::integral_constant values; the <MED> kernels take the view + the media table
template <class Launch>
void textbook_kernel(const TextbookLaunch& a, Launch&& launch) {
  const auto with_view = [&](auto TEX, auto VER, auto LSEL) {
    if (a.media != nullptr) {
      SceneViewMed mv;
      static_cast<SceneView&>(mv) = *a.view;
      mv.media = a.media;
      launch(TEX, VER, std::true_type{}, LSEL, mv);
    } else {
      launch(TEX, VER, std::false_type{}, LSEL, *a.view);
    }
  };
  const auto with_pick = [&](auto TEX, auto VER) {
    if (a.lsel) with_view(TEX, VER, std::true_type{});
    else with_view(TEX, VER, std::false_type{});
  };
  if (a.ver && a.tex) with_pick(std::true_type{}, std::true_type{});
  else if (a.ver) with_pick(std::false_type{}, std::true_type{});
  else if (a.tex) with_pick(std::true_type{}, std::false_type{});
  else with_pick(std::false_type{}, std::false_type{});
}
}  // namespace

void launch_shade_textbook(const TextbookLaunch& a) {
  const PathQueue cur{a.cur[0], a.cur[1], a.cur[2], a.cur[3]}, next{a.next[0], a.next[1], a.next[2], a.next[3]};
  const ShadowQueue sq{a.shadow[0], a.shadow[1], a.shadow[2]};
  textbook_kernel(a, [&](auto TEX, auto VER, auto MED, auto LSEL, const auto& sview) {
    hipLaunchKernelGGL((k_shade<decltype(TEX)::value, decltype(VER)::value, decltype(MED)::value, decltype(LSEL)::value, true>), dim3(a.blocks), dim3(kShadeBlock), 0, a.stream,
                       sview, *a.rc, a.n_ptr, cur, a.hits, next, sq, a.result, a.tails, a.live, a.slot_paths, a.chunk, (DevStats*)a.stats);
  });
}

void launch_finish_textbook(const TextbookLaunch& a) {
  const PathQueue q{a.cur[0], a.cur[1], a.cur[2], a.cur[3]};
  textbook_kernel(a, [&](auto TEX, auto VER, auto MED, auto LSEL, const auto& sview) {
    hipLaunchKernelGGL((k_finish<decltype(TEX)::value, decltype(VER)::value, decltype(MED)::value, decltype(LSEL)::value, true>), dim3(a.blocks), dim3(kBlock), 0, a.stream, sview,
                       *a.rc, a.n, q, a.result, a.tails, a.live, a.slot_paths, (DevStats*)a.stats);
  });
}

}  // namespace gsp
