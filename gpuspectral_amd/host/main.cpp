// main.cpp -- headless counterpart of the reference's S/main.cpp:15-30:
//   Engine + PathTracer + loadScene + Window::run(frame loop)
// becomes: load the Mitsuba XML, render N samples per pixel, write the HDR framebuffer.
//   gsp_render [--dormant-features] [--builtin-shapes] [--no-nee] [--memory-share F] [--pool-paths N] <scene.xml> <out.pfm> [width height spp [devices]]
//   devices: "0" (default) or a list "0,1,2,3": the frame is then tiled over those GPUs (MultiGpuPathTracer); an index
//   may repeat.  --dormant-features: LoadOptions::dormantFeatures (bitmap / checkerboard textures, envmap emitter);
//   --builtin-shapes: LoadOptions::builtinShapes (`disk` / `sphere` shapes are tessellated instead of skipped);
//   --no-nee: gsp_render_params.disable_nee = 1 (RenderParams.nee = false); --memory-share / --pool-paths: gsp_ctx_options (how much device memory the path pool takes)
//   --adaptive T [--adaptive-min N] [--adaptive-step N]: adaptive sampling (gsp_render_params.adaptive_*): spp is then the most a
//   pixel gets; a pixel stops at the first checkpoint where its relative standard error is <= T
//   --filter none|box|tent[:r]|gaussian[:s]: pixel filter (gsp_render_params.pixel_filter / _param: anti-aliasing by sub-pixel
//   jitter drawn from the filter); --scene-filter: LoadOptions::readFilter (the film's <rfilter>; --filter other than none wins)
//   --aperture R --focus-distance D | --focus-pixel X,Y [--blades N[:rot_deg]]: thin lens (gsp_set_lens; depth of field).
//   --light-sampling uniform|power: gsp_set_light_sampling (uniform = the reference's pick, the default; power = by emitted power).
//   --estimator reference|textbook: gsp_set_estimator (reference = the reference's weights, the default; textbook = unbiased).
//   --scene-media: LoadOptions::readMedia (the shapes' <medium name="interior">: coloured glass, gsp_set_media).
//   --scene-scattering: LoadOptions::readScattering (implies --scene-media; sigmaS / albedo and the hg phase: gsp_set_media_scattering).
//   --scene-emitters: LoadOptions::readEmitters (top-level point / spot / directional emitters: gsp_set_delta_lights).
//   --env-sampling [--env-extent R]: sample the scene's environment map as a light (gsp_set_envmap_sampling; with --dormant-features, which
//     loads the map).  R = the radius of the scene as the power pick is to see it, default: the radius of the scene's bounds.  Implies
//     --estimator textbook; an error beside an explicit --estimator reference.
//   --light-grid [NX,NY,NZ]: spatial light selection (gsp_set_light_grid), one alias table per cell of a grid over the scene; without a
//     resolution the library chooses one.  It implies nothing else: without --light-sampling power --estimator textbook the run ends
//     with the library's error text and exit code 2.
//   --point-light X,Y,Z,R,G,B (repeatable): one more point light of that position and radiant intensity, for a scene file without an emitter element.
//   --focus-pixel runs the autofocus (gsp_focus_distance) on that fragCoord before rendering; --scene-lens: LoadOptions::readLens
//   (a thinlens sensor's aperture_radius / focus_distance; the flags above override the scene's values one by one)
//   --features PREFIX [--feature-spp N]: also render the feature buffers (gpuspectral_pt.h "Feature buffers"; N samples per pixel,
//   default the frame's spp, under the frame's filter and lens) and write PREFIX.albedo.pfm / .normal.pfm / .depth.pfm and
//   PREFIX.albedo.png / .normal.png (the normal mapped as 0.5 + 0.5 n).  Without --features nothing more is written or printed.
//   --ldr out.png: also write the LDR film (gpuspectral_pt.h "LDR film": tone-mapped and encoded on the GPU) as an 8-bit RGB PNG;
//   --tonemap clamp|aces|reinhard[:key[:burn]], --exposure E (f-stops), --gamma G|srgb: its gsp_display; --scene-film:
//   LoadOptions::readFilm (the sensor's ldrfilm; the flags override the scene's values one by one).  Without --ldr: no PNG
//   --denoise out.pfm [--denoise-iterations N] [--denoise-sigma c,n,z,a]: also write the denoised frame (gpuspectral_pt.h
//   "Denoiser"; N = 1..8 levels, the four sigmas of colour, normal, depth and albedo: 0 = the default, inf = that term off).  It
//   uses the feature planes of --features, or runs a feature pass of its own at the frame's spp, filter and lens.  With --ldr
//   (one device) the LDR film of the denoised frame goes to out.png beside it.  Without --denoise nothing more is written or printed.
//   --temporal out.pfm --temporal-frames N [--temporal-orbit DEG]: render N frames of spp samples each (gpuspectral_pt.h "Temporal
//   accumulation"), the scene's camera turned by DEG degrees about the world y axis through the origin between frames (the
//   loader keeps no look-at point), every frame accumulated into the history; out.pfm receives the history after the last frame
//   and, with --denoise, out.dn.pfm its filtered form.  The files of the other flags are those of the LAST frame.  One device.
//   --temporal-follow [--temporal-move INST,DX,DY,DZ] [--motion out.pfm] (with --temporal): the history follows moved instances
//   (gpuspectral_pt.h "Temporal accumulation: moved instances"); --temporal-move translates render object INST by (DX, DY, DZ)
//   between frames, --motion writes the motion plane of the last frame as {dx, dy, class} (a PFM holds three channels).
//   --temporal-demodulate (with --temporal): the history accumulates colour / first-hit albedo (gpuspectral_pt.h "Illumination
//   history") and out.pfm of --temporal receives the image read-out (the history re-modulated by the last frame's albedo).
//   --svgf-feedback LEVELS (with --svgf): on every frame of --temporal-frames the output of the filter's first LEVELS levels is
//   written back into the history (gsp_temporal_svgf_feedback); the files of --temporal and --denoise show the fed-back history.
//   --temporal-antilag [--antilag-fast N] [--antilag-radius R] [--antilag-sigma S] (with --temporal): on every frame, between the
//   accumulate and any --svgf-feedback, a fast history of at most N frames is kept beside the long one and the long one is clamped
//   into the box of its statistics over (2 R + 1)^2 pixels, S standard deviations wide (gpuspectral_pt.h "Temporal anti-lag").
//   --taa out.png [--taa-alpha A] [--taa-sigma S] (with --temporal and --temporal-follow): on every frame the tone-mapped frame is
//   resolved over its own history (gpuspectral_pt.h "Temporal anti-aliasing"; A = the weight of the new frame in (0, 1], S = the
//   half-width of the neighbourhood box in standard deviations) -- the output of --svgf (of --svgf-feedback where given) as its
//   source, else the image of the history -- under the display of --tonemap / --exposure / --gamma; out.png receives the last
//   frame's resolve.
//   --svgf out.pfm [--svgf-sigma S] [--svgf-min-history N] (with --temporal): the history keeps its luminance moments and out.pfm
//   receives its variance-guided filter (gpuspectral_pt.h "Variance-guided filter"; S = sigma_variance, inf = the term off; N =
//   2..65536), with the levels and guide sigmas of --denoise-iterations / --denoise-sigma where --denoise is given.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <stdexcept>
#include <string>
#include <vector>

#include "Image.h"
#include "Loader.h"
#include "PathTracer.h"

using namespace GPUSpectral;

int main(int argc, char** argv) {
  LoadOptions options;
  gsp_ctx_options ctxOptions;
  gsp_default_ctx_options(&ctxOptions);
  bool nee = true;
  uint32_t lightSampling = GSP_LIGHTS_UNIFORM;
  uint32_t estimator = GSP_ESTIMATOR_REFERENCE;
  bool estimatorGiven = false, envSampling = false;
  bool lightGrid = false;
  uint32_t lightGridRes[3] = {0, 0, 0};  // (0, 0, 0 = the library chooses)
  float envExtent = -1.0f;  // (-1 = not given: the radius of the scene's bounds)
  float adaptive = 0.0f;
  uint32_t adaptiveMin = 0, adaptiveStep = 0;
  uint32_t filter = GSP_FILTER_NONE;
  float filterParam = 0.0f;
  float aperture = -1.0f, focusDistance = -1.0f, focusX = 0.0f, focusY = 0.0f, bladeRotation = 0.0f;  // (-1 = not given)
  bool focusPixel = false;
  int blades = -1;
  std::string ldrPath;
  std::vector<gsp_delta_light> pointLights;  // --point-light, behind the scene's own (--scene-emitters)
  std::string featuresPrefix;
  int featureSpp = -1;  // (-1 = not given: the frame's spp)
  std::string denoisePath;
  std::string temporalPath;
  int temporalFrames = 0;  // (0 = not given)
  float temporalOrbit = 0.0f;
  bool temporalOptions = false;
  bool temporalFollow = false, temporalMove = false;
  long temporalMoveInst = 0;
  float temporalMoveBy[3] = {0.0f, 0.0f, 0.0f};
  std::string motionPath;
  bool temporalDemodulate = false;
  long svgfFeedback = 0;  // (0 = not given)
  bool temporalAntilag = false, antilagOptions = false;
  gsp_antilag antilag{};
  antilag.struct_size = (uint32_t)sizeof(gsp_antilag);
  std::string taaPath;
  bool taaOptions = false;
  gsp_taa taa{};
  taa.struct_size = (uint32_t)sizeof(gsp_taa);
  std::string svgfPath;
  gsp_svgf svgf{};
  svgf.struct_size = (uint32_t)sizeof(gsp_svgf);
  bool svgfOptions = false;
  gsp_denoise denoise{};
  denoise.struct_size = (uint32_t)sizeof(gsp_denoise);
  bool denoiseOptions = false;
  int tonemap = -1;  // (-1 = not given)
  float tmKey = -1.0f, tmBurn = -1.0f, exposure = 0.0f, gamma = -1.0f;
  bool haveExposure = false;
  auto parseFloat = [](const char* s, float& out) {
    char* e = nullptr;
    out = std::strtof(s, &e);
    return e != s && *e == 0 && std::isfinite(out);
  };
  while (argc > 1 && argv[1][0] == '-' && argv[1][1] == '-') {
    const std::string flag = argv[1];
    int used = 1;
    if (flag == "--dormant-features") options.dormantFeatures = true;
    else if (flag == "--builtin-shapes") options.builtinShapes = true;
    else if (flag == "--no-nee") nee = false;
    else if (flag == "--light-sampling" && argc > 2) {
      const std::string v = argv[2];
      if (v == "uniform") lightSampling = GSP_LIGHTS_UNIFORM;
      else if (v == "power") lightSampling = GSP_LIGHTS_POWER;
      else {
        std::fprintf(stderr, "--light-sampling: uniform or power, not '%s'\n", v.c_str());
        return 2;
      }
      used = 2;
    }
    else if (flag == "--estimator" && argc > 2) {
      const std::string v = argv[2];
      if (v == "reference") estimator = GSP_ESTIMATOR_REFERENCE;
      else if (v == "textbook") estimator = GSP_ESTIMATOR_TEXTBOOK;
      else {
        std::fprintf(stderr, "--estimator: reference or textbook, not '%s'\n", v.c_str());
        return 2;
      }
      estimatorGiven = true;
      used = 2;
    }
    else if (flag == "--light-grid") {  // (the resolution is optional: NX,NY,NZ right behind the flag)
      lightGrid = true;
      unsigned a = 0, b = 0, c = 0;
      char tail = 0;
      if (argc > 2 && std::sscanf(argv[2], "%u,%u,%u%c", &a, &b, &c, &tail) == 3) {
        lightGridRes[0] = a, lightGridRes[1] = b, lightGridRes[2] = c;
        used = 2;
      }
    }
    else if (flag == "--env-sampling") envSampling = true;
    else if (flag == "--env-extent" && argc > 2) {
      envExtent = (float)std::atof(argv[2]);
      if (!(envExtent > 0.0f)) {
        std::fprintf(stderr, "gsp_render: --env-extent R: a radius > 0\n");
        return 2;
      }
      used = 2;
    }
    else if (flag == "--memory-share" && argc > 2) ctxOptions.memory_share = std::atof(argv[2]), used = 2;
    else if (flag == "--pool-paths" && argc > 2) ctxOptions.pool_paths = std::strtoull(argv[2], nullptr, 10), used = 2;
    else if (flag == "--adaptive" && argc > 2) adaptive = (float)std::atof(argv[2]), used = 2;
    else if (flag == "--adaptive-min" && argc > 2) adaptiveMin = (uint32_t)std::strtoul(argv[2], nullptr, 10), used = 2;
    else if (flag == "--adaptive-step" && argc > 2) adaptiveStep = (uint32_t)std::strtoul(argv[2], nullptr, 10), used = 2;
    else if (flag == "--scene-filter") options.readFilter = true;
    else if (flag == "--scene-lens") options.readLens = true;
    else if (flag == "--scene-film") options.readFilm = true;
    else if (flag == "--scene-media") options.readMedia = true;
    else if (flag == "--scene-scattering") options.readScattering = true;
    else if (flag == "--scene-emitters") options.readEmitters = true;
    else if (flag == "--point-light" && argc > 2) {
      float v[6];
      int end = 0;
      if (std::sscanf(argv[2], "%f,%f,%f,%f,%f,%f%n", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &end) != 6 || argv[2][end] != 0) {
        std::fprintf(stderr, "gsp_render: --point-light X,Y,Z,R,G,B: a position and a radiant intensity\n");
        return 2;
      }
      gsp_delta_light l{};
      l.kind = GSP_LIGHT_POINT;
      for (int c = 0; c < 3; ++c) l.position[c] = v[c], l.intensity[c] = v[3 + c];
      pointLights.push_back(l);
      used = 2;
    }
    else if (flag == "--ldr" && argc > 2) ldrPath = argv[2], used = 2;
    else if (flag == "--features" && argc > 2) featuresPrefix = argv[2], used = 2;
    else if (flag == "--feature-spp" && argc > 2) {
      char* e = nullptr;
      const long v = std::strtol(argv[2], &e, 10);
      if (e == argv[2] || *e != 0 || v < 1 || v > 1000000) {
        std::fprintf(stderr, "gsp_render: --feature-spp N: a sample count of at least 1\n");
        return 2;
      }
      featureSpp = (int)v, used = 2;
    }
    else if (flag == "--denoise" && argc > 2) denoisePath = argv[2], used = 2;
    else if (flag == "--temporal" && argc > 2) temporalPath = argv[2], used = 2;
    else if (flag == "--temporal-frames" && argc > 2) {
      char* e = nullptr;
      const long v = std::strtol(argv[2], &e, 10);
      if (e == argv[2] || *e != 0 || v < 1 || v > 100000) {
        std::fprintf(stderr, "gsp_render: bad temporal frames '%s' (expected 1..100000)\n", argv[2]);
        return 2;
      }
      temporalFrames = (int)v, temporalOptions = true, used = 2;
    } else if (flag == "--temporal-orbit" && argc > 2) {
      if (!parseFloat(argv[2], temporalOrbit) || temporalOrbit < -360.0f || temporalOrbit > 360.0f) {
        std::fprintf(stderr, "gsp_render: bad temporal orbit '%s' (expected degrees per frame within -360 .. 360)\n", argv[2]);
        return 2;
      }
      temporalOptions = true, used = 2;
    }
    else if (flag == "--temporal-follow") temporalFollow = true, used = 1;
    else if (flag == "--temporal-move" && argc > 2) {
      char* end = nullptr;
      temporalMoveInst = std::strtol(argv[2], &end, 10);
      bool ok = end != argv[2] && temporalMoveInst >= 0;
      for (int k = 0; k < 3 && ok; ++k) {
        ok = *end == ',';
        if (!ok) break;
        const char* from = end + 1;
        temporalMoveBy[k] = std::strtof(from, &end);
        ok = end != from && std::isfinite(temporalMoveBy[k]);
      }
      if (!ok || *end != 0) {
        std::fprintf(stderr, "gsp_render: bad temporal move '%s' (expected INST,DX,DY,DZ: an object index and a finite translation per frame)\n", argv[2]);
        return 2;
      }
      temporalMove = true, used = 2;
    } else if (flag == "--motion" && argc > 2) motionPath = argv[2], used = 2;
    else if (flag == "--temporal-demodulate") temporalDemodulate = true, used = 1;
    else if (flag == "--svgf-feedback" && argc > 2) {
      char* end = nullptr;
      svgfFeedback = std::strtol(argv[2], &end, 10);
      if (end == argv[2] || *end != 0 || svgfFeedback < 1 || svgfFeedback > 8) {
        std::fprintf(stderr, "gsp_render: bad svgf feedback '%s' (expected the number of levels fed back, 1..8 and at most the filter's iterations)\n", argv[2]);
        return 2;
      }
      used = 2;
    } else if (flag == "--temporal-antilag") temporalAntilag = true, used = 1;
    else if ((flag == "--antilag-fast" || flag == "--antilag-radius") && argc > 2) {
      const bool fast = flag == "--antilag-fast";
      char* end = nullptr;
      const long v = std::strtol(argv[2], &end, 10);
      if (end == argv[2] || *end != 0 || v < 1 || v > (fast ? 64 : 3)) {
        if (fast) std::fprintf(stderr, "gsp_render: bad antilag fast history '%s' (expected the cap of the fast history's length, 1..64)\n", argv[2]);
        else std::fprintf(stderr, "gsp_render: bad antilag radius '%s' (expected the half-width of the window, 1..3)\n", argv[2]);
        return 2;
      }
      (fast ? antilag.fast_history : antilag.radius) = (uint32_t)v;
      antilagOptions = true, used = 2;
    } else if (flag == "--antilag-sigma" && argc > 2) {
      if (!parseFloat(argv[2], antilag.sigma_scale) || !(antilag.sigma_scale > 0.0f) || !std::isfinite(antilag.sigma_scale)) {
        std::fprintf(stderr, "gsp_render: bad antilag sigma '%s' (expected the half-width of the box in standard deviations, > 0)\n", argv[2]);
        return 2;
      }
      antilagOptions = true, used = 2;
    } else if (flag == "--taa" && argc > 2) taaPath = argv[2], used = 2;
    else if (flag == "--taa-alpha" && argc > 2) {
      if (!parseFloat(argv[2], taa.alpha) || !(taa.alpha > 0.0f) || !(taa.alpha <= 1.0f)) {
        std::fprintf(stderr, "gsp_render: bad taa alpha '%s' (expected the weight of the new frame, within (0, 1])\n", argv[2]);
        return 2;
      }
      taaOptions = true, used = 2;
    } else if (flag == "--taa-sigma" && argc > 2) {
      if (!parseFloat(argv[2], taa.sigma_clip) || !(taa.sigma_clip > 0.0f)) {
        std::fprintf(stderr, "gsp_render: bad taa sigma '%s' (expected the half-width of the neighbourhood box in standard deviations, > 0)\n", argv[2]);
        return 2;
      }
      taaOptions = true, used = 2;
    } else if (flag == "--svgf" && argc > 2) svgfPath = argv[2], used = 2;
    else if (flag == "--svgf-sigma" && argc > 2) {
      if (std::string(argv[2]) == "inf") svgf.sigma_variance = INFINITY;
      else if (!parseFloat(argv[2], svgf.sigma_variance) || !(svgf.sigma_variance > 0.0f)) {
        std::fprintf(stderr, "gsp_render: bad svgf sigma '%s' (expected a value > 0, or inf = the variance term off)\n", argv[2]);
        return 2;
      }
      svgfOptions = true, used = 2;
    } else if (flag == "--svgf-min-history" && argc > 2) {
      char* e = nullptr;
      const long v = std::strtol(argv[2], &e, 10);
      if (e == argv[2] || *e != 0 || v < 2 || v > 65536) {
        std::fprintf(stderr, "gsp_render: bad svgf min history '%s' (expected 2..65536)\n", argv[2]);
        return 2;
      }
      svgf.min_history = (uint32_t)v, svgfOptions = true, used = 2;
    }
    else if (flag == "--denoise-iterations" && argc > 2) {
      char* e = nullptr;
      const long v = std::strtol(argv[2], &e, 10);
      if (e == argv[2] || *e != 0 || v < 1 || v > 8) {
        std::fprintf(stderr, "gsp_render: bad denoise iterations '%s' (expected 1..8)\n", argv[2]);
        return 2;
      }
      denoise.iterations = (uint32_t)v, denoiseOptions = true, used = 2;
    } else if (flag == "--denoise-sigma" && argc > 2) {
      float* const dst[4] = {&denoise.sigma_color, &denoise.sigma_normal, &denoise.sigma_depth, &denoise.sigma_albedo};
      std::string v = argv[2];
      bool ok = true;
      for (int k = 0; k < 4 && ok; ++k) {
        const size_t comma = v.find(',');
        ok = (comma == std::string::npos) == (k == 3);
        const std::string part = v.substr(0, comma);
        if (ok && part == "inf") *dst[k] = INFINITY;
        else ok = ok && parseFloat(part.c_str(), *dst[k]) && *dst[k] >= 0.0f;
        v = comma == std::string::npos ? "" : v.substr(comma + 1);
      }
      if (!ok) {
        std::fprintf(stderr, "gsp_render: bad denoise sigma '%s' (expected c,n,z,a: four values >= 0, 0 = the default, inf = off)\n", argv[2]);
        return 2;
      }
      denoiseOptions = true, used = 2;
    }
    else if (flag == "--tonemap" && argc > 2) {
      const std::string v = argv[2];
      const size_t c1 = v.find(':'), c2 = c1 == std::string::npos ? c1 : v.find(':', c1 + 1);
      const std::string name = v.substr(0, c1);
      bool ok = true;
      if (name == "clamp") tonemap = (int)GSP_TONEMAP_CLAMP;
      else if (name == "aces") tonemap = (int)GSP_TONEMAP_ACES;
      else if (name == "reinhard") tonemap = (int)GSP_TONEMAP_REINHARD;
      else ok = false;
      if (ok && c1 != std::string::npos) {
        ok = name == "reinhard" && parseFloat(v.substr(c1 + 1, c2 == std::string::npos ? c2 : c2 - c1 - 1).c_str(), tmKey) && tmKey > 0.0f && tmKey <= 1.0f;
        if (ok && c2 != std::string::npos) ok = parseFloat(v.c_str() + c2 + 1, tmBurn) && tmBurn >= 0.0f && tmBurn <= 1.0f;
      }
      if (!ok) {
        std::fprintf(stderr, "gsp_render: bad tonemap '%s' (expected clamp, aces or reinhard[:key[:burn]], key in (0,1], burn in [0,1])\n", argv[2]);
        return 2;
      }
      used = 2;
    } else if (flag == "--exposure" && argc > 2) {
      if (!parseFloat(argv[2], exposure) || exposure < -64.0f || exposure > 64.0f) {
        std::fprintf(stderr, "gsp_render: bad exposure '%s' (expected f-stops within -64 .. 64)\n", argv[2]);
        return 2;
      }
      haveExposure = true;
      used = 2;
    } else if (flag == "--gamma" && argc > 2) {
      if (std::string(argv[2]) == "srgb") gamma = 0.0f;
      else if (!parseFloat(argv[2], gamma) || !(gamma > 0.0f)) {
        std::fprintf(stderr, "gsp_render: bad gamma '%s' (expected a value > 0, or srgb)\n", argv[2]);
        return 2;
      }
      used = 2;
    }
    else if (flag == "--aperture" && argc > 2) {
      if (!parseFloat(argv[2], aperture) || aperture < 0.0f) {
        std::fprintf(stderr, "gsp_render: bad aperture '%s' (expected a radius >= 0)\n", argv[2]);
        return 2;
      }
      used = 2;
    } else if (flag == "--focus-distance" && argc > 2) {
      if (!parseFloat(argv[2], focusDistance) || !(focusDistance > 0.0f)) {
        std::fprintf(stderr, "gsp_render: bad focus distance '%s' (expected a distance > 0)\n", argv[2]);
        return 2;
      }
      used = 2;
    } else if (flag == "--focus-pixel" && argc > 2) {
      const std::string v = argv[2];
      const size_t comma = v.find(',');
      if (comma == std::string::npos || !parseFloat(v.substr(0, comma).c_str(), focusX) || !parseFloat(v.c_str() + comma + 1, focusY)) {
        std::fprintf(stderr, "gsp_render: bad focus pixel '%s' (expected X,Y)\n", argv[2]);
        return 2;
      }
      focusPixel = true;
      used = 2;
    } else if (flag == "--blades" && argc > 2) {
      const std::string v = argv[2];
      const size_t colon = v.find(':');
      char* e = nullptr;
      const std::string nstr = v.substr(0, colon);
      const long n = std::strtol(nstr.c_str(), &e, 10);
      float deg = 0.0f;
      if (e == nstr.c_str() || *e != 0 || !(n == 0 || (n >= 3 && n <= 16)) || (colon != std::string::npos && !parseFloat(v.c_str() + colon + 1, deg))) {
        std::fprintf(stderr, "gsp_render: bad blades '%s' (expected 0 or 3..16, optionally :rotation in degrees)\n", argv[2]);
        return 2;
      }
      blades = (int)n;
      bladeRotation = deg * 3.14159265358979323846f / 180.0f;
      used = 2;
    }
    else if (flag == "--filter" && argc > 2) {
      const std::string v = argv[2];
      const size_t colon = v.find(':');
      const std::string name = v.substr(0, colon);
      filterParam = 0.0f;
      if (name == "none") filter = GSP_FILTER_NONE;
      else if (name == "box") filter = GSP_FILTER_BOX;
      else if (name == "tent") filter = GSP_FILTER_TENT;
      else if (name == "gaussian") filter = GSP_FILTER_GAUSSIAN;
      else {
        std::fprintf(stderr, "gsp_render: bad filter '%s' (expected none, box, tent[:radius] or gaussian[:stddev])\n", argv[2]);
        return 2;
      }
      if (colon != std::string::npos) {
        char* e = nullptr;
        filterParam = std::strtof(v.c_str() + colon + 1, &e);
        if (e == v.c_str() + colon + 1 || *e != 0 || !(filterParam >= 0.0f) || filter == GSP_FILTER_NONE || filter == GSP_FILTER_BOX) {
          std::fprintf(stderr, "gsp_render: bad filter '%s' (expected none, box, tent[:radius] or gaussian[:stddev])\n", argv[2]);
          return 2;
        }
      }
      used = 2;
    } else {
      std::fprintf(stderr, "gsp_render: unknown option '%s'\n", argv[1]);
      return 2;
    }
    argc -= used;
    argv += used;
  }
  if (aperture > 0.0f && !(focusDistance > 0.0f) && !focusPixel && !options.readLens) {
    std::fprintf(stderr, "gsp_render: --aperture needs --focus-distance D, --focus-pixel X,Y or --scene-lens\n");
    return 2;
  }
  if (ldrPath.empty() && taaPath.empty() && (tonemap >= 0 || haveExposure || gamma >= 0.0f || options.readFilm)) {
    std::fprintf(stderr, "gsp_render: --tonemap, --exposure, --gamma and --scene-film need --ldr out.png\n");
    return 2;
  }
  if (featuresPrefix.empty() && featureSpp >= 0) {
    std::fprintf(stderr, "gsp_render: --feature-spp needs --features PREFIX\n");
    return 2;
  }
  if (denoisePath.empty() && denoiseOptions) {
    std::fprintf(stderr, "gsp_render: --denoise-iterations and --denoise-sigma need --denoise out.pfm\n");
    return 2;
  }
  if (temporalPath.empty() && temporalOptions) {
    std::fprintf(stderr, "gsp_render: --temporal-frames and --temporal-orbit need --temporal out.pfm\n");
    return 2;
  }
  if (!temporalPath.empty() && temporalFrames == 0) {
    std::fprintf(stderr, "gsp_render: --temporal needs --temporal-frames N\n");
    return 2;
  }
  if (temporalPath.empty() && temporalFollow) {
    std::fprintf(stderr, "gsp_render: --temporal-follow needs --temporal out.pfm\n");
    return 2;
  }
  if (!temporalFollow && (temporalMove || !motionPath.empty())) {
    std::fprintf(stderr, "gsp_render: --temporal-move and --motion need --temporal-follow\n");
    return 2;
  }
  if (temporalPath.empty() && temporalDemodulate) {
    std::fprintf(stderr, "gsp_render: --temporal-demodulate needs --temporal out.pfm\n");
    return 2;
  }
  if (temporalPath.empty() && temporalAntilag) {
    std::fprintf(stderr, "gsp_render: --temporal-antilag needs --temporal out.pfm\n");
    return 2;
  }
  if (!temporalAntilag && antilagOptions) {
    std::fprintf(stderr, "gsp_render: --antilag-fast, --antilag-radius and --antilag-sigma need --temporal-antilag\n");
    return 2;
  }
  if (taaPath.empty() && taaOptions) {
    std::fprintf(stderr, "gsp_render: --taa-alpha and --taa-sigma need --taa out.png\n");
    return 2;
  }
  if (!taaPath.empty() && (temporalPath.empty() || !temporalFollow)) {
    std::fprintf(stderr, "gsp_render: --taa needs --temporal out.pfm and --temporal-follow (it fetches its history through the motion plane)\n");
    return 2;
  }
  if (svgfPath.empty() && svgfOptions) {
    std::fprintf(stderr, "gsp_render: --svgf-sigma and --svgf-min-history need --svgf out.pfm\n");
    return 2;
  }
  if (!svgfPath.empty() && temporalPath.empty()) {
    std::fprintf(stderr, "gsp_render: --svgf needs --temporal out.pfm (it filters the history)\n");
    return 2;
  }
  if (argc < 3) {
    std::fprintf(stderr, "usage: gsp_render [--dormant-features] [--builtin-shapes] [--no-nee] [--light-sampling uniform|power] [--estimator reference|textbook] [--memory-share F] [--pool-paths N] [--adaptive T [--adaptive-min N] [--adaptive-step N]] [--filter none|box|tent[:r]|gaussian[:s]] [--scene-filter] [--aperture R] [--focus-distance D] [--focus-pixel X,Y] [--blades N[:rot_deg]] [--scene-lens] [--scene-media] [--scene-scattering] [--scene-emitters] [--point-light X,Y,Z,R,G,B]... [--env-sampling [--env-extent R]] [--light-grid [NX,NY,NZ]] [--features PREFIX [--feature-spp N]] [--denoise out.pfm [--denoise-iterations N] [--denoise-sigma c,n,z,a]] [--temporal out.pfm --temporal-frames N [--temporal-orbit DEG]] [--temporal-follow [--temporal-move INST,DX,DY,DZ] [--motion out.pfm]] [--svgf out.pfm [--svgf-sigma S] [--svgf-min-history N]] [--temporal-demodulate] [--svgf-feedback LEVELS] [--temporal-antilag [--antilag-fast N] [--antilag-radius R] [--antilag-sigma S]] [--taa out.png [--taa-alpha A] [--taa-sigma S]] [--ldr out.png [--tonemap clamp|aces|reinhard[:key[:burn]]] [--exposure E] [--gamma G|srgb] [--scene-film]] scene.xml out.pfm [width height spp [device | d0,d1,...]]\n");
    return 2;
  }
  const uint32_t width = argc > 3 ? (uint32_t)std::atoi(argv[3]) : 500;  // S/main.cpp:17: 500x500 window
  const uint32_t height = argc > 4 ? (uint32_t)std::atoi(argv[4]) : 500;
  const uint32_t spp = argc > 5 ? (uint32_t)std::atoi(argv[5]) : 64;
  // device list: decimal indices separated by single commas ("0", "0,1,2,3"; a repeated index = several shares on one
  // GPU); anything else is a usage error, not "device 0"
  std::vector<int> devices;
  {
    const char* p = argc > 6 ? argv[6] : "0";
    bool ok = *p != 0;
    while (ok) {
      if (*p < '0' || *p > '9') {
        ok = false;
        break;
      }
      char* e;
      const long v = std::strtol(p, &e, 10);
      if (e == p || v < 0 || v > 1023) {
        ok = false;
        break;
      }
      devices.push_back((int)v);
      if (*e == 0) break;
      if (*e != ',') ok = false;
      p = e + 1;
    }
    if (!ok || devices.empty()) {
      std::fprintf(stderr, "gsp_render: bad device list '%s' (expected e.g. 0 or 0,1,2,3)\n", argc > 6 ? argv[6] : "");
      return 2;
    }
  }
  if (!temporalPath.empty() && devices.size() > 1) {
    std::fprintf(stderr, "gsp_render: --temporal needs a single device (temporal accumulation has no multi-GPU variant)\n");
    return 2;
  }
  try {
    if (svgfFeedback && svgfPath.empty()) throw std::runtime_error("--svgf-feedback needs --svgf out.pfm (it feeds the filter's first levels back into the history)");
    if (envSampling) {
      if (estimatorGiven && estimator == GSP_ESTIMATOR_REFERENCE)
        throw std::runtime_error("--env-sampling needs the textbook estimator: drop --estimator reference (the option implies --estimator textbook)");
      estimator = GSP_ESTIMATOR_TEXTBOOK;
      options.sampleEnvmap = true;
    } else if (envExtent > 0.0f) {
      throw std::runtime_error("--env-extent needs --env-sampling");
    }
    Scene scene = loadScene(argv[1], "", options);
    for (auto& w : scene.warnings) std::fprintf(stderr, "WARN: %s\n", w.c_str());
    scene.deltaLights.insert(scene.deltaLights.end(), pointLights.begin(), pointLights.end());
    if (envSampling && envExtent > 0.0f) scene.envmapSampling.extent = envExtent;  // (LoadOptions::sampleEnvmap has set the switch and the bounds' radius)
    // thin lens: the scene's (--scene-lens), overridden flag by flag
    if (aperture >= 0.0f || focusDistance > 0.0f || blades >= 0 || focusPixel) {
      float fd = focusDistance > 0.0f ? focusDistance : scene.camera.getFocusDistance();
      if (focusPixel) {  // autofocus on one GPU, before the renderer proper is set up
        PathTracer af(width, height, devices[0], {}, &ctxOptions);
        fd = af.focusDistance(scene, focusX, focusY);
        if (!(fd > 0.0f)) throw std::runtime_error("--focus-pixel: the ray through that pixel hits nothing");
        std::printf("focus distance %g (pixel %g,%g)\n", fd, focusX, focusY);
      }
      scene.camera.setLens(aperture >= 0.0f ? aperture : scene.camera.getApertureRadius(), fd,
                           blades >= 0 ? (uint32_t)blades : scene.camera.getApertureBlades(),
                           blades >= 0 ? bladeRotation : scene.camera.getApertureRotation());
    }
    // LDR film: the scene's (--scene-film), overridden flag by flag
    gsp_display display = scene.film.display();
    if (tonemap >= 0) display.tonemap = (uint32_t)tonemap;
    if (tmKey > 0.0f) display.key = tmKey;
    if (tmBurn >= 0.0f) display.burn = tmBurn;
    if (haveExposure) display.exposure = exposure;
    if (gamma >= 0.0f) display.gamma = gamma;
    if (!denoisePath.empty() && !ldrPath.empty() && devices.size() > 1)
      throw std::runtime_error("--denoise with --ldr needs a single device (the LDR film of the denoised frame is a single-context call)");
    std::vector<uint32_t> ldr, denoisedLdr, taaLdr;
    double taaUsed = 0.0;
    std::vector<float> img, featAlbedo, featGeom, denoised, temporal, temporalDenoised, temporalSvgf, motion;
    double temporalLength = 0.0;
    double fastLength = 0.0;
    const uint32_t fspp = featureSpp > 0 ? (uint32_t)featureSpp : spp;
    gsp_stats st;
    double s;
    if (devices.size() == 1) {
      PathTracer pt(width, height, devices[0], {}, &ctxOptions);
      pt.params.disable_nee = nee ? 0u : 1u;
      pt.setLightSampling(lightSampling);
      pt.setEstimator(estimator);
      if (lightGrid) {
        try {
          pt.setLightGrid(true, lightGridRes[0], lightGridRes[1], lightGridRes[2]);
        } catch (const std::exception& e) {  // (a missing prerequisite, a resolution out of range: the library's own words)
          std::fprintf(stderr, "gsp_render: --light-grid: %s\n", e.what());
          return 2;
        }
      }
      pt.params.adaptive_threshold = adaptive;
      pt.params.adaptive_min_spp = adaptiveMin;
      pt.params.adaptive_step = adaptiveStep;
      pt.params.pixel_filter = filter;
      pt.params.pixel_filter_param = filterParam;
      if (!svgfPath.empty()) pt.temporalTrackMoments(true);  // (before the first accumulate: moments and history of one age)
      if (temporalFollow) pt.temporalFollowInstances(true);
      if (temporalDemodulate) pt.temporalDemodulate(true);
      if (temporalMove && (size_t)temporalMoveInst >= scene.renderObjects.size())
        throw std::runtime_error("--temporal-move: the scene has " + std::to_string(scene.renderObjects.size()) + " render objects, there is no object " +
                                 std::to_string(temporalMoveInst));
      // temporal accumulation: the frames before the last one, each rendered, given a feature pass and accumulated, then the
      // camera turned about the world y axis; the last frame is the ordinary frame below
      for (int f = 0; f + 1 < temporalFrames; ++f) {
        pt.render(scene, spp);
        pt.renderFeatures(scene, spp);
        pt.temporalAccumulate();
        if (temporalAntilag) pt.temporalAntilag(&antilag);
        std::vector<float> filtered;  // (the source of --taa: the filter's output where --svgf is given)
        if (svgfFeedback) filtered = pt.temporalSvgfFeedback(&denoise, &svgf, (uint32_t)svgfFeedback, !taaPath.empty());
        if (!taaPath.empty()) {
          if (!svgfPath.empty() && !svgfFeedback) filtered = pt.downloadTemporalSvgf(&denoise, &svgf);
          pt.temporalTaa(&taa, &display, svgfPath.empty() ? nullptr : filtered.data(), filtered.size());
        }
        const float a = temporalOrbit * 3.14159265358979323846f / 180.0f, cs = std::cos(a), sn = std::sin(a);
        const mat4 m = scene.camera.getToWorld();
        mat4 r = m;
        for (int c = 0; c < 4; ++c) {  // R_y(a) * m, column by column
          r[c][0] = cs * m[c][0] + sn * m[c][2];
          r[c][2] = -sn * m[c][0] + cs * m[c][2];
        }
        scene.camera.setToWorld(r);
        if (temporalMove)  // (the next frame's render uploads the edit: before its feature pass, as following asks)
          for (int k = 0; k < 3; ++k) scene.renderObjects[(size_t)temporalMoveInst].transform[3][k] += temporalMoveBy[k];
        pt.nextFrame();
      }
      auto t0 = std::chrono::steady_clock::now();
      pt.render(scene, spp);
      img = pt.download();
      s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      st = pt.stats();
      if (!ldrPath.empty()) {
        pt.display = display;
        ldr = pt.downloadDisplay();
      }
      if (!featuresPrefix.empty()) {  // after the timed frame: the feature planes (gpuspectral_pt.h "Feature buffers")
        pt.renderFeatures(scene, fspp);
        pt.downloadFeatures(&featAlbedo, &featGeom, nullptr);
      }
      if (!denoisePath.empty()) {  // the denoiser (gpuspectral_pt.h "Denoiser"), on the planes above or on a pass of its own
        if (featuresPrefix.empty()) pt.renderFeatures(scene, spp);
        denoised = pt.downloadDenoised(&denoise);
        if (!ldrPath.empty()) denoisedLdr = pt.downloadDenoisedDisplay(&denoise);
      }
      if (!temporalPath.empty()) {  // the last frame into the history, on the planes above or on a pass of its own
        if (featuresPrefix.empty() && denoisePath.empty()) pt.renderFeatures(scene, spp);
        pt.temporalAccumulate();
        if (temporalAntilag) {  // (before the feedback: the filter starts from the clamped history)
          pt.temporalAntilag(&antilag);
          const std::vector<float> fast = pt.downloadTemporalFast();
          for (size_t i = 3; i < fast.size(); i += 4) fastLength += fast[i];
          fastLength /= (double)width * height;
        }
        if (svgfFeedback) temporalSvgf = pt.temporalSvgfFeedback(&denoise, &svgf, (uint32_t)svgfFeedback);  // (first: the files below show the fed-back history)
        temporal = temporalDemodulate ? pt.downloadTemporalImage() : pt.downloadTemporal();
        if (!denoisePath.empty()) temporalDenoised = pt.downloadTemporalDenoised(&denoise);
        if (!svgfPath.empty() && !svgfFeedback) temporalSvgf = pt.downloadTemporalSvgf(&denoise, &svgf);
        if (!motionPath.empty()) motion = pt.downloadTemporalMotion();
        if (!taaPath.empty()) {  // (last: the filter's output is its source)
          pt.temporalTaa(&taa, &display, svgfPath.empty() ? nullptr : temporalSvgf.data(), temporalSvgf.size());
          taaLdr = pt.downloadTaaDisplay();
          const std::vector<float> d = pt.downloadTaa();
          for (size_t i = 3; i < d.size(); i += 4) taaUsed += d[i];
          taaUsed /= (double)width * height;
        }
        for (size_t i = 3; i < temporal.size(); i += 4) temporalLength += temporal[i];
        temporalLength /= (double)width * height;
      }
    } else {
      MultiGpuPathTracer pt(width, height, devices, &ctxOptions);
      pt.params.disable_nee = nee ? 0u : 1u;
      pt.setLightSampling(lightSampling);
      pt.setEstimator(estimator);
      if (lightGrid) {
        try {
          pt.setLightGrid(true, lightGridRes[0], lightGridRes[1], lightGridRes[2]);
        } catch (const std::exception& e) {  // (a missing prerequisite, a resolution out of range: the library's own words)
          std::fprintf(stderr, "gsp_render: --light-grid: %s\n", e.what());
          return 2;
        }
      }
      pt.params.adaptive_threshold = adaptive;  // (gsp_multi_render refuses adaptive sampling: reported as an error)
      pt.params.pixel_filter = filter;
      pt.params.pixel_filter_param = filterParam;
      auto t0 = std::chrono::steady_clock::now();
      pt.render(scene, spp);
      img = pt.download();
      s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      st = pt.stats();
      if (!ldrPath.empty()) {
        pt.display = display;
        ldr = pt.downloadDisplay();
      }
      if (!featuresPrefix.empty()) {  // after the timed frame: the feature planes (gpuspectral_pt.h "Feature buffers")
        pt.renderFeatures(scene, fspp);
        pt.downloadFeatures(&featAlbedo, &featGeom, nullptr);
      }
      if (!denoisePath.empty()) {
        if (featuresPrefix.empty()) pt.renderFeatures(scene, spp);
        denoised = pt.downloadDenoised(&denoise);
      }
      std::printf("%zu shares (32x32 tiles), gathered on device %d\n", devices.size(), devices[0]);
    }
    writePfm(argv[2], img.data(), width, height);
    writePpm(std::string(argv[2]) + ".ppm", img.data(), width, height, false);  // LDR preview, gamma 2.2
    if (!ldrPath.empty()) writePng(ldrPath, ldr.data(), width, height, false);
    if (!featuresPrefix.empty()) {
      // albedo and normal as RGB PFM + an 8-bit PNG (the normal mapped as 0.5 + 0.5 n), the depth as a PFM with t in every channel
      const size_t n = (size_t)width * height;
      std::vector<float> depth(4 * n);
      std::vector<uint32_t> a8(n), n8(n);
      auto byte = [](float v) { return (uint32_t)(std::min(std::max(v, 0.0f), 1.0f) * 255.0f + 0.5f); };
      for (size_t i = 0; i < n; ++i) {
        depth[4 * i] = depth[4 * i + 1] = depth[4 * i + 2] = featGeom[4 * i + 3];
        depth[4 * i + 3] = 1.0f;
        a8[i] = byte(featAlbedo[4 * i]) | (byte(featAlbedo[4 * i + 1]) << 8) | (byte(featAlbedo[4 * i + 2]) << 16) | 0xff000000u;
        n8[i] = byte(0.5f + 0.5f * featGeom[4 * i]) | (byte(0.5f + 0.5f * featGeom[4 * i + 1]) << 8) | (byte(0.5f + 0.5f * featGeom[4 * i + 2]) << 16) | 0xff000000u;
      }
      writePfm(featuresPrefix + ".albedo.pfm", featAlbedo.data(), width, height);
      writePfm(featuresPrefix + ".normal.pfm", featGeom.data(), width, height);
      writePfm(featuresPrefix + ".depth.pfm", depth.data(), width, height);
      writePng(featuresPrefix + ".albedo.png", a8.data(), width, height, false);
      writePng(featuresPrefix + ".normal.png", n8.data(), width, height, false);
      std::printf("features: %u samples per pixel -> %s.{albedo,normal,depth}.pfm, %s.{albedo,normal}.png\n", fspp, featuresPrefix.c_str(), featuresPrefix.c_str());
    }
    if (!denoisePath.empty()) {
      writePfm(denoisePath, denoised.data(), width, height);
      std::string png;
      if (!denoisedLdr.empty()) {
        const size_t dot = denoisePath.rfind('.');
        png = (dot != std::string::npos && denoisePath.find('/', dot) == std::string::npos ? denoisePath.substr(0, dot) : denoisePath) + ".png";
        writePng(png, denoisedLdr.data(), width, height, false);
      }
      std::printf("denoised: %u levels -> %s%s%s\n", denoise.iterations ? denoise.iterations : 5u, denoisePath.c_str(), png.empty() ? "" : ", ", png.c_str());
    }
    if (!temporalPath.empty()) {
      writePfm(temporalPath, temporal.data(), width, height);
      std::string dn;
      if (!temporalDenoised.empty()) {
        const size_t dot = temporalPath.rfind('.');
        dn = (dot != std::string::npos && temporalPath.find('/', dot) == std::string::npos ? temporalPath.substr(0, dot) : temporalPath) + ".dn.pfm";
        writePfm(dn, temporalDenoised.data(), width, height);
      }
      std::printf("temporal: %d frame%s of %u spp, %g degrees per frame, mean history length %.2f -> %s%s%s\n", temporalFrames, temporalFrames == 1 ? "" : "s",
                  spp, (double)temporalOrbit, temporalLength, temporalPath.c_str(), dn.empty() ? "" : ", ", dn.c_str());
      if (temporalDemodulate) std::printf("temporal: the history holds illumination (colour / albedo); %s is its image read-out\n", temporalPath.c_str());
      if (temporalAntilag)
        std::printf("temporal antilag: the history clamped into the box of the fast history on each of %d frame%s, mean fast history length %.2f\n", temporalFrames,
                    temporalFrames == 1 ? "" : "s", fastLength);
      if (svgfFeedback)
        std::printf("svgf feedback: the first %ld level%s fed back into the history on each of %d frame%s\n", svgfFeedback, svgfFeedback == 1 ? "" : "s",
                    temporalFrames, temporalFrames == 1 ? "" : "s");
      if (!taaPath.empty()) {
        writePng(taaPath, taaLdr.data(), width, height, false);
        std::printf("taa: %s resolved over its history on each of %d frame%s, alpha %g, sigma %g, %.1f %% of the last frame's pixels blended -> %s\n",
                    svgfPath.empty() ? "the image of the history" : "the filter's output", temporalFrames, temporalFrames == 1 ? "" : "s",
                    taa.alpha != 0.0f ? (double)taa.alpha : 0.1, taa.sigma_clip != 0.0f ? (double)taa.sigma_clip : 1.0, 100.0 * taaUsed, taaPath.c_str());
      }
      if (!motionPath.empty()) {
        size_t followed = 0;
        for (size_t i = 3; i < motion.size(); i += 4) {
          followed += motion[i] == 2.0f;
          motion[i - 1] = motion[i];  // (a PFM holds three channels: dx, dy and the class)
        }
        writePfm(motionPath, motion.data(), width, height);
        std::printf("motion: %zu followed pixels -> %s\n", followed, motionPath.c_str());
      }
      if (!svgfPath.empty()) {
        writePfm(svgfPath, temporalSvgf.data(), width, height);
        if (std::isinf(svgf.sigma_variance)) std::printf("svgf: %u levels, the variance term off -> %s\n", denoise.iterations ? denoise.iterations : 5u, svgfPath.c_str());
        else
          std::printf("svgf: %u levels, sigma_variance %g, min history %u -> %s\n", denoise.iterations ? denoise.iterations : 5u,
                      svgf.sigma_variance != 0.0f ? (double)svgf.sigma_variance : 4.0, svgf.min_history ? svgf.min_history : 4u, svgfPath.c_str());
      }
    }
    std::printf("%llu triangles, %ux%u x %u spp in %.3f s: %.1f Mrays/s, %.2f Msamples/s (BVH build %.1f ms)\n",
                (unsigned long long)st.num_triangles, width, height, spp, s,
                (st.extension_rays + st.shadow_rays) / s / 1e6, st.samples / s / 1e6, st.bvh_build_ms);
    if (adaptive > 0.0f)
      std::printf("adaptive %g: %llu samples taken (%.2f per pixel of at most %u), %llu pixels still active, %llu rounds\n", adaptive,
                  (unsigned long long)st.samples, (double)st.samples / ((double)width * height), spp,
                  (unsigned long long)st.adaptive_active_pixels, (unsigned long long)st.adaptive_rounds);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
