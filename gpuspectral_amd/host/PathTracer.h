// PathTracer.h -- host half of the path-tracing pass, the drop-in for the reference's
// `class PathTracer : public RenderPassCreator` (S/renderer/PathTracer.h:48-68,
// S/renderer/Renderer.h:22-25).
//
// Same two-phase shape as the reference:
//   construction  = setup(): allocate the frame-sized RGBA32F accumulate buffer
//                   (PathTracer.cpp:5-7)
//   createRenderPass(scene) = one call per presented frame: prepareScene + traceRays
//                   -> ONE more sample per pixel folded into the running mean, with the
//                   internal `timestamp` counter advanced (PathTracer.cpp:9-56,91-92)
// plus `render(scene, spp)` for offline use.  Instead of recording Vulkan passes into a
// FrameGraph it drives the HIP wavefront tracer through the C ABI
// (include/gpuspectral_pt.h).  Errors are C++ exceptions (std::runtime_error), as in the
// reference.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "Scene.h"

namespace GPUSpectral {

// What a pass last handed to the device, BY VALUE.  The reference's createRenderPass(fg, scene) re-reads the camera, every
// object's transform and material, the eight BSDF tables and the lights on every call and keeps only the BLAS of a mesh,
// cached by mesh id (S/renderer/PathTracer.cpp:10-19,58-93; Renderer.cpp:122-131).  Its Scene is a plain struct with
// public vectors, so no mutator could keep a revision counter honest; the tracker therefore compares VALUES each frame
// (~100 B per object + the tables: microseconds) and answers with the cheapest C-ABI call that brings the device up to
// date.  Mesh identity is the MeshPtr itself, HELD here: while the tracker holds it no other Mesh can be constructed at
// that address, so a different scene built in the same stack slot can never be mistaken for the uploaded one.
struct SceneTracker {
  enum Change : unsigned { None = 0, CameraChanged = 1, TablesChanged = 2, InstancesChanged = 4, Everything = 8, LensChanged = 16 };
  // what differs between `scene` and the snapshot (Everything: other meshes / object list / textures: a full upload)
  unsigned diff(const Scene& scene, std::vector<gsp_instance>& instances) const;
  void remember(const Scene& scene, const std::vector<gsp_instance>& instances);
  void forget() { valid = false; meshes.clear(); }
  // the camera's thin lens (Camera::setLens) against the one last sent; context state of its own (gsp_set_lens), so it is
  // tracked beside the snapshot: a full upload does not resend it, a changed value does
  bool lensChanged(const Scene& scene, gsp_lens& out) const;
  void rememberLens(const gsp_lens& l) { lens = l; }
  // the scene's interior media (Scene::media) against the table last sent; context state of its own too (gsp_set_media)
  bool mediaChanged(const Scene& scene) const;
  // ... and its delta lights (Scene::deltaLights) against the table last sent (gsp_set_delta_lights)
  bool deltaLightsChanged(const Scene& scene) const;
  void rememberDeltaLights(const Scene& scene) { deltaLights = scene.deltaLights; }
  // ... and its environment-light switch (Scene::envmapSampling) against the one last sent (gsp_set_envmap_sampling)
  bool envmapSamplingChanged(const Scene& scene) const;
  void rememberEnvmapSampling(const Scene& scene) { envmapSampling = scene.envmapSampling; }
  void rememberMedia(const Scene& scene) {
    media = scene.media;
    mediaScattering = scene.mediaScattering;
  }

 private:
  bool valid = false;
  std::vector<MeshPtr> meshes;          // per render object
  std::vector<gsp_instance> instances;  // transform, emission, bsdf, twofaced, vertex range per object
  std::vector<unsigned char> tables;    // counts + the eight BSDF arrays + the lights, back to back
  gsp_camera camera{};
  gsp_lens lens{};                      // (zeroed = pinhole = a fresh context's state)
  std::vector<gsp_medium> media;        // (empty = none = a fresh context's state)
  std::vector<gsp_medium_scatter> mediaScattering;  // ... and the scattering table parallel to it (gsp_set_media_scattering)
  std::vector<gsp_delta_light> deltaLights;         // (empty = none = a fresh context's state)
  gsp_envmap_sampling envmapSampling{};             // (zeroed = off = a fresh context's state)
  std::vector<uint64_t> assets;         // dormant features: texture / environment-map sizes, flags, envmap transform
};

// The plugin interface of the reference (Renderer.h:22-25) without the Vulkan FrameGraph.
class RenderPassCreator {
 public:
  virtual ~RenderPassCreator() = default;
  virtual void createRenderPass(const Scene& scene) = 0;
};

class PathTracer : public RenderPassCreator {
 public:
  // `pixelIds` optionally restricts this tracer to a subset of the frame (multi-GPU tiles).
  // `options` (optional): per-context resources, gsp_ctx_options of include/gpuspectral_pt.h (path-pool size, memory share, ...)
  PathTracer(uint32_t width, uint32_t height, int device = 0, const std::vector<uint32_t>& pixelIds = {},
             const gsp_ctx_options* options = nullptr);
  ~PathTracer() override;
  PathTracer(const PathTracer&) = delete;
  PathTracer& operator=(const PathTracer&) = delete;

  void setup();
  void createRenderPass(const Scene& scene) override;  // +1 spp
  void render(const Scene& scene, uint32_t spp);       // +spp samples
  // Brings the device up to date with `scene` as it is NOW (the reference re-reads it every frame): nothing when nothing
  // changed, gsp_update_camera / _tables / _instances for edits, a full flatten + upload + BVH build for another object list.
  void prepareScene(const Scene& scene);
  // Autofocus (gsp_focus_distance): brings the device up to date with `scene`, then the camera-space depth of what the pinhole
  // ray through fragCoord (fx, fy) hits, 0 on a miss: the value for Camera::setLens's focus distance
  float focusDistance(const Scene& scene, float fx, float fy);
  // Forget what was uploaded: the next pass uploads everything.  Needed only after texel CONTENTS of a texture or
  // environment map were rewritten in place (dormant features; sizes and flags are tracked, contents are not).
  void invalidateScene() { tracker.forget(); }
  // Light selection (gpuspectral_pt.h "Light selection"): GSP_LIGHTS_UNIFORM (the reference's pick, the default) or GSP_LIGHTS_POWER
  // (by emitted power).  Context state: it holds across scenes; reset() after a change starts a frame of one estimator.
  void setLightSampling(uint32_t mode);
  std::vector<gsp_light_pick> downloadLightPick();  // the resident alias table (GSP_LIGHTS_POWER with a scene uploaded)
  // Estimator (gpuspectral_pt.h "Estimator"): GSP_ESTIMATOR_REFERENCE (the reference's weights, the default) or GSP_ESTIMATOR_TEXTBOOK
  // (textbook multiple importance sampling: unbiased).  Context state: it holds across scenes; reset() after a change.
  void setEstimator(uint32_t mode);
  // Light grid (gpuspectral_pt.h "Light grid"): spatial light selection, one alias table per cell of a grid over the scene.  Needs
  // setLightSampling(GSP_LIGHTS_POWER) and setEstimator(GSP_ESTIMATOR_TEXTBOOK) first (the library's error otherwise).  nx = ny = nz
  // = 0: the library chooses the resolution.  Context state: it holds across scenes; reset() after a change.
  void setLightGrid(bool enabled, uint32_t nx = 0, uint32_t ny = 0, uint32_t nz = 0);

  // RGBA32F, row-major, width*height*4 floats (running mean, alpha 1)
  std::vector<float> download();
  // The frame as it stands without waiting for paths still in flight (what the reference's blit pass shows every
  // frame, PathTracer.cpp:41-55): compact RGBA32F over the owned pixels; *samplesFolded = timestamps in every pixel.
  std::vector<float> peek(uint32_t* samplesFolded = nullptr);
  // ... into caller-owned DEVICE memory (>= owned pixels * 16 bytes): the blit's source without a trip through the host
  void peekToDevice(void* deviceDst, uint64_t bytes, uint32_t* samplesFolded = nullptr);
  // LDR film (gpuspectral_pt.h "LDR film"): the frame tone-mapped and encoded on the GPU with `display`, RGBA8 words (R in bits
  // 0-7).  downloadDisplay: the full frame after every queued sample; peekDisplay: compact, as it stands -- what a viewer
  // presents each frame instead of peek() + a host tone map (4 bytes per pixel over PCIe instead of 16)
  std::vector<uint32_t> downloadDisplay();
  std::vector<uint32_t> peekDisplay(uint32_t* samplesFolded = nullptr);
  void peekDisplayToDevice(void* deviceDst, uint64_t bytes, uint32_t* samplesFolded = nullptr);
  // the frame statistics Reinhard measures (drain = false: the buffer as it stands)
  gsp_luminance frameLuminance(bool drain = true);
  // Feature buffers (gpuspectral_pt.h "Feature buffers"): `spp` feature samples per owned pixel -- the first hit of the beauty
  // samples' camera rays under this tracer's filter and the scene's lens -- from timestamp 0 on the first call of a frame and
  // continuing from there; independent of render() and of getTimestamp().  downloadFeatures: full-frame planes, width*height*4
  // values each ({r, g, b, coverage}, {nx, ny, nz, t}, {triangle, bsdf, instance, samples}); any pointer may be null.
  void renderFeatures(const Scene& scene, uint32_t spp);
  void downloadFeatures(std::vector<float>* albedo, std::vector<float>* geom, std::vector<uint32_t>* ids);
  void copyFeaturesToDevice(void* albedo, void* geom, void* ids, uint64_t bytesEach);  // compact planes, device memory
  // Denoiser (gpuspectral_pt.h "Denoiser"): the frame through the edge-avoiding a-trous filter, guided by the planes of a
  // renderFeatures call of this frame; RGBA32F, width*height*4 floats.  nullptr = every default.  downloadDenoisedDisplay: the LDR
  // film (`display`) of the denoised frame, RGBA8 words.  The frame itself is not changed.
  std::vector<float> downloadDenoised(const gsp_denoise* denoise = nullptr);
  std::vector<uint32_t> downloadDenoisedDisplay(const gsp_denoise* denoise = nullptr);
  // Temporal accumulation (gpuspectral_pt.h "Temporal accumulation"): the viewer loop is nextFrame() -> render -> renderFeatures ->
  // temporalAccumulate -> downloadTemporal / downloadTemporalDenoised.  temporalAccumulate reprojects the history of earlier
  // frames into the scene's current camera and blends this frame in (once per frame; nullptr = every default); downloadTemporal
  // is that history (RGBA32F, .w = the history length), downloadTemporalDenoised its a-trous filter guided by this frame's planes.
  void temporalAccumulate(const gsp_temporal* temporal = nullptr);
  void temporalReset();
  std::vector<float> downloadTemporal();
  std::vector<float> downloadTemporalDenoised(const gsp_denoise* denoise = nullptr);
  // Variance-guided filter (gpuspectral_pt.h "Variance-guided filter"): temporalTrackMoments(true) before the first
  // temporalAccumulate makes the history keep its luminance moments (a change of the value drops the history);
  // downloadTemporalMoments is that plane {m1, m2, r, 0}, downloadTemporalSvgf the a-trous filter of the history whose luminance
  // edge-stop follows the per-pixel variance (RGBA32F, .w = the history length; nullptr = every default).
  void temporalTrackMoments(bool on);
  std::vector<float> downloadTemporalMoments();
  std::vector<float> downloadTemporalSvgf(const gsp_denoise* denoise = nullptr, const gsp_svgf* svgf = nullptr);
  // Moved instances (gpuspectral_pt.h "Temporal accumulation: moved instances"): temporalFollowInstances(true) makes
  // temporalAccumulate take a pixel of an object whose transform changed back through that motion (a change of the value drops the
  // history).  render() uploads an edited transform, so it belongs before the frame's renderFeatures.  downloadTemporalMotion is
  // the motion plane {dx, dy, kept weight, class} of the newest accumulate.
  void temporalFollowInstances(bool on);
  std::vector<float> downloadTemporalMotion();
  // Illumination history (gpuspectral_pt.h "Illumination history"): temporalDemodulate(true) makes the history accumulate colour /
  // first-hit albedo (a change of the value drops the history); downloadTemporalImage / temporalImageToDevice are what a viewer
  // shows of it -- re-modulated by this frame's albedo, or the history itself with demodulation off -- and need this frame's
  // temporalAccumulate.  temporalSvgfFeedback is downloadTemporalSvgf that also writes the output of its first `levels` levels
  // into the history (once per temporalAccumulate; wantOutput = false: nothing is read back, the vector is empty).
  void temporalDemodulate(bool on);
  std::vector<float> downloadTemporalImage();
  void temporalImageToDevice(void* deviceDst, uint64_t bytes);
  std::vector<float> temporalSvgfFeedback(const gsp_denoise* denoise, const gsp_svgf* svgf, uint32_t levels, bool wantOutput = true);
  void temporalSvgfFeedbackToDevice(const gsp_denoise* denoise, const gsp_svgf* svgf, uint32_t levels, void* deviceDst, uint64_t bytes);
  // Temporal anti-lag (gpuspectral_pt.h "Temporal anti-lag"): temporalAntilag keeps a short history beside the long one and clamps
  // the long one into the box of its window statistics, so that a change of the lighting is forgotten in a few frames.  Once per
  // temporalAccumulate, before any temporalSvgfFeedback.  downloadTemporalFast / temporalFastToDevice: the short history.
  void temporalAntilag(const gsp_antilag* antilag = nullptr);
  std::vector<float> downloadTemporalFast();
  void temporalFastToDevice(void* deviceDst, uint64_t bytes);
  // Temporal anti-aliasing (gpuspectral_pt.h "Temporal anti-aliasing"): temporalTaa resolves the tone-mapped frame over its own
  // history -- src = an HDR frame of width*height*4 floats (the output of temporalSvgf / temporalSvgfFeedback, say), nullptr = the
  // image of the newest history (srcFloats: what the caller's buffer holds); displayOverride nullptr = the LDR film `display`.  Once per temporalAccumulate, with
  // temporalFollowInstances on.  downloadTaa: the resolved display-linear frame; downloadTaaDisplay / taaDisplayToDevice: its RGBA8 encode.
  void temporalTaa(const gsp_taa* taa = nullptr, const gsp_display* displayOverride = nullptr, const float* src = nullptr, uint64_t srcFloats = ~0ull);
  void temporalTaaFromDevice(const gsp_taa* taa, const gsp_display* displayOverride, const void* deviceSrc, uint64_t bytes);
  std::vector<float> downloadTaa();
  std::vector<uint32_t> downloadTaaDisplay();
  void taaDisplayToDevice(void* deviceDst, uint64_t bytes);
  void nextFrame();  // a new frame (accumulate buffer and feature planes cleared) whose samples continue the timestamp sequence
  void reset();  // timestamp = 0, accumulate buffer and feature planes cleared
  int getTimestamp() const { return timestamp; }
  gsp_stats stats();
  // reference literals by default (MAX_DEPTH 50, RR > 10, clamp 20).  params.pixel_filter != GSP_FILTER_NONE overrides the
  // filter a scene carries (Scene::pixelFilter, LoadOptions::readFilter); NONE leaves the choice to the scene
  gsp_render_params params;
  gsp_display display{};  // the LDR film of downloadDisplay / peekDisplay; zeroed = clamp + sRGB

 private:
  void check(int rc, const char* what);
  gsp_context* ctx = nullptr;
  uint32_t width, height;
  int device;
  std::vector<uint32_t> pixelIds;
  gsp_ctx_options options{};
  SceneTracker tracker;
  int timestamp{0};
  int featureTimestamp{0};  // feature samples folded since the last reset()
};

// The same pass over several GPUs of one node: the frame is cut into interleaved 32x32 tiles (one share per entry of
// `devices`; an index may repeat), the scene is replicated, every GPU renders all samples of its tiles and download()
// gathers the HDR tiles into the first GPU (device-to-device over xGMI) before the one copy to the host
// (gsp_multi_*, include/gpuspectral_pt.h).  Same two-phase shape and the same image, bit for bit, as
// PathTracer on one GPU.
class MultiGpuPathTracer : public RenderPassCreator {
 public:
  MultiGpuPathTracer(uint32_t width, uint32_t height, const std::vector<int>& devices, const gsp_ctx_options* options = nullptr);
  ~MultiGpuPathTracer() override;
  MultiGpuPathTracer(const MultiGpuPathTracer&) = delete;
  MultiGpuPathTracer& operator=(const MultiGpuPathTracer&) = delete;

  void createRenderPass(const Scene& scene) override;  // +1 spp on every GPU's share
  void render(const Scene& scene, uint32_t spp);
  void prepareScene(const Scene& scene);  // as PathTracer::prepareScene, on every share
  void invalidateScene() { tracker.forget(); }
  void setLightSampling(uint32_t mode);  // as PathTracer::setLightSampling, on every share
  void setEstimator(uint32_t mode);      // as PathTracer::setEstimator, on every share
  void setLightGrid(bool enabled, uint32_t nx = 0, uint32_t ny = 0, uint32_t nz = 0);  // as PathTracer::setLightGrid, on every share
  std::vector<float> download();  // RGBA32F, row-major, width*height*4 floats
  std::vector<uint32_t> downloadDisplay();  // as PathTracer::downloadDisplay, on the gathered frame
  void renderFeatures(const Scene& scene, uint32_t spp);  // as PathTracer::renderFeatures, on every share
  void downloadFeatures(std::vector<float>* albedo, std::vector<float>* geom, std::vector<uint32_t>* ids);  // the gathered planes
  std::vector<float> downloadDenoised(const gsp_denoise* denoise = nullptr);  // as PathTracer::downloadDenoised, on the gathered frame
  void reset();
  int getTimestamp() const { return timestamp; }
  int numShares() const { return (int)devices.size(); }
  gsp_stats stats(std::vector<gsp_stats>* perShare = nullptr);  // totals over the shares
  gsp_render_params params;
  gsp_display display{};

 private:
  void check(int rc, const char* what);
  gsp_multi* multi = nullptr;
  uint32_t width, height;
  std::vector<int> devices;
  SceneTracker tracker;
  int timestamp{0};
  int featureTimestamp{0};
};

// Headless output step: little-endian PFM ("PF", bottom-to-top rows) of the RGB channels.
void writePfm(const std::string& path, const float* rgba, uint32_t width, uint32_t height);

// Display transform of the presentation pass.  The reference blits the accumulate image unchanged
// (S/assets/shaders/DrawTexture.frag:9-13; `RenderParams.toneMap` is never read, S/renderer/
// PathTracer.h:36-41) and keeps the ACES fit as a dormant helper (S/assets/shaders/common.glsl:74-82).
// toneMap = false: clamp + gamma 2.2 (the ldrfilm setting of the shipped scenes); true: ACESFilm, then gamma.
void toneMapToRgb8(const float* rgba, uint32_t width, uint32_t height, bool toneMap, std::vector<uint8_t>& rgb8);
// Binary PPM ("P6") of the tone-mapped image (top-to-bottom rows).
void writePpm(const std::string& path, const float* rgba, uint32_t width, uint32_t height, bool toneMap);

}  // namespace GPUSpectral
