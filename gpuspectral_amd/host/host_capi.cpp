// host_capi.cpp -- C wrappers over the C++ host layer (Scene / loadScene / PathTracer) so
// that the Python tests can drive exactly the classes a C++ caller would use.
#include <cstring>
#include <exception>
#include <stdexcept>
#include <string>

#include "Image.h"
#include "Loader.h"
#include "PathTracer.h"

using namespace GPUSpectral;

namespace {
thread_local std::string g_err;
struct SceneBox {
  Scene scene;
  FlatScene flat;
};
template <class F>
int guard(F&& f) {
  try {
    f();
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return 1;
  }
}
}  // namespace

extern "C" {

const char* gsph_last_error(void) { return g_err.c_str(); }

void* gsph_load_scene(const char* path, const char* asset_dir) {
  SceneBox* b = nullptr;
  int rc = guard([&] {
    b = new SceneBox();
    b->scene = loadScene(path, asset_dir ? asset_dir : "");
    flattenScene(b->scene, b->flat);
  });
  if (rc) {
    delete b;
    return nullptr;
  }
  return b;
}
// dormant != 0: loadScene with LoadOptions{dormantFeatures = true, srgbTextures = srgb != 0}
void* gsph_load_scene_ex(const char* path, const char* asset_dir, int dormant, int srgb) {
  SceneBox* b = nullptr;
  int rc = guard([&] {
    b = new SceneBox();
    LoadOptions opt;
    opt.dormantFeatures = dormant != 0;
    opt.srgbTextures = srgb != 0;
    b->scene = loadScene(path, asset_dir ? asset_dir : "", opt);
    flattenScene(b->scene, b->flat);
  });
  if (rc) {
    delete b;
    return nullptr;
  }
  return b;
}
// flags: 1 = LoadOptions::dormantFeatures, 2 = srgbTextures, 4 = builtinShapes (disk / sphere),
// 8 = readFilter (the film's <rfilter>), 16 = readLens (a thinlens sensor's aperture_radius / focus_distance),
// 32 = readFilm (an ldrfilm's gamma / exposure / tonemapMethod / key / burn), 64 = readMedia (the shapes' interior media),
// 128 = readScattering (their sigmaS / albedo and hg phase; implies 64), 256 = readEmitters (top-level point / spot / directional emitters),
// 512 = sampleEnvmap (the environment-light switch, extent = the radius of the scene's bounds)
void* gsph_load_scene_opts(const char* path, const char* asset_dir, unsigned flags) {
  SceneBox* b = nullptr;
  int rc = guard([&] {
    b = new SceneBox();
    LoadOptions opt;
    opt.dormantFeatures = (flags & 1u) != 0;
    opt.srgbTextures = (flags & 2u) != 0;
    opt.builtinShapes = (flags & 4u) != 0;
    opt.readFilter = (flags & 8u) != 0;
    opt.readLens = (flags & 16u) != 0;
    opt.readFilm = (flags & 32u) != 0;
    opt.readMedia = (flags & 64u) != 0;
    opt.readScattering = (flags & 128u) != 0;
    opt.readEmitters = (flags & 256u) != 0;
    opt.sampleEnvmap = (flags & 512u) != 0;
    b->scene = loadScene(path, asset_dir ? asset_dir : "", opt);
    flattenScene(b->scene, b->flat);
  });
  if (rc) {
    delete b;
    return nullptr;
  }
  return b;
}
void gsph_scene_free(void* s) { delete (SceneBox*)s; }

// Image.h readers.  Two calls: texels == NULL returns the size, the second call fills width * height RGBA8 words
// (floats x 4 for the HDR reader); rows bottom-up.
int gsph_load_bitmap(const char* path, uint32_t* width, uint32_t* height, uint32_t* texels) {
  return guard([&] {
    Image8 img = loadBitmap(path);
    *width = img.width;
    *height = img.height;
    if (texels) std::memcpy(texels, img.texels.data(), img.texels.size() * sizeof(uint32_t));
  });
}
int gsph_load_hdr_bitmap(const char* path, uint32_t* width, uint32_t* height, float* texels) {
  return guard([&] {
    ImageF img = loadHdrBitmap(path);
    *width = img.width;
    *height = img.height;
    if (texels) std::memcpy(texels, img.texels.data(), img.texels.size() * sizeof(float));
  });
}
// The flattened scene (pointers stay valid until gsph_scene_free).
const gsp_scene_desc* gsph_scene_desc(void* s) { return &((SceneBox*)s)->flat.desc; }
uint32_t gsph_scene_num_warnings(void* s) { return (uint32_t)((SceneBox*)s)->scene.warnings.size(); }
const char* gsph_scene_warning(void* s, uint32_t i) { return ((SceneBox*)s)->scene.warnings[i].c_str(); }
uint32_t gsph_scene_pixel_filter(void* s, float* param) {
  if (param) *param = ((SceneBox*)s)->scene.pixelFilterParam;
  return ((SceneBox*)s)->scene.pixelFilter;
}
// out4 = {aperture radius, focus distance, blades, rotation} of the scene's camera (Camera::setLens)
void gsph_scene_lens(void* s, float* out4) {
  const Camera& c = ((SceneBox*)s)->scene.camera;
  out4[0] = c.getApertureRadius();
  out4[1] = c.getFocusDistance();
  out4[2] = (float)c.getApertureBlades();
  out4[3] = c.getApertureRotation();
}
void gsph_scene_set_lens(void* s, float radius, float focus, uint32_t blades, float rotation) {
  ((SceneBox*)s)->scene.camera.setLens(radius, focus, blades, rotation);
}
// the scene's interior media (LoadOptions::readMedia / Scene::media): the count; out = 3 floats (sigma_a) per medium, may be NULL
uint32_t gsph_scene_media(void* s, float* out) {
  const std::vector<gsp_medium>& m = ((SceneBox*)s)->scene.media;
  if (out)
    for (size_t k = 0; k < m.size(); ++k)
      for (int c = 0; c < 3; ++c) out[3 * k + c] = m[k].sigma_a[c];
  return (uint32_t)m.size();
}
// ... and their scattering coefficients (LoadOptions::readScattering / Scene::mediaScattering): the count, 0 or that of the media;
// out = 4 floats (sigma_s, g) per medium, may be NULL
uint32_t gsph_scene_media_scattering(void* s, float* out) {
  const std::vector<gsp_medium_scatter>& m = ((SceneBox*)s)->scene.mediaScattering;
  if (out)
    for (size_t k = 0; k < m.size(); ++k) {
      for (int c = 0; c < 3; ++c) out[4 * k + c] = m[k].sigma_s[c];
      out[4 * k + 3] = m[k].g;
    }
  return (uint32_t)m.size();
}
// the scene's delta lights (LoadOptions::readEmitters / Scene::deltaLights): the count; out = one gsp_delta_light (64 B) each, may be NULL
uint32_t gsph_scene_delta_lights(void* s, gsp_delta_light* out) {
  const std::vector<gsp_delta_light>& l = ((SceneBox*)s)->scene.deltaLights;
  if (out && !l.empty()) std::memcpy(out, l.data(), l.size() * sizeof(gsp_delta_light));
  return (uint32_t)l.size();
}
// Scene::envmapSampling: the switch (return value) and its extent; and its setter
uint32_t gsph_scene_envmap_sampling(void* s, float* extent) {
  const gsp_envmap_sampling& e = ((SceneBox*)s)->scene.envmapSampling;
  if (extent) *extent = e.extent;
  return e.enabled;
}
void gsph_scene_set_envmap_sampling(void* s, uint32_t enabled, float extent) {
  ((SceneBox*)s)->scene.envmapSampling = gsp_envmap_sampling{enabled ? 1u : 0u, extent, {0u, 0u}};
}
// Scene::deltaLights = the n records at `lights` (n = 0: none)
void gsph_scene_set_delta_lights(void* s, const gsp_delta_light* lights, uint32_t n) {
  ((SceneBox*)s)->scene.deltaLights.assign(lights, lights + (lights ? n : 0u));
}
// Scene::addMedium with scattering: sigma_a (3 floats), sigma_s (3 floats), g
uint32_t gsph_scene_add_scattering_medium(void* s, const float* sigma_a3, const float* sigma_s3, float g) {
  return ((SceneBox*)s)->scene.addMedium(gsp_medium{{sigma_a3[0], sigma_a3[1], sigma_a3[2]}, 0.0f}, gsp_medium_scatter{{sigma_s3[0], sigma_s3[1], sigma_s3[2]}, g});
}
// RenderObject::interiorMedium of an object (0 = none); set: the number of an entry of the scene's media, which
// gsph_scene_add_medium appends (equal coefficients share one entry).  gsph_scene_reflatten rebuilds the flattened handles.
uint32_t gsph_scene_object_medium(void* s, uint32_t object) {
  const Scene& sc = ((SceneBox*)s)->scene;
  return object < sc.renderObjects.size() ? sc.renderObjects[object].interiorMedium : 0u;
}
uint32_t gsph_scene_add_medium(void* s, const float* sigma_a3) {
  return ((SceneBox*)s)->scene.addMedium(gsp_medium{{sigma_a3[0], sigma_a3[1], sigma_a3[2]}, 0.0f});
}
int gsph_scene_set_object_medium(void* s, uint32_t object, uint32_t number) {
  return guard([&] {
    Scene& sc = ((SceneBox*)s)->scene;
    if (object >= sc.renderObjects.size()) throw std::runtime_error("object index out of range");
    if (number > sc.media.size()) throw std::runtime_error("medium number beyond the scene's media");
    sc.renderObjects[object].interiorMedium = number;
  });
}
// the scene's film (LoadOptions::readFilm) as the gsp_display PathTracer::display takes; returns 1 when an ldrfilm was read
int gsph_scene_film(void* s, gsp_display* out) {
  const Scene::Film& f = ((SceneBox*)s)->scene.film;
  if (out) *out = f.display();
  return f.ldr ? 1 : 0;
}
uint32_t gsph_scene_num_materials(void* s) { return (uint32_t)((SceneBox*)s)->scene.materials.size(); }

// ---- scene edits between frames (what a host application does to its Scene; the tests drive PathTracer::prepareScene's
// value comparison with them) ----
uint32_t gsph_scene_num_objects(void* s) { return (uint32_t)((SceneBox*)s)->scene.renderObjects.size(); }
int gsph_scene_set_camera(void* s, const float* to_world16, float fov) {
  return guard([&] {
    Scene& sc = ((SceneBox*)s)->scene;
    sc.camera.setToWorld(make_mat4(to_world16));
    sc.camera.setFov(fov);
  });
}
int gsph_scene_set_transform(void* s, uint32_t object, const float* m16) {
  return guard([&] {
    Scene& sc = ((SceneBox*)s)->scene;
    if (object >= sc.renderObjects.size()) throw std::runtime_error("object index out of range");
    sc.renderObjects[object].transform = make_mat4(m16);
  });
}
// the material of render object `object`: emission (rgb or NULL = keep), twofaced (-1 = keep)
int gsph_scene_set_object_material(void* s, uint32_t object, const float* emission3, int twofaced) {
  return guard([&] {
    Scene& sc = ((SceneBox*)s)->scene;
    if (object >= sc.renderObjects.size()) throw std::runtime_error("object index out of range");
    Material& m = sc.getMaterial(sc.renderObjects[object].material);
    if (emission3) m.emission = vec3{emission3[0], emission3[1], emission3[2]};
    if (twofaced >= 0) m.twofaced = twofaced != 0;
  });
}
int gsph_scene_set_diffuse_reflectance(void* s, uint32_t index, const float* rgb) {
  return guard([&] {
    Scene& sc = ((SceneBox*)s)->scene;
    if (index >= sc.diffuseBSDFs.size()) throw std::runtime_error("diffuse BSDF index out of range");
    for (int k = 0; k < 3; ++k) sc.diffuseBSDFs[index].reflectance[k] = rgb[k];
  });
}
// gives render object `object` a NEW rough-conductor BSDF (appended to the table): tables and instances change together
int gsph_scene_make_object_rough_conductor(void* s, uint32_t object, const float* eta3, const float* k3, float alpha) {
  return guard([&] {
    Scene& sc = ((SceneBox*)s)->scene;
    if (object >= sc.renderObjects.size()) throw std::runtime_error("object index out of range");
    RoughConductorBSDF b{};
    for (int c = 0; c < 3; ++c) b.eta[c] = eta3[c], b.k[c] = k3[c], b.reflectance[c] = 1.0f;
    b.alpha = alpha;
    sc.getMaterial(sc.renderObjects[object].material).bsdf = sc.addRoughConductorBSDF(b);
  });
}
int gsph_scene_reflatten(void* s) {
  return guard([&] { flattenScene(((SceneBox*)s)->scene, ((SceneBox*)s)->flat); });
}

// SceneTracker (host/PathTracer.h) without a device: what would PathTracer::prepareScene send?
static SceneTracker g_tracker;
int gsph_tracker_remember(void* s) {
  return guard([&] {
    std::vector<gsp_instance> inst;
    (void)g_tracker.diff(((SceneBox*)s)->scene, inst);
    g_tracker.remember(((SceneBox*)s)->scene, inst);
  });
}
int gsph_tracker_diff(void* s) {
  std::vector<gsp_instance> inst;
  return (int)g_tracker.diff(((SceneBox*)s)->scene, inst);
}
int gsph_tracker_probe(void* uploaded, void* now) {
  SceneTracker t;
  std::vector<gsp_instance> inst;
  (void)t.diff(((SceneBox*)uploaded)->scene, inst);
  t.remember(((SceneBox*)uploaded)->scene, inst);
  return (int)t.diff(((SceneBox*)now)->scene, inst);
}

void* gsph_pathtracer_create(uint32_t width, uint32_t height, int device, const uint32_t* pixel_ids, uint64_t n) {
  PathTracer* pt = nullptr;
  int rc = guard([&] {
    std::vector<uint32_t> ids;
    if (pixel_ids) ids.assign(pixel_ids, pixel_ids + n);
    pt = new PathTracer(width, height, device, ids);
  });
  return rc ? nullptr : pt;
}
void gsph_pathtracer_free(void* pt) { delete (PathTracer*)pt; }
int gsph_pathtracer_create_render_pass(void* pt, void* scene) {
  return guard([&] { ((PathTracer*)pt)->createRenderPass(((SceneBox*)scene)->scene); });
}
int gsph_pathtracer_render(void* pt, void* scene, uint32_t spp) {
  return guard([&] { ((PathTracer*)pt)->render(((SceneBox*)scene)->scene, spp); });
}
int gsph_pathtracer_set_params(void* pt, const gsp_render_params* p) {
  return guard([&] { ((PathTracer*)pt)->params = *p; });
}
int gsph_pathtracer_timestamp(void* pt) { return ((PathTracer*)pt)->getTimestamp(); }
int gsph_pathtracer_reset(void* pt) {
  return guard([&] { ((PathTracer*)pt)->reset(); });
}
int gsph_pathtracer_download(void* pt, float* out, uint64_t count) {
  return guard([&] {
    auto img = ((PathTracer*)pt)->download();
    if (count < img.size()) throw std::runtime_error("output buffer too small");
    std::memcpy(out, img.data(), img.size() * sizeof(float));
  });
}
int gsph_pathtracer_stats(void* pt, gsp_stats* out) {
  return guard([&] { *out = ((PathTracer*)pt)->stats(); });
}
// TEST of the stale-scene hazard: every file is loaded into a `Scene` that lives in the SAME stack slot of this frame (the
// loop body's local), rendered with `spp` samples from timestamp 0 and downloaded; addresses[i] receives &scene of
// iteration i so that the caller can assert they really coincided.  out = n images of width*height*4 floats.
int gsph_pathtracer_render_files_same_slot(void* pt, const char* const* paths, const char* asset_dir, uint32_t n, uint32_t spp,
                                           float* out, uint64_t* addresses) {
  return guard([&] {
    PathTracer* p = (PathTracer*)pt;
    for (uint32_t i = 0; i < n; ++i) {
      Scene scene = loadScene(paths[i], asset_dir ? asset_dir : "");
      addresses[i] = (uint64_t)(uintptr_t)&scene;
      p->reset();
      p->render(scene, spp);
      const std::vector<float> img = p->download();
      std::memcpy(out + (size_t)i * img.size(), img.data(), img.size() * sizeof(float));
    }
  });
}
int gsph_write_pfm(const char* path, const float* rgba, uint32_t width, uint32_t height) {
  return guard([&] { writePfm(path, rgba, width, height); });
}

int gsph_write_ppm(const char* path, const float* rgba, uint32_t width, uint32_t height, int tone_map) {
  return guard([&] { writePpm(path, rgba, width, height, tone_map != 0); });
}
// Image.h PNG writer.  gsph_encode_png: two calls, out == NULL returns the size
int gsph_write_png(const char* path, const uint32_t* rgba8, uint32_t width, uint32_t height, int alpha) {
  return guard([&] { writePng(path, rgba8, width, height, alpha != 0); });
}
int gsph_encode_png(const uint32_t* rgba8, uint32_t width, uint32_t height, int alpha, uint8_t* out, uint64_t* size) {
  return guard([&] {
    const std::vector<uint8_t> f = encodePng(rgba8, width, height, alpha != 0);
    if (out && *size >= f.size()) std::memcpy(out, f.data(), f.size());
    *size = f.size();
  });
}
// decodePng of a buffer: texels == NULL returns the size; rows bottom-up
int gsph_decode_png(const uint8_t* data, uint64_t size, uint32_t* width, uint32_t* height, uint32_t* texels) {
  return guard([&] {
    Image8 img = decodePng(data, size);
    *width = img.width;
    *height = img.height;
    if (texels) std::memcpy(texels, img.texels.data(), img.texels.size() * sizeof(uint32_t));
  });
}
int gsph_pathtracer_set_display(void* pt, const gsp_display* d) {
  return guard([&] { ((PathTracer*)pt)->display = *d; });
}
int gsph_pathtracer_download_display(void* pt, uint32_t* out, uint64_t count) {
  return guard([&] {
    auto img = ((PathTracer*)pt)->downloadDisplay();
    if (count < img.size()) throw std::runtime_error("output buffer too small");
    std::memcpy(out, img.data(), img.size() * sizeof(uint32_t));
  });
}
// feature pass + denoiser of a PathTracer (gpuspectral_pt.h "Feature buffers", "Denoiser"); denoise may be NULL
int gsph_pathtracer_render_features(void* pt, void* scene, uint32_t spp) {
  return guard([&] { ((PathTracer*)pt)->renderFeatures(*(Scene*)scene, spp); });
}
int gsph_pathtracer_download_features(void* pt, float* albedo, float* geom, uint64_t floats_each) {
  return guard([&] {
    std::vector<float> a, g;
    ((PathTracer*)pt)->downloadFeatures(&a, &g, nullptr);
    if (floats_each < a.size()) throw std::runtime_error("output buffer too small");
    std::memcpy(albedo, a.data(), a.size() * sizeof(float));
    std::memcpy(geom, g.data(), g.size() * sizeof(float));
  });
}
int gsph_pathtracer_download_denoised(void* pt, const gsp_denoise* denoise, float* out, uint64_t floats) {
  return guard([&] {
    auto img = ((PathTracer*)pt)->downloadDenoised(denoise);
    if (floats < img.size()) throw std::runtime_error("output buffer too small");
    std::memcpy(out, img.data(), img.size() * sizeof(float));
  });
}
int gsph_pathtracer_download_denoised_display(void* pt, const gsp_denoise* denoise, uint32_t* out, uint64_t count) {
  return guard([&] {
    auto img = ((PathTracer*)pt)->downloadDenoisedDisplay(denoise);
    if (count < img.size()) throw std::runtime_error("output buffer too small");
    std::memcpy(out, img.data(), img.size() * sizeof(uint32_t));
  });
}
// temporal accumulation of a PathTracer (gpuspectral_pt.h "Temporal accumulation"); temporal / denoise may be NULL
int gsph_pathtracer_next_frame(void* pt) {
  return guard([&] { ((PathTracer*)pt)->nextFrame(); });
}
int gsph_pathtracer_temporal_accumulate(void* pt, const gsp_temporal* temporal) {
  return guard([&] { ((PathTracer*)pt)->temporalAccumulate(temporal); });
}
int gsph_pathtracer_temporal_reset(void* pt) {
  return guard([&] { ((PathTracer*)pt)->temporalReset(); });
}
int gsph_pathtracer_download_temporal(void* pt, float* out, uint64_t floats) {
  return guard([&] {
    auto img = ((PathTracer*)pt)->downloadTemporal();
    if (floats < img.size()) throw std::runtime_error("output buffer too small");
    std::memcpy(out, img.data(), img.size() * sizeof(float));
  });
}
int gsph_pathtracer_download_temporal_denoised(void* pt, const gsp_denoise* denoise, float* out, uint64_t floats) {
  return guard([&] {
    auto img = ((PathTracer*)pt)->downloadTemporalDenoised(denoise);
    if (floats < img.size()) throw std::runtime_error("output buffer too small");
    std::memcpy(out, img.data(), img.size() * sizeof(float));
  });
}
// variance-guided filter of a PathTracer (gpuspectral_pt.h "Variance-guided filter"); denoise / svgf may be NULL
int gsph_pathtracer_temporal_track_moments(void* pt, int on) {
  return guard([&] { ((PathTracer*)pt)->temporalTrackMoments(on != 0); });
}
int gsph_pathtracer_download_temporal_moments(void* pt, float* out, uint64_t floats) {
  return guard([&] {
    auto img = ((PathTracer*)pt)->downloadTemporalMoments();
    if (floats < img.size()) throw std::runtime_error("output buffer too small");
    std::memcpy(out, img.data(), img.size() * sizeof(float));
  });
}
int gsph_pathtracer_download_temporal_svgf(void* pt, const gsp_denoise* denoise, const gsp_svgf* svgf, float* out, uint64_t floats) {
  return guard([&] {
    auto img = ((PathTracer*)pt)->downloadTemporalSvgf(denoise, svgf);
    if (floats < img.size()) throw std::runtime_error("output buffer too small");
    std::memcpy(out, img.data(), img.size() * sizeof(float));
  });
}
// moved instances of a PathTracer (gpuspectral_pt.h "Temporal accumulation: moved instances")
// PathTracer::setLightSampling / downloadLightPick (out: `capacity` entries of 16 B; returns through *count)
int gsph_pathtracer_set_light_sampling(void* pt, uint32_t mode) {
  return guard([&] { ((PathTracer*)pt)->setLightSampling(mode); });
}
int gsph_pathtracer_set_estimator(void* pt, uint32_t mode) {  // PathTracer::setEstimator
  return guard([&] { ((PathTracer*)pt)->setEstimator(mode); });
}
int gsph_pathtracer_set_light_grid(void* pt, uint32_t enabled, uint32_t nx, uint32_t ny, uint32_t nz) {  // PathTracer::setLightGrid
  return guard([&] { ((PathTracer*)pt)->setLightGrid(enabled != 0u, nx, ny, nz); });
}
int gsph_pathtracer_download_light_pick(void* pt, gsp_light_pick* out, uint32_t capacity, uint32_t* count) {
  return guard([&] {
    auto t = ((PathTracer*)pt)->downloadLightPick();
    if (count) *count = (uint32_t)t.size();
    if (t.size() > capacity) throw std::runtime_error("downloadLightPick: capacity below the number of lights");
    if (!t.empty()) std::memcpy(out, t.data(), t.size() * sizeof(gsp_light_pick));
  });
}
int gsph_pathtracer_temporal_follow_instances(void* pt, int on) {
  return guard([&] { ((PathTracer*)pt)->temporalFollowInstances(on != 0); });
}
int gsph_pathtracer_download_temporal_motion(void* pt, float* out, uint64_t floats) {
  return guard([&] {
    auto img = ((PathTracer*)pt)->downloadTemporalMotion();
    if (floats < img.size()) throw std::runtime_error("output buffer too small");
    std::memcpy(out, img.data(), img.size() * sizeof(float));
  });
}
// illumination history of a PathTracer (gpuspectral_pt.h "Illumination history"); out may be NULL for the feedback (no output)
int gsph_pathtracer_temporal_demodulate(void* pt, int on) {
  return guard([&] { ((PathTracer*)pt)->temporalDemodulate(on != 0); });
}
int gsph_pathtracer_download_temporal_image(void* pt, float* out, uint64_t floats) {
  return guard([&] {
    auto img = ((PathTracer*)pt)->downloadTemporalImage();
    if (floats < img.size()) throw std::runtime_error("output buffer too small");
    std::memcpy(out, img.data(), img.size() * sizeof(float));
  });
}
int gsph_pathtracer_temporal_image_to_device(void* pt, void* device_dst, uint64_t bytes) {
  return guard([&] { ((PathTracer*)pt)->temporalImageToDevice(device_dst, bytes); });
}
int gsph_pathtracer_temporal_svgf_feedback(void* pt, const gsp_denoise* denoise, const gsp_svgf* svgf, uint32_t levels, float* out, uint64_t floats) {
  return guard([&] {
    auto img = ((PathTracer*)pt)->temporalSvgfFeedback(denoise, svgf, levels, out != nullptr);
    if (!out) return;
    if (floats < img.size()) throw std::runtime_error("output buffer too small");
    std::memcpy(out, img.data(), img.size() * sizeof(float));
  });
}
int gsph_pathtracer_temporal_svgf_feedback_to_device(void* pt, const gsp_denoise* denoise, const gsp_svgf* svgf, uint32_t levels, void* device_dst,
                                                     uint64_t bytes) {
  return guard([&] { ((PathTracer*)pt)->temporalSvgfFeedbackToDevice(denoise, svgf, levels, device_dst, bytes); });
}
// temporal anti-lag of a PathTracer (gpuspectral_pt.h "Temporal anti-lag")
int gsph_pathtracer_temporal_antilag(void* pt, const gsp_antilag* antilag) {
  return guard([&] { ((PathTracer*)pt)->temporalAntilag(antilag); });
}
int gsph_pathtracer_download_temporal_fast(void* pt, float* out, uint64_t floats) {
  return guard([&] {
    auto img = ((PathTracer*)pt)->downloadTemporalFast();
    if (floats < img.size()) throw std::runtime_error("output buffer too small");
    std::memcpy(out, img.data(), img.size() * sizeof(float));
  });
}
int gsph_pathtracer_temporal_fast_to_device(void* pt, void* device_dst, uint64_t bytes) {
  return guard([&] { ((PathTracer*)pt)->temporalFastToDevice(device_dst, bytes); });
}
// temporal anti-aliasing of a PathTracer (gpuspectral_pt.h "Temporal anti-aliasing"); taa, display and src may be NULL
int gsph_pathtracer_temporal_taa(void* pt, const gsp_taa* taa, const gsp_display* display, const float* src, uint64_t floats) {
  return guard([&] { ((PathTracer*)pt)->temporalTaa(taa, display, src, floats); });
}
int gsph_pathtracer_temporal_taa_from_device(void* pt, const gsp_taa* taa, const gsp_display* display, const void* device_src, uint64_t bytes) {
  return guard([&] { ((PathTracer*)pt)->temporalTaaFromDevice(taa, display, device_src, bytes); });
}
int gsph_pathtracer_download_taa(void* pt, float* out, uint64_t floats) {
  return guard([&] {
    auto img = ((PathTracer*)pt)->downloadTaa();
    if (floats < img.size()) throw std::runtime_error("output buffer too small");
    std::memcpy(out, img.data(), img.size() * sizeof(float));
  });
}
int gsph_pathtracer_download_taa_display(void* pt, uint32_t* out, uint64_t count) {
  return guard([&] {
    auto img = ((PathTracer*)pt)->downloadTaaDisplay();
    if (count < img.size()) throw std::runtime_error("output buffer too small");
    std::memcpy(out, img.data(), img.size() * sizeof(uint32_t));
  });
}
int gsph_pathtracer_taa_display_to_device(void* pt, void* device_dst, uint64_t bytes) {
  return guard([&] { ((PathTracer*)pt)->taaDisplayToDevice(device_dst, bytes); });
}
int gsph_tone_map(const float* rgba, uint32_t width, uint32_t height, int tone_map, uint8_t* rgb8) {
  return guard([&] {
    std::vector<uint8_t> v;
    toneMapToRgb8(rgba, width, height, tone_map != 0, v);
    std::memcpy(rgb8, v.data(), v.size());
  });
}

}  // extern "C"
