// Loader.h -- Mitsuba-XML + OBJ scene loader (kept entry point of the reference,
// S/engine/Loader.h:29: Scene loadScene(Engine&, Renderer&, const std::string& path)).
// Engine/Renderer only supplied the asset directory and GPU mesh uploads; here the
// asset directory is a plain argument and meshes stay on the host.
#pragma once
#include <string>

#include "Scene.h"

namespace GPUSpectral {

// dormantFeatures = false (default): the reference's behaviour -- a textured reflectance falls back to the colour
// default and a top-level emitter is ignored, each with a warning (Loader.cpp:122-143,338-346 are commented out there).
// true: the branches the reference left dormant are live -- `bitmap` textures (PNG / JPEG, Image.h) and `checkerboard`
// textures on diffuse / roughplastic / roughconductor, and an `envmap` emitter (PFM / .hdr) -- see
// include/gpuspectral_pt.h for what the renderer does with them.
struct LoadOptions {
  bool dormantFeatures = false;
  bool srgbTextures = true;
  // `<shape type="disk">` maps to assets/disk.obj in the reference (Loader.cpp:276), a file its checkout does
  // not hold, and `sphere` falls through to an empty file name (:278): both shapes are skipped with a warning by default,
  // as they are there -- which leaves `living-room` without its only emitters and `staircase2` without five of its lights.
  // builtinShapes = true builds them instead: Mitsuba's unit disk (z = 0, radius 1, normal +z; 64 fan triangles) and unit
  // sphere (octahedron subdivided three times, 512 triangles, smooth normals), tessellated with float32 + * / sqrt only
  // (no libm: oracle/mitsuba_loader.py builds the same floats).  `to_world` and `center` as for every shape
  // (Loader.cpp:284-293); `radius` -- which the reference never reads -- scales the sphere.
  bool builtinShapes = false;
  // Every scene the reference ships declares `<rfilter type="tent" />` in its film, and its loader never looks at it.
  // readFilter = true reads it: `box`, `tent` (optional float `radius`) and `gaussian` (optional float `stddev`) under the
  // sensor's film become Scene::pixelFilter / pixelFilterParam (GSP_FILTER_*, include/gpuspectral_pt.h "Pixel filter"; an
  // absent parameter stays 0 = the filter's default), which PathTracer::render hands to the device.  Any other type
  // (mitchell, catmullrom, lanczos: negative lobes, which cannot be importance-sampled with weight 1) is a load error.
  // false (default): the film is ignored and the scene renders unfiltered, as in the reference.
  bool readFilter = false;
  // The reference treats every <sensor> as `perspective`.  readLens = true reads a `thinlens` sensor's float `aperture_radius`
  // (or `apertureRadius`) and `focus_distance` (or `focusDistance`) into the camera (Camera::setLens; circular aperture), which
  // PathTracer hands to the device (gsp_set_lens, include/gpuspectral_pt.h "Thin lens").  A negative or non-finite radius, or a
  // radius > 0 without a finite positive focus distance, is a load error.  Other sensor types are not affected.
  // false (default): the sensor plugin is ignored and the camera is a pinhole, as in the reference.
  bool readLens = false;
  // Every scene the reference ships declares `<film type="ldrfilm">` (fileFormat png, gamma 2.2), and its loader never looks at
  // it.  readFilm = true reads an ldrfilm's float `gamma` (-1, Mitsuba's default, becomes 0 = the sRGB curve), float `exposure`,
  // string `tonemapMethod` (`gamma` | `reinhard`), float `key` and `burn` into Scene::film (include/gpuspectral_pt.h "LDR film");
  // a value gsp_display would refuse is a load error.  Any other film type leaves the record at its defaults, with a warning.
  // false (default): the film is ignored, as in the reference.
  bool readFilm = false;
  // The reference never looks at the named children of a shape, so the <medium type="homogeneous" name="interior"> of its glass
  // shapes (living-room, staircase2) does nothing and the glasses render clear.  readMedia = true reads them (include/
  // gpuspectral_pt.h "Interior media"): inline or as a <ref> to a top-level <medium id=..>; `sigmaA` as an rgb or spectrum triple, or
  // `sigmaT` with `albedo` (sigma_a = sigmaT * (1 - albedo)); an optional float `scale` multiplies.  Equal triples share one entry of
  // Scene::media; RenderObject::interiorMedium names it.  A medium with sigmaS != 0 or albedo != 0, a name="exterior" medium and a
  // type other than homogeneous are skipped with one warning each, as `disk` shapes are.
  bool readMedia = false;
  // readScattering = true (implies readMedia) also reads what makes a medium scatter (include/gpuspectral_pt.h "Scattering media"):
  // `sigmaS`, or `sigmaT` with `albedo` (sigma_s = sigmaT * albedo, sigma_a = sigmaT * (1 - albedo)), times `scale`; and a
  // <phase type="hg"><float name="g" ../></phase> child (`isotropic` or no child: g = 0; any other phase type: one warning, g = 0).
  // Scene::mediaScattering then runs parallel to Scene::media.  false: a scattering medium is skipped with its warning, as above.
  bool readScattering = false;
  // readEmitters = true reads the top-level delta emitters (include/gpuspectral_pt.h "Delta lights") into Scene::deltaLights:
  //   <emitter type="point">: `position`, or the translation of `toWorld`; `intensity`
  //   <emitter type="spot">: `toWorld` (position = its translation, axis = the image of +z); `intensity`; `cutoffAngle` (default 20
  //     degrees) and `beamWidth` (default 3 / 4 of the cutoff); the cosines are formed in double.  The falloff between them is the
  //     library's smoothstep of the cosine, not Mitsuba's ramp in the angle
  //   <emitter type="directional">: `direction`, or the image of +z under `toWorld`; `irradiance`; extent = half the diagonal of the
  //     world-space bounding box of the scene's vertices (1 for a scene without any)
  // A `scale` multiplies the intensity / irradiance.  Every other emitter type keeps its warning.  false: the scene and its warnings are
  // what they were before this option existed.
  bool readEmitters = false;
  // sampleEnvmap = true switches the environment light on (include/gpuspectral_pt.h "Environment light"): Scene::envmapSampling =
  // {enabled, extent = half the diagonal of the world-space bounding box of the scene's vertices (1 for a scene without any)}.  It
  // takes effect only for a scene that carries an environment map (dormantFeatures) and needs GSP_ESTIMATOR_TEXTBOOK.  false: the
  // scene is what it was before this option existed.
  bool sampleEnvmap = false;
};

// assetDir: where rect.obj / box.obj / disk.obj live (Engine::assetPath); "" = the
// directory shipped with this library (gpuspectral_amd/assets).
Scene loadScene(const std::string& path, const std::string& assetDir = "", const LoadOptions& options = LoadOptions());

// Throws std::runtime_error like the reference on unreadable files.
MeshPtr loadMesh(const std::string& objPath, uint32_t id);

void setDefaultAssetDir(const std::string& dir);

}  // namespace GPUSpectral
