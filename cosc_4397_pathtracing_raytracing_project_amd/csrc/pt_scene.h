// pt_scene.h — host-side scene model of the MI355X path tracer (product code).
//
// Mirrors the public surface of the reference's `Scene` (src/scene.h:20-25:
// geoms, materials, state) with plain structs from include/pt_amd.h so it can cross
// the C ABI, and restates the arithmetic of the reference's loader in GLM 0.9.6
// operation order so the transform/inverse/invTranspose matrices and the camera
// basis are bit-identical to what `new Scene(file)` + main.cpp produce.
#pragma once
#include <string>
#include <vector>

#include "../../include/pt_amd.h"

namespace pt {

struct RenderState {  // src/sceneStructs.h:61-67
  PtCamera camera{};
  unsigned int iterations = 0;
  int traceDepth = 0;
  std::vector<float> image;  // W*H*3 running sum
  std::string imageName;
};

struct GeomTrs {  // the TRANS / ROTAT / SCALE of the OBJECT a geom came from; mesh: one triangle of a `mesh` object
  float trs[9];
  bool mesh;
};

class Scene {  // src/scene.h:11-26
 public:
  explicit Scene(const std::string& filename);  // throws std::runtime_error if unreadable
  std::vector<PtGeom> geoms;
  std::vector<GeomTrs> geom_trs;  // beside geoms (pt_scene_geom_trs / pt_scene_set_geom_trs)
  std::vector<PtMaterial> materials;
  RenderState state;
  float fovy = 0.0f;

  // scene.cpp:133-140 for a new resolution (headless stand-in for editing RES).
  void overrideResolution(int w, int h);
  // main.cpp:57-71 + 110-128: what the first runCuda() does to the camera.
  void applyInitialCameraState();
  // main.cpp:192-199: a mouse drag in float (phi += dphi, theta and zoom clamped as there), then the camchanged block.
  void orbit(float dphi, float dtheta, float dzoom);
  float phi = 0.0f, theta = 0.0f, zoom = 0.0f;  // main.cpp:63-71, set by applyInitialCameraState()
  PtSceneDesc desc() const;
  // A new TRANS / ROTAT / SCALE for the OBJECT geom `geom` came from (not a mesh triangle): geom_trs and the three matrices, through
  // the loader's buildTransform.
  void placeGeom(int geom, const float trs[9]);
  // A new material in the place of material m (an index inside `materials`): all eleven words as given.  false, nothing changed: one of
  // the words the renderer reads (color, specular_color, hasReflective, hasRefractive, emittance) is not finite.
  bool setMaterial(int m, const PtMaterial& material);

 private:
  void applyOrbitState();  // main.cpp:112-126: the camera from phi, theta, zoom and lookAt
};

// utilities.cpp:64-72 / scene.cpp:83-86 restated (exposed for tests).
void buildTransform(const float trs[9], float transform[16], float inverse[16], float invTranspose[16]);

// pathtrace.cu:34-111.
void buildBVH(const PtGeom* geoms, int n, std::vector<PtBVHNode>& nodes);

}  // namespace pt
