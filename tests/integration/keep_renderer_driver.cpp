// keep_renderer_driver.cpp — the reference's camchanged sequence (main.cpp:110-136: pathtraceFree(); pathtraceInit(scene)) through the
// shim of include/pathtrace_amd.hpp, with and without pathtraceSetKeepRenderer.  Built by tests/test_gpu_set_camera_cli.py against
// pathtrace_amd.hpp and pt::Scene only.
//
//   keep_renderer_driver SCENE_A.txt SCENE_B.txt OUT_PREFIX KEEP CHANGE_MATERIAL
//
// Renders 4 iterations with SCENE_A's camera, frees, takes SCENE_B's camera (and, with CHANGE_MATERIAL, another colour for material 1),
// initialises and renders 4 more; writes the two SUM images as raw float32 to OUT_PREFIX.0.f32 / OUT_PREFIX.1.f32 and prints
// `set_camera_calls N` for the renderer that rendered the second one.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "pathtrace_amd.hpp"
#include "pt_scene.h"

static int write_image(const pt::Scene& s, const std::string& path) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return 1;
  const size_t n = s.state.image.size();
  const bool ok = std::fwrite(s.state.image.data(), sizeof(float), n, f) == n;
  return std::fclose(f) || !ok;
}

int main(int argc, char** argv) {
  if (argc != 6) {
    std::fprintf(stderr, "usage: %s SCENE_A SCENE_B OUT_PREFIX KEEP CHANGE_MATERIAL\n", argv[0]);
    return 2;
  }
  pt::Scene scene(argv[1]), other(argv[2]);
  scene.applyInitialCameraState();
  other.applyInitialCameraState();
  scene.state.iterations = 4;
  const std::string out = argv[3];
  pathtraceSetKeepRenderer(std::atoi(argv[4]));
  pathtraceFree();  // main.cpp:134 frees before the first init
  pathtraceInit(&scene);
  for (int it = 1; it <= 4; ++it) pathtrace(nullptr, 0, it);
  pathtraceFree();  // reads the image back
  if (write_image(scene, out + ".0.f32")) return 1;
  scene.state.camera = other.state.camera;  // camchanged
  if (std::atoi(argv[5])) scene.materials[1].color[0] = 0.25f;
  pathtraceInit(&scene);
  PtSetupTimes times{};
  if (pt_get_setup_times(&times)) return 1;
  for (int it = 1; it <= 4; ++it) pathtrace(nullptr, 0, it);
  pathtraceFree();
  if (write_image(scene, out + ".1.f32")) return 1;
  std::printf("set_camera_calls %d\n", (int)times.set_camera_calls);
  pathtraceShutdown();
  pathtraceShutdown();  // safe twice
  return 0;
}
