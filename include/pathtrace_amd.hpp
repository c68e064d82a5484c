// pathtrace_amd.hpp — C++ source-compatible mirror of the reference's renderer API
// (reference: src/pathtrace.h:6-9) on top of the C ABI in pt_amd.h.
//
//   reference                                   here
//   void InitDataContainer(GuiDataContainer*)   same
//   void pathtraceInit(Scene*)                  same, Scene = pt::Scene (pt_scene.h; same public
//                                               members geoms / materials / state as src/scene.h:20-25)
//   void pathtraceFree()                        same (legal before Init and twice, main.cpp:134); see pathtraceSetKeepRenderer
//   void pathtrace(uchar4* pbo,int frame,int i) same; pbo may be nullptr (headless) or a DEVICE
//                                               pointer to W*H uchar4 (as the GL-mapped PBO is)
// Errors keep the reference's convention: message on stderr + exit(EXIT_FAILURE)
// (pathtrace.cu:141-150).
//
// One deliberate difference: the reference copies the whole accumulation image to
// scene->state.image after EVERY iteration (pathtrace.cu:648-651).  Here iterations
// are queued and traced in batches; scene->state.image is refreshed when the last
// iteration (state.iterations) has been submitted, on pathtraceFree(), or on demand
// with pathtraceSyncImage().  The image content is identical (a pure sum).
#pragma once
#include "pt_amd.h"

namespace pt {
class Scene;
}

class GuiDataContainer {  // src/utilities.h:17-22
 public:
  GuiDataContainer() : TracedDepth(0) {}
  int TracedDepth;
};

struct pt_uchar4 {
  unsigned char x, y, z, w;
};

void InitDataContainer(GuiDataContainer* guiData);
void pathtraceInit(pt::Scene* scene);
void pathtraceFree();
void pathtrace(pt_uchar4* pbo, int frame, int iteration);
// extension: flush queued iterations and refresh scene->state.image (running SUM)
void pathtraceSyncImage();
// extension: arithmetic mode (PT_ARITH_*, pt_amd.h) of the next pathtraceInit; default PT_ARITH_EXACT
void pathtraceSetArith(int pt_arith);
// extension: stochastic anti-aliasing (PtOptions.aa_jitter) of the next pathtraceInit; default off = reference semantics
void pathtraceSetAntialias(int on);
// extension: convergence metric (PtOptions.convergence) of the next pathtraceInit: 0 off (default), N > 0 the reference frame is
// the average after iteration N (the reference's computePSNR uses 10)
void pathtraceSetConvergence(int n);
// extension: flushes queued iterations and returns what the reference prints as "PSNR" after iteration `iter`
// (pathtrace.cu:627-638): FLT_MAX where it prints "Inf" (no reference frame yet, or mse <= 1e-12)
float pathtracePSNR(int iter);
// extension: the reference answers every camera move with pathtraceFree(); pathtraceInit(scene) (main.cpp:110-136).  With this on
// (default off: exactly the behaviour above) pathtraceFree() reads the image back as always but parks the renderer, and the next
// pathtraceInit(scene) moves its camera (pt_set_camera: no teardown, no allocation, no traversal probe) when geoms and materials
// compare equal to the parked renderer's and resolution, trace depth, arithmetic, anti-aliasing and convergence settings are the
// same; in any other case it frees and initialises for real.  The images are the same either way.
void pathtraceSetKeepRenderer(int on);
// extension: frees a parked renderer (and a live one, like pathtraceFree); safe to call twice.  What a program that turned
// pathtraceSetKeepRenderer on calls before it exits.
void pathtraceShutdown();
