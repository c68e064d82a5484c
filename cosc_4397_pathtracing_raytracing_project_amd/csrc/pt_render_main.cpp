// pt_render — headless driver: what the reference's main() / runCuda() / saveImage()
// (src/main.cpp:34-156) do without the GLFW window: load a scene file, run
// state.iterations iterations, write the PNG saveImage() would write.  Flags exist only because
// the reference takes resolution, iteration count and depth from the scene file (scene.cpp:103-114).
//
//   pt_render SCENE.txt [--res WxH] [--spp N] [--depth D] [--out PREFIX] [--pfm] [--hdr] [--orbit N [--device-tables] [--move G:DX,DY,DZ] [--recolor M:DR,DG,DB] [--emit M:DE] [--orbit-still] [--reproject [--history-cap C] [--denoise-history [--history-moments [--history-feedback [--feedback-level L] [--feedback-variance V]]] [--history-threshold E [--history-threshold-cap F] [--history-threshold-min-pixels P] [--history-threshold-group G]]] [--history-extra G [--history-min M] [--history-extra-cap F]] [--history-probe [--probe-radius R] [--probe-gain X]]]]
//                       [--arith exact|fma|fast] [--gpus K | --devices LIST] [--transport rccl|copy] [--stamp] [--aa]
//                       [--preview N] [--convergence N | --reference FILE.pfm] [--clean-db X] [--features]
//                       [--denoise [--denoise-levels N] [--denoise-sigma C,N,P] [--denoise-keep-albedo]]
//                       [--denoise-guided] [--until-db X [--until-group G] [--adaptive F [--denoise-adaptive]]]
//                       [--adaptive-threshold E [--adaptive-cap F] [--adaptive-min-pixels P] [--until-group G] [--denoise-adaptive]]
//
// Without --gpus the run goes through the pathtrace.h-compatible shim (pathtraceInit / pathtrace per
// iteration / pathtraceFree), i.e. the code path a reference main.cpp would take.  With --gpus K (K >= 1;
// K = 0: all visible devices) it goes through pt_group_*: K devices in this one process, row-interleaved
// tiles, one grouped RCCL send/recv at write-out (BASELINE config 4), PNG bytes converted on the devices.
// --devices 0,0,0 names the devices explicitly; a device may appear more than once (several contexts on one GPU — the
// exchange then uses peer / device copies instead of RCCL, PT_GROUP_TRANSPORT_COPY; --transport forces either).
// --preview N (with --gpus): every N iterations the running average is converted on the devices and gathered
// (pt_group_preview_rgba8 — the reference shows it after every iteration, pathtrace.cu:618) into PREFIX.preview.png.
// --convergence N / --reference FILE.pfm: the convergence metric (PtOptions.convergence) against the average after iteration N
// (the reference's computePSNR: N = 10) or against an averaged-radiance image as --pfm writes it (e.g. a 5000-spp render): after
// the render one line `iteration psnr_db` per iteration ("Inf" where the reference prints it) and "Iterations to clean: n", the
// first iteration above --clean-db (default 35; -1 when there is none).  Works with --gpus / --devices.
// --features: after the render a first-hit feature pass over the same iterations (pt_render_features / pt_group_render_features);
// the averages go to <base>.normal.pfm, <base>.albedo.pfm, <base>.position.pfm and <base>.depth.pfm (depth in all three
// channels) next to the image, written like --pfm writes the image (sums / spp).
// --denoise (implies --features): the edge-avoiding filter over the image and the feature buffers (pt_denoise / pt_group_denoise);
// the averaged result goes to <base>.denoised.png and, with --pfm, <base>.denoised.pfm.  --denoise-levels N (1 .. 8, default 5),
// --denoise-sigma C,N,P (colour, normal, position; 0 = the default 4, 0.5, 1; negative = that term off), --denoise-keep-albedo
// (no demodulation by the first-hit albedo) are PtDenoiseOptions' fields.
// --denoise-guided (implies --features; excludes --denoise, takes the --denoise-* options, sigma C's default then being 8): the
// variance-guided form of the filter (pt_denoise_guided / pt_group_denoise_guided), whose colour term follows the per-pixel noise
// estimate.  It needs at least two folded groups: with --until-db it filters what that render left; without it the --spp iterations
// (at least 2) are rendered in groups of --until-group G (default ceil(spp / 4)) with a fold after each.  Same output files as --denoise.
// --until-db X: render until the image's own noise estimate says it is clean (pt_render_until / pt_group_render_until): groups of G
// iterations (--until-group, default 0 = one batch), a fold after each, until the estimated PSNR is above X dB; --spp becomes the cap.
// Prints `noise: <iterations> iterations, <groups> groups, estimated PSNR <x> dB`; the file names, --features, --denoise and the
// curves carry the iterations actually rendered.
// --adaptive F (needs --until-db X, takes --until-group; excludes --gpus / --devices, --denoise, --denoise-guided, --convergence,
// --reference and --preview): adaptive sampling (pt_render_adaptive) — two uniform groups of G iterations, then rounds of G iterations over the
// noisiest fraction F (0 < F <= 1) of the pixels, until the estimated PSNR is above X dB or --spp iteration numbers are used up.
// Prints `adaptive: <iterations> iterations, <rounds> rounds, <samples> samples (<x> of uniform), estimated PSNR <y> dB`, x being
// the samples over iterations * pixels; the PNG / PFM / HDR hold the resolved image (pt_resolve: every pixel's sum over its own
// sample count) and the file name carries ceil(samples / pixels).
// --adaptive-threshold E (takes --until-group, --adaptive-cap F, default 0.25, and --adaptive-min-pixels P, default 0; excludes
// --adaptive, --until-db, --gpus / --devices, --denoise, --denoise-guided, --convergence, --reference and --preview): adaptive sampling
// until every pixel is below a noise threshold (pt_render_threshold) — two uniform groups of G iterations, then rounds of G iterations
// over the pixels whose estimated standard error exceeds E, the noisiest fraction F of the frame at the most, until at most P pixels
// are above or --spp iteration numbers are used up.  The worker's memory follows F and the iterations per batch.  Prints
// `adaptive: threshold <E>: <iterations> iterations, <rounds> rounds, <samples> samples (<x> of uniform), <n> pixels above, estimated
// PSNR <y> dB`; the files are those of --adaptive, named the same way.
// --denoise-adaptive (needs --adaptive F or --adaptive-threshold E; implies --features; excludes --denoise and --denoise-guided, takes the --denoise-* options,
// sigma C's default being 8): the variance-guided filter with per-pixel sample counts (pt_denoise_adaptive) over the adaptive image,
// after the resolved image is written.  Same output files as --denoise.
// --orbit N (1 .. 999; excludes every option from --preview to --denoise-adaptive above): N views of the scene on ONE renderer, a full
// turn around LOOKAT in steps of 2 pi / N — frame 0 is the scene's camera through pt_init (pt_group_create with --gpus / --devices),
// frame f > 0 the viewer's mouse drag (pt_scene_orbit) followed by pt_set_camera (pt_group_set_camera) where the reference frees and
// initialises; every frame renders iterations 1 .. --spp and is written as <base>.orbit<fff>.png (.pfm, .hdr).  Prints the setup
// times once and per frame `orbit: frame f: camera x y z, set_camera a ms, render b ms`.  --device-tables (with --orbit): every move
// passes PT_SET_CAMERA_DEVICE_TABLES (pt_set_camera_ex: the camera-dependent tables are rebuilt on the device, the same images), and the
// frame's line ends `, tables a ms, rearm b ms (device|host tables)` from pt_get_set_camera_times.
// --move G:DX,DY,DZ (with --orbit; works with --gpus / --devices and with --reproject): from frame 1 on the TRANS of geom G grows by the step
// before the camera moves — the scene's geom is placed again as the loader would (pt_scene_set_geom_trs' code) and the live renderer
// takes the new geoms (pt_set_geoms, pt_group_set_geoms).  Prints `move: frame f: geom G at x y z, set_geoms a ms`.  With --reproject
// the lookup follows the object (PT_HISTORY_MOTION).
// --reproject (with --orbit, excludes --gpus / --devices): the image is carried from view to view (pt_history_*).  After a frame's render
// comes pt_render_features(1, 1); from frame 1 on pt_history_reproject; pt_history_resolve, written next to the raw frame as
// <base>.orbit<fff>.reprojected.png (.pfm with --pfm); pt_history_capture; then the move.  --denoise-history (with --reproject, --spp >= 2;
// takes the --denoise-* options, sigma C's default being 8): a frame's iterations are rendered in groups of ceil(spp / 4) with
// pt_noise_fold after each, the lookup and the capture carry the variance (pt_history_*_ex with PT_HISTORY_VARIANCE), and after the
// resolve pt_history_denoise writes <base>.orbit<fff>.reprojected.denoised.png (.pfm); the history keeps the unfiltered blend.  Frame f renders iterations f * spp + 1 ..
// (f + 1) * spp instead of 1 .. spp (printed once).  --history-moments (with --denoise-history; --spp 1 is enough): the lookup and the
// capture carry the history's moments instead (PT_HISTORY_MOMENTS), the filter is pt_history_denoise_ex with them, and a frame is one
// pt_render call without folds; the same output names.  --history-cap C: PtHistoryOptions.cap (default 32).  Prints per frame
// `history: frame f: <valid> of <pixels> pixels carried, mean weight <x>`.
// --history-feedback (with --denoise-history --history-moments; composes with --history-extra, --move and --history-probe): the filtered
// image is fed back into the history (PT_HISTORY_FEEDBACK).  The lookup and the capture carry the flag and the filter is
// pt_history_denoise_feedback, so a frame's order is render, features, lookup, check, round, filter, capture, move; the same output
// names.  --feedback-level L (1 .. the filter's levels) and --feedback-variance V (the rule, 0 or 1): PtHistoryFeedbackOptions, whose
// defaults (pt_amd.h) are level 1, rule 1.  Prints once `feedback: the output of filter level <L> is fed back, variance rule <V>`.
// --history-until-db X (with --denoise-history; excludes --history-moments, --history-extra, --history-probe and --history-feedback): a
// view renders until the estimated PSNR of the BLEND with the carried history is above X (pt_history_render_until), --spp being the cap
// per view.  A frame's order becomes features, lookup, render, resolve, filter, capture, move, with the iterations the view took in
// `samples`; the same output names.  --history-until-group G: the iterations per group (default ceil(spp / 4); 0 = one batch).  Prints
// per frame `until: frame f: <iterations> iterations, <groups> groups, estimated PSNR of the blend <x> dB (the view alone <y> dB)`.
// --history-threshold E (with --denoise-history; excludes --history-until-db, --history-moments, --history-extra, --history-probe,
// --history-feedback and --gpus / --devices): a view is features, lookup, then pt_history_render_threshold — uniform groups until two are
// folded, then rounds over the pixels whose blend's standard error is above E, at most the fraction --history-threshold-cap F (default
// 0.25) of them, until at most --history-threshold-min-pixels P (default 0) are above or --spp iteration numbers are used, in groups of
// --history-threshold-group G (default ceil(spp / 4); 0 = one batch) — then pt_history_resolve_adaptive, pt_history_denoise_adaptive and
// pt_history_capture_adaptive; the same output names, the raw frame resolved by every pixel's own count.  Prints `threshold: frame f: ...`.
// --history-extra G (with --reproject, alone or with --denoise-history --history-moments; refused with --denoise-history alone, whose
// variance comes from the folds and knows nothing of extra samples): between the lookup and the resolve pt_history_round gives the
// pixels whose carried weight is below --history-min M (default 4) G further iterations, --history-extra-cap F of the frame at the
// most (default 1); resolve, filter and capture then count them per pixel.  Frame f takes spp + G iteration numbers: the uniform ones
// f (spp + G) + 1 .., then G for the round.  Prints per frame `history: frame f: <G> extra over <m> of <fresh> fresh pixels`.
// --recolor M:DR,DG,DB / --emit M:DE (with --orbit; each may stand where --move stands, and composes with it; works with --gpus / --devices;
// excludes --history-feedback): from frame 1 on the colour of material M grows by the step (--emit: its emittance by DE) before the camera
// moves, and the live renderer takes the new materials (pt_set_materials, pt_group_set_materials).  Prints `material: frame f: material M
// colour r g b emittance e, set_materials a ms`.  With --reproject the lookup passes PT_HISTORY_MATERIALS.
// --orbit-still (with --orbit N --move): the N frames keep the scene's camera — no pt_scene_orbit, no pt_set_camera between frames; only
// the object moves.  --history-probe (with --orbit N --orbit-still --move --reproject): the history probes (pt_history_probe_*).  A
// frame's order is render, features, lookup (with PT_HISTORY_MOTION), from frame 1 on pt_history_probe_check, then
// pt_history_probe_keep with phase f % 9 and the frame's own iteration range, the round if asked, resolve / filter, capture, move.
// --probe-radius R (0 .. 4) and --probe-gain X: PtHistoryProbeOptions (the defaults: pt_amd.h).  Prints per frame
// `probe: frame f: <changed> of <probes> probes changed, <skipped> skipped`.
// Output name: PREFIX.<spp>samp.png, or with --stamp the reference's own
// <FILE>.<UTC start time>.<spp>samp.png (main.cpp:99-102).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pathtrace_amd.hpp"
#include "pt_scene.h"

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("Usage: %s SCENEFILE.txt [--res WxH] [--spp N] [--depth D] [--out PREFIX] [--pfm] [--hdr] "
                "[--arith exact|fma|fast] [--gpus K | --devices LIST] [--transport rccl|copy] [--stamp] [--aa] [--orbit N [--device-tables] [--reproject [--history-cap C] [--denoise-history [--history-moments [--history-feedback [--feedback-level L] [--feedback-variance V]]] [--history-threshold E [--history-threshold-cap F] [--history-threshold-min-pixels P] [--history-threshold-group G]]] [--history-extra G [--history-min M] [--history-extra-cap F]] [--history-probe [--probe-radius R] [--probe-gain X]]] [--move G:DX,DY,DZ] [--recolor M:DR,DG,DB] [--emit M:DE] [--orbit-still]] [--preview N] "
                "[--convergence N | --reference FILE.pfm] [--clean-db X] [--features] "
                "[--denoise [--denoise-levels N] [--denoise-sigma C,N,P] [--denoise-keep-albedo]] [--denoise-guided] [--until-db X [--until-group G] [--adaptive F [--denoise-adaptive]]] "
                "[--adaptive-threshold E [--adaptive-cap F] [--adaptive-min-pixels P] [--until-group G] [--denoise-adaptive]]\n", argv[0]);
    return 1;
  }
  int rw = 0, rh = 0, spp = 0, depth = 0, gpus = -1, arith = PT_ARITH_EXACT, preview = 0, transport = PT_GROUP_TRANSPORT_AUTO;
  std::vector<int> device_list;
  bool pfm = false, hdr = false, stamp = false, aa = false, features = false, denoise = false, guided = false, dn_adaptive = false;
  PtDenoiseOptions dn_opt{};
  int convergence = 0, until_group = 0, orbit = 0;  // orbit > 0: --orbit N
  bool device_tables = false;                       // --device-tables
  bool move = false;                                // --move G:DX,DY,DZ
  int move_geom = 0;
  float move_step[3] = {0.0f, 0.0f, 0.0f};
  bool reproject = false;                           // --reproject
  bool dn_history = false;                          // --denoise-history
  bool hist_moments = false;                        // --history-moments
  bool hist_feedback = false;                       // --history-feedback
  PtHistoryFeedbackOptions fb_opt{};                // --feedback-level, --feedback-variance
  bool fb_opt_given = false;
  float history_cap = 0.0f;                         // --history-cap C (0: the default)
  bool history_cap_given = false;
  int history_extra = 0;                            // --history-extra G (0: no rounds)
  PtHistoryRoundOptions round_opt{};                // --history-min M, --history-extra-cap F (0: the defaults)
  bool history_min_given = false, history_extra_cap_given = false;
  bool orbit_still = false;                         // --orbit-still
  bool recolor = false, emit = false;               // --recolor M:DR,DG,DB, --emit M:DE
  int recolor_mat = 0, emit_mat = 0;
  float recolor_step[3] = {0.0f, 0.0f, 0.0f}, emit_step = 0.0f;
  bool history_probe = false;                       // --history-probe
  PtHistoryProbeOptions probe_opt{};                // --probe-radius R, --probe-gain X (0: the defaults)
  bool probe_opt_given = false;
  bool hist_until = false, hist_until_group_given = false;  // --history-until-db X, --history-until-group G
  bool hist_threshold = false;                      // --history-threshold E: threshold rounds keyed by the variance of the blend
  float hist_threshold_e = 0.0f, hist_threshold_cap = 0.25f;  // ... --history-threshold-cap F
  int hist_threshold_min_pixels = 0, hist_threshold_group = 0;  // ... --history-threshold-min-pixels P, --history-threshold-group G
  bool hist_threshold_cap_given = false, hist_threshold_min_given = false, hist_threshold_group_given = false;
  float hist_until_db = 0.0f;
  int hist_until_group = 0;
  bool until = false, until_group_given = false;
  float clean_db = 35.0f, until_db = 0.0f, adaptive = 0.0f;  // adaptive > 0: --adaptive F
  float threshold = 0.0f, threshold_cap = 0.25f;           // --adaptive-threshold E, --adaptive-cap F
  int threshold_min_pixels = 0;                            // --adaptive-min-pixels P
  bool by_threshold = false, threshold_cap_given = false, threshold_min_given = false;
  std::string out, reference;
  for (int i = 2; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--res") && i + 1 < argc) std::sscanf(argv[++i], "%dx%d", &rw, &rh);
    else if (!std::strcmp(argv[i], "--spp") && i + 1 < argc) spp = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--depth") && i + 1 < argc) depth = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--out") && i + 1 < argc) out = argv[++i];
    else if (!std::strcmp(argv[i], "--gpus") && i + 1 < argc) gpus = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--preview") && i + 1 < argc) preview = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--orbit") && i + 1 < argc) {
      char* end = nullptr;
      const long v = std::strtol(argv[++i], &end, 10);
      if (end == argv[i] || *end || v < 1 || v > 999) {
        std::fprintf(stderr, "--orbit wants the number of frames of a full turn around the scene, 1 to 999\n");
        return 1;
      }
      orbit = (int)v;
    }
    else if (!std::strcmp(argv[i], "--device-tables")) device_tables = true;
    else if (!std::strcmp(argv[i], "--move") && i + 1 < argc) {
      char tail = 0;
      if (std::sscanf(argv[++i], "%d:%f,%f,%f%c", &move_geom, &move_step[0], &move_step[1], &move_step[2], &tail) != 4 || move_geom < 0 ||
          !std::isfinite(move_step[0]) || !std::isfinite(move_step[1]) || !std::isfinite(move_step[2])) {
        std::fprintf(stderr, "--move wants G:DX,DY,DZ: the index of a geom and the step its TRANS takes from frame to frame, three finite numbers\n");
        return 1;
      }
      move = true;
    }
    else if (!std::strcmp(argv[i], "--reproject")) reproject = true;
    else if (!std::strcmp(argv[i], "--denoise-history")) dn_history = true;  // the blend filtered with the variance the history carries
    else if (!std::strcmp(argv[i], "--history-moments")) hist_moments = true;  // ... with the variance its moments give: no folds
    else if (!std::strcmp(argv[i], "--history-feedback")) hist_feedback = true;  // ... and its output fed back into the history
    else if (!std::strcmp(argv[i], "--history-until-db") && i + 1 < argc) {
      char* end = nullptr;
      hist_until_db = std::strtof(argv[++i], &end);
      if (end == argv[i] || *end || !std::isfinite(hist_until_db)) {
        std::fprintf(stderr, "--history-until-db wants the estimated PSNR of the blend in dB at which a view stops, a finite number\n");
        return 1;
      }
      hist_until = true;
    } else if (!std::strcmp(argv[i], "--history-until-group") && i + 1 < argc) {
      char* end = nullptr;
      const long v = std::strtol(argv[++i], &end, 10);
      if (end == argv[i] || *end || v < 0 || v > INT32_MAX) {
        std::fprintf(stderr, "--history-until-group wants the iterations per group of --history-until-db, G >= 0 (0 = one batch)\n");
        return 1;
      }
      hist_until_group = (int)v, hist_until_group_given = true;
    }
    else if (!std::strcmp(argv[i], "--history-threshold") && i + 1 < argc) {
      char* end = nullptr;
      hist_threshold_e = std::strtof(argv[++i], &end);
      if (end == argv[i] || *end || !std::isfinite(hist_threshold_e) || hist_threshold_e < 0.0f) {
        std::fprintf(stderr, "--history-threshold wants the standard error of the blend above which a pixel gets further samples, finite and >= 0\n");
        return 1;
      }
      hist_threshold = true;
    } else if (!std::strcmp(argv[i], "--history-threshold-cap") && i + 1 < argc) {
      char* end = nullptr;
      hist_threshold_cap = std::strtof(argv[++i], &end);
      if (end == argv[i] || *end || !(hist_threshold_cap > 0.0f && hist_threshold_cap <= 1.0f)) {
        std::fprintf(stderr, "--history-threshold-cap wants the largest fraction of the pixels a round renders, in (0, 1]\n");
        return 1;
      }
      hist_threshold_cap_given = true;
    } else if ((!std::strcmp(argv[i], "--history-threshold-min-pixels") || !std::strcmp(argv[i], "--history-threshold-group")) && i + 1 < argc) {
      const bool is_group = !std::strcmp(argv[i], "--history-threshold-group");
      char* end = nullptr;
      const long v = std::strtol(argv[++i], &end, 10);
      if (end == argv[i] || *end || v < 0 || v > INT32_MAX) {
        std::fprintf(stderr, "%s\n", is_group ? "--history-threshold-group wants the iterations per group and round of --history-threshold, G >= 0 (0 = one batch)"
                                              : "--history-threshold-min-pixels wants the pixels above the threshold at which a view stops, P >= 0");
        return 1;
      }
      if (is_group) hist_threshold_group = (int)v, hist_threshold_group_given = true;
      else hist_threshold_min_pixels = (int)v, hist_threshold_min_given = true;
    }
    else if ((!std::strcmp(argv[i], "--feedback-level") || !std::strcmp(argv[i], "--feedback-variance")) && i + 1 < argc) {
      const bool is_level = !std::strcmp(argv[i], "--feedback-level");
      char* end = nullptr;
      const long v = std::strtol(argv[++i], &end, 10);
      if (end == argv[i] || *end || v < (is_level ? 1 : 0) || v > (is_level ? 8 : 1)) {
        std::fprintf(stderr, is_level ? "--feedback-level wants the filter level whose output is fed back, 1 to the filter's levels\n"
                                      : "--feedback-variance wants 0 (the variance of the raw chain) or 1 (the one the filtered history carries)\n");
        return 1;
      }
      if (is_level) fb_opt.level = (int32_t)v;
      else fb_opt.variance = v ? 1 : -1;  // (the field: 0 = the default, -1 = rule 0)
      fb_opt_given = true;
    }
    else if (!std::strcmp(argv[i], "--history-cap") && i + 1 < argc) {
      history_cap = (float)std::atof(argv[++i]);
      history_cap_given = true;
      if (!std::isfinite(history_cap) || !(history_cap > 0.0f)) {
        std::fprintf(stderr, "--history-cap wants the most samples a carried colour counts for, a positive number\n");
        return 1;
      }
    }
    else if (!std::strcmp(argv[i], "--history-extra") && i + 1 < argc) {
      char* end = nullptr;
      const long v = std::strtol(argv[++i], &end, 10);
      if (end == argv[i] || *end || v < 1 || v > 4096) {
        std::fprintf(stderr, "--history-extra wants the iterations a pixel with a short history gets on top, 1 to 4096\n");
        return 1;
      }
      history_extra = (int)v;
    }
    else if (!std::strcmp(argv[i], "--history-min") && i + 1 < argc) {
      round_opt.min_history = (float)std::atof(argv[++i]);
      history_min_given = true;
      if (!std::isfinite(round_opt.min_history) || !(round_opt.min_history > 0.0f)) {
        std::fprintf(stderr, "--history-min wants the carried samples below which a pixel gets extra ones, a positive number\n");
        return 1;
      }
    }
    else if (!std::strcmp(argv[i], "--history-extra-cap") && i + 1 < argc) {
      round_opt.max_fraction = (float)std::atof(argv[++i]);
      history_extra_cap_given = true;
      if (!(round_opt.max_fraction > 0.0f && round_opt.max_fraction <= 1.0f)) {
        std::fprintf(stderr, "--history-extra-cap wants the largest share of the frame a round may render, in (0, 1]\n");
        return 1;
      }
    }
    else if (!std::strcmp(argv[i], "--orbit-still")) orbit_still = true;
    else if (!std::strcmp(argv[i], "--recolor") && i + 1 < argc) {
      char tail = 0;
      if (std::sscanf(argv[++i], "%d:%f,%f,%f%c", &recolor_mat, &recolor_step[0], &recolor_step[1], &recolor_step[2], &tail) != 4 || recolor_mat < 0 ||
          !std::isfinite(recolor_step[0]) || !std::isfinite(recolor_step[1]) || !std::isfinite(recolor_step[2])) {
        std::fprintf(stderr, "--recolor wants M:DR,DG,DB: the index of a material and the step its colour takes from frame to frame, three finite numbers\n");
        return 1;
      }
      recolor = true;
    } else if (!std::strcmp(argv[i], "--emit") && i + 1 < argc) {
      char tail = 0;
      if (std::sscanf(argv[++i], "%d:%f%c", &emit_mat, &emit_step, &tail) != 2 || emit_mat < 0 || !std::isfinite(emit_step)) {
        std::fprintf(stderr, "--emit wants M:DE: the index of a material and the step its emittance takes from frame to frame, a finite number\n");
        return 1;
      }
      emit = true;
    }
    else if (!std::strcmp(argv[i], "--history-probe")) history_probe = true;
    else if (!std::strcmp(argv[i], "--probe-radius") && i + 1 < argc) {
      char* end = nullptr;
      const long v = std::strtol(argv[++i], &end, 10);
      probe_opt_given = true;
      if (end == argv[i] || *end || v < 0 || v > 4) {
        std::fprintf(stderr, "--probe-radius wants the probe cells around a pixel's own whose probes shorten its history, 0 to 4\n");
        return 1;
      }
      probe_opt.radius = v == 0 ? -1 : (int32_t)v;  // (PtHistoryProbeOptions: 0 is the default, -1 radius 0)
    }
    else if (!std::strcmp(argv[i], "--probe-gain") && i + 1 < argc) {
      probe_opt.gain = (float)std::atof(argv[++i]);
      probe_opt_given = true;
      if (!std::isfinite(probe_opt.gain) || !(probe_opt.gain > 0.0f)) {
        std::fprintf(stderr, "--probe-gain wants the factor between a probe's relative difference and the share of history dropped, a positive number\n");
        return 1;
      }
    }
    else if (!std::strcmp(argv[i], "--convergence") && i + 1 < argc) {
      convergence = std::atoi(argv[++i]);
      if (convergence <= 0) {
        std::fprintf(stderr, "--convergence wants the iteration (>= 1) whose average becomes the reference frame\n");
        return 1;
      }
    } else if (!std::strcmp(argv[i], "--reference") && i + 1 < argc) reference = argv[++i];
    else if (!std::strcmp(argv[i], "--clean-db") && i + 1 < argc) clean_db = (float)std::atof(argv[++i]);
    else if (!std::strcmp(argv[i], "--devices") && i + 1 < argc) {
      for (const char* q = argv[++i]; *q;) {
        char* end = nullptr;
        device_list.push_back((int)std::strtol(q, &end, 10));
        if (end == q) {
          std::fprintf(stderr, "--devices wants a comma-separated list of device ordinals\n");
          return 1;
        }
        q = *end == ',' ? end + 1 : end;
      }
      gpus = (int)device_list.size();
    } else if (!std::strcmp(argv[i], "--transport") && i + 1 < argc) {
      const char* a = argv[++i];
      if (!std::strcmp(a, "rccl")) transport = PT_GROUP_TRANSPORT_RCCL;
      else if (!std::strcmp(a, "copy")) transport = PT_GROUP_TRANSPORT_COPY;
      else {
        std::fprintf(stderr, "unknown transport %s\n", a);
        return 1;
      }
    }
    else if (!std::strcmp(argv[i], "--pfm")) pfm = true;
    else if (!std::strcmp(argv[i], "--hdr")) hdr = true;  // the Radiance file of image::saveHDR (main.cpp:106, commented out there)
    else if (!std::strcmp(argv[i], "--stamp")) stamp = true;
    else if (!std::strcmp(argv[i], "--features")) features = true;  // first-hit feature buffers next to the image
    else if (!std::strcmp(argv[i], "--denoise")) denoise = true;    // the filtered image next to the image
    else if (!std::strcmp(argv[i], "--denoise-guided")) guided = true;  // ... by the variance-guided form of the filter
    else if (!std::strcmp(argv[i], "--denoise-adaptive")) dn_adaptive = true;  // ... by the form that reads per-pixel sample counts
    else if (!std::strcmp(argv[i], "--denoise-keep-albedo")) dn_opt.keep_albedo = 1;
    else if (!std::strcmp(argv[i], "--denoise-levels") && i + 1 < argc) {
      char* end = nullptr;
      const long v = std::strtol(argv[++i], &end, 10);
      if (end == argv[i] || *end || v < 1 || v > 8) {
        std::fprintf(stderr, "--denoise-levels wants a number of levels from 1 to 8\n");
        return 1;
      }
      dn_opt.levels = (int)v;
    } else if (!std::strcmp(argv[i], "--denoise-sigma") && i + 1 < argc) {
      char tail = 0;
      const int got = std::sscanf(argv[++i], "%f,%f,%f%c", &dn_opt.sigma_color, &dn_opt.sigma_normal, &dn_opt.sigma_position, &tail);
      if (got != 3 || !std::isfinite(dn_opt.sigma_color) || !std::isfinite(dn_opt.sigma_normal) || !std::isfinite(dn_opt.sigma_position)) {
        std::fprintf(stderr, "--denoise-sigma wants three finite numbers C,N,P (colour, normal, position; 0 = default, negative = off)\n");
        return 1;
      }
    }
    else if (!std::strcmp(argv[i], "--until-db") && i + 1 < argc) {
      char* end = nullptr;
      until_db = std::strtof(argv[++i], &end);
      if (end == argv[i] || *end || !std::isfinite(until_db)) {
        std::fprintf(stderr, "--until-db wants the estimated PSNR in dB at which to stop, a finite number\n");
        return 1;
      }
      until = true;
    } else if (!std::strcmp(argv[i], "--until-group") && i + 1 < argc) {
      char* end = nullptr;
      const long v = std::strtol(argv[++i], &end, 10);
      if (end == argv[i] || *end || v < 0 || v > INT32_MAX) {
        std::fprintf(stderr, "--until-group wants the iterations per group of --until-db (0 = one batch)\n");
        return 1;
      }
      until_group = (int)v, until_group_given = true;
    }
    else if (!std::strcmp(argv[i], "--adaptive") && i + 1 < argc) {
      char* end = nullptr;
      adaptive = std::strtof(argv[++i], &end);
      if (end == argv[i] || *end || !(adaptive > 0.0f && adaptive <= 1.0f)) {
        std::fprintf(stderr, "--adaptive wants the fraction of the pixels a round samples, 0 < F <= 1\n");
        return 1;
      }
    }
    else if (!std::strcmp(argv[i], "--adaptive-threshold") && i + 1 < argc) {
      char* end = nullptr;
      threshold = std::strtof(argv[++i], &end);
      if (end == argv[i] || *end || !std::isfinite(threshold) || threshold < 0.0f) {
        std::fprintf(stderr, "--adaptive-threshold wants the standard error below which a pixel is left alone, a finite number >= 0\n");
        return 1;
      }
      by_threshold = true;
    } else if (!std::strcmp(argv[i], "--adaptive-cap") && i + 1 < argc) {
      char* end = nullptr;
      threshold_cap = std::strtof(argv[++i], &end);
      if (end == argv[i] || *end || !(threshold_cap > 0.0f && threshold_cap <= 1.0f)) {
        std::fprintf(stderr, "--adaptive-cap wants the largest fraction of the pixels a round samples, 0 < F <= 1\n");
        return 1;
      }
      threshold_cap_given = true;
    } else if (!std::strcmp(argv[i], "--adaptive-min-pixels") && i + 1 < argc) {
      char* end = nullptr;
      const long v = std::strtol(argv[++i], &end, 10);
      if (end == argv[i] || *end || v < 0 || v > INT32_MAX) {
        std::fprintf(stderr, "--adaptive-min-pixels wants the number of pixels above the threshold at which to stop, >= 0\n");
        return 1;
      }
      threshold_min_pixels = (int)v, threshold_min_given = true;
    }
    else if (!std::strcmp(argv[i], "--aa")) aa = true;  // extension: stochastic anti-aliasing (PtOptions.aa_jitter)
    else if (!std::strcmp(argv[i], "--arith") && i + 1 < argc) {
      const char* a = argv[++i];
      if (!std::strcmp(a, "exact")) arith = PT_ARITH_EXACT;
      else if (!std::strcmp(a, "fma")) arith = PT_ARITH_FMA;
      else if (!std::strcmp(a, "fast")) arith = PT_ARITH_FAST;
      else {
        std::fprintf(stderr, "unknown arithmetic mode %s\n", a);
        return 1;
      }
    } else {
      std::fprintf(stderr, "unknown argument %s\n", argv[i]);
      return 1;
    }
  }
  if (convergence > 0 && !reference.empty()) {
    std::fprintf(stderr, "--convergence and --reference exclude each other (one reference frame)\n");
    return 1;
  }
  if (!reference.empty()) convergence = -1;
  if (denoise && guided) {
    std::fprintf(stderr, "--denoise and --denoise-guided exclude each other (one filtered image)\n");
    return 1;
  }
  if (dn_adaptive && (denoise || guided)) {
    std::fprintf(stderr, "--denoise-adaptive excludes --denoise and --denoise-guided (one filtered image)\n");
    return 1;
  }
  if (dn_adaptive && !(adaptive > 0.0f) && !by_threshold) {
    std::fprintf(stderr, "--denoise-adaptive wants --adaptive or --adaptive-threshold (the filter of an adaptively sampled image)\n");
    return 1;
  }
  if ((hist_threshold_cap_given || hist_threshold_min_given || hist_threshold_group_given) && !hist_threshold) {
    std::fprintf(stderr, "%s wants --history-threshold E (the threshold rounds it configures)\n",
                 hist_threshold_cap_given ? "--history-threshold-cap" : hist_threshold_min_given ? "--history-threshold-min-pixels" : "--history-threshold-group");
    return 1;
  }
  if (hist_threshold && !dn_history) {
    std::fprintf(stderr, "--history-threshold wants --orbit N --reproject --denoise-history (its rounds are keyed by the variance the history carries)\n");
    return 1;
  }
  if (hist_threshold && (hist_until || hist_moments || history_extra || history_probe || hist_feedback || gpus >= 0 || !device_list.empty())) {
    std::fprintf(stderr, "--history-threshold excludes %s: threshold rounds over the blend are built for the variance kind of history on one context\n",
                 hist_until ? "--history-until-db" : hist_feedback ? "--history-feedback" : history_probe ? "--history-probe" : history_extra ? "--history-extra"
                 : hist_moments ? "--history-moments" : "--gpus / --devices");
    return 1;
  }
  if (hist_until_group_given && !hist_until) {
    std::fprintf(stderr, "--history-until-group wants --history-until-db (the estimated PSNR of the blend at which a view stops)\n");
    return 1;
  }
  if (hist_until && !dn_history) {
    std::fprintf(stderr, "--history-until-db wants --orbit N --reproject --denoise-history (it stops a view on the variance the history carries)\n");
    return 1;
  }
  if (hist_until && (hist_moments || history_extra || history_probe || hist_feedback)) {
    std::fprintf(stderr, "--history-until-db excludes %s: the estimate of the blend's noise is built for the variance kind of history over uniform samples\n",
                 hist_feedback ? "--history-feedback" : history_probe ? "--history-probe" : history_extra ? "--history-extra" : "--history-moments");
    return 1;
  }
  if (dn_history && (orbit <= 0 || !reproject)) {
    std::fprintf(stderr, "--denoise-history wants --orbit N --reproject (it filters the blend of the view with the reprojected history)\n");
    return 1;
  }
  if (hist_moments && !dn_history) {
    std::fprintf(stderr, "--history-moments wants --denoise-history (it chooses what the filter over the blend takes its variance from)\n");
    return 1;
  }
  if (hist_feedback && !hist_moments) {
    std::fprintf(stderr, "--history-feedback wants --history-moments (the filtered colour travels beside the history's moments)\n");
    return 1;
  }
  if (fb_opt_given && !hist_feedback) {
    std::fprintf(stderr, "--feedback-level and --feedback-variance want --history-feedback\n");
    return 1;
  }
  if (!denoise && !guided && !dn_adaptive && !dn_history && (dn_opt.levels || dn_opt.keep_albedo || dn_opt.sigma_color != 0.0f || dn_opt.sigma_normal != 0.0f || dn_opt.sigma_position != 0.0f)) {
    std::fprintf(stderr, "--denoise-levels, --denoise-sigma and --denoise-keep-albedo want --denoise, --denoise-guided, --denoise-adaptive or --denoise-history\n");
    return 1;
  }
  if (denoise || guided || dn_adaptive) features = true;
  if (until_group_given && !until && !guided && !by_threshold) {
    std::fprintf(stderr, "--until-group wants --until-db, --denoise-guided or --adaptive-threshold\n");
    return 1;
  }
  if (guided && preview > 0) {
    std::fprintf(stderr, "--denoise-guided and --preview exclude each other (one loop over the iterations)\n");
    return 1;
  }
  if (adaptive > 0.0f) {
    if (!until) {
      std::fprintf(stderr, "--adaptive wants --until-db (the estimated PSNR at which to stop)\n");
      return 1;
    }
    if (gpus >= 0 || denoise || guided || convergence != 0 || preview > 0) {
      std::fprintf(stderr, "--adaptive excludes --gpus / --devices, --denoise, --denoise-guided, --convergence, --reference and --preview\n");
      return 1;
    }
  }
  if ((threshold_cap_given || threshold_min_given) && !by_threshold) {
    std::fprintf(stderr, "--adaptive-cap and --adaptive-min-pixels want --adaptive-threshold\n");
    return 1;
  }
  if (by_threshold && (adaptive > 0.0f || until || gpus >= 0 || denoise || guided || convergence != 0 || preview > 0)) {
    std::fprintf(stderr, "--adaptive-threshold excludes --adaptive, --until-db, --gpus / --devices, --denoise, --denoise-guided, --convergence, --reference and --preview\n");
    return 1;
  }
  const bool adaptive_mode = adaptive > 0.0f || by_threshold;  // the image is the resolved one, the samples are counted
  if (until && preview > 0) {
    std::fprintf(stderr, "--until-db and --preview exclude each other (one loop over the iterations)\n");
    return 1;
  }
  if (device_tables && orbit <= 0) {
    std::fprintf(stderr, "--device-tables goes with --orbit N (it says how the camera moves rebuild the scene tables)\n");
    return 1;
  }
  if (move && orbit <= 0) {
    std::fprintf(stderr, "--move goes with --orbit N (it moves an object of the live renderer from frame to frame)\n");
    return 1;
  }
  if ((reproject && orbit <= 0) || (history_cap_given && !reproject)) {
    std::fprintf(stderr, "--reproject goes with --orbit N (it carries the image from view to view), --history-cap C with --reproject\n");
    return 1;
  }
  if ((history_min_given || history_extra_cap_given) && !history_extra) {
    std::fprintf(stderr, "--history-min and --history-extra-cap go with --history-extra G\n");
    return 1;
  }
  if (history_extra && (orbit <= 0 || !reproject)) {
    std::fprintf(stderr, "--history-extra wants --orbit N --reproject (it gives extra samples to the pixels whose reprojected history is short)\n");
    return 1;
  }
  if (history_extra && dn_history && !hist_moments) {
    std::fprintf(stderr, "--history-extra excludes --denoise-history without --history-moments: the folds' variance knows nothing of the extra samples\n");
    return 1;
  }
  if ((recolor || emit) && orbit <= 0) {
    std::fprintf(stderr, "%s goes with --orbit N (it edits a material of the live renderer from frame to frame)\n", recolor ? "--recolor" : "--emit");
    return 1;
  }
  if ((recolor || emit) && hist_feedback) {
    std::fprintf(stderr, "%s excludes --history-feedback: the recolour step (PT_HISTORY_MATERIALS) is not built beside the feedback kind\n", recolor ? "--recolor" : "--emit");
    return 1;
  }
  if (orbit_still && !move && !recolor && !emit) {
    std::fprintf(stderr, "--orbit-still wants --orbit N --move G:DX,DY,DZ (with the camera standing still and nothing moving every frame would be the same)\n");
    return 1;
  }
  if (probe_opt_given && !history_probe) {
    std::fprintf(stderr, "--probe-radius and --probe-gain go with --history-probe\n");
    return 1;
  }
  if (history_probe && (!reproject || !(move || recolor || emit) || !orbit_still)) {
    std::fprintf(stderr, "--history-probe wants %s (it renders kept samples again after an object moved; the probes answer for a camera that stands still)\n",
                 !reproject ? "--reproject" : !(move || recolor || emit) ? "--move G:DX,DY,DZ" : "--orbit-still");
    return 1;
  }
  if (reproject && (gpus >= 0 || !device_list.empty())) {
    std::fprintf(stderr, "--reproject excludes --gpus / --devices: a context's interleaved rows cannot look up their neighbours in the previous view\n");
    return 1;
  }
  if (orbit > 0) {  // a plain render per frame: what works on the image of one view is not carried from view to view (but --reproject)
    const struct {
      bool given;
      const char* name;
    } excluded[] = {{preview > 0, "--preview"}, {convergence > 0, "--convergence"}, {!reference.empty(), "--reference"}, {denoise, "--denoise"},
                    {guided, "--denoise-guided"}, {dn_adaptive, "--denoise-adaptive"}, {features, "--features"}, {until, "--until-db"},
                    {until_group_given, "--until-group"}, {adaptive > 0.0f, "--adaptive"}, {by_threshold, "--adaptive-threshold"},
                    {threshold_cap_given, "--adaptive-cap"}, {threshold_min_given, "--adaptive-min-pixels"}};
    for (const auto& e : excluded)
      if (e.given) {
        std::fprintf(stderr, "--orbit excludes %s (it renders --spp iterations per frame and writes the image; allowed: --res --spp --depth --arith --aa --pfm --hdr --out "
                             "--stamp --gpus / --devices --transport)\n", e.name);
        return 1;
      }
  }
  pt::Scene* scene = nullptr;
  try {
    scene = new pt::Scene(argv[1]);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  if (rw > 0 && rh > 0) scene->overrideResolution(rw, rh);
  if (spp > 0) scene->state.iterations = spp;
  if (depth > 0) scene->state.traceDepth = depth;
  scene->applyInitialCameraState();
  if (move && ((size_t)move_geom >= scene->geoms.size() || scene->geom_trs[(size_t)move_geom].mesh)) {
    std::fprintf(stderr, "--move: geom %d is %s\n", move_geom,
                 (size_t)move_geom >= scene->geoms.size() ? "outside the scene's geoms" : "a triangle of a mesh object, which has no TRANS of its own");
    return 1;
  }
  if ((recolor && (size_t)recolor_mat >= scene->materials.size()) || (emit && (size_t)emit_mat >= scene->materials.size())) {
    const bool first = recolor && (size_t)recolor_mat >= scene->materials.size();
    std::fprintf(stderr, "%s: material %d is outside the scene's %zu materials\n", first ? "--recolor" : "--emit", first ? recolor_mat : emit_mat, scene->materials.size());
    return 1;
  }
  const int W = scene->state.camera.resolution[0], H = scene->state.camera.resolution[1];
  int iters = (int)scene->state.iterations;  // with --until-db the cap, until the render has said how many it took
  if (guided && iters < 2) {
    std::fprintf(stderr, "--denoise-guided wants at least 2 iterations (--spp): a variance needs two groups\n");
    return 1;
  }
  if (dn_history && !hist_moments && iters < 2) {
    std::fprintf(stderr, "--denoise-history wants at least 2 iterations (--spp): a variance needs two groups per view\n");
    return 1;
  }
  // --denoise-guided without --until-db: the iterations in groups of G (default ceil(spp / 4)), a fold after each
  const int fold_group = until_group > 0 ? until_group : (iters + 3) / 4;
  if (out.empty()) out = scene->state.imageName;
  std::string base;
  auto name_outputs = [&]() {
    base = out + "." + std::to_string(iters) + "samp";
    if (stamp) {
      char buf[1024];
      pt_output_basename(out.c_str(), iters, buf, sizeof buf);  // (one start time per process)
      base = buf;
    }
  };
  name_outputs();
  // --until-db: what the render took and what it reached; everything after it speaks of the iterations actually rendered
  auto report_noise = [&](int done, int groups, float psnr) {
    std::printf("noise: %d iterations, %d groups, estimated PSNR %.9g dB\n", done, groups, (double)psnr);
    iters = done;
    scene->state.iterations = done;
    name_outputs();
  };

  std::vector<float> ref_frame;  // --reference: W * H averaged radiance
  if (!reference.empty()) {
    int fw = 0, fh = 0;
    if (pt_load_pfm(reference.c_str(), nullptr, 0, &fw, &fh, 1.0f) || fw != W || fh != H) {
      std::fprintf(stderr, "--reference %s: not a PFM image of %dx%d\n", reference.c_str(), W, H);
      return 1;
    }
    ref_frame.resize((size_t)W * H * 3);
    if (pt_load_pfm(reference.c_str(), ref_frame.data(), W * H, &fw, &fh, 1.0f)) {
      std::fprintf(stderr, "--reference %s: cannot read the pixels\n", reference.c_str());
      return 1;
    }
  }
  // the curve after the render: `iteration psnr_db` per line, then the iterations to clean
  auto print_curve = [&](const std::vector<float>& psnr, int clean) {
    for (int it = 1; it <= iters; ++it) {
      if (psnr[it - 1] == FLT_MAX) std::printf("%d Inf\n", it);
      else std::printf("%d %.9g\n", it, psnr[it - 1]);
    }
    std::printf("Iterations to clean: %d\n", clean);
  };

  // --features: the SUM planes (pt_readback_features' layout for the whole frame) as four three-channel PFM files
  auto save_features = [&](const std::vector<float>& planes) {
    const size_t n = (size_t)W * H;
    std::vector<float> rgb(3 * n);
    const struct { const char* name; int plane; bool w_only; } files[] = {{"normal", 0, false}, {"albedo", 1, false}, {"position", 2, false}, {"depth", 0, true}};
    for (const auto& f : files) {
      const float* src = planes.data() + 4 * n * f.plane;
      for (size_t p = 0; p < n; ++p)
        for (int c = 0; c < 3; ++c) rgb[3 * p + c] = src[4 * p + (f.w_only ? 3 : c)];
      const std::string path = base + "." + f.name + ".pfm";
      if (pt_save_pfm(path.c_str(), rgb.data(), W, H, (float)iters) == 0) std::printf("Saved %s.\n", path.c_str());
    }
  };

  // --denoise: the averaged, filtered frame through the writers of the image (samples = 1: it is no SUM)
  auto save_denoised = [&](const std::vector<float>& rgb) {
    if (pt_save_png((base + ".denoised.png").c_str(), rgb.data(), W, H, 1.0f) == 0) std::printf("Saved %s.denoised.png.\n", base.c_str());
    if (pfm && pt_save_pfm((base + ".denoised.pfm").c_str(), rgb.data(), W, H, 1.0f) == 0) std::printf("Saved %s.denoised.pfm.\n", base.c_str());
  };

  double secs = 0;
  if (orbit > 0) {
    // --orbit N: one renderer (or group), N views.  Frame 0 is the scene's camera through init; frame f > 0 follows a drag of 2 pi / N
    // (pt::Scene::orbit, the viewer's mouse rule) and pt_set_camera / pt_group_set_camera where the viewer would free and init.
    PtOptions opt{};
    opt.arith = arith;
    opt.aa_jitter = aa ? 1 : 0;
    PtGroup* grp = nullptr;
    std::vector<int> devices;
    if (gpus >= 0) {
      int ndev = 0;
      if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        std::fprintf(stderr, "no HIP device\n");
        return 1;
      }
      if (gpus == 0) gpus = ndev;
      if (device_list.empty() && gpus > ndev) {
        std::fprintf(stderr, "--gpus %d but only %d device(s) visible\n", gpus, ndev);
        return 1;
      }
      for (int i = 0; i < gpus; ++i) devices.push_back(device_list.empty() ? i : device_list[i]);
      for (int d : devices)
        if (d < 0 || d >= ndev) {
          std::fprintf(stderr, "device %d named but only %d device(s) visible\n", d, ndev);
          return 1;
        }
    }
    const PtSceneDesc desc = scene->desc();
    if (gpus >= 0 ? pt_group_create_ex(&desc, &opt, devices.data(), gpus, transport, &grp) : pt_init(&desc, &opt)) {
      std::fprintf(stderr, "HIP error (pt_init): %s\n", pt_last_error());
      return EXIT_FAILURE;
    }
    PtSetupTimes st{};
    if (grp ? pt_ctx_get_setup_times(pt_group_context(grp, 0), &st) : pt_get_setup_times(&st)) {
      std::fprintf(stderr, "HIP error (pt_get_setup_times): %s\n", pt_last_error());
      return EXIT_FAILURE;
    }
    std::printf("setup: tables %.3f ms, upload %.3f ms, buffers %.3f ms, probe %.3f ms\n", st.tables_ms, st.upload_ms, st.buffers_ms, st.probe_ms);
    scene->state.image.resize((size_t)W * H * 3);
    // --reproject: the history of the views before (pt_history_*).  The RNG is keyed by (iteration, pixel): the same iteration numbers
    // after a small move would repeat almost the same paths, and the history would add nothing — every frame gets numbers of its own.
    std::vector<float> carried, current, filtered;
    PtHistoryOptions hopt{};
    hopt.cap = history_cap;
    if (reproject) {
      if ((int64_t)orbit * (iters + history_extra) > INT32_MAX) {
        std::fprintf(stderr, "--reproject: %d frames of %d iterations run out of iteration numbers\n", orbit, iters);
        return 1;
      }
      carried.resize((size_t)W * H * 3);
      current.resize((size_t)W * H * 4);
      if (dn_history) filtered.resize((size_t)W * H * 3);
      if (hist_feedback) std::printf("feedback: the output of filter level %d is fed back, variance rule %d\n", fb_opt.level ? fb_opt.level : PT_HISTORY_FEEDBACK_LEVEL,
                                     fb_opt.variance ? (fb_opt.variance > 0 ? 1 : 0) : PT_HISTORY_FEEDBACK_VARIANCE);
      if (history_extra)
        std::printf("history: frame f renders iterations f * %d + 1 .. f * %d + %d, then %d more for the pixels whose history is short\n", iters + history_extra,
                    iters + history_extra, iters, history_extra);
      else
        std::printf("history: frame f renders iterations f * %d + 1 .. (f + 1) * %d, not 1 .. %d: repeated iteration numbers would repeat the paths\n", iters, iters, iters);
    }
    const float step = (float)(2.0 * 3.14159265358979323846 / orbit);
    const uint32_t edit_flag = (recolor || emit) ? PT_HISTORY_MATERIALS : 0u;  // the lookup follows the edited material
    for (int f = 0; f < orbit; ++f) {
      double move_ms = 0.0;
      PtSetCameraTimes ct{};
      if (f > 0 && move) {  // the object first, then the camera: TRANS grows by the step, the live renderer takes the new geoms
        float trs[9];
        std::memcpy(trs, scene->geom_trs[(size_t)move_geom].trs, sizeof trs);
        for (int k = 0; k < 3; ++k) trs[k] += move_step[k];
        scene->placeGeom(move_geom, trs);
        const auto g0 = std::chrono::high_resolution_clock::now();
        if (grp ? pt_group_set_geoms(grp, scene->geoms.data(), (int)scene->geoms.size()) : pt_set_geoms(scene->geoms.data(), (int)scene->geoms.size())) {
          std::fprintf(stderr, "HIP error (pt_set_geoms): %s\n", pt_last_error());
          return EXIT_FAILURE;
        }
        const double geoms_ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - g0).count();
        std::printf("move: frame %d: geom %d at %.9g %.9g %.9g, set_geoms %.3f ms\n", f, move_geom, (double)trs[0], (double)trs[1], (double)trs[2], geoms_ms);
      }
      if (f > 0 && (recolor || emit)) {  // ... and the material: its colour or its emittance grows by the step, the live renderer takes the new materials
        for (int pass = 0; pass < 2; ++pass) {  // through pt_scene_set_material's code, which refuses a word that is not finite
          if (!(pass == 0 ? recolor : emit)) continue;
          const int mi = pass == 0 ? recolor_mat : emit_mat;
          PtMaterial m = scene->materials[(size_t)mi];
          if (pass == 0)
            for (int k = 0; k < 3; ++k) m.color[k] += recolor_step[k];
          else
            m.emittance += emit_step;
          if (!scene->setMaterial(mi, m)) {
            std::fprintf(stderr, "%s: at frame %d material %d has a word that is not finite\n", pass == 0 ? "--recolor" : "--emit", f, mi);
            return EXIT_FAILURE;
          }
        }
        const auto g0 = std::chrono::high_resolution_clock::now();
        if (grp ? pt_group_set_materials(grp, scene->materials.data(), (int)scene->materials.size()) : pt_set_materials(scene->materials.data(), (int)scene->materials.size())) {
          std::fprintf(stderr, "HIP error (pt_set_materials): %s\n", pt_last_error());
          return EXIT_FAILURE;
        }
        const double materials_ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - g0).count();
        for (const auto& e : {std::make_pair(recolor, recolor_mat), std::make_pair(emit && !(recolor && emit_mat == recolor_mat), emit_mat)})
          if (e.first) {
            const PtMaterial& m = scene->materials[(size_t)e.second];
            std::printf("material: frame %d: material %d colour %.9g %.9g %.9g emittance %.9g, set_materials %.3f ms\n", f, e.second, (double)m.color[0], (double)m.color[1],
                        (double)m.color[2], (double)m.emittance, materials_ms);
          }
      }
      if (f > 0 && !orbit_still) {
        scene->orbit(step, 0.0f, 0.0f);
        const uint32_t flags = device_tables ? PT_SET_CAMERA_DEVICE_TABLES : 0u;
        const auto m0 = std::chrono::high_resolution_clock::now();
        if (device_tables ? (grp ? pt_group_set_camera_ex(grp, &scene->state.camera, flags) : pt_set_camera_ex(&scene->state.camera, flags))
                          : (grp ? pt_group_set_camera(grp, &scene->state.camera) : pt_set_camera(&scene->state.camera))) {
          std::fprintf(stderr, "HIP error (pt_set_camera): %s\n", pt_last_error());
          return EXIT_FAILURE;
        }
        move_ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - m0).count();
        if (device_tables && (grp ? pt_ctx_get_set_camera_times(pt_group_context(grp, 0), &ct) : pt_get_set_camera_times(&ct))) {
          std::fprintf(stderr, "HIP error (pt_get_set_camera_times): %s\n", pt_last_error());
          return EXIT_FAILURE;
        }
      }
      const auto t0 = std::chrono::high_resolution_clock::now();
      const int iter_first = reproject ? f * (iters + history_extra) + 1 : 1;
      bool render_failed = false;
      int frame_iters = iters;  // --history-until-db: what the view took
      int until_groups = 0;
      float until_psnr = -1.0f, until_view_psnr = -1.0f;
      int64_t thr_samples = 0;  // --history-threshold: the pixel-samples of the view, the pixels above at the last count, the rounds
      int thr_above = -1, thr_groups = 0;
      if (hist_threshold) {  // features, lookup, then uniform groups until two are folded and rounds over the pixels whose BLEND is above the threshold
        render_failed = pt_render_features(1, 1) || (f > 0 && pt_history_reproject_ex(&hopt, PT_HISTORY_VARIANCE | (move ? PT_HISTORY_MOTION : 0u) | edit_flag)) ||
                        pt_history_render_threshold(iter_first, iters, hist_threshold_group_given ? hist_threshold_group : fold_group, hist_threshold_e,
                                                    hist_threshold_cap, hist_threshold_min_pixels, &frame_iters, &thr_samples, &thr_above) ||
                        pt_get_noise(nullptr, &thr_groups, nullptr) || pt_resolve(scene->state.image.data());
      } else if (hist_until) {  // the lookup needs the view's first hits only: features, lookup, then groups until the BLEND is clean
        render_failed = pt_render_features(1, 1) || (f > 0 && pt_history_reproject_ex(&hopt, PT_HISTORY_VARIANCE | (move ? PT_HISTORY_MOTION : 0u) | edit_flag)) ||
                        pt_history_render_until(iter_first, iters, hist_until_group_given ? hist_until_group : fold_group, hist_until_db, &frame_iters, &until_psnr,
                                                &until_view_psnr) ||
                        pt_get_noise(nullptr, &until_groups, nullptr) || pt_readback(scene->state.image.data());
      } else if (dn_history && !hist_moments) {  // the view's iterations in groups of ceil(spp / 4), a fold after each: the variance of the view's own samples
        for (int done = 0; done < iters && !render_failed; done += fold_group)
          render_failed = pt_render(iter_first + done, std::min(fold_group, iters - done)) || pt_noise_fold();
        render_failed = render_failed || pt_readback(scene->state.image.data());
      } else {
        render_failed = grp ? (pt_group_render(grp, 1, iters) || pt_group_gather(grp, scene->state.image.data()))
                            : (pt_render(iter_first, iters) || pt_readback(scene->state.image.data()));
      }
      if (render_failed) {
        std::fprintf(stderr, "HIP error (pt_render): %s\n", pt_last_error());
        return EXIT_FAILURE;
      }
      const double render_ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - t0).count();
      const float* p = scene->state.camera.position;
      std::printf("orbit: frame %d: camera %.9g %.9g %.9g, set_camera %.3f ms, render %.3f ms", f, (double)p[0], (double)p[1], (double)p[2], move_ms, render_ms);
      if (device_tables && f > 0) std::printf(", tables %.3f ms, rearm %.3f ms (%s tables)", ct.tables_ms, ct.rearm_ms, ct.path ? "device" : "host");
      std::printf("\n");
      char tag[32];
      std::snprintf(tag, sizeof tag, ".orbit%03d", f);
      const std::string frame = base + tag;
      const float frame_scale = hist_threshold ? 1.0f : (float)frame_iters;  // --history-threshold: the image was resolved by every pixel's own count
      if (pt_save_png((frame + ".png").c_str(), scene->state.image.data(), W, H, frame_scale) == 0) std::printf("Saved %s.png.\n", frame.c_str());
      if (pfm && pt_save_pfm((frame + ".pfm").c_str(), scene->state.image.data(), W, H, frame_scale) == 0) std::printf("Saved %s.pfm.\n", frame.c_str());
      if (hdr && pt_save_hdr((frame + ".hdr").c_str(), scene->state.image.data(), W, H, frame_scale) == 0) std::printf("Saved %s.hdr.\n", frame.c_str());
      if (reproject) {  // the view's first hits, the history looked up from them, the blend written, the blend kept for the next view
        const uint32_t hflags = !dn_history     ? 0u  // 0: the plain calls
                                : hist_feedback ? PT_HISTORY_MOMENTS | PT_HISTORY_FEEDBACK
                                : hist_moments  ? PT_HISTORY_MOMENTS
                                                : PT_HISTORY_VARIANCE;
        int fresh = 0, selected = 0;  // --history-extra: the round, between the lookup and the resolve
        int probes = 0, changed = 0, skipped = 0;  // --history-probe: the check after the lookup, the keep before the round
        double thr_sse = -1.0;
        // (--history-until-db, --history-threshold: the features and the lookup came before the render)
        if (hist_threshold) {  // the steps that read every pixel's own count
          if (pt_history_resolve_adaptive(carried.data()) || pt_history_denoise_adaptive(&dn_opt, filtered.data()) || pt_history_noise_adaptive(&thr_sse) ||
              pt_history_capture_adaptive() || pt_readback_history(nullptr, current.data())) {
            std::fprintf(stderr, "HIP error (pt_history): %s\n", pt_last_error());
            return EXIT_FAILURE;
          }
        } else if ((!hist_until && (pt_render_features(1, 1) || (f > 0 && pt_history_reproject_ex(&hopt, hflags | (move ? PT_HISTORY_MOTION : 0u) | edit_flag)))) ||
            (history_probe && ((f > 0 && pt_history_probe_check(&probe_opt, &probes, &changed, &skipped)) || pt_history_probe_keep(iter_first, iters, f % 9))) ||
            (history_extra && pt_history_round(iter_first + iters, history_extra, &round_opt, &fresh, &selected)) || pt_history_resolve((float)frame_iters, carried.data()) ||
            (dn_history && (hist_feedback  ? pt_history_denoise_feedback((float)frame_iters, &dn_opt, &fb_opt, filtered.data())
                            : hist_moments ? pt_history_denoise_ex((float)frame_iters, &dn_opt, PT_HISTORY_MOMENTS, filtered.data())
                                           : pt_history_denoise((float)frame_iters, &dn_opt, filtered.data()))) || pt_history_capture_ex((float)frame_iters, hflags) ||
            pt_readback_history(nullptr, current.data())) {
          std::fprintf(stderr, "HIP error (pt_history): %s\n", pt_last_error());
          return EXIT_FAILURE;
        }
        size_t valid = 0;
        double weight = 0.0;
        for (size_t p = 0; p < (size_t)W * H; ++p)
          if (current[4 * p + 3] > 0.0f) valid += 1, weight += (double)current[4 * p + 3];
        std::printf("history: frame %d: %zu of %zu pixels carried, mean weight %.3f\n", f, valid, (size_t)W * H, valid ? weight / (double)valid : 0.0);
        if (hist_until)
          std::printf("until: frame %d: %d iterations, %d groups, estimated PSNR of the blend %.9g dB (the view alone %.9g dB)\n", f, frame_iters, until_groups,
                      (double)until_psnr, (double)until_view_psnr);
        if (hist_threshold)
          std::printf("threshold: frame %d: %d iterations, %d rounds, %lld samples (%.4f of uniform), %d pixels above, estimated PSNR of the blend %.9g dB\n", f,
                      frame_iters, std::max(0, thr_groups - 2), (long long)thr_samples, (double)thr_samples / ((double)iters * W * H), thr_above,
                      (double)pt_psnr_from_sse(thr_sse, W * H));
        if (history_probe) std::printf("probe: frame %d: %d of %d probes changed, %d skipped\n", f, changed, probes, skipped);
        if (history_extra) std::printf("history: frame %d: %d extra over %d of %d fresh pixels\n", f, history_extra, selected, fresh);
        if (pt_save_png((frame + ".reprojected.png").c_str(), carried.data(), W, H, 1.0f) == 0) std::printf("Saved %s.reprojected.png.\n", frame.c_str());
        if (pfm && pt_save_pfm((frame + ".reprojected.pfm").c_str(), carried.data(), W, H, 1.0f) == 0) std::printf("Saved %s.reprojected.pfm.\n", frame.c_str());
        if (dn_history) {  // the history keeps the unfiltered blend; --history-feedback: and, beside it, the filtered one
          if (pt_save_png((frame + ".reprojected.denoised.png").c_str(), filtered.data(), W, H, 1.0f) == 0) std::printf("Saved %s.reprojected.denoised.png.\n", frame.c_str());
          if (pfm && pt_save_pfm((frame + ".reprojected.denoised.pfm").c_str(), filtered.data(), W, H, 1.0f) == 0)
            std::printf("Saved %s.reprojected.denoised.pfm.\n", frame.c_str());
        }
      }
    }
    if (grp) pt_group_destroy(grp);
    else pt_free();
  } else if (gpus < 0) {
    // the reference's call sequence (main.cpp:133-152) through the pathtrace.h shim
    GuiDataContainer gui;
    InitDataContainer(&gui);
    pathtraceFree();  // main.cpp:134 frees before the first init
    pathtraceSetArith(arith);
    pathtraceSetAntialias(aa);
    pathtraceSetConvergence(convergence);
    pathtraceInit(scene);
    if (!ref_frame.empty() && pt_set_reference(ref_frame.data())) {
      std::fprintf(stderr, "HIP error (pt_set_reference): %s\n", pt_last_error());
      return EXIT_FAILURE;
    }
    const auto t0 = std::chrono::high_resolution_clock::now();
    int64_t adaptive_samples = 0;
    if (by_threshold) {
      int done = 0, groups = 0, above = -1;
      double sse = -1.0;
      scene->state.image.resize((size_t)W * H * 3);
      if (pt_render_threshold(1, iters, until_group, threshold, threshold_cap, threshold_min_pixels, &done, &adaptive_samples, &above) ||
          pt_get_noise(&sse, &groups, nullptr) || pt_resolve(scene->state.image.data())) {
        std::fprintf(stderr, "HIP error (pt_render_threshold): %s\n", pt_last_error());
        return EXIT_FAILURE;
      }
      const int64_t pixels = (int64_t)W * H;
      std::printf("adaptive: threshold %.9g: %d iterations, %d rounds, %lld samples (%.4f of uniform), %d pixels above, estimated PSNR %.9g dB\n", (double)threshold,
                  done, std::max(0, groups - 2), (long long)adaptive_samples, (double)adaptive_samples / ((double)done * (double)pixels), above,
                  sse < 0.0 ? -1.0 : (double)pt_psnr_from_sse(sse, pixels));
      scene->state.iterations = done;
      iters = (int)((adaptive_samples + pixels - 1) / pixels);  // what the file names carry
      name_outputs();
      iters = done;  // (the feature pass covers the iteration numbers used)
    } else if (adaptive > 0.0f) {
      int done = 0, groups = 0;
      float psnr = -1.0f;
      scene->state.image.resize((size_t)W * H * 3);
      if (pt_render_adaptive(1, iters, until_group, adaptive, until_db, &done, &adaptive_samples, &psnr) || pt_get_noise(nullptr, &groups, nullptr) ||
          pt_resolve(scene->state.image.data())) {
        std::fprintf(stderr, "HIP error (pt_render_adaptive): %s\n", pt_last_error());
        return EXIT_FAILURE;
      }
      const int64_t pixels = (int64_t)W * H;
      std::printf("adaptive: %d iterations, %d rounds, %lld samples (%.4f of uniform), estimated PSNR %.9g dB\n", done, std::max(0, groups - 2),
                  (long long)adaptive_samples, (double)adaptive_samples / ((double)done * (double)pixels), (double)psnr);
      scene->state.iterations = done;
      iters = (int)((adaptive_samples + pixels - 1) / pixels);  // what the file names carry
      name_outputs();
      iters = done;  // (the feature pass covers the iteration numbers used)
    } else if (until) {
      int done = 0, groups = 0;
      float psnr = -1.0f;
      if (pt_render_until(1, iters, until_group, until_db, &done, &psnr) || pt_get_noise(nullptr, &groups, nullptr)) {
        std::fprintf(stderr, "HIP error (pt_render_until): %s\n", pt_last_error());
        return EXIT_FAILURE;
      }
      report_noise(done, groups, psnr);
    } else if (guided) {
      for (int it = 1; it <= iters; it += fold_group)
        if (pt_render(it, std::min(fold_group, iters - it + 1)) || pt_noise_fold()) {
          std::fprintf(stderr, "HIP error (pt_noise_fold): %s\n", pt_last_error());
          return EXIT_FAILURE;
        }
    } else {
      for (int it = 1; it <= iters; ++it) pathtrace(nullptr, 0, it);  // main.cpp:138-149
    }
    if (adaptive_mode) pt_sync();  // (the resolved image is already in scene->state.image; the SUM image alone means nothing)
    else pathtraceSyncImage();
    secs = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
    const double samples_done = adaptive_mode ? (double)adaptive_samples : (double)W * H * iters;
    // (adaptive: the spp of the file names, ceil(samples / pixels), beside the rate of the samples actually rendered)
    const int spp_done = adaptive_mode ? (int)((adaptive_samples + (int64_t)W * H - 1) / ((int64_t)W * H)) : iters;
    std::printf("%dx%d, %d spp, depth %d: %.3f s, %.2f Msamples/s\n", W, H, spp_done, scene->state.traceDepth, secs, samples_done / secs / 1e6);
    const float image_samples = adaptive_mode ? 1.0f : (float)iters;  // the resolved image is averaged radiance already
    if (pt_save_png((base + ".png").c_str(), scene->state.image.data(), W, H, image_samples) == 0)
      std::printf("Saved %s.png.\n", base.c_str());
    if (pfm && pt_save_pfm((base + ".pfm").c_str(), scene->state.image.data(), W, H, image_samples) == 0)
      std::printf("Saved %s.pfm.\n", base.c_str());
    if (hdr && pt_save_hdr((base + ".hdr").c_str(), scene->state.image.data(), W, H, image_samples) == 0)
      std::printf("Saved %s.hdr.\n", base.c_str());
    if (features) {
      std::vector<float> planes((size_t)PT_FEATURE_PLANES * W * H * 4);
      if (pt_render_features(1, iters) || pt_readback_features(planes.data())) {
        std::fprintf(stderr, "HIP error (pt_render_features): %s\n", pt_last_error());
        return EXIT_FAILURE;
      }
      save_features(planes);
    }
    if (denoise) {
      std::vector<float> rgb((size_t)W * H * 3);
      if (pt_denoise((float)iters, &dn_opt, rgb.data())) {
        std::fprintf(stderr, "HIP error (pt_denoise): %s\n", pt_last_error());
        return EXIT_FAILURE;
      }
      save_denoised(rgb);
    }
    if (guided) {
      std::vector<float> rgb((size_t)W * H * 3);
      if (pt_denoise_guided(&dn_opt, rgb.data())) {
        std::fprintf(stderr, "HIP error (pt_denoise_guided): %s\n", pt_last_error());
        return EXIT_FAILURE;
      }
      save_denoised(rgb);
    }
    if (dn_adaptive) {
      std::vector<float> rgb((size_t)W * H * 3);
      if (pt_denoise_adaptive(&dn_opt, rgb.data())) {
        std::fprintf(stderr, "HIP error (pt_denoise_adaptive): %s\n", pt_last_error());
        return EXIT_FAILURE;
      }
      save_denoised(rgb);
    }
    if (convergence) {
      std::vector<float> psnr((size_t)iters);
      for (int it = 1; it <= iters; ++it) psnr[it - 1] = pathtracePSNR(it);  // what the reference prints after every iteration
      int clean = -1;
      if (pt_iterations_to_clean(clean_db, &clean)) {
        std::fprintf(stderr, "HIP error (pt_iterations_to_clean): %s\n", pt_last_error());
        return EXIT_FAILURE;
      }
      print_curve(psnr, clean);
    }
    pathtraceFree();
  } else {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
      std::fprintf(stderr, "no HIP device\n");
      return 1;
    }
    if (gpus == 0) gpus = ndev;
    if (device_list.empty() && gpus > ndev) {
      std::fprintf(stderr, "--gpus %d but only %d device(s) visible\n", gpus, ndev);
      return 1;
    }
    std::vector<int> devices(gpus);
    for (int i = 0; i < gpus; ++i) devices[i] = device_list.empty() ? i : device_list[i];
    for (int d : devices)
      if (d < 0 || d >= ndev) {
        std::fprintf(stderr, "device %d named but only %d device(s) visible\n", d, ndev);
        return 1;
      }
    PtOptions opt{};
    opt.arith = arith;
    opt.aa_jitter = aa ? 1 : 0;
    opt.convergence = convergence;
    const PtSceneDesc desc = scene->desc();
    PtGroup* grp = nullptr;
    if (pt_group_create_ex(&desc, &opt, devices.data(), gpus, transport, &grp)) {
      std::fprintf(stderr, "HIP error (pt_group_create): %s\n", pt_last_error());
      return EXIT_FAILURE;
    }
    if (!ref_frame.empty() && pt_group_set_reference(grp, ref_frame.data())) {
      std::fprintf(stderr, "HIP error (pt_group_set_reference): %s\n", pt_last_error());
      return EXIT_FAILURE;
    }
    std::vector<uint8_t> rgb8((size_t)W * H * 3);
    const auto t0 = std::chrono::high_resolution_clock::now();
    int rc = 0;
    if (preview > 0) {
      std::vector<uint8_t> rgba((size_t)W * H * 4), rgb((size_t)W * H * 3);
      for (int it = 1; it <= iters && !rc; it += preview) {
        const int n = std::min(preview, iters - it + 1);
        rc = pt_group_render(grp, it, n);
        if (!rc && it + n <= iters) {  // progressive preview of what has been accumulated so far
          rc = pt_group_preview_rgba8(grp, it + n - 1, rgba.data());
          for (size_t p = 0; p < (size_t)W * H; ++p) rgb[3 * p] = rgba[4 * p], rgb[3 * p + 1] = rgba[4 * p + 1], rgb[3 * p + 2] = rgba[4 * p + 2];
          if (!rc) pt_write_png_rgb8((out + ".preview.png").c_str(), rgb.data(), W, H);
        }
      }
    } else if (until) {
      int done = 0, groups = 0;
      float psnr = -1.0f;
      rc = pt_group_render_until(grp, 1, iters, until_group, until_db, &done, &psnr) || pt_group_get_noise(grp, nullptr, &groups, nullptr);
      if (!rc) report_noise(done, groups, psnr);
    } else if (guided) {
      for (int it = 1; it <= iters && !rc; it += fold_group) rc = pt_group_render(grp, it, std::min(fold_group, iters - it + 1)) || pt_group_noise_fold(grp);
    } else {
      rc = pt_group_render(grp, 1, iters);
    }
    if (!rc) rc = pt_group_gather_u8(grp, (float)iters, rgb8.data());  // the write-out gather: 3 B per pixel
    secs = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
    if (rc) {
      std::fprintf(stderr, "HIP error (pt_group): %s\n", pt_last_error());
      return EXIT_FAILURE;
    }
    std::printf("%dx%d, %d spp, depth %d on %d GPU(s): %.3f s, %.2f Msamples/s\n", W, H, iters, scene->state.traceDepth, gpus,
                secs, (double)W * H * iters / secs / 1e6);
    if (pt_write_png_rgb8((base + ".png").c_str(), rgb8.data(), W, H) == 0) std::printf("Saved %s.png.\n", base.c_str());
    if (pfm || hdr) {
      scene->state.image.resize((size_t)W * H * 3);
      if (pt_group_gather(grp, scene->state.image.data())) {
        std::fprintf(stderr, "HIP error (pt_group_gather): %s\n", pt_last_error());
        return EXIT_FAILURE;
      }
      if (pfm && pt_save_pfm((base + ".pfm").c_str(), scene->state.image.data(), W, H, (float)iters) == 0)
        std::printf("Saved %s.pfm.\n", base.c_str());
      if (hdr && pt_save_hdr((base + ".hdr").c_str(), scene->state.image.data(), W, H, (float)iters) == 0)
        std::printf("Saved %s.hdr.\n", base.c_str());
    }
    if (features) {
      std::vector<float> planes((size_t)PT_FEATURE_PLANES * W * H * 4);
      if (pt_group_render_features(grp, 1, iters) || pt_group_gather_features(grp, planes.data())) {
        std::fprintf(stderr, "HIP error (pt_group_render_features): %s\n", pt_last_error());
        return EXIT_FAILURE;
      }
      save_features(planes);
    }
    if (denoise) {
      std::vector<float> rgb((size_t)W * H * 3);
      if (pt_group_denoise(grp, (float)iters, &dn_opt, rgb.data())) {
        std::fprintf(stderr, "HIP error (pt_group_denoise): %s\n", pt_last_error());
        return EXIT_FAILURE;
      }
      save_denoised(rgb);
    }
    if (guided) {
      std::vector<float> rgb((size_t)W * H * 3);
      if (pt_group_denoise_guided(grp, &dn_opt, rgb.data())) {
        std::fprintf(stderr, "HIP error (pt_group_denoise_guided): %s\n", pt_last_error());
        return EXIT_FAILURE;
      }
      save_denoised(rgb);
    }
    if (convergence) {
      std::vector<double> sse((size_t)iters);
      int clean = -1;
      if (pt_group_get_convergence(grp, 1, iters, sse.data()) || pt_group_iterations_to_clean(grp, clean_db, &clean)) {
        std::fprintf(stderr, "HIP error (pt_group_get_convergence): %s\n", pt_last_error());
        return EXIT_FAILURE;
      }
      std::vector<float> psnr((size_t)iters);
      for (int it = 1; it <= iters; ++it) psnr[it - 1] = sse[it - 1] < 0.0 ? FLT_MAX : pt_psnr_from_sse(sse[it - 1], (int64_t)W * H);
      print_curve(psnr, clean);
    }
    pt_group_destroy(grp);
  }
  delete scene;
  return 0;
}
