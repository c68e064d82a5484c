/* pt_amd.h — C ABI of the MI355X-native wavefront path tracer (libpt_amd.so).
 *
 * This is the drop-in boundary for the reference's renderer API
 * (reference: src/pathtrace.h:6-9 — InitDataContainer / pathtraceInit /
 * pathtraceFree / pathtrace) and for the host-side scene model it consumes
 * (src/scene.h:20-25, src/sceneStructs.h).  Plain C: pointers, sizes, PODs.
 * No C++ `Scene`, no GLM and no torch types cross this boundary.
 * The C++ source-compatible mirror of pathtrace.h lives in
 * include/pathtrace_amd.hpp; INTEGRATION.md shows the reference-side glue.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; pt_last_error()
 *     gives the message (the reference prints + exit()s, pathtrace.cu:141-150).
 *   - matrices are column-major float[16], element [c*4+r] == glm m[c][r].
 *   - images are float RGB, running SUM over iterations (not the average), in the
 *     reference's raw orientation (index = x + y*W; saveImage() mirrors x later,
 *     src/main.cpp:91-97), exactly what pathtrace() leaves in
 *     scene->state.image (pathtrace.cu:648-651).
 *   - single caller thread.  pt_init / pt_render / pt_free act on one default renderer instance, like the
 *     reference's file-scope state (pathtrace.cu:446-456); pt_ctx_* are the same operations on explicit
 *     instances (one per GPU), and pt_group_* drive several GPUs from one process with one RCCL gather at
 *     image write-out.
 */
#ifndef PT_AMD_H
#define PT_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_GEOM_SPHERE 0 /* sceneStructs.h:10-13 */
#define PT_GEOM_CUBE 1
/* EXTENSION (default scenes never contain it): one triangle of a `mesh` object — the type the scene format names
 * (INSTRUCTION.md:246) and the reference does not implement.  transform[0..8] holds the three WORLD-space vertices
 * v0.xyz, v1.xyz, v2.xyz, every other matrix element is 0; intersected as glm::intersectRayTriangle does (front faces
 * only; the header the reference includes at intersections.h:4).  Parity unpinned: tested GPU == oracle. */
#define PT_GEOM_TRIANGLE 2

/* The fields of `Geom` the renderer reads (sceneStructs.h:20-36). */
typedef struct PtGeom {
  int32_t type;
  int32_t materialid;
  float transform[16];
  float inverseTransform[16];
  float invTranspose[16];
} PtGeom;

/* Same field order and size (44 B) as `Material` (sceneStructs.h:38-48). */
typedef struct PtMaterial {
  float color[3];
  float specular_exponent;
  float specular_color[3];
  float hasReflective;
  float hasRefractive;
  float indexOfRefraction;
  float emittance;
} PtMaterial;

/* Same field order and size (84 B) as `Camera` (sceneStructs.h:50-59). */
typedef struct PtCamera {
  int32_t resolution[2];
  float position[3];
  float lookAt[3];
  float view[3];
  float up[3];
  float right[3];
  float fov[2];
  float pixelLength[2];
} PtCamera;

/* Same layout (36 B) as BVHNodeGPU (pathtrace.cu:24-32); for inspection/tests. */
typedef struct PtBVHNode {
  float bmin[3];
  float bmax[3];
  int32_t left, right, geomIndex;
} PtBVHNode;

typedef struct PtSceneDesc {
  const PtGeom* geoms;
  int32_t num_geoms;
  const PtMaterial* materials;
  int32_t num_materials;
  PtCamera camera;     /* after the main.cpp camera fix-up (see pt_scene_load) */
  int32_t trace_depth; /* RenderState::traceDepth */
} PtSceneDesc;

typedef struct PtOptions {
  int32_t device;          /* HIP device ordinal */
  int32_t pixel_begin;     /* framebuffer tile: global pixel indices             */
  int32_t pixel_count;     /*   [pixel_begin, pixel_begin+pixel_count); 0 = all  */
  int32_t iters_per_batch; /* iterations in flight per wavefront batch; 0 = auto */
  int32_t num_queues;      /* compaction queues; 0 = auto                        */
  int32_t blocks_per_cu;   /* persistent grid = CUs * blocks_per_cu; 0 = auto    */
  int32_t time_kernels;    /* 1: bracket every computeIntersections launch with  */
                           /*    HIP events on the render stream (pt_get_stats)  */
  int32_t legacy_traversal; /* 1: per-lane BVH walk kernel instead of the wave-cooperative one (A/B) */
  int32_t debug_flags;      /* A-B switches with UNCHANGED results: 16 no closer-hit cull in the subtree scans, 32 no
                               near-first subtree order, 64 W / Q waves per queue in every batch of the fused bounce kernel
                               (default: dealt by the time the queues' waves took, PtStats.paths_waves), 128 the fused primary
                               kernel traces its camera rays in every iteration (default without aa_jitter: once per run of
                               iterations, see primary_share), 256 / 512 force /
                               forbid the uniform-grid walk of the fused kernels (default: for large scenes, whichever of the
                               BVH scan and up to three grid resolutions renders a few iterations fastest at pt_init), 1024
                               depth-0 retirees stored and gathered in every iteration (default in the shared form with
                               depth >= 2: a miss or an emitter hit of a camera ray has the same colour in every iteration
                               and is stored and gathered in iteration 0 of a batch only), 4096
                               whole 40-byte depth-1 records in every iteration (default under the same conditions: origin and
                               material of a surviving pixel are stored once per batch, direction, sample id and the
                               specular / diffuse choice per iteration, and the throughput is formed where the path is taken), 8192
                               split records where the default is less still (scenes whose tables the fused kernels keep in LDS,
                               under the conditions of 1024 and 4096 together, while iterations per batch and materials fit their
                               words: ONE record per surviving pixel and batch — bounce origin, hit normal, camera direction,
                               pixel and material — the primary kernel traces every chunk once per batch, and the bounce kernel
                               decides depth 0 and samples the first bounce of every iteration's path when a lane takes it;
                               primary_pieces and primary_share are ignored by that form; PtStats.record_form tells), 16384
                               retirement records in order of retirement, gathered through a tile (default in a batch of the
                               8192 form whose words fit: a path's record goes to the slot its position in its list gives, so a
                               slot holds the same pixel in every iteration of the batch and the gather streams the records,
                               one thread per slot; PtStats.gather_form tells), 32768 the tile gather over such fixed slots, 65536
                               the primary kernel runs in every batch (default in a batch of the 8192 form with the fixed slots
                               of 16384: its output there depends on neither the iteration nor the batch's length, so it runs
                               in the first batch after pt_init or pt_set_camera and later batches read what it left;
                               PtStats.primary_launches tells), 131072 every batch is gathered by a launch of its own (default for
                               the batches of the 16384 form's stream gather that another batch of the same pt_render call follows
                               with the same camera, tile and plan: the next batch's bounce kernel adds their records to the image
                               beside its own work, from the other of two record planes; PtStats.inline_gathers counts), 2048
                               keep the reference's leaf boxes for spheres (default for large scenes: tightened to the
                               ellipsoid's box, PtStats.tight_leaves; pt_stage_intersect on such a scene then expects ray
                               origins inside the scene bounds or at the camera).  pt_init fails on any other bit. */
  int32_t unfused_primary;  /* 1: run depth 0 as generate + intersect + shade launches instead of the fused
                               primary kernel (A/B and stage-parity runs) */
  int32_t unfused_bounces;  /* 1: depths >= 1 as separate computeIntersections + shade launches (hit records
                               through HBM) instead of the fused bounce kernel (A/B and stage-parity runs) */
  int32_t stripe_pixels;    /* striped tile for multi-GPU load balance: the tile consists of runs of          */
  int32_t stripe_stride;    /*   stripe_pixels pixels starting every stripe_stride pixels from pixel_begin;     */
                            /*   pixel_count counts the tile's own pixels.  0 = one contiguous run              */
  int32_t arith;            /* arithmetic mode of the kernels, PT_ARITH_*                                      */
  int32_t aa_jitter;        /* EXTENSION, default 0 = reference semantics.  1: stochastic anti-aliasing — the camera
                               ray of sample (iteration, pixel) goes through (x + u1 - .5, y + u2 - .5) instead of
                               the pixel centre; the reference's generateRayFromCamera ignores `iter`
                               (pathtrace.cu:270-286) although its assignment text asks for this (INSTRUCTION.md:96).
                               u1, u2 come from a hash domain of their own, every other random stream is unchanged.
                               Parity unpinned (nothing in the reference to compare with): tested GPU == oracle. */
  int32_t convergence;      /* convergence metric (computePSNR, pathtrace.cu:184-201), computed inside the gather: 0 off (default;
                               nothing is allocated, the kernels are the ones that run without this field); N > 0: the frame
                               every iteration is compared with is the average after iteration N (the reference's N is 10), kept
                               on the device, and iterations <= N have no value; -1: the frame is supplied with
                               pt_set_reference before the first pt_render.  pt_init fails on any other value.  See
                               pt_get_convergence. */
  /* Overrides of automatic choices (tests, A/B): 0 = automatic; no value changes the image. */
  int32_t lds_table_kb;     /* LDS staging limit of the scene tables: N > 0 forces N KB (at most 64), < 0 keeps the tables
                               in memory (automatic: staged when every leaf is a top-list entry and staging costs the fused
                               bounce kernel no resident workgroup) */
  int32_t primary_pieces;   /* the fused primary kernel's per-wave strands cut into this many pieces (automatic:
                               max(2, iterations per batch / 64 rounded up) when it traces once per run of iterations; with a trace per
                               iteration min(4, max(1, strand groups / 48))).  Bits 16-22 of the same word hold primary_share
                               (PT_PRIMARY_PIECES below; the struct keeps its 20 words): the kernel traces a group of camera
                               rays once for at most that many iterations of a batch and shades it in each of them (0 =
                               automatic: a whole piece, at most 64; 1: a trace per iteration, as debug_flags 128; always a
                               trace per iteration with aa_jitter, whose rays differ from iteration to iteration).  Both are
                               ignored where the kernel traces once per batch (PtStats.record_form 2, see debug_flags 8192). */
  int32_t paths_pieces;     /* the fused bounce kernel's depth-1 rays cut into this many pieces per wave (automatic: 2) */
  int32_t paths_min_piece;  /* fewest paths in one of those pieces (automatic: 64; small values send small images through
                               the piece switches).  The three piece counts are clamped to 1..0x7fff (of primary_pieces: its low 16
                               bits; a negative word counts as 1 piece; pt_init fails when bits 16 and up hold more than 64). */
} PtOptions;
/* PtOptions.primary_pieces from a piece count (0 .. 0x7fff) and primary_share (0 .. 64). */
#define PT_PRIMARY_PIECES(pieces, share) ((int32_t)((pieces) | (share) << 16))

/* Arithmetic modes (PtOptions.arith).  All modes run the same algorithm with the same random draws and decisions;
 * they differ in how float expressions are rounded.
 *   EXACT  every operation in the reference's source order without FMA contraction, IEEE divide / sqrt, portable
 *          sin / cos / acos: bit-identical to the CPU oracle (oracle/pt_oracle.cpp, PORTABLE mode).  The parity anchor.
 *   FMA    the same source with FMA contraction (what nvcc does to the reference's kernels by default), IEEE
 *          divide / sqrt kept; direction sampling with float-only sin / cos (<= 1.6 ulp, the accuracy class of the
 *          sinf / cosf nvcc links; the diffuse lobe through square roots instead of acos).
 *   FAST   FMA + hardware reciprocal / rsqrt / sqrt / sin / cos, nested-FMA matrix products, float-only
 *          direction sampling.
 * FMA and FAST are held to the stated tolerance against the reference semantics (tests/test_gpu_arith.py):
 * finite; at <= 16 spp >= 99.8 % of pixels within 1e-5; PSNR >= 45 dB + 10 log10(spp / 8). */
#define PT_ARITH_EXACT 0
#define PT_ARITH_FMA 1
#define PT_ARITH_FAST 2

#define PT_MAX_DEPTH 64
typedef struct PtStats {
  int64_t samples;                    /* pixel-samples rendered since pt_init            */
  int64_t live_rays[PT_MAX_DEPTH];    /* rays traced by computeIntersections per depth   */
  int64_t intersect_launches;         /* timed computeIntersections launches             */
  double intersect_ms;                /* sum of their HIP-event durations (time_kernels) */
  double render_ms;                   /* HIP-event time of all pt_render calls           */
  int32_t num_cus, grid_blocks, num_queues, iters_per_batch;
  int64_t device_bytes;               /* device memory held by the renderer              */
  int32_t primary_fused;              /* 1: depth 0 ran in the fused primary kernel, so the timed
                                         computeIntersections launches cover depths >= 1 only   */
  int32_t bounces_fused;              /* 1: depths >= 1 ran in the fused bounce kernel; the timed launches
                                         (intersect_ms / intersect_launches) are then those kernels      */
  int32_t arith;                      /* PT_ARITH_* in use                                               */
  int32_t grid_cells;                 /* > 0: the fused kernels walk the uniform grid over the leaf boxes (large scenes on
                                         which it beat the BVH scan at pt_init) with this many cells; 0: the BVH         */
  int32_t tight_leaves;               /* sphere leaves whose traversal box was tightened from the reference's box of the
                                         transformed unit cube to the box of the ellipsoid (large scenes; same image)     */
  int32_t paths_waves;                /* 0: every queue has the same number of waves in the fused bounce kernel; otherwise
                                         fewest << 16 | most waves a queue gets in the next batch — dealt by the time the
                                         queues' waves took in the last one (small tiles; same image, debug_flags 64 turns it off) */
  int32_t record_form;                /* how the last batch handed depth 0 to the fused bounce kernel: 0 whole 40-byte records per
                                         sample, 1 split records (debug_flags 4096 turns them off), 2 one record per surviving pixel
                                         and batch, the first bounce sampled in the bounce kernel (debug_flags 8192 turns it off) */
  int32_t gather_form;                /* how the last batch was gathered: 0 through a tile, from records in order of retirement
                                         (debug_flags 16384 asks for it), 1 through a tile, from fixed record slots (debug_flags
                                         32768, and every batch that computes the convergence metric), 2 as a stream over fixed slots,
                                         3 as that stream inside the next batch's bounce kernel (only while a pt_render call is
                                         being submitted: the last batch of every call is gathered by a launch of its own) */
  int64_t primary_launches;           /* launches of the fused primary kernel by pt_render since pt_init (pt_reset_stats and pt_clear
                                         leave it): with record_form 2 one per camera — the first batch after pt_init or
                                         pt_set_camera — instead of one per batch (debug_flags 65536 asks for every batch) */
  int64_t inline_gathers;             /* batches gathered inside the next batch's bounce kernel since pt_init (debug_flags 131072: none);
                                         the second record plane this needs counts in device_bytes */
} PtStats;

/* ---- scene loading (host).  Replaces `new Scene(file)` (src/main.cpp:45,
 * src/scene.cpp:7-188) plus the camera state main.cpp derives before the first
 * frame (main.cpp:57-71, 110-128).  res_w/res_h > 0 override the RES line,
 * recomputing fov/pixelLength as scene.cpp:133-140 does. */
typedef struct PtScene PtScene;
int pt_scene_load(const char* path, int res_w, int res_h, PtScene** out);
void pt_scene_free(PtScene* s);
int pt_scene_desc(const PtScene* s, PtSceneDesc* out); /* pointers valid until pt_scene_free */
int pt_scene_iterations(const PtScene* s);             /* CAMERA ITERATIONS */
/* A mouse drag of the reference's viewer (main.cpp:192-199) in float on the orbit state pt_scene_load derived (main.cpp:63-71):
 * phi += dphi; theta = fmaxf(0.001f, fminf(theta + dtheta, PI)); zoom = fmaxf(0.1f, zoom + dzoom); then the camchanged block
 * (main.cpp:112-126) through the code pt_scene_load ran.  (0, 0, 0) leaves the camera as it is, bit for bit, for a scene whose
 * theta and zoom lie inside the clamps.  pt_scene_desc must be called again to see the new camera. */
int pt_scene_orbit(PtScene* s, float dphi, float dtheta, float dzoom);
int pt_scene_camera(const PtScene* s, PtCamera* out);
int pt_scene_orbit_state(const PtScene* s, float* phi, float* theta, float* zoom); /* any pointer may be NULL */
const char* pt_scene_image_name(const PtScene* s);     /* CAMERA FILE */
/* The TRANS / ROTAT / SCALE of the OBJECT geom `geom` came from, as the loader read them (trs[0..2] translation, [3..5] rotation in
 * degrees, [6..8] scale), and moving that object as the loader would have placed it: the setter rebuilds the geom's three matrices
 * through the loader's own code (pt_build_transform), so they are byte for byte what loading a file with that TRS gives.  Refused
 * by name: a null argument, an index outside the scene's geoms, a geom that comes from a `mesh` object (its triangles hold
 * world-space vertices), a component that is not finite.  pt_scene_desc must be called again afterwards, as after pt_scene_orbit. */
int pt_scene_geom_trs(const PtScene* s, int geom, float trs[9]);
int pt_scene_set_geom_trs(PtScene* s, int geom, const float trs[9]);
/* Material `m` of the scene as the loader read it, and a new one in its place (all eleven words are stored as given; pt_set_materials
 * hands the edited materials to a live renderer).  Refused by name: a null argument, an index outside the scene's materials, a word
 * the renderer reads (color, specular_color, hasReflective, hasRefractive, emittance) that is not finite.  pt_scene_desc must be
 * called again afterwards. */
int pt_scene_material(const PtScene* s, int m, PtMaterial* out);
int pt_scene_set_material(PtScene* s, int m, const PtMaterial* material);

/* BVH exactly as pathtraceInit builds it (pathtrace.cu:34-111, 483-489).
 * Returns node count (2n-1); writes up to `cap` nodes if `out` != NULL. */
int pt_build_bvh(const PtGeom* geoms, int num_geoms, PtBVHNode* out, int cap);

/* The traversal structure of our own for large scenes (the reference has only the median-split
 * BVH of pathtrace.cu:52-111): a uniform grid over the leaf boxes, walked by the depth-0 and depth >= 1 kernels instead of
 * the BVH.  The image is the same either way: a primitive is tested exactly when the ray passes the primitive's own box
 * test, and every leaf is listed in all cells its box, grown by `pad`, touches.  A scene is a CANDIDATE when it has
 * >= 600 BVH nodes and its lists stay moderate (at most 64 cell references per primitive; `forced` skips both
 * conditions, as PtOptions.debug_flags 256 does); for a candidate pt_init / pt_ctx_create time a few iterations of the
 * tile with the BVH scan, with a grid of the cost model's resolution and with two finer ones (4 and 8 cells per
 * primitive) and keep the fastest (PtStats.grid_cells > 0: a grid, with that many cells).  This function builds the grid
 * of the cost model's resolution over the reference's leaf boxes, without the camera (csrc/pt_tables.cpp build_grid).  The
 * renderer's grids cover its traversal boxes (pt_traversal_boxes: tightened sphere leaves), their pad also covers the
 * camera's coordinates and their cell table carries empty guard cells: built the same way, but not byte for byte this grid.
 * Host-only (no GPU needed).  Returns 1 and fills `info` for a candidate, 0 otherwise, -1 on error; cell c's records
 * are records[cell_start[c] .. cell_start[c + 1]), c = x + res[0] * (y + res[1] * z); either array may be NULL (sizes
 * are in `info`). */
typedef struct PtGridInfo {
  int32_t res[3];
  float origin[3], cell_size[3], pad;
  int32_t num_cells, num_records, num_leaves;
} PtGridInfo;
typedef struct PtGridRecord {
  float bmin[3], bmax[3]; /* the leaf's box (the reference's worldBounds)                                     */
  int32_t leaf;           /* index of the leaf in the reference's visiting order (threaded BVH)              */
  int32_t neighbours;     /* bits 0-5: the leaf is also listed in the neighbour cell -x, +x, -y, +y, -z, +z;
                             bits 6-7: primitive type; bits 8-31: index of the primitive in PtSceneDesc.geoms  */
} PtGridRecord;
int pt_build_grid(const PtGeom* geoms, int num_geoms, int forced, PtGridInfo* info, uint32_t* cell_start, PtGridRecord* records);

/* Host-only: the box our traversal structures test for each geom's leaf — the reference's leaf box (pathtrace.cu:36-50),
 * except for spheres of large scenes, where it is intersected with the box of the ellipsoid itself (grown by a bound on
 * what sphereIntersectionTest's float arithmetic, intersections.h:102-144, can still report as a hit for ray origins inside
 * the scene bounds or at `camera_position`; csrc/pt_tables.cpp sphere_tight_box).  A ray that passes the tightened box passes the
 * reference's; a ray that passes only the reference's misses the sphere: same hits, fewer candidates.  boxes[g] = {min xyz, max xyz}.
 * Returns the number of tightened leaves (pt_init applies it from 64 BVH nodes on; PtOptions.debug_flags 2048 turns it off). */
int pt_traversal_boxes(const PtGeom* geoms, int num_geoms, const float camera_position[3], float* boxes);

/* Host-only: a traversal box as the FAST build's bounce kernels test it — centre and half extent instead of min / max, so that
 * the slab test is three FMAs per axis (csrc/pt_arith.inc slab_t; min / max issue at half the rate of an FMA on gfx950).  The
 * half extent is rounded up from the distance between the float centre and the farther face, so [c - h, c + h] contains
 * [lo, hi] in real arithmetic; `inner` != 0 (inner nodes, subtree entries of the top list: pure acceleration) adds 1e-5 of the
 * extent and 1e-5 * `magnitude`, the largest coordinate magnitude of the scene bounds and the camera position (what pt_init passes: the
 * test's rounding follows the ray origin), so that a ray passing a leaf's box in the test's float arithmetic passes every box
 * above it (the bound is derived at csrc/pt_tables.cpp center_half_box).  `magnitude` is not used for leaves.
 * Depth 0 and the exact / fma builds test the reference's min / max boxes with the reference's arithmetic. */
void pt_center_half_box(const float lo[3], const float hi[3], int inner, float magnitude, float center[3], float half_extent[3]);

/* transform / inverse / inverse-transpose of an OBJECT block's TRANS ROTAT SCALE
 * (trs[9]), as utilityCore::buildTransformationMatrix + glm::inverse +
 * glm::inverseTranspose compute them (src/utilities.cpp:64-72, src/scene.cpp:83-86). */
int pt_build_transform(const float* trs, float* transform, float* inverse, float* invTranspose);

/* ---- renderer (replaces src/pathtrace.h) -------------------------------- */
int pt_init(const PtSceneDesc* scene, const PtOptions* opt); /* pathtraceInit, pathtrace.cu:462 */
int pt_free(void);                                           /* pathtraceFree, pathtrace.cu:518; safe
                                                                before init and twice in a row */
/* Runs iterations iter_first .. iter_first+iter_count-1 (1-based, as main.cpp:141-145
 * passes them) and adds them to the accumulation image.  Equivalent to iter_count
 * calls of pathtrace(pbo=NULL, 0, iter) (pathtrace.cu:529).  Asynchronous on the
 * renderer's stream; pt_sync / pt_readback wait. */
int pt_render(int iter_first, int iter_count);
int pt_sync(void);
/* Tile SUM image → host (pixel_count*3 floats), pathtrace.cu:648-651. */
int pt_readback(float* rgb_sum_host);
/* Tile SUM image → caller-owned device buffer (pixel_count*3 floats) on the
 * renderer's device; used to feed the RCCL gather without a host hop. */
int pt_readback_device(void* rgb_sum_dev);
/* Display conversion of sendImageToPBO (pathtrace.cu:250-268): average, gamma 1/2.2,
 * clamp → RGBA8 into a host buffer of pixel_count*4 bytes. */
int pt_preview_rgba8(int iterations, uint8_t* rgba_host);
int pt_preview_rgba8_device(int iterations, void* rgba_dev); /* same, into a device buffer (the PBO) */
int pt_get_stats(PtStats* out);
int pt_reset_stats(void);
/* Restart the accumulation without giving up the renderer: the SUM image and the statistics are zeroed, every buffer
 * stays allocated (and warm).  The camera stays where it is: what the reference does by pathtraceFree() + pathtraceInit()
 * when the camera moves (main.cpp:134-135) is pt_set_camera, below. */
int pt_clear(void);
/* ---- moving the camera of a live renderer: what the reference answers with pathtraceFree() + pathtraceInit() after every
 * mouse drag (main.cpp:110-136), without the teardown, the allocations, the host build of the camera-independent tables and the
 * timing probe of the traversal structures.
 * Contract: after a successful call every later call on the renderer gives what a renderer freshly created from the same scene,
 * options and `cam` gives, bit for bit in all three PT_ARITH_* modes: the image, the feature buffers, the noise planes, the
 * adaptive lists and counts, the resolved and the filtered images.  What may differ from a fresh renderer: the timing fields of
 * PtStats, which traversal structure is walked (the choice of pt_init is kept, the probe does not run again; any valid structure
 * gives the same image) and PtStats.device_bytes.
 * A camera move is more than a new kernel argument: the tightened sphere leaves (pt_traversal_boxes) and their copies in the
 * top list, the cull margin, the centre / half extent copies and the grid's pad all follow the camera position, so they are
 * rebuilt on the host from a copy of the camera-independent tables the renderer keeps from pt_init (the threaded BVH, the top
 * list, the PtGeoms), and uploaded: into the buffers they have when the size is unchanged, else into new ones.  A renderer that
 * walks a grid rebuilds it at the resolution pt_init chose; where no grid can be built for the new camera (a camera so far away
 * that the pad would swallow the cells) it walks the BVH scan (PtStats.grid_cells == 0) until a later camera allows the grid again.
 * Then everything pt_clear does happens (the adaptive state is left, a supplied reference frame survives), the launch widths
 * are planned again, an existing worker of the adaptive rounds receives the new camera and tables, and the path buffers and
 * retirement records return to the state a new renderer has (every word a NaN).  Workspaces (features, filter, noise, selection,
 * resolve, the byte image) stay allocated.  Synchronises.
 * Refused, in this order, with nothing changed, allocated or launched: no renderer; a failed renderer; a null `cam`; a resolution
 * other than the renderer's (a new resolution needs pt_init); a component of position, view, up, right, fov or pixelLength that
 * is not finite.  lookAt is not read by the renderer. */
int pt_set_camera(const PtCamera* cam);
/* pt_set_camera with options.  The contract is pt_set_camera's, word for word, refusals and their order included (under the name
 * pt_set_camera_ex), with one more refusal, placed after the null camera: a bit of `flags` that is not defined below.  flags == 0 is
 * pt_set_camera.
 * PT_SET_CAMERA_DEVICE_TABLES: the camera-dependent tables are rebuilt ON THE DEVICE (csrc/pt_camera_tables.hip) from a device copy of
 * the camera-independent tables: per node, per top entry and per (leaf, cell) reference the kernels run the very functions the host
 * build runs (csrc/pt_camera_tables.h), the grid is a counting sort whose records are placed by rank, and the host contributes the
 * scalars it computes as ever (origin region, scene magnitude, cull margin, the grid's pad, corner, extent and refusals).  The tables
 * are the host build's byte for byte, so everything pt_set_camera promises holds.  One 16-byte record is read back between the
 * grid's count and its scan (references, longest list, tightened leaves); nothing else crosses the bus.  The first such move of a
 * renderer uploads that copy (base nodes, base top list, 80 bytes per geom) and allocates the build's workspace (a word per grid
 * cell, the scan's sums, a word per possible reference: at most 64 per leaf, 2^22 for a forced grid); both stay and count in
 * PtStats.device_bytes from then on.  A renderer that never asks for the device path allocates nothing of this.
 * What the device build does not take runs on the host, with the same result, and PtSetCameraTimes.fallback says why:
 * PT_DEVICE_TABLES_LIST: a cell of a forced grid (debug_flags 256) lists more than 4096 records (the host refuses such a grid unless
 * it is forced); PT_DEVICE_TABLES_CELLS: the grid has more than 2^22 cells. */
#define PT_SET_CAMERA_DEVICE_TABLES 1u
#define PT_DEVICE_TABLES_LIST 1
#define PT_DEVICE_TABLES_CELLS 2
int pt_set_camera_ex(const PtCamera* cam, uint32_t flags);
/* The last move of the renderer (pt_set_camera or pt_set_camera_ex), host wall clock, milliseconds; all zero before the first. */
typedef struct PtSetCameraTimes {
  double tables_ms;  /* the camera-dependent tables: host build + upload, or the device build with its one readback (the first
                        device-path move: with the upload of the camera-independent tables and the workspace's allocation)   */
  double rearm_ms;   /* launch plan, path buffers and records back to their first state, the worker, pt_clear              */
  double total_ms;   /* = PtSetupTimes.set_camera_ms                                                                        */
  int32_t path;      /* 0 host tables, 1 device tables                                                                     */
  int32_t fallback;  /* 0, or why a requested device build ran on the host (PT_DEVICE_TABLES_*); path is then 0            */
} PtSetCameraTimes;
int pt_get_set_camera_times(PtSetCameraTimes* out);
/* ---- moving the objects of a live renderer: new transforms for the geoms it was created with, without pt_free + pt_init.
 * Only the three matrices of a geom may change (for a PT_GEOM_TRIANGLE: its vertex words, which live in `transform`); num_geoms and
 * every type and materialid stay, so the material table, the mesh switch and the per-geom tables of the history stay valid.
 * Contract: pt_set_camera's, word for word — after a successful call every later call gives what a renderer freshly created from the
 * same scene with these geoms, the same options and the renderer's current camera gives, bit for bit in all three PT_ARITH_* modes
 * (image, feature buffers, noise planes, adaptive lists and counts, resolved and filtered images); the timing fields, which traversal
 * structure is walked and PtStats.device_bytes may differ.
 * What happens: synchronise; the scene tables are built on the host by the code pt_init runs (the BVH, the top list, the geom table,
 * the root bounds, everything that follows the camera), with the grid resolution pt_init chose or no grid (a grid that cannot be
 * built for the new geoms falls back to the BVH scan until a later call allows it again: the camera move's rule) and WITHOUT the
 * materials: the material table on the device is left alone, so the renderer keeps no materials on the host.  Every table is written
 * into the buffer it has where its size is unchanged, else into a new one (the top list's length follows the tree).  The device
 * copy of the camera-independent tables (PT_SET_CAMERA_DEVICE_TABLES) is dropped; the next such move uploads the new one.  Then what
 * pt_set_camera does after its tables: the launch plan, the worker, the batch buffers' first state, pt_clear.
 * History: K, the kept camera and the kept geoms survive; C, VC and E become absent.  The plain lookup knows nothing of the move: it
 * treats the world as static.  PT_HISTORY_MOTION (below) follows moved objects.
 * Refused, in this order, with nothing changed, allocated or launched: no renderer; a failed renderer; null `geoms`; num_geoms other
 * than the renderer's; the first geom whose type or materialid differs (named by index); the first geom with a matrix element
 * that is not finite (named by index). */
int pt_set_geoms(const PtGeom* geoms, int num_geoms);
/* The last pt_set_geoms of the renderer, host wall clock, milliseconds; all zero before the first. */
typedef struct PtSetGeomsTimes {
  double build_ms;  /* synchronise + the host build of the tables                                          */
  double upload_ms; /* the tables onto the device                                                          */
  double rearm_ms;  /* launch plan, path buffers and records back to their first state, the worker, pt_clear */
  double total_ms;
} PtSetGeomsTimes;
int pt_get_set_geoms_times(PtSetGeomsTimes* out);
/* ---- editing the materials of a live renderer: new PtMaterials for the ones it was created with, without pt_free + pt_init.
 * The count stays; every word of a material may change.  The words the renderer reads are color, specular_color, hasReflective,
 * hasRefractive and emittance (the nine words of the device table).
 * Contract: pt_set_camera's and pt_set_geoms', word for word — after a successful call every later call gives what a renderer
 * freshly created from the same scene with these materials, the same options and the renderer's current camera and geoms gives, bit
 * for bit in all three PT_ARITH_* modes (image, feature buffers — the albedo plane changes —, noise planes, adaptive lists and
 * counts, resolved and filtered images); the timing fields, which traversal structure is walked and PtStats.device_bytes may differ.
 * What happens: synchronise; the material table is made by the code pt_init runs and uploaded into the table the renderer has
 * (nothing is allocated); the per-geom tables of the history that follow the materials (reject_geom, emitter_geom) are rebuilt at
 * their next use, in place; then what pt_set_camera does after its tables: the launch plan, the worker, the batch buffers' first
 * state, pt_clear.  The full re-arm is deliberate: whether a camera ray survives depth 0 follows the emittance of what it hits, and
 * the first-hit records are reused from batch to batch.  The renderer keeps a host copy of its PtMaterials from pt_init on (44 B each).
 * History: K, VK, FK, the kept camera, the kept geoms and the kept materials survive, and so do the probes PK; C, VC, FC, P and E
 * become absent.  The lookup without PT_HISTORY_MATERIALS (below) knows nothing of the edit.
 * Refused, in this order, with nothing changed, allocated or launched: no renderer; a failed renderer; null `materials`;
 * num_materials other than the renderer's (adding or removing materials needs pt_init); the first material, named by index, with a
 * word the renderer reads that is not finite.
 * Not built: adding or removing materials or objects; textures; a re-arm lighter than the camera move's; the pathtrace.h shim, which
 * keeps re-initialising when materials differ. */
int pt_set_materials(const PtMaterial* materials, int num_materials);
/* The last pt_set_materials of the renderer, host wall clock, milliseconds; all zero before the first. */
typedef struct PtSetMaterialsTimes {
  double upload_ms; /* synchronise + the table onto the device                                             */
  double rearm_ms;  /* launch plan, path buffers and records back to their first state, the worker, pt_clear */
  double total_ms;
} PtSetMaterialsTimes;
int pt_get_set_materials_times(PtSetMaterialsTimes* out);
/* Host wall-clock times of a renderer's setup, in milliseconds: the host build of the scene tables, their upload, the
 * allocation of the batch buffers, the timing probe of the traversal structures (0 where none ran), and the last pt_set_camera
 * (its synchronise included) with the number of such calls since the renderer was created. */
typedef struct PtSetupTimes {
  double tables_ms, upload_ms, buffers_ms, probe_ms, set_camera_ms;
  int32_t set_camera_calls;
} PtSetupTimes;
int pt_get_setup_times(PtSetupTimes* out);
/* Host-only check of the rebuild (no GPU): builds the tables for `scene`, moves them to `cam` with the code pt_set_camera runs,
 * builds fresh tables for `scene` with `cam` at the same grid resolution (the cost model's for scene->camera, where the scene
 * has a grid) and compares byte for byte.  *differing receives a bit per table that differs: 1 nodes, 2 their centre / half
 * extent copies, 4 the top list, 8 its copies, 16 geoms, 32 materials, 64 the cull margin, 128 the grid's shape (or that only one
 * side has a grid), 256 its cell table with the guard cells, 512 its records, 1024 their copies, 2048 the count of tightened
 * leaves; bits 16 and up: the same after moving back to scene->camera, against the tables built first.  It must be 0.
 * grid_res_out: the grid at `cam` (0 0 0: none); *tight_leaves: the tightened leaves at `cam`.  center_half != 0: with the copies
 * the FAST build uploads. */
int pt_camera_tables_host(const PtSceneDesc* scene, const PtCamera* cam, int debug_flags, int center_half, int32_t grid_res_out[3],
                          int32_t* tight_leaves, int32_t* differing);
/* Host-only: the grid of a kFixed request over caller-supplied nodes, as the host build makes it for a forced grid and with the
 * decisions of the device build, so that it can be compared with pt_stage_camera_grid (below) byte for byte; the arguments, the
 * outputs and the refusals are that function's, under the name pt_camera_grid_host.  The grid is pt::build_grid's (forced, `res` taken as
 * given) with the guard cells and the centre / half extent copies camera_tables() adds. */
typedef struct PtTableNode { /* a node of the threaded BVH as the tables hold it (csrc/pt_device.h ptd::Node), 32 bytes */
  float bmin[3], bmax[3];
  int32_t skip; /* not read by the grid build                   */
  int32_t geom; /* >= 0: a leaf of that geom; -1: an inner node */
} PtTableNode;
#define PT_CAMERA_GRID_NONE 3 /* status: no grid (no frame for these bounds, no leaf, or more than 2^22 references) */
typedef struct PtCameraGridResult {
  int32_t res[3];                           /* `res` clamped to [1, 512]                                                         */
  float origin[3], cell_size[3], inv_cell_size[3], pad; /* the shape the kernels read (SceneTables::grid_*)                      */
  uint32_t guard;                           /* guard cells in front of and behind the cell table proper                          */
  int64_t num_cells;
  uint64_t refs;                            /* (leaf, cell) references; 0 where nothing was counted (PT_DEVICE_TABLES_CELLS, no frame) */
  uint32_t longest;                         /* records of the fullest cell; 0 where refs exceeds 2^22 (nothing is counted then)   */
  int32_t status;                           /* 0 built, PT_DEVICE_TABLES_LIST, PT_DEVICE_TABLES_CELLS or PT_CAMERA_GRID_NONE      */
} PtCameraGridResult;
int pt_camera_grid_host(const PtTableNode* nodes, int num_nodes, const int32_t* geom_types, int num_geoms, const float root_min[3],
                        const float root_max[3], double coord_mag, const int32_t res[3], int center_half, PtCameraGridResult* out,
                        uint32_t* start, uint64_t start_cap, PtGridRecord* items, PtGridRecord* items_b, uint64_t items_cap);
const char* pt_last_error(void);
/* Device self-check.  The exact and fma kernels (and depth 0 of every mode) take correctly rounded square roots,
 * reciprocals and quotients from instruction sequences shorter than the compiler's general expansions whenever every
 * lane's operands are in a range where the two are the same computation (csrc/pt_kernels.hip, namespace ieee).  This runs
 * both side by side on the GPU and counts results that differ in any bit: kind 0 sqrt(x), 1 1/x, 2 1/sqrt(x) over the
 * `count` bit patterns starting at `first` (2^32 patterns = every float); kind 3 a/b, 4 the shared-reciprocal forms over
 * `count` pseudo-random operand sets derived from `seed` and the set's index first + i.  `arith` selects the kernel build. */
int pt_selfcheck_ieee(int arith, int kind, uint64_t first, uint64_t count, uint32_t seed, uint64_t* mismatches);
/* Device measurement of the scalar primitives a mode's kernels are built from, against double precision on the GPU
 * (csrc/pt_fast_math_check.inc): *max_err = the largest error over `count` operands starting at `first`.
 * kind 0 the reciprocal, 1 the square root, 2 normalize()'s 1 / sqrt(x): x = the float with the bit pattern first + i, error in ulp
 * of the double result (zeros, subnormals, infinities, NaNs and results outside the normal range are passed over; 1, 2: x > 0);
 * kind 3 sin(2 pi u), 4 cos(2 pi u) of the direction sampling: u = the draw of the minstd state first + i (1 .. 2^31 - 2 covers every
 * value a draw can return), absolute error; 5, 6 sin and cos of the specular lobe's angle roughness u pi / 2 for roughness 1, 0.7,
 * 0.5 and 0.05, absolute; 7, 8 as 3, 4 but in ulp over the values above 1e-3 in magnitude.
 * fast: v_rcp_f32, v_sqrt_f32, v_rsq_f32, v_sin_f32 / v_cos_f32; fma: the IEEE sequences and ptmath::sincos_rev; exact: the IEEE
 * sequences and ptmath::sin_r / cos_r.  A NaN result reads as an infinite error. */
int pt_selfcheck_fast_math(int arith, int kind, uint64_t first, uint64_t count, double* max_err);
/* ---- convergence metric (PtOptions.convergence != 0).  For a tile pixel p after iteration i, with S the running SUM image and R
 * the reference frame (averaged radiance), computePSNR's terms (pathtrace.cu:184-201) in float32: cur = S[p] / float(i) per
 * component (correctly rounded), d = cur - R[p], term = d.x*d.x + d.y*d.y + d.z*d.z left to right without FMA contraction in
 * every arithmetic mode; SSE_i = sum over the tile's pixels of (double)term, added in a fixed order (no atomics: equal options give
 * equal bits).  The sums stay on the device until they are asked for; pt_render gains no synchronisation and no allocation.
 * Device memory the metric adds (PtStats.device_bytes), all allocated by pt_init:
 *     12 * pixel_count                                                   the reference frame
 *   +  8 * iters_per_batch * num_queues * PT_CONVERGENCE_WAVES           partial sums of one batch (PtStats has both factors)
 *   +  8 * PT_CONVERGENCE_CAPACITY                                       one SSE per iteration
 * pt_render fails for iterations outside 1 .. PT_CONVERGENCE_CAPACITY while the metric is on.
 * pt_clear (and a new pt_init) forget the curve and re-arm the capture of iteration N; a supplied frame survives pt_clear.
 * Unlike the reference, whose frame is a file-scope static that survives pathtraceInit, the frame belongs to the renderer. */
#define PT_CONVERGENCE_WAVES 16
#define PT_CONVERGENCE_CAPACITY 65536
/* The frame of PtOptions.convergence == -1: pixel_count * 3 floats of averaged radiance in tile order (pt_readback's layout
 * divided by the sample count), e.g. a 5000-spp render.  Synchronises. */
int pt_set_reference(const float* rgb_avg_host);
/* sse[j] = SSE of iteration iter_first + j, or -1 where there is none: the iteration was not rendered, lies outside the capacity,
 * or the frame did not exist yet (captured frame: iterations <= N).  Synchronises. */
int pt_get_convergence(int iter_first, int iter_count, double* sse);
/* "Iterations to clean image" (the reference's README metric): the smallest rendered iteration that has a PSNR above
 * threshold_db (the reference uses 35), or -1.  The reference's own code always reports 1, because iteration 1's FLT_MAX
 * placeholder passes `psnr > 35.0f` (pathtrace.cu:629); this is the README's meaning.  Synchronises. */
int pt_iterations_to_clean(float threshold_db, int* iteration);
/* Host-only: computePSNR's last lines.  mse = sse / (pixels * 3.0); FLT_MAX (the reference prints "Inf") when mse <= 1e-12,
 * else 10.0f * log10f(1.0f / float(mse)). */
float pt_psnr_from_sse(double sse, int64_t pixels);

/* ---- first-hit feature buffers: what the camera ray of every sample sees, summed per tile pixel (for a denoiser, an edge-avoiding
 * filter, per-object decisions, compositing).  For tile pixel p and iteration i the camera ray is the one depth 0 of pt_render
 * traces for sample (i, global pixel) — generateRayFromCamera, plus PtOptions.aa_jitter when the renderer has it on — and its
 * closest hit is computeIntersections' record: t, world normal, intersection point, geom.  The renderer keeps a SUM buffer of
 * PT_FEATURE_PLANES planes, each pixel_count float4 in tile order:
 *     plane   .x .y .z                                                   .w
 *     0       sum of the normals                                         sum of t over the iterations that hit
 *     1       sum of materials[geoms[g].materialid].color                number of iterations that hit (a float)
 *             (any material, emitters too)
 *     2       sum of the intersection points                             object id of the LAST iteration added: the int32 bit
 *                                                                        pattern of 1 + index in PtSceneDesc.geoms, 0 = miss
 *                                                                        (or nothing rendered yet)
 * A miss adds +0 to every sum.  Every sum is a float32 running sum in iteration order, ((s + v_a) + v_a+1) + ..., plain adds:
 * without anti-aliasing the same value is added iter_count times (not multiplied).  Depth 0 runs the reference's arithmetic in
 * every PT_ARITH_* mode, so the buffers are the same bit for bit in all three.  They accumulate across calls like the image and
 * independently of it (pt_render neither reads nor writes them, PtStats.samples / live_rays do not count feature passes);
 * pt_clear zeroes them, ids included.  Memory: 48 bytes per tile pixel, allocated and zeroed by the first pt_render_features
 * call (iter_count == 0 allocates and does nothing else) and part of PtStats.device_bytes from then on; pt_init and pt_render
 * allocate and launch nothing for them.  A call reads and writes the buffer once (96 B per pixel) whatever iter_count is.
 * iter_first < 1 or iter_count < 0 is an error, as is a readback before the first feature pass. */
#define PT_FEATURE_PLANES 3
int pt_render_features(int iter_first, int iter_count); /* asynchronous on the renderer's stream, like pt_render */
int pt_readback_features(float* planes_host);          /* PT_FEATURE_PLANES * pixel_count * 4 floats; synchronises */

/* ---- edge-avoiding à-trous wavelet filter (Dammertz et al. 2010) over the image and the first-hit feature buffers: a low-spp image
 * made usable on the device.  Specified to the bit: float32 throughout, every operation a separate IEEE operation in the order written
 * (no FMA contraction, correctly rounded division, denormals kept, no library transcendentals), so the result is the same in all
 * three PT_ARITH_* builds, on the host (pt_denoise_host) and on the device.  The tile must be whole contiguous rows (W x R); the filter
 * treats them as an image of their own.  With S the SUM image, s0 s1 s2 the feature SUM planes:
 *   prepare  hit = s1.w > 0;  c = S / samples;  hit: n = s0.xyz / s1.w, a = s1.xyz / s1.w, p = s2.xyz / s1.w;  miss: n = a = p = 0;
 *            unless keep_albedo: c_k = a_k > 0 ? c_k / a_k : c_k  (the filter then runs on irradiance-like values, textures stay sharp)
 *   level l = 0 .. levels - 1, step s = 1 << l, pixel (x, y):  acc = 0, wsum = 0; for j = -2 .. 2 (rows, outer), i = -2 .. 2:
 *            q = (x + i s, y + j s); the tap is skipped when q is outside the W x R rectangle or hit(q) != hit(x, y);
 *            dc = |c_l(q) - c_l(x, y)|^2, dn = |n(q) - n(x, y)|^2, dp = |p(q) - p(x, y)|^2, each (d.x d.x + d.y d.y) + d.z d.z;
 *            e = (dc * (inv_c * 4^l) + dn * inv_n) + dp * inv_p;  w = (H[j + 2] * H[i + 2]) * exp32(-e), H = 1/16 1/4 3/8 1/4 1/16;
 *            acc += w * c_l(q) per component (multiply, then add);  wsum += w;   c_l+1(x, y) = acc / wsum   (wsum >= 9/64: the centre)
 *   finish   out_k = a_k > 0 ? c_levels,k * a_k : c_levels,k unless keep_albedo, else c_levels
 * inv_* = 1.0f / (sigma * sigma) in float32, 0 for a term that is switched off; exp32 is ptmath::exp32 (csrc/pt_portable_math.h: +0
 * below -80, else a float32 polynomial).  The output is AVERAGED radiance (not a SUM), 3 floats per pixel, tile order, raw orientation.
 * Every field of the options: 0 = the default; the defaults were tuned on the cornell box at 4 spp (mean squared error against a
 * 1024-spp render 0.085 of the unfiltered image's). */
typedef struct PtDenoiseOptions {
  int32_t levels;       /* 1 .. 8; default 5 (reach 2 * 2^levels - 2 = 62 pixels)                               */
  float sigma_color;    /* default 4.0; < 0 switches the colour term off.  Tightens by 2 per level (4^l above)  */
  float sigma_normal;   /* default 0.5; < 0 switches the normal term off                                        */
  float sigma_position; /* default 1.0, scene units; < 0 switches the position term off                         */
  int32_t keep_albedo;  /* 0 = demodulate by the first-hit albedo (default); 1 = filter the radiance as it is   */
} PtDenoiseOptions;
/* Reads the image and the feature buffers (pt_render_features must have run) and changes neither, nor PtStats.samples.  Errors with a
 * message, allocating nothing: a striped or ragged tile, no feature pass yet, samples <= 0, levels outside 1 .. 8, a sigma that is
 * not finite, a failed context.  Workspace: 80 bytes per tile pixel (normal + hit flag, position, albedo, two colour buffers, float4
 * each), allocated by the first denoise call of a renderer, part of PtStats.device_bytes from then on, kept across pt_clear.
 * opt == NULL: all defaults.  rgb_avg_host receives pixel_count * 3 floats.  Synchronises. */
int pt_denoise(float samples, const PtDenoiseOptions* opt, float* rgb_avg_host);
/* The same filter on the host, for a frame of w x rows pixels: S w*rows*3 floats, planes PT_FEATURE_PLANES * w*rows * 4 floats
 * (pt_readback_features' layout), out w*rows*3 floats.  Needs no GPU; the device result equals it bit for bit. */
int pt_denoise_host(int w, int rows, const float* rgb_sum, const float* planes, float samples, const PtDenoiseOptions* opt, float* rgb_avg);

/* ---- noise estimate from batch sums, and rendering until a target PSNR.  pt_get_convergence says how far the image is from a given
 * frame; this says how noisy the image is when there is no such frame, so that a renderer can stop by itself.  The SUM image S is
 * looked at only at group boundaries (batches of iterations, never single samples) by a streaming kernel of its own
 * (csrc/pt_noise.hip); pt_render and its kernels know nothing of it.  Specified to the bit, like the filter above: float32 throughout,
 * every operation a separate IEEE operation in the order written (no FMA contraction, correctly rounded division, denormals kept),
 * so the planes are the same in all three PT_ARITH_* builds, on the host (pt_noise_fold_host) and on the device.
 * State: PT_NOISE_PLANES planes, each pixel_count float4 in tile order:
 *   plane 0  prev.xyz (S at the last fold), w   (the estimate, below)
 *   plane 1  q.xyz,                          +0
 * all zero at allocation and after pt_clear (S is zero then too).  Per renderer: groups M, iterations T folded so far, and `rendered`,
 * the iterations handed to pt_render since pt_init or pt_clear (pt_reset_stats leaves it alone).
 * A fold takes all iterations rendered since the last fold as ONE group of n = rendered - T iterations; n == 0: nothing happens.
 * Then M += 1, T += n and, with nf = (float)n, Tf = (float)T, Df = (float)(M - 1) * Tf, per pixel and component k = x, y, z:
 *   b = S_k - prev_k;   q_k = q_k + (b * b) / nf;   prev_k = S_k
 *   M >= 2:  d = q_k - (S_k * S_k) / Tf;   v_k = (d > 0 ? d : 0) / Df
 *   w = M >= 2 ? (v_x + v_y) + v_z : +0
 * w estimates the variance of the pixel's AVERAGED radiance, summed over the channels: with group sums B_j of n_j samples,
 * sum_j B_j^2 / n_j - S^2 / T has expectation (M - 1) sigma^2 for any group sizes, and sigma^2 / T is the variance of the mean.
 * Frame statistic: SSE_est = sum over the tile pixels of (double)w, in the unit of pt_get_convergence's SSE against a converged
 * frame; estimated PSNR = pt_psnr_from_sse(SSE_est, pixel_count).  On the device every PT_NOISE_PIXELS_PER_PARTIAL consecutive tile
 * pixels give one double, and a second launch adds those in index order: no atomics, equal tiles and equal folds give equal bits.
 * The host function adds in pixel order; the two may differ in the last bits.
 * Memory: 32 * N + 8 * (ceil(N / PT_NOISE_PIXELS_PER_PARTIAL) + 1) bytes for a tile of N pixels, allocated and zeroed by the first
 * fold that has something to fold, part of PtStats.device_bytes from then on, kept across pt_clear, which zeroes it and M, T. */
#define PT_NOISE_PLANES 2
#define PT_NOISE_PIXELS_PER_PARTIAL 1024
int pt_noise_fold(void); /* asynchronous on the renderer's stream; changes neither the image nor PtStats.samples */
/* Synchronises.  *sse = SSE_est of the last fold, -1 while groups < 2 (or nothing has been folded); any pointer may be NULL. */
int pt_get_noise(double* sse, int* groups, int* iterations);
int pt_readback_noise(float* planes_host); /* PT_NOISE_PLANES * pixel_count * 4 floats; synchronises; an error before the first fold */
/* Render until the image is clean: groups of group_iters iterations (0 = PtStats.iters_per_batch; the last one is cut so that no
 * more than max_iters are rendered) from iteration iter_first on, a fold after each, then the one double is read (one synchronise
 * per group).  Stops after the first fold with groups >= 2 whose estimated PSNR is above target_db (`>`, like
 * pt_iterations_to_clean), or at max_iters; returns 0 either way.  *iters_done: iterations rendered by this call; *psnr_db: the
 * last estimate, -1 when there is none (either may be NULL).  Groups folded before the call count; iterations rendered but not
 * yet folded join the first group.  Errors, with nothing rendered or allocated: iter_first < 1, max_iters < 1 (or iterations past
 * 2^31 - 1), group_iters < 0, a target that is not finite, a failed context. */
int pt_render_until(int iter_first, int max_iters, int group_iters, float target_db, int* iters_done, float* psnr_db);
/* One fold on the host (no GPU): rgb_sum pixels*3 floats (S), planes PT_NOISE_PLANES * pixels * 4 floats, updated in place;
 * group_iters = n, groups_after = M and iters_after = T after this fold; *sse (may be NULL) = the estimates added in pixel order, -1
 * while groups_after < 2.  The device's planes equal it bit for bit. */
int pt_noise_fold_host(int pixels, const float* rgb_sum, float* planes, int group_iters, int groups_after, int64_t iters_after, double* sse);

/* ---- variance-guided form of the filter above (the step from Dammertz-style a-trous to SVGF-style filtering): the colour term of a
 * pixel is scaled by that pixel's own variance, taken from the noise estimate, instead of one global sigma_color tightened by 4^l.
 * Clean pixels keep their detail, noisy ones are smoothed, and the variance is filtered along with the colour, so it shrinks by
 * itself from level to level.  pt_denoise keeps its specification and its results.  Same rules: float32 throughout, every operation
 * a separate IEEE operation in the order written, no contraction, correctly rounded division, denormals kept.  Everything not
 * mentioned is pt_denoise's specification (skipped taps, dn, dp, H, exp32, rows outer and columns inner, finish).
 * Inputs: S, s0 s1 s2 as above; the noise planes prev.xyz | w and q.xyz | 0; the fold counters M >= 2 and T;
 * Tf = (float)T, Df = (float)(M - 1) * Tf.  `samples` is no parameter: c = S / Tf.
 *   prepare  as pt_denoise with samples = Tf, plus per component k:  d = q_k - (prev_k * prev_k) / Tf;  v_k = (d > 0 ? d : 0) / Df
 *            (the fold's own v_k, bit for bit, when nothing was rendered since the last fold);
 *            unless keep_albedo: v_k = a_k > 0 ? v_k / (a_k * a_k) : v_k;    var_raw = (v_x + v_y) + v_z
 *   variance prefilter, once:  var_0(x, y) = (sum g var_raw(q)) / (sum g)  over j = -1 .. 1 (rows, outer), i = -1 .. 1, q = (x + i, y + j),
 *            g = G[j + 1] * G[i + 1], G = 1/4 1/2 1/4, both sums started at 0 and added to in that order (multiply, then add); a tap is
 *            skipped when q is outside the rectangle or hit(q) != hit(x, y).  (A batch estimate from M - 1 = 1 .. 3 degrees of freedom
 *            is too noisy to guide a filter raw.)
 *   level l  per centre, once:  cf = inv_c / (var_l(x, y) + PT_DENOISE_VARIANCE_FLOOR)   (no 4^l);  vsum = 0
 *            per tap:  e = (dc * cf + dn * inv_n) + dp * inv_p;  w = h * exp32(-e);  the colour sums as in pt_denoise;
 *                      vsum = vsum + (w * w) * var_l(q)
 *            c_l+1 = acc / wsum;   var_l+1 = vsum / (wsum * wsum)
 * A centre of variance 0 (a miss, an emitter, a pixel whose groups agree) accepts only taps of its own colour: intended.
 * PtDenoiseOptions is reused; here sigma_color == 0 means 8.0, and sigma_color < 0 switches the colour term off (inv_c = 0, cf = +0):
 * the result then equals pt_denoise's with the colour term off and samples = T, bit for bit.
 * Errors with a message, allocating nothing: everything pt_denoise refuses, nothing folded yet, fewer than 2 groups folded, iterations
 * rendered since the last fold ("fold first": the planes would not belong to the image).  The workspace is pt_denoise's 80 bytes per
 * pixel, shared with it (var_raw lives in the albedo buffer's spare word, var_l in the colour buffers'); neither the image, the
 * feature buffers, the noise planes nor any counter changes.  Synchronises. */
#define PT_DENOISE_VARIANCE_FLOOR 1e-8f
int pt_denoise_guided(const PtDenoiseOptions* opt, float* rgb_avg_host);
/* The same on the host (no GPU): pt_denoise_host's arrays, noise_planes PT_NOISE_PLANES * w*rows * 4 floats (pt_readback_noise's
 * layout), groups = M and iters = T of the folds that made them.  The device result equals it bit for bit. */
int pt_denoise_guided_host(int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, int groups, int64_t iters,
                           const PtDenoiseOptions* opt, float* rgb_avg);
/* Host-only, for tests and tuning: the two variances the levels start from, w*rows floats each (either may be NULL). */
int pt_denoise_guided_variance_host(int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, int groups, int64_t iters,
                                    const PtDenoiseOptions* opt, float* var_raw, float* var_0);

/* ---- adaptive sampling: after a uniform warm-up, further groups of iterations are rendered over the noisiest pixels only.  The
 * noise estimate above says where the variance is; a ROUND picks the m pixels with the largest (prefiltered) estimate, renders a
 * group of iterations for those pixels alone and merges the group into the image and the estimate.  From the first round on the
 * renderer is in the ADAPTIVE STATE (until pt_clear): pixels differ in their sample counts, the SUM image S means something only
 * together with the per-pixel counts, and pt_resolve gives the averaged radiance.  Selection, merge and resolve are kernels of
 * their own (csrc/pt_adaptive.hip), specified to the bit like the fold: float32 throughout, every operation a separate IEEE
 * operation in the order written (no FMA contraction, correctly rounded division, denormals kept), the same in all three PT_ARITH_*
 * builds, on the host (pt_adaptive_select_host, pt_adaptive_merge_host) and on the device.  The tile must be whole contiguous rows
 * (W x R), as for pt_denoise.
 * State: the plane cnt, N x {int32 T_p, int32 M_p} (iterations and groups of pixel p; 8 bytes per pixel), allocated by the first
 * round together with the selection's workspace (4 B per pixel of keys, 4 B per pixel of list, 24 KiB of histograms, 8 B per 1024
 * pixels), set to the fold's (T, M) for every pixel by the first round since pt_init / pt_clear; pt_clear frees nothing and zeroes it.
 * Key, per pixel p before every round, with w_p the estimate in noise plane 0:
 *   Tf_p = (float)T_p;   s_p = w_p * Tf_p                      (the per-sample variance)
 *   num = 0, den = 0;  for j = -1, 0, 1 (rows, outer) and i = -1, 0, 1, skipping only taps outside the W x R rectangle:
 *       g = G[j + 1] * G[i + 1]  with G = 1/4, 1/2, 1/4;   num = num + g * s(q);   den = den + g        (multiply, then add)
 *   f_p = num / den;   key_p = f_p / Tf_p
 * The sort key is the uint32 bit pattern of key_p (every value is >= +0, so the order is the float order); a NaN of any sign and
 * payload becomes 0xffffffff and so sorts first.  The raw w_p, with one to three degrees of freedom behind it, must not be the key:
 * pixels whose first groups happen to agree would be starved for good (simulated: worse than uniform sampling by 1.2x to 3.7x in MSE);
 * the 3x3 binomial prefilter is the one pt_denoise_guided applies to its variance for the same reason.
 * Select: m = clamp(ceil((double)fraction * N), 1, N).  The list holds the m pixels with the largest key, equal keys resolved by
 * the smaller tile index, stored in ascending tile index.  On the device a radix select (11 / 11 / 10 bits, integer atomics on
 * histogram bins only) finds the threshold key and the number of pixels equal to it to take, and a counting pass, a scan and a
 * scatter write the list; no host synchronisation, equal inputs give an equal list.
 * Render: a worker context owned by the renderer, whose tile is the list (created by the first round, replaced when m differs from the capacity it was planned for,
 * its memory part of PtStats.device_bytes), renders iterations iter_first .. iter_first + G - 1 (global iteration numbers, the RNG
 * keyed by the global pixel as everywhere) for the listed pixels into a cleared group sum Sw[m][3], with the renderer's arithmetic
 * mode, scene tables, traversal choice and options; iters_per_batch and num_queues of 0 are automatic for m pixels.  Pixels outside
 * the list have no sample in those iterations.  PtStats.samples counts the worker's samples; live_rays, the kernel timings and
 * iters_per_batch stay those of the renderer's own whole-tile launches.
 * Merge, for i < m with p = list[i], nf = (float)G, per component k:
 *   b = Sw[i].k;   S_p.k = S_p.k + b;   q_k = q_k + (b * b) / nf;   prev_k = S_p.k
 * then  T_p += G;  M_p += 1;  Tf = (float)T_p;  Df = (float)(M_p - 1) * Tf;
 *   d = q_k - (S_k * S_k) / Tf;   v_k = (d > 0 ? d : 0) / Df;   w = (v_x + v_y) + v_z
 * Pixels outside the list keep every word.  SSE_est = sum of (double)w over ALL tile pixels in the fold's order (one double per
 * PT_NOISE_PIXELS_PER_PARTIAL consecutive pixels, those in index order), left where a fold leaves it.
 * Resolve: c_p = S_p / (float)T_p per component, averaged radiance.  Valid in the uniform state too (T_p = T for every pixel);
 * needs at least one fold and nothing rendered since the last fold.
 * What to know before relying on it:
 *   - Sampling by an ESTIMATED variance makes the image a biased estimator: whether a pixel receives more samples depends on the
 *     samples it already has.  The bias falls with the warm-up length; it is not corrected.
 *   - The frame statistic turns optimistic under selection: the pixels that underestimate their variance are the ones skipped.
 *     Simulated on the CPU (cornell 96x54, depth 8, two uniform groups of 4, rounds of 4 over a quarter of the pixels, 32 iterations'
 *     worth of samples): SSE_est is 0.80 to 0.90 of the actual squared error, 0.5 to 1 dB in the estimated PSNR; measured on an
 *     MI355X in that configuration (tests/test_gpu_adaptive.py): 0.843, the estimate reading 33.84 dB where the image has 33.10 dB.
 *   - A pixel whose first two groups agree exactly has w = 0 and is sampled again only through its neighbours' variance (the
 *     prefilter).  For background and emitter pixels that is the point; a pixel that is noisy but unlucky twice is reached the same way.
 * A group (pt_group_*) has the threshold round and its driver, below: the frame's selection runs once, on the root device.  Out of
 * scope: a group form of THIS round and of pt_render_adaptive, and any tuning of the path-tracing kernels for incoherent lists; a list
 * length that varies from round to round is pt_adaptive_round_threshold, below.  pt_denoise and pt_denoise_guided refuse the adaptive state; pt_denoise_adaptive
 * (below) is the filter that reads the per-pixel counts.
 * In the adaptive state pt_readback (S), pt_get_noise (sse = the last merge's, groups = M + rounds, iterations = the highest
 * iteration number folded or merged), pt_readback_noise, pt_render_features and pt_get_stats still work; pt_render, pt_noise_fold,
 * pt_render_until, pt_denoise, pt_denoise_guided, pt_save_u8 and pt_preview_rgba8* fail with a message that names pt_resolve and
 * pt_clear.  A renderer that never calls the functions below behaves, allocates and launches as before. */
/* One round: key, select, render, merge; asynchronous on the renderer's stream.  Errors, with nothing rendered or allocated: fewer
 * than 2 groups folded, iterations rendered since the last fold ("fold first"), a striped or ragged tile, PtOptions.convergence != 0,
 * fraction outside (0, 1], group_iters < 1, iter_first < 1, a failed context. */
int pt_adaptive_round(int iter_first, int group_iters, float fraction);
/* pt_render_until with rounds: while fewer than 2 groups are folded, uniform groups of group_iters iterations with a fold each,
 * exactly as pt_render_until; then rounds of group_iters iterations over the fraction.  group_iters == 0: the worker's iterations
 * per batch.  One synchronise per group or round; stops after the first estimate above target_db or when max_iters iteration
 * numbers are used up (the last group is cut).  *iters_done: iteration numbers used; *samples_done: pixel-samples rendered by this
 * call; *psnr_db: the last estimate, -1 when there is none (any may be NULL). */
int pt_render_adaptive(int iter_first, int max_iters, int group_iters, float fraction, float target_db, int* iters_done, int64_t* samples_done,
                       float* psnr_db);
int pt_readback_adaptive(int32_t* counts); /* pixel_count * 2 int32: T_p, M_p (the uniform state: the fold's T, M); synchronises */
int pt_resolve(float* rgb_avg_host);       /* pixel_count * 3 floats of averaged radiance; synchronises */
/* The selection on the host (no GPU): noise_planes as pt_readback_noise gives them (plane 0 is read), counts w*rows * 2 int32 with
 * every T_p >= 1, 1 <= m <= w*rows; list receives m tile indices.  The device's list equals it. */
int pt_adaptive_select_host(int w, int rows, const float* noise_planes, const int32_t* counts, int m, int32_t* list);
/* A merge on the host (no GPU): rgb_sum (S), planes and counts of `pixels` tile pixels are updated in place from group_sum (m * 3
 * floats, the sums of group_iters iterations of the pixels list[0 .. m), distinct); *sse (may be NULL) = the estimates of all
 * pixels added in pixel order.  The device's image, planes and counts equal it bit for bit. */
int pt_adaptive_merge_host(int pixels, float* rgb_sum, float* planes, int32_t* counts, const int32_t* list, int m, const float* group_sum,
                           int group_iters, double* sse);

/* ---- adaptive sampling until every pixel is below a noise threshold: rounds whose list is the pixels ABOVE an absolute threshold,
 * so that it shrinks as the frame cleans up and a round over an almost clean frame costs what its few pixels cost.  Key, render,
 * merge, resolve and the adaptive state are those of pt_adaptive_round, bit for bit; only the selection differs, and the two kinds of
 * round may alternate on one renderer.
 * Threshold: thr = threshold * threshold, ONE float32 multiply (threshold is a standard error of the pixel's mean, summed over the
 * three channels like w; it must be finite and >= 0).  Pixel p is ABOVE iff bits(key_p) > bits(thr) as uint32, key_p exactly the key
 * above (NaN -> 0xffffffff): a key equal to thr is not above, a NaN key is above, a zero-variance pixel never is.
 * Counts: above = #{p above};  cap = clamp(ceil((double)max_fraction * N), 1, N)  (the fixed-fraction round's m);  m = min(above, cap).
 * List: the m above-pixels with the largest keys, equal keys resolved by the smaller tile index, in ascending tile index: every
 * above-pixel when above <= cap, and bit for bit the list of the top-cap selection when above > cap.
 * On the device the radix select runs for rank cap and leaves (tau, r); one more counting pass counts `above` (integer atomics only,
 * no float atomics: equal inputs give an equal list); count, scan and scatter then run with tau' = max(tau, bits(thr)) and
 * r' = tau > bits(thr) ? r : 0.  above and m stay in the selection's workspace, which is as large as it was.
 * Render: the worker context is planned and allocated ONCE, for cap pixels, as a fixed-fraction round's for m = cap; a round over
 * m <= cap pixels plans again only what follows from N (chunks per queue, paths per queue and batch, record slots per region) and
 * frees, allocates and clears nothing but the 3 * m floats of the group sum.  iters_per_batch and num_queues of 0 are automatic for
 * cap pixels.  A fixed-fraction round whose m equals the worker's capacity uses the same worker; another m replaces it.
 * What to know, besides the three caveats above, which all hold:
 *   - The threshold is ONE SIGMA of an ESTIMATE, not a bound, and the estimate reads low under selection (the pixels that
 *     underestimate their variance are the ones that stop).  Simulated (cornell 96x54, depth 8, groups of 4, threshold 0.05, cap 1):
 *     15 % of the pixels of the finished image have an actual error above the threshold, 1.6 % above twice the threshold.
 *   - Every round SYNCHRONISES: above and m are read back (8 bytes) before the group is launched, because the list's length decides
 *     the launches.  A fixed-fraction round does not.
 * A group runs these rounds as pt_group_adaptive_round_threshold / pt_group_render_threshold (below, after pt_group_render_until).  Out
 * of scope: longer groups for short lists, load balance between the contexts of a group whose parts differ in length, and a threshold relative to the pixel's brightness (simulated: worse than
 * uniform sampling at loose thresholds, the brightness of 8 samples being too noisy to normalise by). */
/* One round: key, select, read back, render, merge.  Refuses what pt_adaptive_round refuses, in the same order (max_fraction for
 * fraction), then a threshold that is negative or not finite; a refusal allocates and launches nothing.  The first call enters the
 * adaptive state even if it selects nothing.  m == 0: nothing is rendered or merged, no round is counted, SSE_est stays.  Otherwise
 * the first m entries of the list are rendered and merged and PtStats.samples grows by group_iters * m.  *above, *selected (either
 * may be NULL): the two counts. */
int pt_adaptive_round_threshold(int iter_first, int group_iters, float threshold, float max_fraction, int* above, int* selected);
/* The driver: while fewer than 2 groups are folded, uniform groups with a fold each exactly as pt_render_adaptive; then threshold
 * rounds.  Stops BEFORE rendering when above <= min_pixels (>= 0; the tail of short lists is mostly fixed cost), or when max_iters
 * iteration numbers are used up (the last group is cut).  group_iters == 0: the iterations per batch of a worker for cap pixels.
 * *iters_done: iteration numbers used; *samples_done: pixel-samples rendered by this call; *above_left: the last count, -1 when no
 * selection ran (any may be NULL).  pt_get_noise, pt_resolve, pt_readback_adaptive and pt_denoise_adaptive work afterwards as in any
 * adaptive state. */
int pt_render_threshold(int iter_first, int max_iters, int group_iters, float threshold, float max_fraction, int min_pixels, int* iters_done,
                        int64_t* samples_done, int* above_left);
/* The selection by threshold on the host (no GPU): pt_adaptive_select_host's arrays, 1 <= cap <= w*rows; list (cap entries) receives
 * *m tile indices, *above the count.  The device's list and counts equal it. */
int pt_adaptive_select_threshold_host(int w, int rows, const float* noise_planes, const int32_t* counts, float threshold, int cap, int32_t* list,
                                      int* above, int* m);
/* A round over a CALLER'S list: pt_adaptive_round without the selection, on any tile (a list needs no rows, so a striped or ragged
 * tile is not refused).  list_host: m distinct tile indices in ascending order, 0 <= m <= capacity; the worker is the one kept for
 * `capacity` pixels (1 <= capacity <= pixel_count; pt_adaptive_round_threshold's for cap), made live for m.  Render, merge, the
 * counters and PtStats.samples are pt_adaptive_round's, bit for bit.  m == 0 enters the adaptive state if need be, renders and merges
 * nothing and leaves SSE_est where it was, but DOES count the round and the highest iteration number (the contexts of a group stay
 * in step that way).  Asynchronous: the list is uploaded on the renderer's stream and nothing synchronises.
 * Refuses what pt_adaptive_round refuses, in its order, apart from the fraction and the tile's rows; then capacity or m out of range, a
 * null list with m > 0, and the first entry that is outside the tile or not above its predecessor, named by index.  A refusal
 * allocates and launches nothing.
 * On a striped tile the kernels want a list entry as an offset in the frame, p + (p / stripe) * (stride - stripe), where the merge
 * wants the tile index p: the renderer keeps the tile list and derives a second list for the worker on the device (4 more bytes per
 * tile pixel from the first such round on).  A contiguous tile has one list, as before. */
int pt_adaptive_round_list(int iter_first, int group_iters, const int32_t* list_host, int m, int capacity);

/* ---- variance-guided filter with per-pixel sample counts: pt_denoise_guided for an adaptively sampled image.  Valid in both states;
 * in the uniform state every pixel has the fold's (T, M), exactly as pt_readback_adaptive reports them.  Everything not stated here
 * is pt_denoise_guided's specification word for word: float32 throughout, every operation a separate IEEE operation in the order
 * written, no contraction, correctly rounded division, denormals kept; skipped taps, dn, dp, H, exp32, rows outer and columns inner;
 * the level formula with cf = inv_c / (var_l + PT_DENOISE_VARIANCE_FLOOR); var_l+1 = vsum / (wsum * wsum); finish; PtDenoiseOptions
 * with sigma_color == 0 meaning 8.0 and < 0 switching the colour term off.
 * Inputs: S, s0 s1 s2, the noise planes prev.xyz | w and q.xyz | 0 (the merge keeps prev == S), and the plane cnt = {T_p, M_p}.
 *   prepare  per pixel p:  Tf_p = (float)T_p;  Df_p = (float)(M_p - 1) * Tf_p;  c = S_p / Tf_p per component (pt_resolve's value bit
 *            for bit, before demodulation); n, a, p, hit and demodulation as pt_denoise; per component k:
 *            d = q_k - (prev_k * prev_k) / Tf_p;  v_k = (d > 0 ? d : 0) / Df_p   (the merge's own v_k bit for bit, or the fold's for
 *            a pixel no round has touched);  unless keep_albedo: v_k = a_k > 0 ? v_k / (a_k * a_k) : v_k;   var_raw = (v_x + v_y) + v_z
 *   variance prefilter, once, over the PER-SAMPLE variance (var_raw is the variance of a mean: where neighbours differ in their
 *            counts it is not one quantity; the argument and the arithmetic of pt_adaptive_round's selection key):
 *            num = 0, den = 0;  for j = -1 .. 1 (rows, outer), i = -1 .. 1, q = (x + i, y + j), skipped when q is outside the W x R
 *            rectangle or hit(q) != hit(x, y):   g = G[j + 1] * G[i + 1], G = 1/4 1/2 1/4;   s = var_raw(q) * Tf_q;
 *            num = num + g * s;   den = den + g   (multiply, then add);      var_0(x, y) = (num / den) / Tf_(x, y)
 *   levels and finish: the guided form's, unchanged (the same kernels).
 * In the uniform state with T a power of two the multiplication and the division by Tf are exact, and the result equals
 * pt_denoise_guided's bit for bit (barring subnormal products); with any other T the two agree to a few roundings of var_0
 * (tests/test_denoise_adaptive_host.py, 97 x 61: no pixel differs at T = 8; at T = 7, 1,920 of 5,917 differ, by at most 2.3e-7 relative).
 * Errors with a message, before anything is allocated or launched, in this order: a failed context; a striped or ragged tile; no
 * feature pass yet; nothing folded; iterations rendered since the last fold ("fold first"); fewer than 2 groups folded; levels, a
 * sigma or keep_albedo as pt_denoise_guided refuses them.  The adaptive state is not refused.
 * Nothing new is allocated: the workspace is the 80 bytes per pixel of pt_denoise and pt_denoise_guided, allocated by whichever of
 * the three runs first.  Tf_p travels in the position buffer's spare word (no tap reads it; the other two filters leave it 0),
 * var_raw in the albedo buffer's, var_l in the colour buffers'.  Neither the image, the feature buffers, the noise planes, the count
 * plane, the fold and round counters nor PtStats.samples change: a round after a filter call selects and renders what it would have
 * without the call.  Synchronises.
 * What it buys (cornell 96x54, depth 8, PT_ARITH_EXACT, MSE against 2048 spp; two uniform groups of 4 then rounds of 4 over a quarter
 * of the pixels, 32 iterations' worth of samples; default options): the raw adaptive image (a) has 4.903e-4, the filtered one (b) 8.080e-5, 32 uniform
 * iterations folded in four groups of 8 and filtered by pt_denoise_guided (c) 1.294e-4: b / a = 0.1648, b / c = 0.6242 — at equal
 * samples, filtered adaptive beats filtered uniform here.  These figures were simulated on the CPU (the oracle's samples with the
 * host fold, select, merge and filters) and measured on an MI355X (tests/test_gpu_denoise_adaptive.py); the two agree in every
 * printed digit, as they should: the exact build reproduces the oracle's samples bit for bit and the filter is specified to the bit.
 * One scene, one sample budget: no claim beyond it. */
int pt_denoise_adaptive(const PtDenoiseOptions* opt, float* rgb_avg_host);
/* The same on the host (no GPU): pt_denoise_guided_host's arrays, counts w*rows * 2 int32 (T_p, M_p; pt_readback_adaptive's layout)
 * with every M_p >= 2 and T_p >= M_p (the first pixel that breaks this is named in the refusal).  The device result equals it bit
 * for bit. */
int pt_denoise_adaptive_host(int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, const int32_t* counts,
                             const PtDenoiseOptions* opt, float* rgb_avg);
/* Host-only, for tests and tuning: the two variances the levels start from, w*rows floats each (either may be NULL). */
int pt_denoise_adaptive_variance_host(int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, const int32_t* counts,
                                      const PtDenoiseOptions* opt, float* var_raw, float* var_0);

/* ---- reprojected sample history: carry the image across a camera move.  pt_set_camera restores the state of a new renderer, so
 * every view of a moving camera starts at 0 spp; this unit keeps the previous view's blended image with its first-hit surface, looks
 * it up again from the new view's first hits, and blends it with the new samples.  Streaming kernels of their own
 * (csrc/pt_history.hip); pt_render, pt_clear, pt_set_camera and their kernels know nothing of it.  Specified to the bit like the
 * filters above: float32 throughout, every operation a separate IEEE operation in the order written (no FMA contraction, correctly
 * rounded division, denormals kept), dot products (a.x*b.x + a.y*b.y) + a.z*b.z, so the planes are the same in all three PT_ARITH_*
 * builds, on the host (pt_history_*_host) and on the device.
 * State, 64 bytes per tile pixel, allocated and zeroed by the first pt_history_capture and part of PtStats.device_bytes from then on
 * (a renderer that never calls these functions allocates and launches nothing for them):
 *   kept planes, PT_HISTORY_KEPT_PLANES planes of pixel_count float4, aligned to the camera of the last capture (kept on the host):
 *     K0 = blended colour xyz | weight Tk (a float sample count)      K1 = first-hit position xyz | object id (int32 bit pattern)
 *     K2 = first-hit normal xyz | +0
 *   current plane C = {h.xyz, Th}: the history resampled to the renderer's CURRENT camera; "absent" counts as all zero.
 * pt_history_reproject also keeps one byte per geom, reject_geom[g] = materials[geoms[g].materialid].hasReflective > 0 (a mirror's
 * radiance follows the view and must not be carried), allocated by the first call and counted like any buffer.
 * The tile must be whole contiguous rows (W x R), starting at frame row row0 = pixel_begin / W; taps outside the tile's rows are outside.
 * Lifetime: K and the kept camera survive pt_clear and pt_set_camera[_ex]; C becomes absent on both; pt_history_drop forgets K and C
 * and keeps the memory.
 *   blend, per component k:  m = h_k * Th;  a = S_k + m;  d = samples + Th;  c_k = a / d      (C absent: S_k / samples)
 *   capture  hit = s1.w > 0;  hit: n = s0.xyz / s1.w, p = s2.xyz / s1.w, id = bits(s2.w);  miss: n = p = 0, id = 0   (pt_denoise's prepare)
 *            K0.xyz = blend, K0.w = samples + Th;  K1 = p | id;  K2 = n | +0;  kept camera = the renderer's
 *   reproject  tile pixel (x, r), n p id from the CURRENT feature sums as above, cam = the kept camera, hw = (float)W * 0.5f,
 *            hh = (float)H * 0.5f — the inverse of generateRayFromCamera (pathtrace.cu:270-286) for the orthonormal view / up / right of
 *            pt_scene_load.  "Rejected" = C := 0.
 *     1  rejected on a miss; and, unless keep_view_dependent, when id is outside 1 .. num_geoms or reject_geom[id - 1] != 0
 *     2  v = p - cam.position;  dz = v . view;  rejected unless dz > 0
 *     3  sx = hw - (v . right) / (dz * pixelLength.x);  sy = hh - (v . up) / (dz * pixelLength.y)
 *     4  fx = floorf(sx), fy = floorf(sy);  rejected unless fx >= -1 && fx <= W - 1 && fy >= -1 && fy <= H - 1 (compared as floats
 *        before any conversion: NaN and infinity are rejected)
 *     5  ax = sx - fx;  ay = sy - fy
 *     6  acc = 0, tacc = 0, wsum = 0;  for j = 0, 1 (rows, outer), i = 0, 1:  q = (fx + i, fy + j - row0);  the tap is skipped when q is
 *        outside the W x R tile, K0(q).w is not > 0, id_K(q) != id, n . n_K(q) < min_normal_dot, or |n . (p_K(q) - p)| > plane_tol * dz;
 *        else b = (i ? ax : 1 - ax) * (j ? ay : 1 - ay);  acc_k = acc_k + b * K0(q).k;  tacc = tacc + b * K0(q).w;  wsum = wsum + b
 *     7  wsum >= 0.015625f:  h = acc / wsum;  t = tacc / wsum;  Th = t < cap ? t : cap;   else C = 0
 * The defaults are those of a CPU simulation on the cornell box (tests/test_history_sim.py; README "Reprojected history" has its
 * figures).  The bilinear lookup also smooths: the carried image is a BIASED estimator, and nothing here corrects that.
 * Groups of contexts: "history in groups" below (pt_group_history_*: a context's interleaved rows cannot look up their neighbours,
 * so the frame's history lives on the root device).  Out of scope: a selection key that uses the carried
 * variance; motion of anything but the camera.  (The filter over the blend: "variance of the history" below; extra samples for short
 * histories: "the history round" below; the history in the noise estimate, and a view rendered until the blend is clean: "the noise
 * estimate of the blend" below.) */
#define PT_HISTORY_KEPT_PLANES 3
typedef struct PtHistoryOptions { /* every field: 0 = the default */
  float cap;                   /* default 32: the most samples a carried colour counts for; finite and > 0                 */
  float min_normal_dot;        /* default 0.9; < 0 switches the normal test off                                            */
  float plane_tol;             /* default 0.02 (of the view depth dz); < 0 switches the plane-distance test off            */
  int32_t keep_view_dependent; /* 0 = pixels of reflective geoms carry nothing (default); 1 = they are carried like others */
} PtHistoryOptions;
/* Each refuses with a message that names it, nothing allocated or launched, in this order — capture: no renderer / a failed context; a
 * striped or ragged tile; the adaptive state (read the image with pt_resolve, or return with pt_clear); no feature pass
 * (pt_render_features) since the last clear or move; samples not finite or <= 0.  reproject: the same first three; nothing captured;
 * no feature pass since the last clear or move; an option out of range.  resolve: the same first three; samples; a null pointer.
 * capture and reproject are asynchronous on the renderer's stream; resolve (the blend for every pixel, pixel_count * 3 floats) and
 * the readback synchronise.  `samples` is the number of iterations the SUM image holds. */
int pt_history_capture(float samples);
int pt_history_reproject(const PtHistoryOptions* opt); /* NULL: all defaults.  Fills C from K and the current feature sums */
int pt_history_resolve(float samples, float* rgb_avg_host);
/* kept_planes: PT_HISTORY_KEPT_PLANES * pixel_count * 4 floats; current_plane: pixel_count * 4 floats, zeros while C is absent.  Either
 * may be NULL.  An error before the first capture. */
int pt_readback_history(float* kept_planes, float* current_plane);
int pt_history_drop(void);
/* The same arithmetic on the host (no GPU); the device results equal these bit for bit.  current_plane of the capture and the blend
 * may be NULL (absent).  reject_geom: num_geoms bytes, read unless opt->keep_view_dependent.  kept_cam->resolution is the FRAME's
 * W x H; the tile is rows row0 .. row0 + rows - 1 of it. */
int pt_history_capture_host(int pixels, const float* rgb_sum, const float* feature_planes, const float* current_plane, float samples, float* kept_planes);
int pt_history_reproject_host(int w, int rows, int row0, const PtCamera* kept_cam, const float* kept_planes, const float* feature_planes,
                              const uint8_t* reject_geom, int num_geoms, const PtHistoryOptions* opt, float* current_plane);
int pt_history_blend_host(int pixels, const float* rgb_sum, float samples, const float* current_plane, float* rgb_avg);

/* ---- variance of the history, and the variance-guided filter over the blend (temporal SVGF).  pt_denoise_guided sees the variance of
 * the current view's few samples only; the blend of pt_history_resolve has many effective samples but no variance.  With
 * PT_HISTORY_VARIANCE a variance travels with the history, and pt_history_denoise runs the guided filter on the blend with it.  Opt-in:
 * flags == 0 is the old call (the same kernels, arithmetic, memory and launches), and a renderer that never sets the flag allocates and
 * launches nothing for it.  Specified like the history above: float32 throughout, every operation a separate IEEE operation in the
 * order written, no FMA contraction, correctly rounded division, denormals kept; one implementation for kernels and host loops.
 * Variance state, a buffer of its own, 32 bytes per tile pixel, allocated and zeroed by the first capture with the flag and part of
 * PtStats.device_bytes from then on (the 64 bytes of the state above and K2.w = +0 stay as they are):
 *   VK = {vk.xyz, +0}: per-channel variance of the kept blended colour K0.xyz, aligned with K
 *   VC = {vh.xyz, +0}: VK resampled to the current camera, aligned with C
 * Lifetime: VK survives pt_clear and pt_set_camera[_ex] like K; VC becomes absent on both like C; pt_history_drop forgets both; a plain
 * pt_history_capture after a capture with the flag leaves VK invalid ("kept without variance"), a plain pt_history_reproject leaves
 * VC absent while C is present.
 *   new-sample variance, per component k, from the fold's planes prev, q with Tf = (float)T, Df = (float)(M - 1) * Tf:
 *            d = q_k - (prev_k * prev_k) / Tf;  vn_k = (d > 0 ? d : 0) / Df          (pt_denoise_guided's v_k before the albedo step)
 *   variance of the blend:  dn = samples + Th;  wn = samples / dn;  wh = Th / dn;  vb_k = (wn * wn) * vn_k + (wh * wh) * vh_k
 *            (C absent: Th = vh = +0)
 *   capture with the flag:  K exactly as without;  VK = {vb.xyz, +0}
 *   reproject with the flag:  C exactly as without, the same bits.  Step 6 also starts vacc = 0 and, for a tap that passed every
 *            test, adds vacc_k = vacc_k + b * VK(q).k after tacc (VK(q) is read after K0(q), for such a tap only);  step 7:
 *            vh_k = vacc_k / wsum.  A rejected pixel gets VC = 0.  Capping Th does not touch vh.  The variance is interpolated
 *            linearly, as SVGF interpolates its moments: conservative, since the lookup's smoothing lowers the true variance.
 *   pt_history_denoise: pt_denoise_guided with another prepare.  n, a, p and the hit flag as pt_denoise;
 *            c_k = blend(S_k, samples, C.k, C.w) (the blend above), demodulated like any colour;  v_k = vb_k, and unless keep_albedo
 *            v_k = a_k > 0 ? v_k / (a_k * a_k) : v_k;  var_raw = (v_x + v_y) + v_z in the albedo buffer's spare word.  Then the
 *            guided form's variance prefilter (the one without counts), levels and finish, unchanged: the same kernels.
 *            sigma_color == 0 means 8.0.  The workspace is the shared 80 bytes per pixel of the other filters.
 * With C and VC absent, samples == (float)T and S >= 0, wn = 1 and wh = 0, so vb = vn and the result equals pt_denoise_guided's bit
 * for bit (tests/test_history_variance_host.py).
 * Refusals, each with a message that names the function, nothing allocated or launched, in this order.  capture_ex and reproject_ex:
 * no renderer / a failed context; an undefined flag bit; then what pt_history_capture / _reproject refuse, in their order.  With the
 * flag capture_ex then refuses: nothing folded, or fewer than 2 groups folded; iterations rendered since the last fold ("fold
 * first"); samples != (float)T of the folds; C present but VC absent (the lookup was made without the flag).  With the flag
 * reproject_ex then refuses: nothing captured with variance.  pt_history_denoise: a failed context, a striped or ragged tile, the
 * adaptive state; no feature pass since the last clear or move; samples; levels, a sigma or keep_albedo as pt_denoise refuses them;
 * the fold conditions above; C without VC; a null buffer.
 * What it buys (cornell 96x54, depth 8, 8 views 3 degrees apart, 4 spp per view in 4 groups of 1, MSE against 1024 spp at the last
 * camera; tests/test_history_variance_sim.py on the CPU, tests/test_gpu_history_variance.py on an MI355X, the same digits): the blend
 * 4.525e-4, the filtered blend 1.396e-4 (0.3086 of it), pt_denoise_guided on the last view's own 4 spp 4.539e-4 (the filtered blend is
 * 0.3076 of it): history plus filter beats either alone.  The carried variance reads high (sum of VK 15.39 against the blend's squared
 * error 7.037 over the last view): recorded, not bounded.  One scene, one orbit: no claim beyond it.
 * Out of scope: pt_group_*.  (K keeps the unfiltered blend; feeding the FILTERED image back beside it: "the feedback" below, with the
 * moments kind only.)  A view with fewer than 2
 * folds (1 spp per frame) and a spatial estimate for disoccluded pixels: PT_HISTORY_MOMENTS, "moments with the history" below. */
#define PT_HISTORY_VARIANCE 1u
int pt_history_capture_ex(float samples, uint32_t flags);
int pt_history_reproject_ex(const PtHistoryOptions* opt, uint32_t flags);
int pt_history_denoise(float samples, const PtDenoiseOptions* opt, float* rgb_avg_host); /* synchronises; pixel_count * 3 floats */
/* pixel_count * 4 floats each; either may be NULL; zeros while the plane is absent (or kept without variance). */
int pt_readback_history_variance(float* kept_var, float* current_var);
/* The same arithmetic on the host (no GPU); the device results equal these bit for bit.  The capture's K is pt_history_capture_host's;
 * this gives VK beside it from the fold's planes (groups = M >= 2 folds over iters = T iterations, samples == (float)T) and C, VC
 * (both NULL: absent).  The lookup gives C — pt_history_reproject_host's, bit for bit — and VC in one pass. */
int pt_history_capture_variance_host(int pixels, const float* noise_planes, int groups, int64_t iters, float samples, const float* current_plane,
                                     const float* current_var, float* kept_var);
int pt_history_reproject_variance_host(int w, int rows, int row0, const PtCamera* kept_cam, const float* kept_planes, const float* feature_planes,
                                       const uint8_t* reject_geom, int num_geoms, const PtHistoryOptions* opt, const float* kept_var, float* current_plane,
                                       float* current_var);
/* pt_denoise_guided_host's arrays, samples, and C, VC (both NULL: absent). */
int pt_history_denoise_host(int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, int groups, int64_t iters, float samples,
                            const float* current_plane, const float* current_var, const PtDenoiseOptions* opt, float* rgb_avg);

/* ---- moments with the history: a variance from the differences BETWEEN views, and a spatial estimate for fresh pixels (SVGF's two
 * devices).  PT_HISTORY_VARIANCE takes the new samples' variance from pt_noise_fold, which needs two folded groups per view; a
 * moving camera at 1 spp per view has none.  With PT_HISTORY_MOMENTS the history carries a second moment beside the colour instead,
 * and pixels whose history is too short take their variance from their neighbourhood.  A third kind of history state beside "none"
 * and the variance; opt-in like it: with flags == 0 and with PT_HISTORY_VARIANCE every call keeps its results, memory, launches and
 * refusals, and a renderer that never sets the flag allocates and launches nothing for it.  Specified like the rest: float32
 * throughout, every operation a separate IEEE operation in the order written, no FMA contraction, correctly rounded division,
 * denormals kept; one implementation for kernels and host loops; the same result in all three PT_ARITH_* builds, host and device.
 * State: the moments reuse the 32-byte buffer of the variance kind (allocated by the first capture with either flag), and the
 * renderer remembers which kind each plane holds:
 *   VK = {m2.xyz, r}: m2 the per-channel second moment of the views' mean colours that formed K0.xyz, weighted as the colour was;
 *        r the sum of the squared weights of those views (1 for one view, 1/L for L equal views); aligned with K
 *   VC = {m2h.xyz, rh}: VK resampled to the current camera, aligned with C
 * Lifetime: that of VK / VC above.  pt_readback_history_variance returns the planes whichever kind they hold.
 *   capture with the flag:  K exactly as without; no fold is needed and none is read.  Per component k, with Th = C.w and
 *            m2h = rh = Th = +0 when C is absent:
 *            x_k = S_k / samples;  dn = samples + Th;  wn = samples / dn;  wh = Th / dn
 *            m2b_k = wn * (x_k * x_k) + wh * m2h_k;  rb = wn * wn + (wh * wh) * rh;  VK = {m2b.xyz, rb}
 *   reproject with the flag:  C exactly as without, the same bits.  Step 6 accumulates vacc over FOUR components x, y, z, w:
 *            vacc_k = vacc_k + b * VK(q).k after tacc, for a tap that passed every test;  step 7: VC.k = vacc_k / wsum for the four.
 *            A rejected pixel gets VC = 0.  Capping Th touches neither m2h nor rh.  (The lookup with PT_HISTORY_VARIANCE is untouched:
 *            three components, w = +0.)
 *   pt_history_denoise_ex(samples, opt, flags, rgb_avg_host): flags == 0 is pt_history_denoise, with its refusals under the new name;
 *            PT_HISTORY_VARIANCE is an undefined bit here; PT_HISTORY_MOMENTS selects the moments form, which reads no noise planes and
 *            has no fold conditions:
 *     prepare:  n, a, p and the hit flag as pt_denoise;  cb_k = blend(S_k, samples, C.k, C.w);  m2b, rb as in the capture above;
 *            d_k = m2b_k - cb_k * cb_k;  d_k = d_k > 0 ? d_k : 0
 *            rb <= PT_HISTORY_MOMENTS_R_MAX:  f = rb / (1.0f - rb);  v_k = d_k * f;  unless keep_albedo
 *                 v_k = a_k > 0 ? v_k / (a_k * a_k) : v_k;  var_raw = (v_x + v_y) + v_z
 *            otherwise (C absent included):  var_raw = -1.0f, the mark for the spatial estimate
 *            The colour c is cb demodulated as in every form.  d r / (1 - r) is the unbiased variance of the weighted mean: m2 - c^2
 *            underestimates the per-view variance by the factor (1 - r), and the blend's variance is r times that.
 *     spatial estimate, a launch of its own between prepare and the variance prefilter, for the marked pixels (var_raw == -1.0f)
 *            only, on the DEMODULATED colour c that prepare wrote:  wsum = s1 = s2 = 0;  for j = -3 .. 3 (rows, outer), i = -3 .. 3,
 *            q = (x + i, y + j), skipped when outside the W x R rectangle or hit(q) != hit(x, y):
 *            dn, dp as pt_denoise;  e = dn * inv_n + dp * inv_p;  w = exp32(-e)      (no colour term, no H)
 *            wsum = wsum + w;  s1_k = s1_k + w * c_k(q);  s2_k = s2_k + w * (c_k(q) * c_k(q))
 *            then  mean_k = s1_k / wsum;  u_k = s2_k / wsum;  d_k = u_k - mean_k * mean_k;  d_k = d_k > 0 ? d_k : 0;
 *            var_raw = (d_x + d_y) + d_z, written to the centre's own spare word only (the centre tap passes with w = 1, so
 *            wsum >= 1; no neighbour's var_raw is read, so the update in place has no hazard).
 *     then the guided form's variance prefilter (the one without counts), levels and finish, unchanged: the same kernels.
 *            sigma_color == 0 means 8.0.  The workspace is the shared 80 bytes per pixel.
 * Refusals, each with a message that names the function, nothing allocated or launched.  capture_ex / reproject_ex: the check of
 * the flag word keeps its place and now also refuses both bits together (the flags exclude each other).  After what
 * pt_history_capture / _reproject refuse, with the moments flag: capture — C present but filled by a lookup of another kind;
 * reproject — nothing captured with moments.  (Likewise the variance flag refuses a C or a K of the moments kind.)
 * pt_history_denoise_ex with the moments flag, in this order: a failed context; an undefined flag bit; a striped or ragged tile; the
 * adaptive state; no feature pass since the last clear or move; samples; levels, a sigma or keep_albedo as pt_denoise refuses them;
 * C present with VC absent or of the variance kind; a null buffer.
 * What it buys: README "Moments with the history" (tests/test_history_moments_sim.py on the CPU, tests/test_gpu_history_moments.py on
 * an MI355X, the same digits).  One scene, one orbit: no claim beyond it.
 * Groups of contexts: "history in groups" below.  Out of scope: feeding the moments into the noise estimate ("the noise estimate of the blend" below says why); a luminance-only variant; motion of anything but the
 * camera.  (Extra samples for the marked pixels: "the history round" below; feeding the FILTERED image back into the history: "the
 * feedback" below, opt-in — without it K keeps the unfiltered blend.) */
#define PT_HISTORY_MOMENTS 2u
#define PT_HISTORY_MOMENTS_R_MAX 0.3f /* four equal views or more (r = 1/4): the literature's history length 4 */
int pt_history_denoise_ex(float samples, const PtDenoiseOptions* opt, uint32_t flags, float* rgb_avg_host); /* synchronises */
/* The same arithmetic on the host (no GPU); the device results equal these bit for bit.  The capture's K is pt_history_capture_host's;
 * this gives VK beside it from the SUM image and C, VC (both NULL: absent).  The lookup gives C — pt_history_reproject_host's, bit
 * for bit — and VC in one pass. */
int pt_history_capture_moments_host(int pixels, const float* rgb_sum, float samples, const float* current_plane, const float* current_var, float* kept_var);
int pt_history_reproject_moments_host(int w, int rows, int row0, const PtCamera* kept_cam, const float* kept_planes, const float* feature_planes,
                                      const uint8_t* reject_geom, int num_geoms, const PtHistoryOptions* opt, const float* kept_var, float* current_plane,
                                      float* current_var);
/* pt_denoise_host's arrays, samples, and C, VC (both NULL: absent).  var_raw (w*rows floats; after the spatial step) and mark (w*rows
 * bytes: 1 where prepare marked the pixel) are optional outputs; with one of them rgb_avg may be NULL, and no level runs. */
int pt_history_denoise_moments_host(int w, int rows, const float* rgb_sum, const float* planes, float samples, const float* current_plane,
                                    const float* current_var, const PtDenoiseOptions* opt, float* rgb_avg, float* var_raw, uint8_t* mark);

/* ---- the history round: extra samples for the pixels whose history is short.  After the lookup, the pixels whose carried weight
 * Th = C.w is below min_history get a group of further iterations, for those pixels alone; blend, capture and the moments filter then
 * count these samples per pixel.  A capture writes K0.w = samples_p + Th, so a pixel that received extras is no longer short at the
 * next view: the round limits itself (but for the pixels of reflective geoms, which carry nothing and are selected at every view).
 * Opt-in: a renderer that never calls these functions allocates and launches nothing new, and every other call keeps its kernels,
 * memory, launches, results and refusals.  Specified like the rest of the history: float32, separate IEEE operations in the order
 * written, one implementation for kernels and host loops, the same bits in all three PT_ARITH_* builds, host and device.
 * State:
 *   E, the extra plane: pixel_count floats; E_p = the extra samples the SUM image holds for pixel p beyond the uniform `samples`.
 *        The first round that renders something allocates and zeroes it (PtStats.device_bytes counts it from then on); it is
 *        "present" from that round until pt_clear or pt_set_camera[_ex], which zero it and make it absent (S is zero then too).
 *        pt_history_drop leaves it: E belongs to S, not to K.
 *   emitter_geom: one byte per geom, materials[geoms[g].materialid].emittance > 0; the first round builds it.  An emitter seen
 *        directly has the same colour in every sample, so extra samples there buy nothing.
 *   the selection workspace and the worker of the adaptive rounds (pt_adaptive_round_threshold).
 * key (one thread per tile pixel; s1, s2 the feature sums, C the current plane — absent reads as Th = +0):
 *        hit = s1.w > 0;  id = bits(s2.w)
 *        key = +0 if !hit, or id outside 1 .. num_geoms, or emitter_geom[id - 1] != 0
 *        else Th = C.w;  d = min_history - Th;  key = d > 0 ? d : +0
 *        stored as its uint32 bit pattern.  A pixel is FRESH when bits(key) > 0.
 * select: pt_adaptive_round_threshold's selection on these keys with threshold bits 0 and cap = clamp(ceil((double)max_fraction * N), 1, N):
 *        fresh = #{key > 0}, m = min(fresh, cap); the list holds the m fresh pixels with the largest keys (the shortest histories),
 *        equal keys by the smaller tile index, in ascending tile index.  The two counts are read back: 8 bytes and ONE synchronise.
 * render: the worker, kept for cap pixels and live for m, renders iterations iter_first .. iter_first + G - 1 of the listed pixels
 *        into its cleared group sum Sw[m][3].  m == 0: nothing is rendered, merged or allocated beyond the selection; E keeps its state.
 * merge (one thread per list entry), p = list[i]:  S_p.k = S_p.k + Sw[i].k per component;  E_p = E_p + (float)G.  Pixels outside the
 *        list keep every word.  PtStats.samples grows by G * m.
 * Counted forms: while E is present, pt_history_resolve, pt_history_capture, pt_history_capture_ex with PT_HISTORY_MOMENTS and
 *        pt_history_denoise_ex with PT_HISTORY_MOMENTS use ns = samples + E_p — one float add per pixel, made before anything else —
 *        wherever their specification says `samples`: d = ns + Th, K0.w = ns + Th, x_k = S_k / ns, wn = ns / (ns + Th),
 *        wh = Th / (ns + Th), and the filter's prepare.  Kernel instantiations of their own; with E absent the ones that run are those
 *        that ran before.  With E all zero the counted forms give the uncounted results bit for bit.
 * While E is present, what reads S as a uniform SUM refuses with a message that names the function, pt_history_resolve and
 *        pt_clear, nothing allocated or launched: pt_noise_fold, pt_render_until, pt_denoise, pt_denoise_guided, pt_denoise_adaptive,
 *        pt_history_denoise, pt_history_denoise_ex with flags 0, pt_history_capture_ex with PT_HISTORY_VARIANCE (the fold's variance
 *        knows nothing of the extras), every adaptive round and driver, pt_resolve, pt_save_u8*, pt_preview_rgba8*.  These keep
 *        working: pt_render, pt_readback, pt_render_features, the lookups, pt_get_stats.
 * pt_history_round refuses, in this order, nothing allocated or launched: no renderer or a failed context; iter_first < 1,
 *        group_iters < 1 or iterations past 2^31 - 1; PtOptions.convergence != 0; a striped or ragged tile; the adaptive state; no
 *        feature pass since the last clear or move; an option that is not finite or out of range.  It needs no capture and no
 *        lookup: with C absent every non-emitter hit pixel is fresh (the first view).  fresh / selected may be NULL.
 * What it buys: README "History-guided sampling" (tests/test_history_round_sim.py).
 * Groups of contexts: "history in groups" below (pt_group_history_round).  Out of scope: a noise estimate of the blend while E is present (pt_history_noise refuses); scaling the spatial variance estimate by a pixel's extras;
 * a key that uses rh (one that uses the carried variance: "threshold rounds over the blend" below); motion of anything but the camera. */
#define PT_HISTORY_ROUND_MIN_HISTORY 4.0f /* the default of PtHistoryRoundOptions.min_history, in samples */
typedef struct PtHistoryRoundOptions { /* every field: 0 = the default */
  float min_history;  /* default 4.0 (samples): finite and > 0 */
  float max_fraction; /* default 1.0; in (0, 1] */
} PtHistoryRoundOptions;
int pt_history_round(int iter_first, int group_iters, const PtHistoryRoundOptions* opt, int* fresh, int* selected);
int pt_readback_history_extra(float* extra_host); /* pixel_count floats, zeros while E is absent; synchronises */
/* The round over a caller's list: to pt_history_round what pt_adaptive_round_list is to the threshold round — its second half,
 * without key and selection.  list_host holds m distinct tile indices in ascending order; the worker is kept for `capacity` pixels and
 * live for m; render and merge as above; PtStats.samples grows by G * m.  It reads no features and no C and needs no whole rows, so it
 * is allowed on a striped tile (the list then goes through the stripe's offsets as in pt_adaptive_round_list): this is what every
 * context of a group runs over its part of the frame's list (pt_group_history_round).  With m == 0 nothing is rendered, but E is still
 * ensured (zeroed) and made present, so that the contexts of a group agree on whether E exists.  Asynchronous.
 * Refuses, in this order, nothing allocated or launched: no renderer or a failed context; iter_first < 1, group_iters < 1 or iterations
 * past 2^31 - 1; PtOptions.convergence != 0; the adaptive state; capacity outside 1 .. pixel_count or m outside 0 .. capacity; a null
 * list with m > 0; an entry outside the tile or not above its predecessor. */
int pt_history_round_list(int iter_first, int group_iters, const int32_t* list_host, int m, int capacity);
/* The same arithmetic on the host (no GPU); the device results equal these bit for bit.  list: cap = clamp(ceil(max_fraction * w * rows),
 * 1, w * rows) entries, of which the first *m are written.  current_plane may be NULL (absent); emitter_geom may be NULL when num_geoms == 0. */
int pt_history_select_host(int w, int rows, const float* feature_planes, const float* current_plane, const uint8_t* emitter_geom, int num_geoms,
                           const PtHistoryRoundOptions* opt, int32_t* list, int* fresh, int* m);
/* list: m >= 1 distinct tile pixels; group_sum: m * 3 floats in list order; rgb_sum and extra are updated in place. */
int pt_history_merge_host(int pixels, float* rgb_sum, float* extra, const int32_t* list, int m, const float* group_sum, int group_iters);
/* The counted twins of pt_history_blend_host, pt_history_capture_host, pt_history_capture_moments_host and
 * pt_history_denoise_moments_host: the same arguments and `extra`, pixels (w * rows) floats, finite and >= 0. */
int pt_history_blend_counted_host(int pixels, const float* rgb_sum, float samples, const float* extra, const float* current_plane, float* rgb_avg);
int pt_history_capture_counted_host(int pixels, const float* rgb_sum, const float* feature_planes, const float* current_plane, float samples,
                                    const float* extra, float* kept_planes);
int pt_history_capture_moments_counted_host(int pixels, const float* rgb_sum, float samples, const float* extra, const float* current_plane,
                                            const float* current_var, float* kept_var);
int pt_history_denoise_moments_counted_host(int w, int rows, const float* rgb_sum, const float* planes, float samples, const float* extra,
                                            const float* current_plane, const float* current_var, const PtDenoiseOptions* opt, float* rgb_avg,
                                            float* var_raw, uint8_t* mark);

/* ---- the history across a moved object: PT_HISTORY_MOTION for pt_history_reproject_ex.  The lookup above assumes a static world: a
 * pixel of an object that pt_set_geoms moved projects to where the object is now, not to where it was at the capture.  With the flag,
 * a pixel of a moved geom is first taken back to where its surface point was.
 * Kept geoms: every capture remembers, beside the kept camera, the geoms the renderer had (a host copy, retaken only when
 * pt_set_geoms has run since the last copy; a renderer that never moves an object copies once at most and uploads nothing).
 * Motion table (pt_history_motion_host), per geom g from the kept and the current geom, matrices column-major m[c*4+r]:
 *   kind[g] = 0 (still) when the 48 matrix words are bytewise equal; 2 (carries nothing) for a changed triangle or when an entry
 *   below is not finite; 1 (moved) otherwise.
 *   D[r][c] = (float)(((A_k[r][0]*B_c[0][c] + A_k[r][1]*B_c[1][c]) + A_k[r][2]*B_c[2][c]) + A_k[r][3]*B_c[3][c]), r = 0..2, c = 0..3:
 *   A_k the kept transform, B_c the current inverseTransform; every factor widened to double, plain double operations in this order.
 *   Nm[r][c] = (float)((IT_k[r][0]*A_c[c][0] + IT_k[r][1]*A_c[c][1]) + IT_k[r][2]*A_c[c][2]): IT_k the kept invTranspose, A_c the
 *   current transform, 3 x 3 parts (a normal goes back through the current transform's transpose, forward through the kept inverse
 *   transpose).  Row g of the table: D as 12 floats row-major, Nm as 9, then 3 zeros (24 floats).
 * The lookup with the flag is pt_history_reproject[_ex]'s with one step after step 1, for the pixel's geom g = id - 1 (an id outside
 * 1 .. num_geoms, possible only with keep_view_dependent, counts as still):  kind 0: nothing changes;  kind 2: rejected (C = VC = 0);
 *   kind 1: p'_x = ((D00*p.x + D01*p.y) + D02*p.z) + D03, y and z likewise;  m = Nm n, each row a dot product as above;  l = m . m;
 *   rejected unless l > 0;  r = sqrtf(l), correctly rounded;  n' = m / r;  steps 2 - 7 read p', n' for p, n (dz and the plane
 *   tolerance follow p').  float32, separate IEEE operations, the same bits on host and device in all three builds.
 * Flags: PT_HISTORY_MOTION alone, or with PT_HISTORY_VARIANCE or PT_HISTORY_MOMENTS (those two together stay refused, first).  Where no
 * geom moved since the capture the renderer uploads nothing and launches the kernel of the call without the flag: the same planes
 * bit for bit.  Otherwise 96 + 1 bytes per geom go to the device (allocated by the first such call, counted in device_bytes; the
 * table is built and uploaded by the first lookup after a capture or a pt_set_geoms changed its inputs, which synchronises) and
 * k_history_reproject_motion runs.  pt_history_capture_ex does not define the bit.  Without the flag the lookup is what it was and
 * treats the world as static even after pt_set_geoms.
 * Caveat: a moved object changes shadows and indirect light on surfaces that stand still.  The lookup does not detect that: their
 * history goes stale until `cap` washes it out, unless the history probes below shorten it (a camera that stands still only).
 * Out of scope: adding or removing objects; deformation; a device-side tree build.  (Material edits: PT_HISTORY_MATERIALS below.  Groups of contexts: "history in groups" below.) */
#define PT_HISTORY_MOTION 4u
int pt_history_motion_host(const PtGeom* kept, const PtGeom* cur, int n, float* table /* n * 24 */, uint8_t* kind /* n */);
/* pt_history_reproject_host / _variance_host / _moments_host (flags & 3 picks which; kept_var, current_var NULL for the plain one)
 * with the motion step: table and kind as above for num_geoms >= 1 geoms.  PT_HISTORY_MOTION in `flags` is implied. */
int pt_history_reproject_motion_host(int w, int rows, int row0, const PtCamera* kept_cam, const float* kept_planes, const float* feature_planes,
                                     const uint8_t* reject_geom, int num_geoms, const PtHistoryOptions* opt, const float* kept_var, const float* table,
                                     const uint8_t* kind, uint32_t flags, float* current_plane, float* current_var);

/* ---- the history across a recoloured surface: PT_HISTORY_MATERIALS for pt_history_reproject_ex.  The lookup above knows nothing of
 * pt_set_materials: a pixel of a wall whose colour changed since the capture carries the old colour.  With the flag the history of
 * such a pixel is scaled by the ratio of the colours, and the history of a pixel whose material changed in any other way is dropped.
 * Kept materials: every capture remembers, beside the kept camera and geoms, the materials the renderer had (a host copy, retaken
 * only when pt_set_materials has run since the last copy; a renderer that never edits copies once at most and uploads nothing).
 * Recolour table (pt_history_recolor_host), per material m with k the kept and c the current material; "the nine words" are color,
 * specular_color, hasReflective, hasRefractive and emittance:
 *   mk = 0 (unchanged) when the nine words are bytewise equal;
 *   mk = 2 (carries nothing) when any of the six words that are not `color` differs bytewise, or k.emittance > 0 (an emitter's pixel
 *   is its colour times its emittance), or k.hasReflective > 0 (a mix of two colours, not a product), or for some channel j
 *   !(k.color[j] > 0), or !(c.color[j] >= 0), or r_j = c.color[j] / k.color[j] (float32, correctly rounded) is not finite;
 *   mk = 1 (recoloured) otherwise: only the colour of a diffuse material that does not emit changed.
 *   Row g of the table: {r_x, r_y, r_z, +0} of geoms[g].materialid for kind 1, four zeros otherwise; kind[g] = mk of that material.
 * The lookup with the flag is the lookup without it (with PT_HISTORY_MOTION: that lookup) with one step more for the pixel's geom
 * g = id - 1 (an id outside 1 .. num_geoms counts as unchanged, as the motion step has it):  kind 0: nothing changes;  kind 2:
 * rejected (C = VC = 0);  kind 1, after step 7, for a pixel that was not rejected: h_j = h_j * r_j, Th untouched; the variance kind
 * vh_j = (vh_j * r_j) * r_j; the moments kind m2h_j = (m2h_j * r_j) * r_j, rh untouched.  float32, separate IEEE multiplications in
 * the order written, the same bits on host and device in all three builds.  Every tap that passed has the pixel's own object id and
 * therefore one factor, so scaling after the bilinear average is the demodulate-then-remodulate step of SVGF applied to a history
 * that stores modulated radiance.  It corrects the first-hit albedo; it does NOT correct the colour that the recoloured surface
 * bleeds onto other surfaces, whose history stays stale until `cap` washes it out.
 * Flags: PT_HISTORY_MATERIALS alone, or with PT_HISTORY_VARIANCE or PT_HISTORY_MOMENTS, each also with PT_HISTORY_MOTION.  With
 * PT_HISTORY_FEEDBACK it is refused by name (FC carries one variance for three channels, which a per-channel factor cannot scale: not
 * built).  pt_history_capture_ex does not define the bit; a group refuses it by name (not built for a group).  Where no material
 * changed since the capture the renderer uploads nothing and launches the kernel of the same call without the flag: the same planes
 * bit for bit, no growth of device_bytes.  Otherwise 16 + 1 bytes per geom go to the device (allocated by the first such call, counted
 * in device_bytes; the table is built and uploaded by the first lookup after a capture or a pt_set_materials changed its inputs,
 * which synchronises) and k_history_reproject_materials runs.
 * Out of scope: the recolour step beside the feedback kind and in groups; textures.  (The light an edit changes on OTHER surfaces: the
 * history probes below.) */
#define PT_HISTORY_MATERIALS 32u
int pt_history_recolor_host(const PtMaterial* kept, const PtMaterial* cur, int num_materials, const PtGeom* geoms, int num_geoms,
                            float* table /* num_geoms * 4 */, uint8_t* kind /* num_geoms */);
/* pt_history_reproject_motion_host with the recolour step: recolor and rkind as above for num_geoms >= 1 geoms; table and kind (the
 * motion table) may both be NULL when PT_HISTORY_MOTION is not in `flags`.  flags & 3 picks the kind; PT_HISTORY_MATERIALS is implied. */
int pt_history_reproject_materials_host(int w, int rows, int row0, const PtCamera* kept_cam, const float* kept_planes, const float* feature_planes,
                                        const uint8_t* reject_geom, int num_geoms, const PtHistoryOptions* opt, const float* kept_var, const float* table,
                                        const uint8_t* kind, const float* recolor, const uint8_t* rkind, uint32_t flags, float* current_plane,
                                        float* current_var);

/* ---- the history probes: replay kept samples after a move, shorten the history where light changed.  A sample is a pure function
 * of (iteration, pixel, world), and the adaptive rounds' worker renders a chosen list of pixels at chosen iterations bit for bit as a
 * whole-frame render does.  So: keep a sparse set of last view's samples (pt_history_probe_keep), render the same (iteration, pixel)
 * pairs again in the world as it is now (pt_history_probe_check) and compare.  The difference is exactly zero wherever the path met
 * nothing that changed — no noise threshold — and non-zero elsewhere (the temporal gradient of Schied et al. 2018).  What the check
 * finds is written into one word, C.w = Th, the carried weight, which the blend, both captures, the moments filter and the history
 * round's key read already: stale pixels lose their history, are marked fresh, and are resampled.  No downstream step changes.
 * Opt-in: a renderer that never calls these functions allocates and launches nothing for them; every other call keeps its kernels,
 * memory, launches, results and refusals.  Specified like the rest of the history: float32, separate IEEE operations in the order
 * written, one implementation for kernels and host loops, the same bits in all three PT_ARITH_* builds, host and device.
 * The check compares pixel p then with pixel p now: it answers for a camera that stands still, and refuses a moved one by name.
 * Probes: the tile is W x R whole rows; phase in 0 .. 8 gives ox = phase % 3, oy = phase / 3.  Probe (i, j) sits at tile pixel
 *   (3 i + ox, 3 j + oy), i < PW = ceil((W - ox) / 3), j < PR = ceil((R - oy) / 3), each 0 when negative; P = PW * PR; probe index
 *   s = j * PW + i, so the pixel list ascends with s (pt_history_probe_list_host).
 * pt_history_probe_keep (asynchronous; k_history_probe_keep, one thread per probe): PK[s] = {S_p.xyz, bits(id_p)}, id_p read from the
 *   feature sums as pt_history_capture reads it (s1.w > 0 ? bits(s2.w) : 0).  The host remembers iter_first, iter_count, phase, the
 *   renderer's camera, its geoms and its materials (host copies, retaken only when pt_set_geoms / pt_set_materials has run since the
 *   last copy).  State: 16 B per probe, allocated by the first keep for the probes of phase 0 (the most of any phase) and counted in
 *   PtStats.device_bytes.  PK survives pt_clear, pt_set_camera[_ex], pt_set_geoms and pt_set_materials; pt_history_drop forgets it.  P == 0 is kept as "no probes".
 *   Refuses, in this order, nothing changed, allocated or launched: no renderer or a failed context; iter_first < 1, iter_count < 1
 *   or iterations past 2^31 - 1; phase outside 0 .. 8; a striped or ragged tile; the adaptive state; E present (S is no longer a
 *   uniform sum: keep before pt_history_round; pt_clear is the way out); no feature pass since the last clear or move;
 *   iter_count * pixel_count is not the samples rendered since the last clear.  iter_first is the caller's statement, as `samples`
 *   is elsewhere.
 * pt_history_probe_check (ONE synchronise, for the two counts):
 *   1. the probes' pixels are written into the rounds' list;
 *   2. the worker: the existing one as it is when its capacity is >= P, made live for P; else one built for P.  (The history round
 *      with its default fraction asks for capacity N, so a frame that runs check then round rebuilds nothing.)
 *   3. the worker renders the kept iterations of the listed pixels into its cleared sum Sw[P][3]; PtStats.samples grows by iter_count * P;
 *   4. gradient (k_history_probe_gradient, one thread per probe), g = id - 1: the probe is skipped, L[s] = -1.0f, when the id now
 *      at the pixel differs from the kept id, is 0 or outside 1 .. num_geoms, or moved[g] != 0 (moved[g] = 1 when the geom's 48 matrix
 *      words differ bytewise from the kept geoms', or mk of its material against the kept materials — PT_HISTORY_MATERIALS above — is
 *      not 0; built on the host and uploaded, one byte per geom, only when pt_set_geoms or pt_set_materials has run since the keep,
 *      otherwise all zero).  So after a material edit the probes on the edited surface are skipped — its own shading is the recolour
 *      step's business — and every other probe is replayed: L is exactly zero wherever the path met nothing that changed, and
 *      non-zero where it met the recoloured wall or the dimmed light.  Otherwise, o = PK[s].xyz, w = Sw[s]:
 *        d = (|w.x - o.x| + |w.y - o.y|) + |w.z - o.z|;  mo = (o.x + o.y) + o.z, mw likewise;  m = mo > mw ? mo : mw;
 *        lam = m > 0 ? d / m : +0;  L[s] = lam < 1 ? lam : 1.0f (a NaN reads as 1).
 *      changed = #{L[s] > 0}, skipped = #{L[s] < 0}: integer atomics, read back as 8 bytes;
 *   5. apply (k_history_probe_apply, one thread per tile pixel (x, r)): every word is kept for a miss, an id outside 1 .. num_geoms
 *      and a moved or edited geom (left to PT_HISTORY_MOTION / PT_HISTORY_MATERIALS).  Otherwise i0 = x / 3, j0 = r / 3, lam_p = the maximum of L over the probes
 *      (i, j) of the grid with |i - i0| <= radius, |j - j0| <= radius, starting at +0 (skipped probes add nothing).  lam_p == 0:
 *      every word is kept.  Else g = lam_p * gain;  g = g < 1 ? g : 1.0f;  C.w = C.w * (1.0f - g).  Only C.w is written; VC is
 *      untouched; the cap was applied by the lookup.
 *   L: 4 B per probe (and the two counts), allocated by the first check; moved: one byte per geom.
 *   Refuses, in this order: no renderer or a failed context; PtOptions.convergence != 0; a striped or ragged tile; the adaptive
 *   state; nothing kept; a tile other than the one the probes were kept for; a camera that is not bytewise the kept one (position,
 *   view, up, right, fov, pixelLength); C absent (no lookup since the last clear or move); a check already applied to this C (the
 *   next lookup clears that); no feature pass since the last clear or move; an option out of range.  P == 0 succeeds with all counts
 *   0 and launches nothing.  probes / changed / skipped may be NULL.
 * Defaults: radius 0 (the probe of the pixel's own 3 x 3 cell) and gain 0.25, from tests/test_history_probe_sim.py (README "History
 * probes"): at 4 spp per view one changed path of four already gives lam of a quarter and more, and in that simulation every larger
 * radius or gain raised the frame's MSE — shortening history there trades little bias for much noise.  Radius 1 and gain 1 are what
 * makes the history round resample the pixels a move touched; they cost 3.2 x the frame's MSE there.
 * Not built: a camera that moves between keep and check (forward-projecting the probes needs camera rays off the pixel centres);
 * pt_group_*; the shading of the moved object itself (PT_HISTORY_MOTION carries it, skipped here); remodulating the probes' kept sums after a recolour
 * (a probe on a recoloured surface is skipped); feeding L into the filter's variance. */
#define PT_HISTORY_PROBE_RADIUS 0    /* the default of PtHistoryProbeOptions.radius, in probe cells: the pixel's own cell */
#define PT_HISTORY_PROBE_GAIN 0.25f /* the default of PtHistoryProbeOptions.gain */
typedef struct PtHistoryProbeOptions { /* every field: 0 = the default */
  int32_t radius; /* in probe cells: 1 .. 4, or -1 for radius 0; default (0): PT_HISTORY_PROBE_RADIUS, the pixel's own cell */
  float gain;     /* finite and > 0; default (0): PT_HISTORY_PROBE_GAIN */
} PtHistoryProbeOptions;
int pt_history_probe_keep(int iter_first, int iter_count, int phase);
int pt_history_probe_check(const PtHistoryProbeOptions* opt, int* probes, int* changed, int* skipped);
/* kept: P * 4 floats (PK), lam: P floats — the last check's L when it was made of these probes, zeros otherwise (before a check, after
 * a later keep, once C is absent); either may be NULL, *count = P (0: nothing kept).  Synchronises. */
int pt_readback_history_probe(float* kept, float* lam, int* count);
/* The same arithmetic on the host (no GPU); the device results equal these bit for bit.  w x rows the tile; feature_planes its feature
 * SUM planes; moved_geom one byte per geom (may be NULL when num_geoms == 0). */
int pt_history_probe_list_host(int w, int rows, int phase, int32_t* list /* P entries, or NULL */, int* count);
int pt_history_probe_keep_host(int w, int rows, int phase, const float* rgb_sum, const float* feature_planes, float* kept /* P * 4 */);
/* group_sum: the replay Sw, P * 3 floats in probe order; lam: P floats out; changed / skipped may be NULL */
int pt_history_probe_gradient_host(int w, int rows, int phase, const float* kept, const float* group_sum, const float* feature_planes,
                                   const uint8_t* moved_geom, int num_geoms, float* lam, int* changed, int* skipped);
/* current_plane: w * rows * 4 floats, updated in place (its w words only) */
int pt_history_probe_apply_host(int w, int rows, int phase, const float* lam, const float* feature_planes, const uint8_t* moved_geom, int num_geoms,
                                const PtHistoryProbeOptions* opt, float* current_plane);

/* ---- the feedback: the FILTERED image fed back into the history (recurrent SVGF, Schied et al. 2017).  Without it every view filters
 * the raw blend from scratch and the result is shown once; with it the output of filter level L is what the next view accumulates
 * onto.  A fourth kind of history state, beside the moments.  Opt-in: a renderer that never passes PT_HISTORY_FEEDBACK allocates and
 * launches nothing for it, and every other call keeps its kernels, memory, launches, results and refusals.  Specified like the rest
 * of the history: float32, separate IEEE operations in the order written, one implementation for kernels and host loops, the same
 * bits in all three PT_ARITH_* builds, host and device.
 * The raw chain is not touched: K0 keeps the unfiltered blend and VK = {m2.xyz, r} (the moments' variance m2b - cb^2 needs the RAW
 * first moment).  With the flag, K, VK, C, VC and pt_history_resolve's blend are bit for bit those of the same calls without it.
 * State: a buffer of its own, three planes of pixel_count float4, 48 bytes per tile pixel.  The first call that carries the flag (or
 * the first pt_history_denoise_feedback) allocates and zeroes it; PtStats.device_bytes counts it from then on.
 *   P  (pending) = {f.xyz, vf}: the filter's colour after level L, remodulated (radiance), and the variance the guided levels
 *        propagated for it, c_L.w, in the filter's unit (demodulated unless keep_albedo).  Aligned with the current camera.
 *   FK = P as promoted by the last capture with the flag; aligned with K.
 *   FC = FK resampled to the current camera; aligned with C.
 *   FK lives as K does: it survives pt_clear, pt_set_camera[_ex] and pt_set_geoms.  FC and P become absent on all three.  P also
 *   becomes absent on any pt_render, pt_history_round or pt_render_features after the tap.  pt_history_drop forgets all three.  A
 *   capture without the flag after one with it leaves FK invalid (K "kept without feedback"); a lookup without it leaves FC absent.
 *   The renderer remembers the keep_albedo the tap was made with.
 * PT_HISTORY_FEEDBACK in pt_history_reproject_ex and pt_history_capture_ex: only together with PT_HISTORY_MOMENTS (the lookup: also
 *   with PT_HISTORY_MOTION); without PT_HISTORY_MOMENTS, or with PT_HISTORY_VARIANCE, the call is refused, right where the flag word
 *   is checked.  pt_history_denoise_ex keeps refusing the bit.
 *   The lookup with the flag: C and VC as without it, the same bits.  Step 6 also starts facc = 0 over four components and, for a
 *        tap that passed every test, adds after vacc  facc_k = facc_k + b * FK(q).k;  FK(q) is read after VK(q), for such a tap only.
 *        Step 7: FC.k = facc_k / wsum for the four; a rejected pixel gets FC = 0; the cap touches nothing of FC.
 *        Refused after the existing refusals: nothing captured with feedback.
 *   The capture with the flag: K and VK exactly as the moments capture writes them (counted while E is present); FK := P — the planes
 *        change roles, no bytes move — and P becomes absent.  Refused after the existing refusals: P absent (filter first:
 *        pt_history_denoise_feedback).
 * pt_history_denoise_feedback(samples, opt, fb, rgb_avg_host): the moments form of pt_history_denoise_ex with two changes.
 *   fb: level (1 .. the filter's levels; 0 = PT_HISTORY_FEEDBACK_LEVEL) and the variance rule (1, or -1 for rule 0; 0 =
 *        PT_HISTORY_FEEDBACK_VARIANCE); NULL = the defaults.  The defaults are the pair that tests/test_history_feedback_sim.py measured
 *        lowest both on its orbit and with the camera standing still.
 *   prepare: n, a, p, the hit flag, ns, cb_k, m2b, rb and d_k exactly as the moments form.  The colour that is filtered is
 *        cf_k = blend(S_k, ns, FC.k, C.w), demodulated as every form's (FC and C absent: S_k / ns).
 *        rule 0: var_raw and the spatial mark are the moments form's, from the raw chain (SVGF's choice; conservative: it
 *        overstates the variance of a colour that was filtered before).
 *        rule 1, where rb <= PT_HISTORY_MOMENTS_R_MAX:  g = 1.0f - rb;  s_k = d_k / g;  unless keep_albedo
 *        s_k = a_k > 0 ? s_k / (a_k * a_k) : s_k;  sv = (s_x + s_y) + s_z;  wn = ns / (ns + C.w), wh = C.w / (ns + C.w);
 *        var_raw = (wn * wn) * sv + (wh * wh) * FC.w.  Otherwise the mark.
 *   then the moments form's spatial estimate, prefilter and levels, unchanged: the same kernels.  After level L - 1 a streaming kernel
 *        writes P[i] = {finish(c_L, a).xyz, c_L.w} (48 B per pixel moved, no LDS); the remaining levels and the finish run unchanged.
 *        With L == levels the tap's xyz equal the output.
 *   Refusals: the moments form's, in their order; then fb out of range; C present with FC absent; rule 1 with a keep_albedo
 *        other than the remembered one while FC is present; a null buffer.
 * pt_readback_history_feedback(kept, current, pending): FK, FC and P, pixel_count * 4 floats each; an absent plane reads as zeros;
 *   any pointer may be NULL.  Synchronises.
 * What it buys: README "Feedback" (tests/test_history_feedback_sim.py on the CPU, tests/test_gpu_history_feedback.py on an MI355X, the
 * same digits).  One scene, one orbit: no claim beyond it.
 * Out of scope: groups of contexts; the variance kind. */
#define PT_HISTORY_FEEDBACK 16u /* (8u stays undefined) */
#define PT_HISTORY_FEEDBACK_LEVEL 1
#define PT_HISTORY_FEEDBACK_VARIANCE 1
typedef struct PtHistoryFeedbackOptions { /* every field: 0 = the default */
  int32_t level;    /* the filter level whose output is fed back: 1 .. the filter's levels; default (0): PT_HISTORY_FEEDBACK_LEVEL */
  int32_t variance; /* the rule: 1: var_raw from the new view's variance and the one FC carries; -1: rule 0, var_raw from the raw chain;
                       default (0): PT_HISTORY_FEEDBACK_VARIANCE */
} PtHistoryFeedbackOptions;
int pt_history_denoise_feedback(float samples, const PtDenoiseOptions* opt, const PtHistoryFeedbackOptions* fb, float* rgb_avg_host); /* synchronises */
int pt_readback_history_feedback(float* kept, float* current, float* pending);
/* The same arithmetic on the host (no GPU); the device results equal these bit for bit.  The lookup: pt_history_reproject_moments_host's
 * arguments, FK and FC beside VK and VC, and a motion table with its kinds (pt_history_reproject_motion_host's) or both NULL.  The
 * filter: pt_history_denoise_moments_host's arguments, extra (the plane E, or NULL), FC beside C and VC (all three or none), fb, and the
 * tap plane (w*rows*4 floats) as a further optional output; with var_raw or mark alone no level runs. */
int pt_history_reproject_feedback_host(int w, int rows, int row0, const PtCamera* kept_cam, const float* kept_planes, const float* feature_planes,
                                       const uint8_t* reject_geom, int num_geoms, const PtHistoryOptions* opt, const float* kept_var, const float* kept_fb,
                                       const float* table, const uint8_t* kind, float* current_plane, float* current_var, float* current_fb);
int pt_history_denoise_feedback_host(int w, int rows, const float* rgb_sum, const float* planes, float samples, const float* extra, const float* current_plane,
                                     const float* current_var, const float* current_fb, const PtDenoiseOptions* opt, const PtHistoryFeedbackOptions* fb,
                                     float* rgb_avg, float* tap, float* var_raw, uint8_t* mark);

/* ---- the noise estimate of the blend, and rendering a view until the BLEND is clean.  pt_get_noise and pt_render_until judge the
 * view's own samples; a view that starts with a carried history is cleaner than they say.  pt_history_noise sums the variance of the
 * blend, which the capture and pt_history_denoise form per pixel already, into a frame statistic in pt_get_noise's unit, and
 * pt_history_render_until is pt_render_until's loop stopping on it: what makes a carried history save time as well as samples.
 * Opt-in: a renderer that never calls these functions allocates and launches nothing new, and every other call keeps its kernels,
 * memory, launches, results and refusals.  Specified like the rest of the history: float32 throughout, every operation a separate
 * IEEE operation in the order written, no FMA contraction, correctly rounded division, denormals kept; one implementation for the
 * kernels and the host loop (csrc/pt_history.h noise_value); the same bits in all three PT_ARITH_* builds, host and device.
 * pt_history_noise(samples, flags, &sse): the only defined value of flags is PT_HISTORY_VARIANCE.  Per tile pixel, with prev, q the
 *   fold's planes, Tf = (float)T, Df = (float)(M - 1) * Tf, C = {h, Th} and VC = {vh, +0} (both absent: Th = vh = +0), per component k:
 *            vn_k = sample_variance(prev_k, q_k, Tf, Df);  vb_k = blend_variance(vn_k, samples, vh_k, Th)      ("variance of the history")
 *            w = (vb_x + vb_y) + vb_z;   W[p] = w, a plane of pixel_count floats
 *   SSE_blend = sum over the tile of (double)w, in pt_noise_fold's way: a workgroup of 256 threads owns PT_NOISE_PIXELS_PER_PARTIAL
 *   consecutive pixels and leaves one double from the same fixed tree, and the fold's second launch adds the partials in index order.
 *   No atomics: equal inputs give equal bits.  The call synchronises once, for the one double; sse may be NULL.  Estimated PSNR of
 *   the blend = pt_psnr_from_sse(SSE_blend, pixel_count).
 *   With C and VC absent wn = 1 and wh = +0, so w is the fold's plane-0 .w and SSE_blend is pt_get_noise's double, bit for bit.
 *   Memory: 4 * N + 8 * (ceil(N / PT_NOISE_PIXELS_PER_PARTIAL) + 1) bytes, allocated by the first estimate, part of
 *   PtStats.device_bytes from then on, kept across pt_clear.  pt_readback_history_noise returns W (synchronises); an error before the
 *   first estimate and after pt_clear, pt_set_camera[_ex] or pt_set_geoms, which make W absent.
 *   Refusals, each naming the function, nothing allocated or launched, in this order: no renderer, or a failed context; a flags word
 *   other than PT_HISTORY_VARIANCE (PT_HISTORY_MOMENTS: "not built", below); a striped or ragged tile; the adaptive state; the extra
 *   plane E present (the message of the other uniform-sum readers: pt_history_resolve, pt_clear); samples not finite or <= 0; nothing
 *   folded, fewer than 2 groups folded, iterations rendered since the last fold ("fold first"), samples != (float)T; C present with
 *   VC absent or of the moments kind.
 * pt_history_render_until(iter_first, max_iters, group_iters, target_db, &iters_done, &psnr_db, &view_psnr_db): pt_render_until's
 *   loop, judging the blend.  Groups of group_iters iterations (0 = a batch; the last one cut at max_iters); after each a fold and,
 *   once the fold leaves a variance (groups >= 2), the estimate above with samples = (float)T — both in ONE launch
 *   (k_noise_fold_history: fold_pixel, then the estimate on the two words it just wrote; the planes, W and both doubles equal those of
 *   pt_noise_fold followed by pt_history_noise bit for bit).  One synchronise per group that has an estimate, reading both doubles.
 *   Stops after the first fold with groups >= 2 whose blend PSNR is > target_db, or at max_iters; returns 0 either way.
 *   *psnr_db: the blend's last estimate, *view_psnr_db: the view's own (pt_get_noise's) at the same fold, -1 when there is none; all
 *   three outputs may be NULL.  Groups folded before the call count, and iterations rendered but not yet folded join the first group,
 *   as in pt_render_until.  With C absent the call is pt_render_until: the same iterations, PSNR bits, image and planes.
 *   Refusals: no renderer; pt_render_until's argument check, word for word under this name; a failed context; a striped or ragged
 *   tile; the adaptive state; E present; C present with VC absent or of the moments kind.
 *   A view goes: pt_set_camera, pt_render_features(1, 1), pt_history_reproject_ex(PT_HISTORY_VARIANCE), pt_history_render_until,
 *   pt_history_denoise, pt_history_capture_ex(samples = T, PT_HISTORY_VARIANCE) — the lookup needs the view's first hits only, and C
 *   and VC stay until pt_clear, pt_set_camera[_ex] or pt_set_geoms, so rendering after the lookup is within the rules above.
 * What it buys, and how far the estimate is from the truth: README "Noise estimate of the blend" (tests/test_history_noise_sim.py).
 *   The estimate is a variance: the smoothing the lookup adds is not in it, and the carried variance reads high, so on that orbit
 *   it is conservative.  Recorded, not bounded.  One scene, one orbit: no claim beyond it.
 * Out of scope: the moments kind (PT_HISTORY_MOMENTS) — its estimate exists only for pixels with four views of history (none in the
 *   first three views of an orbit at 1 spp; 2000 - 2316 of 5184 pixels from view 3 on), reads 2.2 - 3.1 x high there, and the pixels
 *   without one hold 15 - 31 % of the blend's squared error; rendering longer inside a view raises rb towards 1 and takes estimates
 *   away, so a stopping rule does not fit that kind.  Groups of contexts; correcting the blend's bias; lowering the floor of two
 *   folds per view.  (A per-pixel threshold round over vb: "threshold rounds over the blend" below.) */
int pt_history_noise(float samples, uint32_t flags, double* sse);
int pt_readback_history_noise(float* w_host); /* pixel_count floats */
int pt_history_render_until(int iter_first, int max_iters, int group_iters, float target_db, int* iters_done, float* psnr_db, float* view_psnr_db);
/* The same arithmetic on the host (no GPU): the fold's planes with their counters (groups = M >= 2, iters = T, samples == (float)T)
 * and C, VC (both NULL: absent) in; w_out (pixels floats, may be NULL) and *sse (may be NULL) out.  The device's W equals w_out bit for
 * bit; the host adds in pixel order, so the double may differ from the device's in the last bits, as pt_noise_fold_host's does. */
int pt_history_noise_host(int pixels, const float* noise_planes, int groups, int64_t iters, float samples, const float* current_plane,
                          const float* current_var, float* w_out, double* sse);

/* ---- threshold rounds over the blend: the history in the adaptive state.  pt_adaptive_round_threshold keys a pixel by the variance of
 * its own samples; a view that starts with a carried history is clean nearly everywhere, and pt_history_render_until can answer the
 * exceptions (disocclusions, mirrors, the frame's edge) with whole-frame iterations only.  Here a threshold round is keyed by the
 * variance of the BLEND, and the history steps that follow it read per-pixel counts, so a view sampled that way can be resolved and
 * captured and the next view can carry it on.  The variance kind only.  Opt-in: a renderer that never calls these functions allocates
 * and launches nothing new, and every other call keeps its kernels, memory, launches, results and refusals.  Specified like the rest
 * of the history (float32, separate IEEE operations in the order written, no contraction, correctly rounded division, denormals kept;
 * one implementation for kernels and host loops: csrc/pt_history.h Counts .. capture_counts_pixel; kernels: csrc/pt_history_threshold.hip).
 * Notation: S the SUM image; prev, q the two noise planes; cnt = {T_p, M_p} (the uniform state: the fold's (T, M) in every pixel);
 * C = {h, Th}, VC = {vh, +0} (absent: all +0).
 * Pass A (k_history_noise_counts), per tile pixel p and component k:
 *            Tf = (float)T_p;  Df = (float)(M_p - 1) * Tf
 *            vn_k = sample_variance(prev_k, q_k, Tf, Df);  vb_k = blend_variance(vn_k, Tf, vh_k, Th)
 *            W[p] = (vb_x + vb_y) + vb_z   (pt_history_noise's plane);   NE[p] = Tf + Th   (the blend's effective sample count, what a
 *            capture writes to K0.w)
 * pt_history_noise_adaptive(&sse): pass A, then the fold's reduction exactly as pt_history_noise (one double per
 *   PT_NOISE_PIXELS_PER_PARTIAL pixels from the fixed tree, added in index order, no atomics); one synchronise; sse may be NULL.  Valid
 *   in both states.  pt_readback_history_noise returns W as before, pt_readback_history_noise_samples NE.  NE is a plane of its own,
 *   4 * N bytes, allocated by the first call that needs it and part of PtStats.device_bytes from then on (the first call also
 *   allocates pt_history_noise's buffer if no estimate was made before).  W and NE become absent on pt_clear, pt_set_camera[_ex] and
 *   pt_set_geoms, and after any adaptive round that rendered: the image they described is gone.
 *   Refusals, in this order: no renderer, or a failed context; a striped or ragged tile; the extra plane E present; nothing folded,
 *   fewer than 2 groups folded, iterations rendered since the last fold; C present with VC absent or of the moments kind.
 * Pass B (k_history_key_blend): pt_adaptive_round's key over (W, NE) in place of (plane 0's w, T) — the 3 x 3 binomial prefilter over
 *   the per-sample variance s(q) = W[q] * NE[q], rows outer, taps outside the tile skipped, num = num + g * s, den = den + g;
 *   key = (num / den) / NE[p], a NaN becomes 0xffffffff.  With vh ~ sigma^2 / Th, vb * (T + Th) ~ sigma^2: the one quantity that
 *   neighbours with different counts and different histories share.
 * pt_history_round_threshold(iter_first, group_iters, threshold, max_fraction, &above, &selected) and
 * pt_history_render_threshold(iter_first, max_iters, group_iters, threshold, max_fraction, min_pixels, &iters_done, &samples_done,
 *   &above_left): pt_adaptive_round_threshold and pt_render_threshold word for word, with the key of passes A and B in place of the
 *   adaptive key: the same entry into the adaptive state, worker, selection (thr = threshold * threshold), one synchronise for 8
 *   bytes, render and merge, counters and PtStats.samples; the driver's uniform groups and folds are pt_render_threshold's.
 *   Refusals: what those two refuse, in their order (E included), under these names; then C present with VC absent or of the moments
 *   kind.  C absent is allowed: the calls are then the adaptive ones, bit for bit.
 *   pt_history_reproject_ex keeps refusing the adaptive state, so a view goes: pt_set_camera, pt_render_features(1, 1),
 *   pt_history_reproject_ex(PT_HISTORY_VARIANCE), pt_history_render_threshold, pt_history_denoise_adaptive,
 *   pt_history_capture_adaptive; the move then leaves the adaptive state as pt_clear does.  C and VC stay valid through the rounds.
 * pt_history_resolve_adaptive(rgb_avg_host) (k_history_blend_counts): c_k = blend_component(S_k, Tf_p, C.k, C.w).
 * pt_history_capture_adaptive() (k_history_capture_counts): K0 = {blend, Tf_p + Th}, K1 and K2 pt_history_capture's,
 *   VK = {vb.xyz, +0} of pass A; the kept camera and geoms as in any capture; K is "kept with variance" afterwards, so the next view's
 *   pt_history_reproject_ex(PT_HISTORY_VARIANCE) runs unchanged.  Needs a feature pass since the last clear or move.
 *   Both are valid in both states and take no `samples`: the counts say it.  In the uniform state with counts (T, M) and C, VC present
 *   they equal pt_history_resolve / pt_history_capture_ex(PT_HISTORY_VARIANCE) at samples = (float)T bit for bit, and with C absent the
 *   resolve is pt_resolve.  Refusals: no renderer or a failed context; a striped or ragged tile; (the capture) no feature pass; E present;
 *   nothing folded, fewer than 2 groups folded, iterations rendered since the last fold; C present with VC absent or of the moments kind.
 * pt_history_denoise_adaptive(opt, rgb_avg_host) (ptdn::Form::HistoryAdaptive; a _device form on a context): the guided filter over that
 *   blend.  Prepare: pt_history_denoise's with Tf_p, Df_p per pixel — the colour is the blend, v_k = vb_k, demodulated as there,
 *   var_raw = (v_x + v_y) + v_z — and NE[p] = Tf_p + Th in the position buffer's spare word, where pt_denoise_adaptive keeps Tf_p.
 *   Prefilter (the per-sample one, reading that word), levels and finish are pt_denoise_adaptive's kernels, unchanged: only the prepare
 *   is a new kernel instantiation, and the workspace is the shared 80 B per pixel.  sigma_color == 0 means 8.0, as in the history
 *   form.  With C absent the result is pt_denoise_adaptive's bit for bit.  Valid in both states.  Refusals: pt_history_denoise's in
 *   its order, without the adaptive state and `samples`.
 * pt_render --orbit N --reproject --denoise-history --history-threshold E [--history-threshold-cap F] [--history-threshold-min-pixels P]
 *   [--history-threshold-group G] runs a view this way per frame.  What it buys and costs: README "Threshold rounds over the blend"
 *   (tests/test_history_threshold_sim.py, profiles/history_threshold_cost.log).
 * Not built: the moments kind, the probes and the feedback beside these calls (the moments kind is refused by name; the other two
 *   need it); pt_group_*. */
int pt_history_noise_adaptive(double* sse);
int pt_readback_history_noise_samples(float* ne_host); /* pixel_count floats: NE */
int pt_history_round_threshold(int iter_first, int group_iters, float threshold, float max_fraction, int* above, int* selected);
int pt_history_render_threshold(int iter_first, int max_iters, int group_iters, float threshold, float max_fraction, int min_pixels, int* iters_done,
                                int64_t* samples_done, int* above_left);
int pt_history_resolve_adaptive(float* rgb_avg_host);
int pt_history_capture_adaptive(void);
int pt_history_denoise_adaptive(const PtDenoiseOptions* opt, float* rgb_avg_host);
/* The same arithmetic on the host (no GPU).  counts: pixels * {T_p, M_p}; the first pixel with M_p < 2 or T_p < M_p is named in a
 * refusal.  current_plane / current_var: C and VC, both NULL: absent.  pt_history_noise_adaptive_host: w_out, ne_out (pixels floats),
 * vb_out (pixels float4: {vb.xyz, +0}) and *sse, any of them NULL.  pt_history_select_threshold_blend_host:
 * pt_adaptive_select_threshold_host's arguments and C, VC.  pt_history_capture_adaptive_host: kept_planes (PT_HISTORY_KEPT_PLANES
 * planes) and kept_var (VK). */
int pt_history_noise_adaptive_host(int pixels, const float* noise_planes, const int32_t* counts, const float* current_plane, const float* current_var,
                                   float* w_out, float* ne_out, float* vb_out, double* sse);
int pt_history_select_threshold_blend_host(int w, int rows, const float* noise_planes, const int32_t* counts, const float* current_plane,
                                           const float* current_var, float threshold, int cap, int32_t* list, int* above, int* m);
int pt_history_blend_adaptive_host(int pixels, const float* rgb_sum, const int32_t* counts, const float* current_plane, float* rgb_avg);
int pt_history_capture_adaptive_host(int pixels, const float* rgb_sum, const float* feature_planes, const float* noise_planes, const int32_t* counts,
                                     const float* current_plane, const float* current_var, float* kept_planes, float* kept_var);
/* pt_denoise_adaptive_host's arguments and C, VC; the _variance_host form gives var_raw and var_0 (either may be NULL, not both). */
int pt_history_denoise_adaptive_host(int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, const int32_t* counts,
                                     const float* current_plane, const float* current_var, const PtDenoiseOptions* opt, float* rgb_avg);
int pt_history_denoise_adaptive_variance_host(int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, const int32_t* counts,
                                              const float* current_plane, const float* current_var, const PtDenoiseOptions* opt, float* var_raw, float* var_0);

/* saveImage()'s per-pixel conversion (main.cpp:91-97 x mirror, image.cpp:26-30 clamp * 255 truncated) on the
 * device: pixel_count*3 bytes, row-major, x mirrored inside each row; the tile must consist of whole rows.
 * Reads back 3 B per pixel instead of 12. */
int pt_save_u8(float samples, uint8_t* rgb8_host);

/* ---- explicit renderer instances: the operations above on a context of your own (one per GPU). ---- */
typedef struct PtContext PtContext;
int pt_ctx_create(const PtSceneDesc* scene, const PtOptions* opt, PtContext** out); /* nothing is left behind on failure */
int pt_ctx_destroy(PtContext* c);
int pt_ctx_render(PtContext* c, int iter_first, int iter_count);
int pt_ctx_sync(PtContext* c);
int pt_ctx_readback(PtContext* c, float* rgb_sum_host);
int pt_ctx_readback_device(PtContext* c, void* rgb_sum_dev);
int pt_ctx_save_u8(PtContext* c, float samples, uint8_t* rgb8_host);
int pt_ctx_save_u8_device(PtContext* c, float samples, const uint8_t** rgb8_dev); /* async on the context's stream */
int pt_ctx_preview_rgba8(PtContext* c, int iterations, uint8_t* rgba_host);
int pt_ctx_preview_rgba8_device(PtContext* c, int iterations, void* rgba_dev);
int pt_ctx_get_stats(PtContext* c, PtStats* out);
int pt_ctx_reset_stats(PtContext* c);
int pt_ctx_clear(PtContext* c);
int pt_ctx_set_camera(PtContext* c, const PtCamera* cam);
int pt_ctx_get_setup_times(PtContext* c, PtSetupTimes* out);
int pt_ctx_set_camera_ex(PtContext* c, const PtCamera* cam, uint32_t flags);
int pt_ctx_get_set_camera_times(PtContext* c, PtSetCameraTimes* out);
int pt_ctx_set_geoms(PtContext* c, const PtGeom* geoms, int num_geoms);
int pt_ctx_get_set_geoms_times(PtContext* c, PtSetGeomsTimes* out);
int pt_ctx_set_materials(PtContext* c, const PtMaterial* materials, int num_materials);
int pt_ctx_get_set_materials_times(PtContext* c, PtSetMaterialsTimes* out);
int pt_ctx_set_reference(PtContext* c, const float* rgb_avg_host);
int pt_ctx_get_convergence(PtContext* c, int iter_first, int iter_count, double* sse);
int pt_ctx_iterations_to_clean(PtContext* c, float threshold_db, int* iteration);
int pt_ctx_render_features(PtContext* c, int iter_first, int iter_count);
int pt_ctx_readback_features(PtContext* c, float* planes_host);
int pt_ctx_denoise(PtContext* c, float samples, const PtDenoiseOptions* opt, float* rgb_avg_host);
/* Asynchronous on the context's stream; *rgb_dev (pixel_count * 3 floats, inside the workspace) stays valid until the next denoise call. */
int pt_ctx_denoise_device(PtContext* c, float samples, const PtDenoiseOptions* opt, const float** rgb_dev);
int pt_ctx_denoise_guided(PtContext* c, const PtDenoiseOptions* opt, float* rgb_avg_host);
int pt_ctx_denoise_guided_device(PtContext* c, const PtDenoiseOptions* opt, const float** rgb_dev); /* as pt_ctx_denoise_device */
int pt_ctx_denoise_adaptive(PtContext* c, const PtDenoiseOptions* opt, float* rgb_avg_host);
int pt_ctx_denoise_adaptive_device(PtContext* c, const PtDenoiseOptions* opt, const float** rgb_dev); /* as pt_ctx_denoise_device */
int pt_ctx_noise_fold(PtContext* c);
int pt_ctx_get_noise(PtContext* c, double* sse, int* groups, int* iterations);
int pt_ctx_readback_noise(PtContext* c, float* planes_host);
int pt_ctx_render_until(PtContext* c, int iter_first, int max_iters, int group_iters, float target_db, int* iters_done, float* psnr_db);
int pt_ctx_adaptive_round(PtContext* c, int iter_first, int group_iters, float fraction);
int pt_ctx_render_adaptive(PtContext* c, int iter_first, int max_iters, int group_iters, float fraction, float target_db, int* iters_done,
                           int64_t* samples_done, float* psnr_db);
int pt_ctx_readback_adaptive(PtContext* c, int32_t* counts);
int pt_ctx_adaptive_round_threshold(PtContext* c, int iter_first, int group_iters, float threshold, float max_fraction, int* above, int* selected);
int pt_ctx_adaptive_round_list(PtContext* c, int iter_first, int group_iters, const int32_t* list_host, int m, int capacity);
/* The same with the list on the context's device: copied into the context's own list on the context's stream, entries not checked. */
int pt_ctx_adaptive_round_list_device(PtContext* c, int iter_first, int group_iters, const int32_t* list_dev, int m, int capacity);
const int32_t* pt_ctx_device_counts(PtContext* c); /* device pointer of the plane cnt (T_p, M_p); NULL outside the adaptive state */
int pt_ctx_render_threshold(PtContext* c, int iter_first, int max_iters, int group_iters, float threshold, float max_fraction, int min_pixels,
                            int* iters_done, int64_t* samples_done, int* above_left);
int pt_ctx_resolve(PtContext* c, float* rgb_avg_host);
/* Asynchronous on the context's stream; *rgb_dev (pixel_count * 3 floats, owned by the context, allocated by the first resolve) stays
 * valid until the next resolve: where a later filter of the resolved image can start from. */
int pt_ctx_resolve_device(PtContext* c, const float** rgb_dev);
int pt_ctx_history_capture(PtContext* c, float samples);
int pt_ctx_history_reproject(PtContext* c, const PtHistoryOptions* opt);
int pt_ctx_history_resolve(PtContext* c, float samples, float* rgb_avg_host);
/* Asynchronous on the context's stream; *rgb_dev is pt_ctx_resolve_device's buffer (valid until the next resolve of either kind). */
int pt_ctx_history_resolve_device(PtContext* c, float samples, const float** rgb_dev);
int pt_ctx_readback_history(PtContext* c, float* kept_planes, float* current_plane);
int pt_ctx_history_drop(PtContext* c);
int pt_ctx_history_capture_ex(PtContext* c, float samples, uint32_t flags);
int pt_ctx_history_reproject_ex(PtContext* c, const PtHistoryOptions* opt, uint32_t flags);
int pt_ctx_history_denoise(PtContext* c, float samples, const PtDenoiseOptions* opt, float* rgb_avg_host);
int pt_ctx_history_denoise_device(PtContext* c, float samples, const PtDenoiseOptions* opt, const float** rgb_dev); /* as pt_ctx_denoise_device */
int pt_ctx_readback_history_variance(PtContext* c, float* kept_var, float* current_var);
int pt_ctx_history_denoise_ex(PtContext* c, float samples, const PtDenoiseOptions* opt, uint32_t flags, float* rgb_avg_host);
int pt_ctx_history_denoise_ex_device(PtContext* c, float samples, const PtDenoiseOptions* opt, uint32_t flags, const float** rgb_dev); /* as pt_ctx_denoise_device */
int pt_ctx_history_round(PtContext* c, int iter_first, int group_iters, const PtHistoryRoundOptions* opt, int* fresh, int* selected);
int pt_ctx_readback_history_extra(PtContext* c, float* extra_host);
int pt_ctx_history_round_list(PtContext* c, int iter_first, int group_iters, const int32_t* list_host, int m, int capacity);
/* the same with the list in device memory of the context's device (its entries are not checked); copied on the context's stream */
int pt_ctx_history_round_list_device(PtContext* c, int iter_first, int group_iters, const int32_t* list_dev, int m, int capacity);
int pt_ctx_history_probe_keep(PtContext* c, int iter_first, int iter_count, int phase);
int pt_ctx_history_probe_check(PtContext* c, const PtHistoryProbeOptions* opt, int* probes, int* changed, int* skipped);
int pt_ctx_readback_history_probe(PtContext* c, float* kept, float* lam, int* count);
int pt_ctx_history_noise(PtContext* c, float samples, uint32_t flags, double* sse);
int pt_ctx_readback_history_noise(PtContext* c, float* w_host);
int pt_ctx_history_noise_adaptive(PtContext* c, double* sse);
int pt_ctx_readback_history_noise_samples(PtContext* c, float* ne_host);
int pt_ctx_history_round_threshold(PtContext* c, int iter_first, int group_iters, float threshold, float max_fraction, int* above, int* selected);
int pt_ctx_history_render_threshold(PtContext* c, int iter_first, int max_iters, int group_iters, float threshold, float max_fraction, int min_pixels,
                                    int* iters_done, int64_t* samples_done, int* above_left);
int pt_ctx_history_resolve_adaptive(PtContext* c, float* rgb_avg_host);
int pt_ctx_history_resolve_adaptive_device(PtContext* c, const float** rgb_dev);
int pt_ctx_history_capture_adaptive(PtContext* c);
int pt_ctx_history_denoise_adaptive(PtContext* c, const PtDenoiseOptions* opt, float* rgb_avg_host);
int pt_ctx_history_denoise_adaptive_device(PtContext* c, const PtDenoiseOptions* opt, const float** rgb_dev);
int pt_ctx_history_render_until(PtContext* c, int iter_first, int max_iters, int group_iters, float target_db, int* iters_done, float* psnr_db,
                                float* view_psnr_db);
int pt_ctx_history_denoise_feedback(PtContext* c, float samples, const PtDenoiseOptions* opt, const PtHistoryFeedbackOptions* fb, float* rgb_avg_host);
int pt_ctx_history_denoise_feedback_device(PtContext* c, float samples, const PtDenoiseOptions* opt, const PtHistoryFeedbackOptions* fb,
                                           const float** rgb_dev); /* as pt_ctx_denoise_device */
int pt_ctx_readback_history_feedback(PtContext* c, float* kept, float* current, float* pending);
const float* pt_ctx_device_noise(PtContext* c); /* device pointer of plane 0; the planes are contiguous; NULL before the first fold */
const float* pt_ctx_device_features(PtContext* c); /* device pointer of plane 0; the planes are contiguous; NULL before the first pt_ctx_render_features */
const float* pt_ctx_device_image(PtContext* c); /* device pointer of the tile SUM image */
void* pt_ctx_stream(PtContext* c);              /* the context's hipStream_t */
int pt_ctx_pixel_count(const PtContext* c);
int pt_ctx_device(const PtContext* c);

/* ---- one process, several GPUs (BASELINE config 4).  The framebuffer is cut into row-interleaved
 * tiles (device i of n owns rows i, i+n, ...; RNG keyed by the GLOBAL pixel index, so the assembled image is
 * bit-identical to the single-GPU image), every device renders its tile on its own stream with no data-path
 * collective, and the tiles meet once, at image write-out: one grouped RCCL send/recv (ncclCommInitAll
 * communicator) into device devices[0], placed row by row there, one D2H copy.  Replaces the reference's single
 * device (src/preview.cpp:112 cudaGLSetGLDevice(0)) and its write-out point (src/main.cpp:86-107). */
typedef struct PtGroup PtGroup;
/* Transport of that one exchange.  RCCL: grouped ncclSend / ncclRecv (default for distinct devices).  COPY:
 * hipMemcpyPeerAsync / hipMemcpyAsync of every tile into the same receive buffer, ordered by events — chosen
 * automatically when the device list names a device more than once (several contexts on one GPU, e.g. {0, 0, 0}:
 * RCCL cannot put two ranks of a communicator on one device), which makes the whole multi-context path runnable on a
 * one-GPU machine; selectable explicitly as a fallback.  The assembled image is the same bit for bit. */
#define PT_GROUP_TRANSPORT_AUTO 0
#define PT_GROUP_TRANSPORT_RCCL 1
#define PT_GROUP_TRANSPORT_COPY 2
int pt_group_create_ex(const PtSceneDesc* scene, const PtOptions* base, const int* devices, int num_devices, int transport,
                       PtGroup** out);
int pt_group_transport(const PtGroup* g); /* the resolved transport (PT_GROUP_TRANSPORT_RCCL or _COPY) */
/* = pt_group_create_ex(..., PT_GROUP_TRANSPORT_AUTO, out) */
int pt_group_create(const PtSceneDesc* scene, const PtOptions* base, const int* devices, int num_devices, PtGroup** out);
int pt_group_destroy(PtGroup* g);
int pt_group_size(const PtGroup* g);
PtContext* pt_group_context(PtGroup* g, int i);
int pt_group_render(PtGroup* g, int iter_first, int iter_count); /* asynchronous on every device */
int pt_group_sync(PtGroup* g);
/* pt_set_camera on every context: the camera is checked against all of them before any of them changes, so a refusal leaves
 * the whole group as it was; the group's own buffers on the root device stay. */
int pt_group_set_camera(PtGroup* g, const PtCamera* cam);
int pt_group_set_camera_ex(PtGroup* g, const PtCamera* cam, uint32_t flags); /* pt_set_camera_ex on every context, asked first in the same way */
int pt_group_set_geoms(PtGroup* g, const PtGeom* geoms, int num_geoms);      /* pt_set_geoms on every context, asked first in the same way */
int pt_group_set_materials(PtGroup* g, const PtMaterial* materials, int num_materials);  /* pt_set_materials on every context, asked first in the same way */
int pt_group_gather(PtGroup* g, float* rgb_sum_host);             /* W*H*3 floats, raw orientation */
int pt_group_gather_u8(PtGroup* g, float samples, uint8_t* rgb8_host); /* W*H*3 bytes as pt_save_u8, converted on each device */
/* The feature buffers of the whole frame: every context sums its own rows, the planes meet at the root like the image (one
 * exchange of 16 B per pixel and plane, either transport; the root's buffers are allocated on first use). */
int pt_group_render_features(PtGroup* g, int iter_first, int iter_count); /* asynchronous on every device */
int pt_group_gather_features(PtGroup* g, float* planes_host);            /* PT_FEATURE_PLANES * W*H * 4 floats, raw orientation */
/* pt_denoise of the whole frame (W*H*3 floats of averaged radiance, raw orientation), bit-identical to a single context's.  A
 * context of a group owns interleaved rows and cannot filter its own tile: the SUM image and the three planes are assembled on the
 * root device as for the two gathers above, and the filter runs there, on the root's stream, with a workspace of 80 B per frame
 * pixel owned by the group.  Errors as pt_denoise (before a feature pass: an error). */
int pt_group_denoise(PtGroup* g, float samples, const PtDenoiseOptions* opt, float* rgb_avg_host);
/* pt_denoise_guided of the whole frame, bit-identical to a single context's: as pt_group_denoise, and the two noise planes of every
 * context meet on the root like the feature planes (16 B per pixel and plane, either transport; the root's buffers are allocated on
 * first use).  The contexts of a group share M and T (pt_group_noise_fold keeps them so); a group whose contexts do not is refused. */
int pt_group_denoise_guided(PtGroup* g, const PtDenoiseOptions* opt, float* rgb_avg_host);
/* The noise estimate of the whole frame: every context folds its own rows (nothing is exchanged), the contexts' SSE_est are added
 * in context order on the host, and the estimated PSNR is taken over W*H pixels.  pt_group_render_until is pt_render_until with
 * pt_group_render, one synchronise of every device per group; group_iters 0 = the first context's iters_per_batch.  Gathering the
 * planes of a group is not offered (pt_ctx_readback_noise of pt_group_context(g, i) gives a context's rows). */
int pt_group_noise_fold(PtGroup* g);
int pt_group_get_noise(PtGroup* g, double* sse, int* groups, int* iterations);
int pt_group_render_until(PtGroup* g, int iter_first, int max_iters, int group_iters, float target_db, int* iters_done, float* psnr_db);
/* ---- adaptive sampling by threshold across a group (pt_adaptive_round_threshold, pt_render_threshold).  A context owns the rows
 * i, i + n, ...: the 3x3 prefilter of the key reads rows of other contexts, and "the cap largest keys" are the frame's, not a tile's.
 * So the frame is selected ONCE, on the root device, and the frame's list is cut into one list per context:
 *   pack       every context, on its own stream: {float w_p, int32 T_p} of its tile pixels, 8 bytes per pixel: all the key reads.
 *   exchange   one exchange of those 8 bytes per pixel to the root (either transport), the rows placed into the frame.
 *   select     the key of pt_adaptive_round on the packed frame (the same arithmetic on the same values over W x H), then the
 *              selection by threshold for cap = clamp(ceil((double)max_fraction * W*H), 1, W*H): the single context's kernels.
 *   partition  frame pixel f of the list belongs to context i = (f / W) % n as tile pixel ((f / W) / n) * W + f % W; part i holds
 *              them in input order, which is ascending tile index; the parts lie back to back.  Positions come from counts and a
 *              scan; integer atomics on counters only, so equal inputs give equal parts.  At most 64 contexts.
 *   read back  above, m and the n lengths m_i: 8 + 4n bytes and ONE synchronise of the root's stream, as a context's round has.
 *   render     part i goes to context i (a copy on context i's stream behind an event of the root's, or a grouped RCCL send /
 *              receive), and every context runs pt_ctx_adaptive_round_list_device over it on a worker for min(cap, its pixels),
 *              contexts with m_i == 0 included; they render concurrently and the call returns without a further synchronise.
 * After the same calls the SUM image, the noise planes, the counts, (above, m) of every round, the iteration numbers, the samples,
 * the resolved and the filtered image are a single context's, bit for bit.  SSE_est is added per context and then in context order
 * (pt_group_get_noise), so it may differ from the single context's in the last bits.
 * Refuses, allocating and launching nothing: what pt_adaptive_round_threshold refuses of any context, in its order, apart from the
 * tile's rows; then contexts that differ in the groups or iterations folded or in being in the adaptive state, naming the context.
 * m == 0 (or, in the driver, above <= min_pixels): nothing is rendered and no context counts a round.
 * The group's buffers (the packed frame, the selection's workspace for W*H pixels, the frame's list and the parts, all on the root;
 * 8 + 4 bytes per tile pixel on every device) are allocated by the first round and freed by pt_group_destroy; the exchange goes through
 * the one receive buffer of all the group's write-outs (16 bytes per pixel of the other contexts' tiles, allocated by the first of them).
 * pt_group_render_threshold is pt_render_threshold's loop over pt_group_render, pt_group_noise_fold and the round; group_iters 0 =
 * the first context's iters_per_batch, as in pt_group_render_until.
 * Out of scope: a group form of pt_adaptive_round / pt_render_adaptive, load balance between contexts whose parts differ in length
 * (interleaved rows are what a group has for that), and the command-line driver, which keeps --adaptive-threshold to one device. */
int pt_group_adaptive_round_threshold(PtGroup* g, int iter_first, int group_iters, float threshold, float max_fraction, int* above, int* selected);
int pt_group_render_threshold(PtGroup* g, int iter_first, int max_iters, int group_iters, float threshold, float max_fraction, int min_pixels,
                              int* iters_done, int64_t* samples_done, int* above_left);
int pt_group_gather_adaptive(PtGroup* g, int32_t* counts); /* W*H*2 int32 (T_p, M_p), raw orientation; the uniform state: the shared T, M */
int pt_group_resolve(PtGroup* g, float* rgb_avg_host);     /* W*H*3 floats: every context resolves its rows, the rows meet like the image */
/* pt_denoise_adaptive of the whole frame, bit-identical to a single context's: as pt_group_denoise_guided, and in the adaptive state
 * the count planes meet on the root as well.  Refuses what pt_denoise_adaptive refuses, in its order, apart from the tile's rows, and
 * contexts that differ as above. */
int pt_group_denoise_adaptive(PtGroup* g, const PtDenoiseOptions* opt, float* rgb_avg_host);
/* The partition on the host (no GPU): list holds m frame pixels of a frame w x h in ascending order (0 <= m <= w*h), 1 <= n <= min(h, 64);
 * parts receives m tile indices, part after part, counts the n lengths.  The device's parts equal it. */
int pt_group_partition_host(int w, int h, int n, const int32_t* list, int m, int32_t* parts, int32_t* counts);
/* Progressive preview of the running average (sendImageToPBO, pathtrace.cu:250-268, which the reference runs after every
 * iteration): W*H RGBA8 bytes, raw orientation, converted on each device, one exchange of 4 B per pixel. */
int pt_group_preview_rgba8(PtGroup* g, int iterations, uint8_t* rgba_host);

/* ---- history in groups: the reprojected history of the whole frame (pt_history_capture_ex / _reproject_ex / _resolve /
 * _denoise_ex with PT_HISTORY_MOMENTS / pt_history_round / pt_history_drop and their readbacks).  A context owns the rows i, i + n, ...
 * and cannot look up its neighbours, so the group keeps the history of the FRAME on the root device and runs the single context's
 * kernels there over W x H pixels; no kernel is the group's own.  Contract: after the same sequence of calls a group of n contexts
 * holds what ONE renderer of the whole frame holds, bit for bit, in PT_ARITH_EXACT, _FMA and _FAST — K0..K2, C, VK, VC and E in frame
 * order, the blend, the filtered image, the gathered SUM image, (fresh, selected) of every round; the contexts' PtStats.samples add up
 * to the renderer's.  Built: the plain kind, the moments kind (PT_HISTORY_MOMENTS), the objects' motion (PT_HISTORY_MOTION) and the round.
 * State, all of it on the root device, allocated (and zeroed) at first use and counted by pt_group_device_bytes: 64 bytes per frame pixel
 *   for K0 K1 K2 and C from the first capture; 32 for VK and VC from the first capture with PT_HISTORY_MOMENTS; 12 for the blend from the
 *   first resolve; 4 for the assembled E from the first call that reads E; beside the frames every filter of a group assembles (the SUM
 *   image, the features, the filter's workspace) and the selection's buffers of the threshold round, which the history round shares.
 *   On the host: the kept camera, kept / current, the kind VK and VC hold, the kept geoms and the motion table, as a context has them.
 *   reject_geom, emitter_geom and the motion table are per geom and the same for every context: context 0 builds and keeps them.
 * Lifetimes, a single context's: K, VK, the kept camera and the kept geoms survive pt_group_clear, pt_group_set_camera[_ex] and
 *   pt_group_set_geoms; C and VC become absent on each of them; pt_group_history_drop forgets K, C, VK and VC and keeps the memory.  E
 *   lives in the contexts, beside their rows of the image.  A caller who clears, moves or runs rounds on single contexts through
 *   pt_group_context breaks the group, exactly as for the fold counters; where it shows (contexts that disagree on E) the call refuses.
 * Steps of every call for n > 1: the refusals; the gathers onto the root (one exchange and row placement per payload, as every
 *   write-out) — the capture assembles S, the features and E, the lookup the features, the resolve S and E, the filter S, the features
 *   and E; E travels as a payload of 4 bytes per pixel and only while it is present, when the counted launches run; the single context's
 *   launch on the root's stream with the view of the kept camera over H rows from row 0; one copy to the host and a synchronise of every
 *   context where something is returned.  The capture and the lookup return nothing and do not synchronise.  Nothing assembled is kept
 *   from one call to the next.  n == 1 forwards to context 0.
 * The round: what pt_history_round refuses of any context; the features gathered; the key over the frame with the group's C (absent:
 *   every non-emitter hit pixel is fresh); the threshold selection with threshold bits 0 and cap = clamp(ceil((double)max_fraction *
 *   W*H), 1, W*H); the partition; fresh, m and the n lengths read back, 8 + 4n bytes behind ONE synchronise of the root's stream.
 *   m == 0: nothing is rendered, merged or allocated, E keeps its state.  Otherwise part i goes to context i as in the threshold round
 *   and every context runs pt_ctx_history_round_list_device over it on a worker for min(cap, its pixels), contexts with an empty part
 *   included (they render nothing and hold E from then on); the contexts render concurrently, the call returns without a further synchronise.
 * Refuses, under the group function's name, nothing allocated or launched, nothing changed in the group or in any context — first what
 *   pt_history_* refuses of any context, in the single context's order and apart from the tile's rows, each condition over the contexts
 *   in turn: a failed context; an undefined flag bit or an excluded pair; the adaptive state; no feature pass since the last clear or
 *   move (not the resolve); samples; the options (the round: the iterations and PtOptions.convergence come right after the failed
 *   context) — then the group's own: PT_HISTORY_VARIANCE, PT_HISTORY_FEEDBACK and pt_group_history_denoise_ex with flags 0, "not built
 *   for a group"; nothing captured, or nothing captured with moments (the lookup); a C without moments (the capture with
 *   PT_HISTORY_MOMENTS, the filter); contexts that disagree on E being present, naming the context; for the round the threshold
 *   round's limits (at most 64 contexts, fewer than 32768 rows, at most 2^30 pixels); last a null output buffer.
 * While any context holds E, every group entry point that reads the image as a uniform SUM refuses as the single context does:
 *   pt_group_denoise, _denoise_guided, _denoise_adaptive, pt_group_noise_fold, pt_group_render_until, the adaptive round and driver,
 *   pt_group_resolve, pt_group_gather_u8, pt_group_preview_rgba8; nothing allocated or launched.  pt_group_gather keeps working.
 * Cost on one GPU and what share of a view the gathers take: README "History in groups" (profiles/group_history_cost.log).
 * Out of scope: PT_HISTORY_VARIANCE, pt_history_noise / _render_until, the probes and the feedback in groups; the command line
 *   (pt_render refuses --reproject with --gpus); caching assembled frames between calls; distributing the lookup or the filter over
 *   the devices; load balance between parts. */
int pt_group_clear(PtGroup* g); /* pt_clear on every context; the group's C and VC become absent */
int pt_group_history_capture_ex(PtGroup* g, float samples, uint32_t flags);             /* flags: 0 or PT_HISTORY_MOMENTS */
int pt_group_history_reproject_ex(PtGroup* g, const PtHistoryOptions* opt, uint32_t flags); /* 0 or PT_HISTORY_MOMENTS, each alone or with PT_HISTORY_MOTION */
int pt_group_history_resolve(PtGroup* g, float samples, float* rgb_avg_host);           /* W*H*3 floats, raw orientation */
int pt_group_history_denoise_ex(PtGroup* g, float samples, const PtDenoiseOptions* opt, uint32_t flags, float* rgb_avg_host); /* flags == PT_HISTORY_MOMENTS */
int pt_group_history_round(PtGroup* g, int iter_first, int group_iters, const PtHistoryRoundOptions* opt, int* fresh, int* selected);
int pt_group_history_drop(PtGroup* g);
int pt_group_readback_history(PtGroup* g, float* kept_planes, float* current_plane);    /* pt_readback_history's layouts over W*H pixels */
int pt_group_readback_history_variance(PtGroup* g, float* kept_var, float* current_var);
int pt_group_readback_history_extra(PtGroup* g, float* extra);                          /* E of the frame, W*H floats; zeros while absent */
int64_t pt_group_device_bytes(const PtGroup* g); /* bytes of the group's own device buffers, on every device (the contexts': PtStats.device_bytes) */

/* The convergence metric of the whole frame: the reference frame is a W*H image (raw orientation, averaged radiance) of which
 * every context receives its rows; the contexts' SSEs are added in context order (one double per iteration and context crosses to
 * the host, nothing goes on the data path); the PSNR of pt_group_iterations_to_clean is over all W*H pixels. */
int pt_group_set_reference(PtGroup* g, const float* rgb_avg_host);
int pt_group_get_convergence(PtGroup* g, int iter_first, int iter_count, double* sse);
int pt_group_iterations_to_clean(PtGroup* g, float threshold_db, int* iteration);

/* ---- stage-level entry points (same kernels, caller-supplied HOST arrays, SoA:
 * vec3 arrays are [3][n]).  Used by the parity tests; each uploads, launches the
 * production kernel, downloads. ----------------------------------------------- */
/* generateRayFromCamera (pathtrace.cu:270-286) for pixels [pix_begin, pix_begin+n). */
int pt_stage_generate(int pix_begin, int n, float* origin, float* dir);
/* computeIntersections (pathtrace.cu:288-333): closest hit per ray. */
int pt_stage_intersect(int n, const float* origin, const float* dir, float* t, float* normal, int32_t* material,
                       float* point);
/* The same closest hits, found with the uniform-grid walk of the fused kernels instead of the BVH scan (arrays and miss
 * convention of pt_stage_intersect): the walk hands the leaf tests a superset of the leaves whose box the ray passes, so
 * every ray's record equals pt_stage_intersect's bit for bit, in every arithmetic mode (tests/test_gpu_grid_rays.py).
 * primary_form 1: the walk as depth 0 runs it — the reference's arithmetic on the reference's (or tightened) boxes, as
 * pt_stage_intersect of an exact-mode renderer computes; 0: as the bounce kernel runs it, in the mode's arithmetic.  Refused
 * when the renderer walks no grid (PtStats.grid_cells == 0; PtOptions.debug_flags 256 forces one), on a null pointer and,
 * with primary_form 0 on tightened leaves (PtStats.tight_leaves > 0), for the origins pt_stage_intersect refuses. */
int pt_stage_intersect_grid(int n, const float* origin, const float* dir, int primary_form, float* t, float* normal,
                            int32_t* material, float* point);
/* The grid that walk runs on, read from the host copy of the uploaded cell table: shape, pad, cells, records
 * (num_leaves: the scene's primitives) and the length of the longest cell list.  pt_build_grid builds the cost model's
 * grid without the camera; this is the one pt_init kept.  Refused when the renderer walks no grid. */
int pt_stage_grid_info(PtGridInfo* info, int32_t* max_cell_records);
/* The camera-dependent tables of the default renderer as they lie on the device, byte for byte: `which` 0 nodes, 1 their centre / half
 * extent copies, 2 the top list, 3 its copies, 4 the cell table of the grid with its guard cells, 5 the grid's records, 6 their copies,
 * 7 the cull margin (4 bytes), 8 the geom table (which pt_set_geoms rewrites).  *bytes receives the table's size; up to `cap` bytes of it go to `out` (may be NULL with cap 0).  A
 * table the renderer does not have (copies outside the fast build, a grid where none is built) gives *bytes = 0.  Synchronises. */
int pt_stage_read_tables(int which, void* out, uint64_t cap, uint64_t* bytes);
/* Device self-check of csrc/pt_camera_tables.h, in the manner of pt_selfcheck_ieee: one of its functions runs on the GPU and on the
 * host over the same operands, and *mismatches counts the operand sets whose results differ in any bit.  kind 0 double sqrt, 1 double
 * a / b (a result that is a NaN on both sides counts as equal), 2 (float) of a double and nextafterf of it in both directions (also
 * against libm's nextafterf on the host), 3 center_half_box (leaf and inner form), 4 sphere_tight_box, 5 the grid's cell_range.
 * The operands are a fixed list of edge values per kind (+-0, denormals, the largest finite values, values that convert to infinity,
 * singular matrices) followed by `count` pseudo-random sets derived from `seed`.  Needs no renderer; runs on the current device. */
int pt_selfcheck_camera_math(int kind, uint64_t count, uint32_t seed, uint64_t* mismatches);
/* The grid half of the device build (csrc/pt_camera_tables.hip: count, scan, scatter, records) on caller-supplied nodes instead of a
 * scene's: `num_nodes` nodes of which those with geom >= 0 are leaves, the types of `num_geoms` geoms, the bounds and the coordinate
 * magnitude the frame is computed from (pt::grid_frame), the resolution (clamped to [1, 512] per axis) and whether the centre / half
 * extent copies are made.  The scalars, the launches and the decisions between them are those of pt_set_camera_ex with
 * PT_SET_CAMERA_DEVICE_TABLES on a renderer with a forced grid (debug_flags 256).  Needs the default renderer for its device and
 * stream only: the workspace is scratch, the renderer's tables and its device copy of the camera-independent tables are left alone.
 * *out always receives the shape, the guard, the cells, and what was counted; with status 0 `start` receives the cell table with
 * both runs of guard cells (num_cells + 1 + 2 * guard words), `items` the records (refs of them) and, with center_half, `items_b`
 * their copies.  start_cap and items_cap are the arrays' capacities in words and records: a built grid that does not fit is refused.
 * With `start` and `items` both NULL nothing is built beyond the count (a query for the sizes).
 * Refused: no renderer; a null pointer (items_b only with center_half); num_nodes < 1 or num_geoms < 1; a coord_mag that is negative
 * or not finite; a node whose geom is outside [-1, num_geoms); a node whose box has bmin > bmax or a NaN. */
int pt_stage_camera_grid(const PtTableNode* nodes, int num_nodes, const int32_t* geom_types, int num_geoms, const float root_min[3],
                         const float root_max[3], double coord_mag, const int32_t res[3], int center_half, PtCameraGridResult* out,
                         uint32_t* start, uint64_t start_cap, PtGridRecord* items, PtGridRecord* items_b, uint64_t items_cap);
/* shadeAndExtendRays (pathtrace.cu:336-437) for live paths at `depth`:
 * in/out origin, dir, color; out alive[n] (1 = path continues).  Dead paths get the
 * retirement colour (sky factor applied (trace_depth - depth) times on a miss). */
int pt_stage_shade(int n, int depth, const int32_t* iter, const int32_t* pixel, const float* t, const float* normal,
                   const int32_t* material, const float* point, float* origin, float* dir, float* color,
                   int32_t* alive);

/* saveImage + savePNG conversion kernel (pt_save_u8) on a caller-supplied SUM image of w*h pixels (tests). */
int pt_stage_save_u8(int w, int h, float samples, const float* rgb_sum, uint8_t* rgb8);

/* The filter kernels of pt_denoise on caller-supplied host arrays (pt_denoise_host's arguments; rows < 32768). */
int pt_stage_denoise(int w, int rows, const float* rgb_sum, const float* planes, float samples, const PtDenoiseOptions* opt, float* rgb_avg);
/* The kernels of pt_denoise_guided on caller-supplied host arrays (pt_denoise_guided_host's arguments; rows < 32768). */
int pt_stage_denoise_guided(int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, int groups, int64_t iters,
                            const PtDenoiseOptions* opt, float* rgb_avg);

/* The kernels of pt_denoise_adaptive on caller-supplied host arrays (pt_denoise_adaptive_host's arguments; rows < 32768). */
int pt_stage_denoise_adaptive(int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, const int32_t* counts,
                              const PtDenoiseOptions* opt, float* rgb_avg);
/* The selection's kernels on caller-supplied host arrays (pt_adaptive_select_host's arguments; rows < 32768). */
int pt_stage_adaptive_select(int w, int rows, const float* noise_planes, const int32_t* counts, int m, int32_t* list);
/* The worker context of pt_adaptive_round alone: iterations iter_first .. iter_first + iter_count - 1 of the m listed tile pixels
 * (distinct, in any order) — rgb_sum_host receives their group sum, m * 3 floats in list order: bit for bit the listed rows of what
 * pt_render adds to the image for the same iterations.  Changes neither the image nor the folds nor the state of the renderer. */
int pt_stage_render_list(const int32_t* list, int m, int iter_first, int iter_count, float* rgb_sum_host);
/* pt_stage_render_list on a worker planned for `capacity` >= m pixels (pt_adaptive_round_threshold's): the worker is kept across
 * calls while the capacity is equal, so calls with different m run one set of buffers under different live plans. */
int pt_stage_render_list_capacity(const int32_t* list, int m, int capacity, int iter_first, int iter_count, float* rgb_sum_host);
/* The threshold selection's kernels on caller-supplied host arrays (pt_adaptive_select_threshold_host's arguments; rows < 32768). */
/* The partition's kernels on caller-supplied host arrays (pt_group_partition_host's arguments). */
int pt_stage_group_partition(int w, int h, int n, const int32_t* list, int m, int32_t* parts, int32_t* counts);
int pt_stage_adaptive_select_threshold(int w, int rows, const float* noise_planes, const int32_t* counts, float threshold, int cap, int32_t* list,
                                       int* above, int* m);

/* The reprojection's kernel on caller-supplied host arrays (pt_history_reproject_host's arguments; rows < 32768). */
int pt_stage_history_reproject(int w, int rows, int row0, const PtCamera* kept_cam, const float* kept_planes, const float* feature_planes,
                               const uint8_t* reject_geom, int num_geoms, const PtHistoryOptions* opt, float* current_plane);
/* The same with the variance side (pt_history_reproject_variance_host's arguments), and the history filter's kernels on
 * caller-supplied host arrays (pt_history_denoise_host's arguments; rows < 32768). */
int pt_stage_history_reproject_variance(int w, int rows, int row0, const PtCamera* kept_cam, const float* kept_planes, const float* feature_planes,
                                        const uint8_t* reject_geom, int num_geoms, const PtHistoryOptions* opt, const float* kept_var, float* current_plane,
                                        float* current_var);
int pt_stage_history_denoise(int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, int groups, int64_t iters, float samples,
                             const float* current_plane, const float* current_var, const PtDenoiseOptions* opt, float* rgb_avg);
/* The lookup with moments (pt_history_reproject_moments_host's arguments) and the moments form of the filter — prepare, the spatial
 * estimate, prefilter, levels, finish — (pt_history_denoise_moments_host's arguments but its optional outputs; rows < 32768). */
int pt_stage_history_reproject_moments(int w, int rows, int row0, const PtCamera* kept_cam, const float* kept_planes, const float* feature_planes,
                                       const uint8_t* reject_geom, int num_geoms, const PtHistoryOptions* opt, const float* kept_var, float* current_plane,
                                       float* current_var);
/* The lookup with the objects' motion through k_history_reproject_motion (pt_history_reproject_motion_host's arguments; rows < 32768). */
int pt_stage_history_reproject_motion(int w, int rows, int row0, const PtCamera* kept_cam, const float* kept_planes, const float* feature_planes,
                                      const uint8_t* reject_geom, int num_geoms, const PtHistoryOptions* opt, const float* kept_var, const float* table,
                                      const uint8_t* kind, uint32_t flags, float* current_plane, float* current_var);
/* The lookup with the materials' edits through k_history_reproject_materials (pt_history_reproject_materials_host's arguments; rows < 32768). */
int pt_stage_history_reproject_materials(int w, int rows, int row0, const PtCamera* kept_cam, const float* kept_planes, const float* feature_planes,
                                         const uint8_t* reject_geom, int num_geoms, const PtHistoryOptions* opt, const float* kept_var, const float* table,
                                         const uint8_t* kind, const float* recolor, const uint8_t* rkind, uint32_t flags, float* current_plane,
                                         float* current_var);
int pt_stage_history_denoise_moments(int w, int rows, const float* rgb_sum, const float* planes, float samples, const float* current_plane,
                                     const float* current_var, const PtDenoiseOptions* opt, float* rgb_avg);
/* The history round's key and selection, and its merge, through the device kernels on caller-supplied host arrays
 * (pt_history_select_host's and pt_history_merge_host's arguments; rows < 32768).  list: all cap entries are returned, those behind
 * *m are -1. */
int pt_stage_history_select(int w, int rows, const float* feature_planes, const float* current_plane, const uint8_t* emitter_geom, int num_geoms,
                            const PtHistoryRoundOptions* opt, int32_t* list, int* fresh, int* m);
int pt_stage_history_merge(int pixels, float* rgb_sum, float* extra, const int32_t* list, int m, const float* group_sum, int group_iters);
/* The estimate of the blend's noise through k_history_noise and the reduction, on caller-supplied host arrays (pt_history_noise_host's
 * arguments and refusals; *sse is the device's double). */
int pt_stage_history_noise(int pixels, const float* noise_planes, int groups, int64_t iters, float samples, const float* current_plane,
                           const float* current_var, float* w_out, double* sse);
/* Threshold rounds over the blend through their kernels on caller-supplied host arrays (the *_host twins' arguments and refusals;
 * rows < 32768): pass A and the reduction (*sse is the device's double); passes A and B and the round's selection (list: all cap
 * entries are returned, those behind *m are -1); the capture and the blend (rgb_avg may be NULL); the filter. */
int pt_stage_history_noise_adaptive(int pixels, const float* noise_planes, const int32_t* counts, const float* current_plane, const float* current_var,
                                    float* w_out, float* ne_out, double* sse);
int pt_stage_history_select_threshold_blend(int w, int rows, const float* noise_planes, const int32_t* counts, const float* current_plane, const float* current_var,
                                            float threshold, int cap, int32_t* list, int* above, int* m);
int pt_stage_history_capture_adaptive(int pixels, const float* rgb_sum, const float* feature_planes, const float* noise_planes, const int32_t* counts,
                                      const float* current_plane, const float* current_var, float* kept_planes, float* kept_var, float* rgb_avg);
int pt_stage_history_denoise_adaptive(int w, int rows, const float* rgb_sum, const float* planes, const float* noise_planes, const int32_t* counts,
                                      const float* current_plane, const float* current_var, const PtDenoiseOptions* opt, float* rgb_avg);
/* The lookup with the filtered colour through k_history_reproject_feedback, and the feedback form of the filter — its prepare (counted
 * when `extra` is given), the moments form's kernels, the tap — on caller-supplied host arrays (the host forms' arguments but var_raw and
 * mark; rgb_avg or tap may be NULL, not both; rows < 32768). */
int pt_stage_history_reproject_feedback(int w, int rows, int row0, const PtCamera* kept_cam, const float* kept_planes, const float* feature_planes,
                                        const uint8_t* reject_geom, int num_geoms, const PtHistoryOptions* opt, const float* kept_var, const float* kept_fb,
                                        const float* table, const uint8_t* kind, float* current_plane, float* current_var, float* current_fb);
int pt_stage_history_denoise_feedback(int w, int rows, const float* rgb_sum, const float* planes, float samples, const float* extra, const float* current_plane,
                                      const float* current_var, const float* current_fb, const PtDenoiseOptions* opt, const PtHistoryFeedbackOptions* fb,
                                      float* rgb_avg, float* tap);

/* ---- image output (src/image.cpp:22-45, src/main.cpp:86-107) ------------- */
/* rgb_sum: W*H*3 floats (raw orientation); writes <path> as 8-bit PNG of
 * clamp(sum/samples)*255 with the x mirror of saveImage(); no gamma. */
int pt_save_png(const char* path, const float* rgb_sum, int w, int h, float samples);
/* The same file from bytes that are already converted and mirrored (pt_save_u8 / pt_group_gather_u8). */
int pt_write_png_rgb8(const char* path, const uint8_t* rgb8, int w, int h);
/* "<name>.<UTC yyyy-mm-dd_hh-mm-ssz>.<samples>samp": the base name saveImage() composes (main.cpp:99-102,
 * preview.cpp:18-24 currentTimeString, taken once per process like main.cpp:35; `samples` is streamed as a float like
 * the reference's); writes at most cap bytes incl. the terminator, returns the full length. */
int pt_output_basename(const char* name, int samples, char* out, int cap);
int pt_save_pfm(const char* path, const float* rgb_sum, int w, int h, float samples);
/* The inverse of pt_save_pfm: *w, *h receive the size; rgb_sum (may be NULL to ask for the size only; else cap_pixels * 3 floats,
 * cap_pixels >= w * h) receives the raw-orientation image times `samples` — the SUM image bit for bit when the file was written
 * with samples = 1, and the averaged radiance pt_set_reference wants when read with samples = 1.  Three-channel "PF" files of
 * either byte order. */
int pt_load_pfm(const char* path, float* rgb_sum, int cap_pixels, int* w, int* h, float samples);
/* image::saveHDR (src/image.cpp:41-45, stbi_write_hdr; main.cpp:106 keeps the call commented out) with saveImage()'s x
 * mirror and division by `samples`: Radiance RGBE, run-length coded, byte for byte what the reference's writer emits
 * (tests/golden/ref_hdr.json, made by the reference's image.cpp + stb.cpp compiled in place). */
int pt_save_hdr(const char* path, const float* rgb_sum, int w, int h, float samples);

#ifdef __cplusplus
}
#endif
#endif /* PT_AMD_H */
