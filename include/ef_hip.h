/* libefusion_hip.so — C ABI of the MI355X-native ElasticFusion per-frame engine.
 *
 * Plain C, opaque context, raw pointers and sizes only; every call returns 0 on success or a negative
 * EF_E* code (ef_last_error() gives the message).  Nothing exits the process, nothing is global: the
 * reference's process-wide Resolution/Intrinsics singletons (Core/Utils/Resolution.h:25-58,
 * Intrinsics.h:25-51) become fields of ef_config.  A context is single-owner and externally
 * synchronised, the same contract as the reference's ElasticFusion object.
 *
 * Three tiers, mirroring the reference's own layering:
 *   1. frame tier      ef_create / ef_process_frame / getters      <-> class ElasticFusion
 *                                                                       (Core/ElasticFusion.h:40-255)
 *   2. subsystem tier  ef_preprocess / ef_track / ef_predict / ...  <-> RGBDOdometry, IndexMap,
 *                                                                       GlobalModel, FillIn, ComputePack
 *   3. operator tier   ef_op_*  on raw DEVICE pointers               <-> the 17 free functions of
 *                                                                       Core/Cuda/cudafuncs.cuh:61-169
 *                                                                       and the GLSL passes (one each)
 * All image layouts are the reference's (planar float[3*rows][cols] maps, 16-byte DataTerm,
 * 48-byte surfels = 3 x vec4).  "dev" pointers are HIP device pointers.
 */
#ifndef EF_HIP_H_
#define EF_HIP_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define EF_OK 0
#define EF_EINVAL (-1)   /* bad argument */
#define EF_EHIP (-2)     /* HIP runtime error (message has the hipError string) */
#define EF_ENOMEM (-3)
#define EF_ESTATE (-4)   /* call not valid in the current state */
#define EF_ECAPACITY (-5) /* surfel capacity exceeded: the map was clamped to max_surfels (a warning: ef_synchronize reports it once and clears it; the clamped map stays readable) */

typedef struct ef_ctx ef_ctx;

/* ---- configuration: ElasticFusion ctor arguments (Core/ElasticFusion.h:42-58) + the two singletons */
typedef struct ef_config {
  int width, height;          /* Resolution::getInstance(w,h)                       */
  float fx, fy, cx, cy;       /* Intrinsics::getInstance(fx,fy,cx,cy)               */
  int time_delta;             /* timeDelta       (200; INT_MAX/2 in open loop)      */
  float confidence;           /* confidence      (10)                               */
  float depth_cut;            /* depthCut        (3 m)                              */
  float icp_weight;           /* icpThresh       (10)                               */
  int fast_odom;              /* fastOdom        (0)                                */
  int so3;                    /* so3             (1)                                */
  int frame_to_frame_rgb;     /* frameToFrameRGB (0)                                */
  int pyramid;                /* setPyramid      (1)                                */
  int rgb_only;               /* setRgbOnly      (0)                                */
  int close_loops;            /* closeLoops (0 = -o): 1 runs the LOCAL loop closure every frame (below) and, once
                                 ef_enable_global_closure was called, the fern-based GLOBAL one before it */
  uint32_t max_surfels;       /* surfel capacity; reference: 3072*3072 (GlobalModel.cpp:22-24) */
  int device;                 /* HIP device ordinal                                 */
  void* stream;               /* hipStream_t to run on, or NULL to create a private one */
} ef_config;

void ef_default_config(ef_config* cfg);   /* front-end defaults, MainController.cpp:37-43,69-104, -o */

/* ---- lifecycle ---- */
int ef_create(const ef_config* cfg, ef_ctx** out);
void ef_destroy(ef_ctx* ctx);
const char* ef_last_error(const ef_ctx* ctx);   /* ctx may be NULL: last error of a failed ef_create */
void* ef_stream(ef_ctx* ctx);                   /* the hipStream_t all work is enqueued on */
int ef_synchronize(ef_ctx* ctx);

/* ---- frame tier ----
 * ef_process_frame == ElasticFusion::processFrame(rgb, depth, timestamp, weightMultiplier, in_T_wc)
 * (Core/ElasticFusion.h:70-75).  rgb: W*H*3 bytes row-major; depth: W*H uint16 millimetres, 0 invalid.
 * Host pointers are borrowed for the duration of the call (staged synchronously, like the reference's
 * glTexture upload, ElasticFusion.cpp:278-280); all device work is only ENQUEUED: the call does not
 * wait for the GPU.  in_T_wc: 16 doubles row-major or NULL.
 * ef_process_frame_dev takes DEVICE pointers (frames already resident in HBM; the bench path). */
int ef_process_frame(ef_ctx* ctx, const uint8_t* rgb, const uint16_t* depth, int64_t timestamp,
                     float weight_multiplier, const double* in_T_wc16);
int ef_process_frame_dev(ef_ctx* ctx, const uint8_t* rgb_dev, const uint16_t* depth_dev, int64_t timestamp,
                         float weight_multiplier, const double* in_T_wc16);
/* Input-stage overlap (default off; on = 1, or 2 to start the copy-in and the bilateral filter already during the previous tracker): the part of a frame that
 * needs only the new images (copy-in, bilateral filter + metric depth, frame-side pyramids) is enqueued on a second
 * internal stream and runs while the previous frame is still being fused.  Results are identical either way.  A context whose tracker is the
 * persistent launch (ef_set_persistent_tracker 1, the default on a 256-CU chip) treats 2 as 1: that launch needs every CU to itself. */
int ef_set_input_overlap(ef_ctx* ctx, int on);
/* ... and that second stream restricted to every n-th CU of the chip (n <= 1: no restriction, the default): the bilateral filter of frame k + 1,
 * the one ALU-bound kernel of a frame, then shares the chip with the latency-bound fusion / prediction kernels of frame k instead of displacing
 * them.  (With the persistent tracker, which needs the whole chip to itself, use overlap mode 1: the input stage waits for the tracker.) */
int ef_set_input_cu_mask(ef_ctx* ctx, int one_in_n);
/* hipGraph replay of the tracker (default off): the ~70 kernel launches of one getIncrementalTransformation
 * (RGBDOdometry.cpp:259-571) are captured once per pyramid parity and replayed with one hipGraphLaunch per frame.
 * Identical results; it only trims host-side launch work (BASELINE.json configs[4]). */
int ef_set_graph_replay(ef_ctx* ctx, int on);
/* The whole of RGBDOdometry::getIncrementalTransformation (RGBDOdometry.cpp:259-553: the SO(3) pre-alignment loop and every Gauss-Newton
 * iteration of every pyramid level, with their update steps) as ONE persistent launch of 256 co-resident workgroups, one per CU (default, on)
 * instead of one launch per step (off: 68 launches per call).  The same sums in the same order: results are bit-identical either way
 * (tests/test_gpu_frame.py runs both).  The launch needs the whole chip at once; it checks that at its start, and when other work holds
 * part of the chip for milliseconds (another process, a long kernel on another stream) the call runs on one workgroup instead — slower, the
 * same results, nothing for the caller to do (ef_get_tracker_fallbacks counts these).  Persistent launches of one process on one device are
 * chained in enqueue order, so several contexts never starve one another.  With rgbOnly and under ef_set_graph_replay the launch-per-step
 * script runs.  on = 2 (reference-order builds: the default library; what a device that reports 128 .. 255 CUs gets by default, fewer: 0):
 * round 3's form — the levels of at most 131072 pixels + the SO(3) loop as one launch of 128 workgroups, three launches per level-0 iteration —
 * whose time-out makes ef_synchronize return EF_EHIP.  A protocol failure of either persistent form (a wait that timed out after the whole
 * grid had reported in) is sticky and is reported by the NEXT ef_process_frame[_dev] and by ef_synchronize (EF_EHIP). */
int ef_set_persistent_tracker(ef_ctx* ctx, int on);
/* Level-0 Gauss-Newton iterations as TWO launches instead of three: the update step (one workgroup's worth of work) is evaluated by
 * workgroup 0 of the correspondence-search launch and handed to that launch's other workgroups as tagged granules (they poll with their
 * pixel loads in flight) instead of being a launch of its own.  Same arithmetic, bit-identical results.  Off by default (measured:
 * DESIGN.md 6). */
int ef_set_fused_step(ef_ctx* ctx, int on);
/* The persistent tracker launch keeps the pose-INDEPENDENT inputs of a pyramid level's pixel visits (current vertex / normal maps: the operands
 * of icpStep's search that the pixel itself addresses, Core/Cuda/reduce.cu:228-262; the frame's depth, intensity, gradients and the photometric
 * gate: residualKernel's, reduce.cu:631-667) in LDS for all iterations of the level (round 6; default on).  0 = stream them from memory in every
 * iteration as round 5's launch did (A/B).  Same arithmetic on the same values: bit-identical results. */
int ef_set_resident_levels(ef_ctx* ctx, int on);
/* Odometry only (BASELINE.json configs[4], "open-loop odometry-only ... throughput ceiling"): frames are pre-processed, tracked against
 * the model prediction and the prediction is renewed at the new pose, but nothing is fused (the map stays as it is: indexMap, fuse and
 * clean of ElasticFusion.cpp:536-585 are skipped, like a frame whose tracking failed under relocalisation).  Off by default. */
int ef_set_track_only(ef_ctx* ctx, int on);
/* Device half of a loop closure: hands a deformation graph (HOST pointer, nodes x 16 floats sorted by time, layout of
 * GlobalModel::clean's rawGraph, GlobalModel.cpp:536-546) to the NEXT ef_process_frame, whose clean pass applies it to the
 * whole map exactly as ElasticFusion.cpp:558-585 does (synthesizeDepth first unless is_fern).  For a caller that finds loop closures
 * and optimises the graph itself — or with ef_closure_* / ef_solve_deformation below. */
int ef_set_deformation(ef_ctx* ctx, const float* graph_host, int nodes, int is_fern);
/* ---- local loop closure, front half (ElasticFusion.cpp:447-527; contexts created with close_loops = 1) ----
 * After tracking, every frame: the INACTIVE part of the model (surfels not seen for time_delta frames) is predicted into the
 * camera (IndexMap::combinedPredict(..., INACTIVE), IndexMap.cpp:293-393), a second tracker (RGBDOdometry modelToModel) registers
 * it against the ACTIVE prediction, and if the covariance / ICP-count / ICP-error gates hold (:473-484) the surface constraints
 * of :485-509 are sampled every 20 pixels (Resize::vertex / Resize::time).  What the reference does next — Deformation::constrain,
 * a sparse non-linear solve with CHOLMOD — is the registered solver's job: it receives the constraints and may return a
 * deformation graph (same layout as ef_set_deformation); the engine then does what :514-527 and :558-585 do: T_wc := T_wc_est,
 * synthesizeDepth, and this frame's clean pass applies the graph to the whole map.  Costs one stream synchronisation per frame,
 * where the reference reads the constraint buffers back. */
typedef struct ef_local_loop {
  int attempted;            /* the front half ran in the last ef_process_frame (tick > 1) */
  int cov_ok;               /* no diagonal entry of modelToModel's covariance above covThresh */
  int gates_ok;             /* cov_ok && lastICPCount > icpCountThresh && lastICPError < icpErrThresh */
  int n_constraints;        /* surface constraints sampled (0 unless gates_ok) */
  int applied;              /* the solver accepted: pose replaced, graph (if any) applied by this frame's clean */
  int graph_nodes;
  int graph_capacity;       /* nodes the solver's graph_out has room for (1023 = GlobalModel::MAX_NODES - 1); set before the solver is called */
  int reserved_;
  float stats[6];           /* modelToModel: lastICPError, lastICPCount, lastRGBError, lastRGBCount, lastSO3Error, lastSO3Count */
  double cov_diag[6];       /* diagonal of getCovariance() up to and including the first entry above covThresh */
  double T_wc_curr[16];     /* pose after frame-to-model tracking, row-major */
  double T_wc_est[16];      /* pose proposed by the model-to-model registration */
} ef_local_loop;
/* constraints: n rows of 8 doubles {vert_w_curr xyz (source), vert_w_est xyz (target), time the inactive surface was last seen,
 * pin (1 while no deformation has been applied yet, ElasticFusion.cpp:507-508)}.  graph_out has room for info->graph_capacity x 16 floats
 * (1023): a solver must not write more; a *nodes_out beyond it makes the frame fail with EF_EINVAL.
 * Return non-zero to accept (Deformation::constrain returning true); called on the thread inside ef_process_frame. */
typedef int (*ef_loop_solver)(void* user, const ef_local_loop* info, const double* constraints, int n, float* graph_out, int* nodes_out);
int ef_set_loop_solver(ef_ctx* ctx, ef_loop_solver fn, void* user);   /* NULL: gates and constraints are still evaluated */
/* The built-in solver in that place: Deformation::constrain(..., fernMatch = false) re-implemented as a host-side banded Gauss-Newton
 * optimiser of the embedded deformation graph (Deformation.cpp:88-215, DeformationGraph.cpp; no CHOLMOD), run on the graph nodes
 * ef_sample_graph yields for the current map.  With it a closeLoops context closes LOCAL loops end to end.  A registered
 * ef_loop_solver takes precedence. */
int ef_use_builtin_loop_solver(ef_ctx* ctx, int on);
/* the same optimiser on explicit inputs (host arrays, no context, no GPU): nodes4 = n_nodes x {x, y, z, time} ascending in time,
 * constraints8 as ef_get_local_loop returns them (all sourced at src_time), nodes no younger than last_deform_time stay fixed;
 * graph16_out = n_nodes x 16 floats in the layout ef_set_deformation takes.  EF_ESTATE when there are not more than 4 nodes. */
int ef_solve_local_deformation(const float* nodes4, int n_nodes, const double* constraints8, int n_constraints, int64_t src_time,
                               int64_t last_deform_time, float* graph16_out, float* error_out, float* mean_constraint_error_out);
/* Deformation::constrain in its general form (Deformation.cpp:88-215), the GLOBAL deformation included: constraints are the entries of
 * Deformation::constraints — `relative`: the source has to land wherever the graph carries the target (the constraints a local closure
 * leaves behind, Deformation.cpp:160-173); `pin`: a target held in place (src == target) —, fern_match selects the global closure's
 * rules (nothing to do below 0.06 m mean constraint error; accepted only when the optimised mean error is below 3e-4 and the energy
 * below 0.12; pass last_deform_time = 0 as Deformation.cpp:143 does).  poses16 (n_poses x 16, in/out) with pose_times: the keyframe
 * poses (and with fern_match the trajectory) carried along by DeformationGraph::applyGraphToPoses — translation only, as observed in
 * the reference.  For the global graph nodes4 is every 5th node of ef_sample_graph (Deformation::sampleGraphFrom, :217-237).
 * new_relative_out (room for n_constraints entries, optional): after an accepted LOCAL solve, the relative constraints to hand to
 * later global ones (newRelativeCons: the deformed source of every plain constraint against its target).
 * EF_OK: accepted, graph16_out / poses16 written; EF_ESTATE: rejected (or not more than 4 nodes). */
typedef struct ef_graph_constraint {
  double src[3], target[3];
  int64_t src_time, target_time;
  int relative, pin;
} ef_graph_constraint;
int ef_solve_deformation(const float* nodes4, int n_nodes, const ef_graph_constraint* constraints, int n_constraints, int fern_match,
                         int64_t last_deform_time, double* poses16_inout, const int64_t* pose_times, int n_poses, float* graph16_out,
                         float* error_out, float* mean_constraint_error_out, ef_graph_constraint* new_relative_out_or_null,
                         int* n_new_relative_out_or_null);
/* the same with the three gates of a global closure spelled out (NULL = the reference's constants {0.06, 3e-4, 0.12}: entry below which
 * there is nothing to close, acceptance bounds on the optimised mean constraint error and on the energy) */
int ef_solve_deformation_gated(const float* nodes4, int n_nodes, const ef_graph_constraint* constraints, int n_constraints, int fern_match,
                               int64_t last_deform_time, double* poses16_inout, const int64_t* pose_times, int n_poses, float* graph16_out,
                               float* error_out, float* mean_constraint_error_out, ef_graph_constraint* new_relative_out_or_null,
                               int* n_new_relative_out_or_null, const float* gates3_or_null);
/* icpCountThresh, icpErrThresh, covThresh of the constructor (ElasticFusion.h:44-46; defaults 35000, 5e-05, 1e-05) */
int ef_set_loop_thresholds(ef_ctx* ctx, int icp_count_thresh, float icp_err_thresh, float cov_thresh);
int ef_get_local_loop(ef_ctx* ctx, ef_local_loop* info, double* constraints_or_null, int max_constraints, int* n_out_or_null);
/* Deformation::sampleGraphModel (Deformation.cpp:232-306, sample.vert + sample.geom): the deformation graph's nodes, every 5000th
 * surfel of the current model in map order as {x, y, z, initTime} (times ascend because the map keeps creation order); what the
 * reference hands to DeformationGraph::initialiseGraph.  nodes4_host: max_nodes x 4 floats.  Synchronises. */
int ef_sample_graph(ef_ctx* ctx, float* nodes4_host, int max_nodes, int* n_out);
/* ---- fern database (Core/Ferns.h:35-184, Core/Ferns.cpp:22-393): the keyframe store of the GLOBAL loop closure and of
 * relocalisation.  Host-side object with no GPU state of its own: it encodes the 1/8-resolution predicted views
 * (ef_get_image_resized(EF_IMG_FILL_*, 8, ...)) with `num` random ferns (4 binary tests each: r, g, b
 * against 0..255, depth in mm against 400..max_depth_mm), keeps a frame when it differs enough from all stored ones, and proposes
 * the most similar stored frame for a new view.  The fern-to-view registration (an 80x60 ICP, Ferns.cpp:243-258) is the caller's:
 * ef_fern_tracker gets both vertex / normal images and the stored pose, refines T_inout16 and reports the ICP statistics.
 * Images: rgb = rows of `rgb_channels` (3 or 4) bytes per pixel, verts4 / norms4 = f32x4 per pixel, (W/8) x (H/8) pixels. */
typedef struct ef_ferns ef_ferns;
/* Ferns::Ferns(n, maxDepth, photoThresh) with Resolution / Intrinsics spelled out; the table is drawn from std::mt19937(seed) in the
 * reference's order (Ferns.cpp:62-77; the reference seeds with time(0)). */
ef_ferns* ef_ferns_create(int num, int max_depth_mm, float photo_thresh, int width, int height, float fx, float fy, float cx, float cy,
                          unsigned seed);
void ef_ferns_destroy(ef_ferns* f);
/* the fern table, num rows of {x, y, r, g, b, d}; setting it is only allowed while no frame is stored */
int ef_ferns_get_table(const ef_ferns* f, int* table6);
int ef_ferns_set_table(ef_ferns* f, const int* table6);
/* Ferns::addFrame (Ferns.cpp:78-160): returns 1 when the frame was stored, 0 when it was too similar (or had no valid code),
 * a negative EF_E* on bad arguments */
int ef_ferns_add_frame(ef_ferns* f, const uint8_t* rgb, int rgb_channels, const float* verts4, const float* norms4, const double* T_wc16,
                       int src_time, float threshold);
typedef void (*ef_fern_tracker)(void* user, const float* fern_verts4, const float* fern_norms4, const double* T_wc_fern16,
                                const float* cur_verts4, const float* cur_norms4, double* T_inout16, float* icp_error, float* icp_count);
/* Ferns::findFrame (Ferns.cpp:162-298).  T_est16_out: the recovered pose (identity when no candidate passed the code gates);
 * constraints6_out: up to max_constraints rows {T_wc * p (source), T_est * p (target)} (Ferns.cpp:268-293).  Returns lastClosest
 * (the matched frame's id) or -1. */
int ef_ferns_find_frame(ef_ferns* f, const uint8_t* rgb, int rgb_channels, const float* verts4, const float* norms4, const double* T_wc16,
                        int time, int lost, ef_fern_tracker tracker, void* user, double* T_est16_out, double* constraints6_out,
                        int max_constraints, int* n_constraints_out);
/* The same two with the view's fern codes computed by the CALLER — on the device: ef_process_frame runs one 512-thread kernel over
 * the full-resolution fill-in maps (texel (8 x + 4, 8 y + 4) under each fern = what Resize::image / Resize::vertex would hand to
 * Ferns.cpp:97-118) and reads back `num` code bytes (255 = no valid depth) + their count instead of three 1/8-resolution images.  The
 * view itself is asked for through `fetch` only when it is needed: a keyframe passed the code gates (findFrame) or the frame is kept
 * (addFrame).  fetch returns EF_OK and the three images (rgb with 3 or 4 channels); at most one call per call. */
typedef int (*ef_view_fetch)(void* user, const uint8_t** rgb_out, int* rgb_channels_out, const float** verts4_out, const float** norms4_out);
int ef_ferns_add_frame_coded(ef_ferns* f, const uint8_t* codes, int good_codes, ef_view_fetch fetch, void* fetch_user, const double* T_wc16, int src_time,
                             float threshold);
int ef_ferns_find_frame_coded(ef_ferns* f, const uint8_t* codes, int good_codes, ef_view_fetch fetch, void* fetch_user, const double* T_wc16, int time,
                              int lost, ef_fern_tracker tracker, void* user, double* T_est16_out, double* constraints6_out, int max_constraints,
                              int* n_constraints_out);
/* 1 when some stored frame is more than 300 ticks older than `time` (Ferns.cpp:218), i.e. findFrame CAN match; 0: it returns -1 whatever the view */
int ef_ferns_candidate_possible(ef_ferns* f, int time);   /* answering 0 it also resets lastClosest to -1, as the findFrame it stands for would */
int ef_ferns_table_version(const ef_ferns* f);            /* bumped by every ef_ferns_set_table */
int ef_ferns_count(const ef_ferns* f);          /* frames.size() */
int ef_ferns_last_closest(const ef_ferns* f);   /* lastClosest */
/* one stored frame: any output may be NULL.  codes_out: num bytes (255 = no valid depth under that fern). */
int ef_ferns_get_frame(const ef_ferns* f, int id, uint8_t* codes_out, int* good_codes_out, int* src_time_out, double* T_wc16_out,
                       uint8_t* rgb3_out, float* verts4_out, float* norms4_out);
/* Deformation::constrain's applyGraphToPoses (Deformation.cpp:196-203) hands the deformed poses back to the stored frames */
int ef_ferns_set_frame_pose(ef_ferns* f, int id, const double* T_wc16);
/* the two private measures, for tests: Ferns::blockHDAware of two stored frames; Ferns::photometricCheck of a view against frame id */
float ef_ferns_block_hd_aware(const ef_ferns* f, int id_a, int id_b);
float ef_ferns_photometric_check(const ef_ferns* f, const uint8_t* rgb, int rgb_channels, const float* verts4, const double* T_est16, int id);
/* ---- the host side of the loop closures around that database (ElasticFusion.cpp:392-445, 511-526, 588-589, 609-618): one object holds
 * the fern database, the relative constraints local closures leave behind, the trajectory (t_T_wc) and the two deformation counters, and
 * takes the decisions — which constraints go to which graph, what an accepted closure changes (keyframe and trajectory poses deformed
 * along).  No device work: the caller brings the 1/8-resolution fill-in views, the pose, the sampled graph (ef_sample_graph; the global
 * graph is every 5th node of it, Deformation::sampleGraphFrom) and the fern-to-view registration (ef_fern_tracker).  ef_process_frame
 * drives one of these itself once ef_enable_global_closure was called (below). */
typedef struct ef_closure ef_closure;
ef_closure* ef_closure_create(int num_ferns, float depth_cut, float photo_thresh, float fern_thresh, int width, int height, float fx, float fy, float cx,
                              float cy, unsigned seed);   /* Ferns(500, depthCut * 1000, photoThresh); fernThresh 0.3095 */
void ef_closure_destroy(ef_closure* c);
ef_ferns* ef_closure_ferns(ef_closure* c);                /* owned by the closure object */
/* mid-frame, after predict() (:392-445): fern match -> fern constraints with their pins + the kept relative constraints -> global
 * deformation.  1: accepted — T_recovery16_out is the new pose, graph16_out / nodes_out go to the clean pass with is_fern = 1 and the
 * local closure is skipped; 0: no match or rejected (T_recovery16_out still holds the registration, identity without a candidate). */
int ef_closure_global(ef_closure* c, const uint8_t* rgb, int rgb_channels, const float* verts4, const float* norms4, const double* T_wc16, int tick,
                      ef_fern_tracker tracker, void* user, const float* nodes4, int n_nodes, double* T_recovery16_out, float* graph16_out, int* nodes_out);
/* the local closure's far half (:511-526), gates already open: constraints8 as ef_get_local_loop returns them.  1: accepted (graph16_out
 * over all n_nodes; the keyframe poses followed; a third of the new relative constraints kept), 0: rejected */
int ef_closure_local(ef_closure* c, const double* constraints8, int n, int tick, const float* nodes4, int n_nodes, float* graph16_out, int* nodes_out);
/* end of the frame (:588-589, 609-618): pose -> trajectory, final fill-in view -> Ferns::addFrame; returns 1 when it became a keyframe */
int ef_closure_end_frame(ef_closure* c, const uint8_t* rgb, int rgb_channels, const float* verts4, const float* norms4, const double* T_wc16, int tick);
int ef_closure_counts(const ef_closure* c, int* deforms, int* fern_deforms, int* relative_constraints, int* trajectory_poses);
/* the gates of the GLOBAL deformation (defaults = the reference's hard-coded 0.06 m entry, 3e-4 m / 0.12 acceptance: DeformationGraph.cpp:425,
 * Deformation.cpp:154; tuned on room-scale trajectories) */
int ef_closure_set_gates(ef_closure* c, float entry_mean_error, float accept_mean_error, float accept_energy);
int ef_closure_set_fern_thresh(ef_closure* c, float fern_thresh);   /* ElasticFusion::setFernThresh: Ferns::addFrame's threshold from now on */
/* introspection for tests: the rows the last closure handed to the optimiser (returns their number) and its two error figures */
int ef_closure_last_rows(const ef_closure* c, ef_graph_constraint* rows_or_null, int max_rows, float* error_or_null, float* mean_constraint_error_or_null);
int ef_closure_relative(const ef_closure* c, ef_graph_constraint* rows_or_null, int max_rows);
int ef_closure_trajectory(const ef_closure* c, double* poses16_or_null, int max_poses);
/* a LOST camera's frame (ElasticFusion.cpp:395-413 with lost = true): Ferns::findFrame only — 1 and the registered pose when a keyframe
 * passes the gates (ICP count > 1400), 0 otherwise; and its end (:588-589 without :601-604): the pose joins the trajectory, no keyframe */
int ef_closure_relocalise(ef_closure* c, const uint8_t* rgb, int channels, const float* verts4, const float* norms4, const double* T_wc16, int tick,
                          ef_fern_tracker tracker, void* user, double* T_recovery16_out);
int ef_closure_log_pose(ef_closure* c, const double* T_wc16, int tick);
/* ef_closure_global / ef_closure_end_frame / ef_closure_relocalise on device-computed fern codes (ef_ferns_*_coded above) */
int ef_closure_global_coded(ef_closure* c, const uint8_t* codes, int good_codes, ef_view_fetch fetch, void* fetch_user, const double* T_wc16, int tick,
                            ef_fern_tracker tracker, void* user, const float* nodes4, int n_nodes, double* T_recovery16_out, float* graph16_out,
                            int* nodes_out);
int ef_closure_candidate_possible(ef_closure* c, int tick);   /* 0: this frame's findFrame cannot match (no keyframe older than 300 ticks); the object is left as after such a call */
int ef_closure_end_frame_coded(ef_closure* c, const uint8_t* codes, int good_codes, ef_view_fetch fetch, void* fetch_user, const double* T_wc16, int tick);
int ef_closure_relocalise_coded(ef_closure* c, const uint8_t* codes, int good_codes, ef_view_fetch fetch, void* fetch_user, const double* T_wc16, int tick,
                                ef_fern_tracker tracker, void* user, double* T_recovery16_out);
/* ---- the GLOBAL loop closure inside ef_process_frame (ElasticFusion.cpp:392-445, 588-589, 609-618; contexts created with
 * close_loops = 1).  Creates the context's closure object (ef_closure_* above: Ferns(num_ferns, depth_cut * 1000, photo_thresh), the
 * relative constraints, the trajectory) and a third tracker instance at 1/8 resolution.  From then on every frame (tick > 1):
 *   after tracking    predict() (ACTIVE + fill-in) at the new pose; the fill-in view, NEAREST-resized by 8, goes to Ferns::findFrame;
 *                     a candidate keyframe is registered against the view by the 1/8-resolution tracker on the device (ICP only,
 *                     10 iterations at one level); its surface constraints with their pins + the kept relative constraints go to the
 *                     global deformation (every 5th graph node); accepted => T_wc := the recovered pose, keyframe and trajectory poses
 *                     deformed along, the graph applied by this frame's clean pass as a fern match, the local closure skipped;
 *                     otherwise the local closure runs — through the closure object when the built-in solver is on
 *                     (ef_use_builtin_loop_solver), so keyframe poses follow and a third of the new relative constraints is kept;
 *   end of the frame  the final fill-in view goes to Ferns::addFrame, the pose joins the trajectory.
 * Two stream synchronisations per frame, where the reference reads the views back (Resize.cpp:50-159).  The reference seeds its fern
 * table from time(0); here the seed is an argument (equal seeds => equal runs). */
int ef_enable_global_closure(ef_ctx* ctx, int num_ferns, float photo_thresh, float fern_thresh, unsigned seed);
/* ---- relocalisation (the reference constructor's `reloc`; ElasticFusion.cpp:326-366, 402-413, 536, 601-604, 624-649).  With it on,
 * every TRACKED frame (no injected pose) is judged by its own statistics, read back right after the tracker (one more synchronisation
 * per frame): trackingOk = lastICPError < 1e-4 and no diagonal entry of getCovariance() above 1e-4.  A frame that is not ok is not
 * fused; more than ten of them in a row and the camera is LOST: the fill-in passes the raw frame through, the tick stands still, no
 * keyframe is stored, neither closure runs — but Ferns::findFrame keeps looking (ICP count gate 1400 instead of 2400) and a match
 * becomes the pose (ef_global_loop.closest >= 0 with accepted = 0).  The frame after such a recovery is predicted from the whole model
 * (time = 0) and, if its tracking is ok, the camera is found again.  Recovery needs the global closure (ef_enable_global_closure);
 * without it a lost camera stays lost, as in the reference with closeLoops = false. */
int ef_set_relocalisation(ef_ctx* ctx, int on);
typedef struct ef_reloc_state {
  int lost;                 /* ElasticFusion::getLost() */
  int tracking_ok;          /* of the last frame (1 for frames with an injected pose) */
  int tracking_count;       /* consecutive frames not ok, towards "lost" at > 10 */
  int last_frame_recovery;  /* the last frame's pose came from a fern match while lost */
} ef_reloc_state;
int ef_get_relocalisation(ef_ctx* ctx, ef_reloc_state* out);
typedef struct ef_global_loop {
  int attempted;            /* Ferns::findFrame ran in the last ef_process_frame */
  int closest;              /* matched keyframe (Ferns::lastClosest), -1: none passed the gates */
  int n_constraints;        /* surface constraints of the match */
  int accepted;             /* the global deformation was accepted: pose replaced, graph applied as a fern match */
  int graph_nodes;
  float icp_error, icp_count;   /* of the 1/8-resolution registration, when it ran */
  double T_wc_recovery[16];     /* the registered pose (identity without a candidate) */
} ef_global_loop;
int ef_get_global_loop(ef_ctx* ctx, ef_global_loop* info);
ef_closure* ef_get_closure(ef_ctx* ctx);   /* the context's closure object (NULL before ef_enable_global_closure); owned by the context */
int ef_predict(ef_ctx* ctx);                                  /* ElasticFusion::predict() */
int ef_get_pose(ef_ctx* ctx, double* T_wc16);                 /* get_T_wc(); synchronises */
int ef_get_tick(ef_ctx* ctx, int* tick);                      /* getTick() */
int ef_set_tick(ef_ctx* ctx, int tick);                       /* setTick() */
/* lastICPError, lastICPCount, lastRGBError, lastRGBCount, lastSO3Error, lastSO3Count (RGBDOdometry.h:74-79) */
int ef_get_tracking_stats(ef_ctx* ctx, float* out6, double* lastA36_or_null, double* lastb6_or_null);
/* RGBDOdometry::getCovariance (RGBDOdometry.cpp:573-575): lastA.lu().inverse(), 36 doubles row-major; synchronises */
int ef_get_covariance(ef_ctx* ctx, double* cov36);
int ef_get_trajectory(ef_ctx* ctx, double* T_wc16_array, int64_t* timestamps, int max_frames, int* n_frames);
int ef_map_count(ef_ctx* ctx, uint32_t* count);               /* GlobalModel::lastCount(); synchronises */
int ef_map_download(ef_ctx* ctx, float* surfels, uint32_t max_surfels, uint32_t* count); /* downloadMap(), 12 floats each */
int ef_map_upload(ef_ctx* ctx, const float* surfels, uint32_t count);  /* test/bench seeding */
/* Checkpoint / resume of a replay.  What ElasticFusion carries from one processFrame to the next is the map, the tick,
 * T_wc and the previous frame (its intensity pyramid is the SO(3) reference of RGBDOdometry.cpp:284-288, its filtered depth and colour
 * feed FillIn, ElasticFusion.cpp:621-653); everything else is re-derived.  ef_get_pose_qt returns T_wc exactly as the engine holds it
 * (unit quaternion x y z w + translation, doubles: no round trip through a matrix).  ef_restore_state, called on a context whose map
 * was brought in with ef_map_upload, sets tick and pose, takes the frame that was processed LAST before the checkpoint (host pointers,
 * W*H*3 bytes and W*H uint16), rebuilds its pre-processing and SO(3) reference and runs predict(): the next ef_process_frame then tracks
 * and fuses exactly as the checkpointed context's next frame does (tests/test_gpu_one_frame.py).  The velocity weighting needs no extra
 * state: it compares the pose before and after the tracker of the same frame. */
int ef_get_pose_qt(ef_ctx* ctx, double* q4_t3);
int ef_restore_state(ef_ctx* ctx, int tick, const double* q4_t3, const uint8_t* rgb_prev, const uint16_t* depth_prev);
/* Which buffer ef_map_download / ef_save_ply read.  0 (default): model(), the map as it stands after the frame's clean pass.
 * 1: what GlobalModel::downloadMap really reads (GlobalModel.cpp:673-706, quirk Q14): vbos[renderSource], i.e. the buffer the frame's
 * UPDATE pass wrote (the map before clean) truncated to the count AFTER clean — entries beyond the pre-clean count are whatever older
 * update passes left there (zeros at first).  Byte-for-byte the reference's downloadMap / savePly output for a run; costs one map copy
 * per frame.  Switch it on before the first frame (class ElasticFusion of libefusion.so does). */
int ef_set_reference_download(ef_ctx* ctx, int on);
int ef_save_freiburg(ef_ctx* ctx, const char* path);          /* trajectory dump of ~ElasticFusion, :112-139 */
int ef_save_ply(ef_ctx* ctx, const char* path);               /* ElasticFusion::savePly, :684-781 */
/* the same two writers on HOST arrays (no context, no GPU): byte for byte the reference's files — the trajectory with six
 * significant digits per number as its ostream prints them, the PLY with the normals negated as savePly does (:741-743) */
int ef_write_freiburg(const char* path, const double* T_wc16_array, const int64_t* timestamps, int n);
int ef_write_ply(const char* path, const float* surfels12, uint32_t count, float confidence_threshold);
/* setters (Core/ElasticFusion.h:135-183) */
int ef_set_rgb_only(ef_ctx*, int v);
int ef_set_icp_weight(ef_ctx*, float v);
int ef_set_pyramid(ef_ctx*, int v);
int ef_set_fast_odom(ef_ctx*, int v);
int ef_set_so3(ef_ctx*, int v);
int ef_set_frame_to_frame_rgb(ef_ctx*, int v);
int ef_set_confidence_threshold(ef_ctx*, float v);
int ef_set_depth_cutoff(ef_ctx*, float v);

/* ---- GlobalModel::renderPointCloud (GlobalModel.cpp:286-350) without OpenGL: the current map, the buffer ef_map_download reads with the
 * reference download off, drawn on the device from any pinhole camera and pose into plain row-major images.  A surfel is drawn when
 * conf > threshold || draw_unstable (draw_global_surface.vert:44) and 0 <= z_cam <= max_depth; there is no time-window cull.  Its footprint
 * and its ray / disc intersection are the model prediction's (ef_op_combined_predict), with this camera.  Nearest wins, ties go to the lower
 * surfel row; an unstable surfel drawn under draw_unstable competes at z + radius (its outputs still carry the real z).  RGBA is shaded per
 * surfel as draw_global_surface.geom:49-79 does: with s = |n.x + n.y + n.z| of the stored normal n, color_type 0 (lit) 0.5 s + 0.1,
 * 1 (normals) n, 2 (colours) the surfel's colour, 3 (times) the init-time ramp times s + 0.1; with draw_window a surfel whose last time
 * lies more than time_delta before `time` is dimmed to a quarter; each channel roundf(clamp(c, 0, 1) * 255), alpha 255.
 * Outputs (any may be NULL: not written), width x height each:
 *   rgba u8 x 4 (0 where nothing is drawn)         depth  f32 (camera z; 0)
 *   vertex f32 x 4 camera frame, w = confidence     normal f32 x 4 camera frame, w = radius
 *   index u32: the surfel's row in ef_map_download (0xFFFFFFFF where nothing is drawn)
 * Work is enqueued on the context's stream behind the frames before it; it changes nothing a frame reads. */
typedef struct ef_render_params {
  int width, height;          /* 1 .. 4096 each */
  float fx, fy, cx, cy;
  double T_wc[16];            /* world <- camera, row-major, as ef_get_pose returns it */
  float max_depth;            /* far cull in metres (the GUI's far plane, 1000, by default) */
  float threshold;            /* getConfidenceThreshold() by default */
  int draw_unstable;          /* drawUnstable */
  int color_type;             /* 0 lit, 1 normals, 2 colours, 3 times: drawNormals ? 1 : drawColors ? 2 : drawTimes ? 3 : 0 */
  int draw_window;            /* drawWindow */
  int time;                   /* getTick() by default */
  int time_delta;             /* getTimeDelta() by default */
} ef_render_params;
/* the frame camera, the current pose (synchronises), the context's confidence threshold, tick and time delta, max_depth 1000, colour
 * type 0, both switches off */
int ef_default_render_params(ef_ctx* ctx, ef_render_params* params);
/* HOST output pointers; synchronises.  EF_EINVAL for a NULL params, a size outside 1 .. 4096, a colour type outside 0 .. 3,
 * non-finite intrinsics or a NULL context, before anything is read or enqueued (the parameters are checked first; with a NULL context
 * ef_last_error(NULL) has the message). */
int ef_render_model(ef_ctx* ctx, const ef_render_params* params, uint8_t* rgba, float* depth, float* vertex, float* normal,
                    uint32_t* index);
/* the same with DEVICE output pointers: enqueued on the context's stream, no synchronisation (as ef_process_frame_dev) */
int ef_render_model_dev(ef_ctx* ctx, const ef_render_params* params, uint8_t* rgba_dev, float* depth_dev, float* vertex_dev,
                        float* normal_dev, uint32_t* index_dev);

/* ---- Stable surfel IDs and per-surfel label fusion (SemanticFusion-style class probabilities, or any per-surfel distribution).  Off by
 * default; with both switches off nothing of this runs and every output is what it is without it.  Frames never read IDs or labels.
 *
 * IDs: with IDs on, every surfel of model() carries a uint32 ID >= 1, stored as the RAW BIT PATTERN of the colour stream's unused lane: float 5
 * (from 0) of the 12 per surfel that ef_map_download returns (read it as uint32, never as a float value; small IDs are denormal patterns).
 * IDs are unique for the context's lifetime, never reused, and strictly increasing with map row (the map keeps creation order).  They are
 * handed out lazily: every ID-consuming call (ef_get_surfel_ids, the label calls, ef_map_download while IDs are on) first numbers the rows
 * created since the last one.  Switching on numbers the current map (1 .. N the first time); switching off zeroes the lane, so a download equals
 * that of a context that never had IDs, and switches labels off.  ef_map_upload while IDs are on keeps the uploaded lane when it is a strictly
 * increasing non-zero prefix followed by a zero suffix (a map downloaded with IDs; an all-zero lane, numbered by the next call); the counter
 * continues above its largest ID.  The zero suffix of an upload, z rows, is numbered from b = max(one past the largest ID of the prefix, one
 * past every ID the context has handed out); the upload is valid only if b + z <= 0xFFFFFFFF, so that the numbering ends at 0xFFFFFFFE at
 * the latest and cannot wrap (an uploaded ID of 0xFFFFFFFF is therefore never valid).  Any other lane, a lane of one row included, makes
 * every later ID-consuming call fail with EF_ESTATE until the next valid upload or switch-on.  A counter that the creation of surfels drives
 * past 2^32 - 1 (four billion surfels created in one context, or fewer on top of uploaded IDs that close to the end) is outside the contract
 * and is not detected.  With ef_set_reference_download on, the downloaded buffer is the pre-clean copy (quirk Q14) and its lane is whatever that buffer
 * holds: IDs as of the last frame's update pass, zero for surfels created after it.
 *
 * Labels: a float32 table [rows][C] in map row order on the device.  Every label call first re-aligns it to the current rows: a row whose ID was
 * present at the previous label call keeps its C floats bit for bit, a new row gets the prior 1 / C.  ef_map_upload while labels are on resets
 * every row to the prior.
 *
 * Fusion (ef_fuse_labels): probs_chw is C x height x width float32 for the view (a network's NCHW output without N; a network at a lower
 * resolution passes scaled intrinsics).  I is the view's index image exactly as ef_render_model returns it for the same parameters.  Surfel
 * row s is OBSERVED when, with p = T_cw p_world (the float T_cw the render uses) and z > 0, u = floor(fx x / z + cx), v = floor(fy y / z + cy)
 * (f32, no contraction) lie in the image and I[v width + u] == s.  For an observed row, with o the C values at (u, v): q_c = p_c o_c,
 * Z = sum of q_c in ascending c, p_c <- q_c / Z when Z is finite and > 0 (otherwise the row stays).  Inputs are used as given, not
 * renormalised.  One observation per surfel per call: no atomics, deterministic.
 *
 * All label calls are refused with EF_ESTATE while the context's stream is being captured and while labels are off; bad parameters are refused
 * with EF_EINVAL before anything is enqueued (with a NULL context, ef_last_error(NULL) has the message).  The _dev variants enqueue on the
 * context's stream; they wait for the device only when the table has to grow (the count bound outgrows it) or for a NULL view (the pose). */
int ef_set_surfel_ids(ef_ctx* ctx, int on);
/* the ID of every row of model(), at most max_ids of them; *count = rows written.  EF_ESTATE when IDs are off.  Synchronises. */
int ef_get_surfel_ids(ef_ctx* ctx, uint32_t* ids, uint32_t max_ids, uint32_t* count);
/* num_classes 1 .. 256 (implies IDs on; every row starts at 1 / C); 0 switches labels off and frees the table.  EF_EINVAL outside 0 .. 256. */
int ef_enable_labels(ef_ctx* ctx, int num_classes);
/* the whole table from HOST memory: count rows (must equal the current map count, else EF_EINVAL) of C floats, in ef_get_surfel_ids order.
 * Restores a checkpoint.  Synchronises. */
int ef_set_labels(ef_ctx* ctx, const float* probs, uint32_t count);
/* aligns, then copies up to max_rows rows: their IDs and C floats each (either pointer may be NULL); *count = rows.  Synchronises. */
int ef_get_labels(ef_ctx* ctx, uint32_t* ids_or_null, float* probs_or_null, uint32_t max_rows, uint32_t* count);
/* one observation.  view NULL = ef_default_render_params with draw_unstable = 1; color_type, draw_window, time and time_delta are ignored.
 * HOST probs_chw: staged and synchronised.  EF_EINVAL for a NULL image or view parameters ef_render_model refuses. */
int ef_fuse_labels(ef_ctx* ctx, const ef_render_params* view_or_null, const float* probs_chw);
/* the same with a DEVICE image, enqueued on the context's stream */
int ef_fuse_labels_dev(ef_ctx* ctx, const ef_render_params* view_or_null, const float* probs_chw_dev);
/* per pixel of the view's index image: label = argmax of the surfel's row (ties to the lowest class), prob = that maximum; -1 and 0 where
 * nothing is drawn.  The argmax is the FIRST STRICT MAXIMUM starting from class 0: best = 0, m = p[0]; for c = 1 .. C-1 in ascending order, if
 * p[c] > m then best = c, m = p[c].  Comparisons with NaN are false, so a NaN at a later class is passed over, and a NaN at class 0 is never
 * replaced: such a row gives label 0 and prob NaN (an all-NaN row too).  width x height each, row-major, HOST pointers (either may be NULL);
 * synchronises. */
int ef_render_labels(ef_ctx* ctx, const ef_render_params* params, int32_t* label, float* prob);
/* the same with DEVICE pointers, enqueued on the context's stream */
int ef_render_labels_dev(ef_ctx* ctx, const ef_render_params* params, int32_t* label_dev, float* prob_dev);

/* ---- Spatial index and nearest-surfel / kNN queries: what is near this point?  Off until first used: no query call, nothing allocated,
 * nothing run, and no frame kernel knows of it.
 *
 * Semantics.  All arithmetic is f32, one rounding per operation, no contraction.  For a query point q and the surfel in map row s with
 * position p, stored normal n (not renormalised) and confidence c:
 *   d2(q, s)    = ((qx-px)*(qx-px) + (qy-py)*(qy-py)) + (qz-pz)*(qz-pz)
 *   plane(q, s) = ((qx-px)*nx + (qy-py)*ny) + (qz-pz)*nz
 *   s is ELIGIBLE iff c > min_conf and d2 <= r2, r2 = max_dist * max_dist computed once in f32 on the host.  Comparisons with NaN are
 *   false: a surfel with a non-finite position and a query with a non-finite coordinate never match.
 * Eligible surfels are ordered by (d2, row) ascending: ties go to the lower row.  "Row" is the map row at the time of the call: the row space
 * of ef_map_download (reference download off), ef_get_surfel_ids and the index image of ef_render_model.  The answer is, bit for bit, that of
 * an exhaustive scan over all rows, for any cell size: the grid only selects candidates.
 *
 * min_conf: a negative value for every surfel, the context's confidence threshold for stable surfels only; NaN is refused.
 * A miss is row 0xFFFFFFFF, id 0, dist2 +inf, plane 0.  n = 0 and an empty map are valid (all misses).
 * EF_EINVAL, before any GPU work: a NULL context or required pointer, n > 0 with NULL points3, k outside 1 .. 16, max_dist or cell_m not finite
 * and positive (or cell_m so small that 1 / cell_m is not finite), NaN min_conf, max_dist / cell above EF_QUERY_MAX_RATIO (a query visits
 * the cells its ball's bounding box overlaps, about (2 max_dist / cell + 1)^3).
 * EF_ESTATE: the context's stream is being captured; id asked for while surfel IDs are off.
 *
 * The index is built on demand, on the context's stream behind earlier frames, and reused until a call that can change the map
 * (ef_process_frame*, ef_map_upload, ef_restore_state) or another cell size makes it stale.  Host variants stage their arrays and synchronise.
 * The _dev variants take DEVICE pointers and only enqueue, except that a call which has to rebuild the index first waits for the device once
 * (the map count sizes the index). */
#define EF_QUERY_MAX_RATIO 16
#define EF_QUERY_DEFAULT_CELL 0.02f
/* the grid's cell edge in metres (> 0, finite; default EF_QUERY_DEFAULT_CELL, chosen by measurement: profiles/r12_query_kernel_times.txt) */
int ef_set_query_cell(ef_ctx* ctx, float cell_m);
/* per point (points3: n x 3 floats) the first eligible surfel: row[n]; id (needs ef_set_surfel_ids on; new rows are numbered first), dist2 and
 * plane may be NULL */
int ef_query_nearest(ef_ctx* ctx, const float* points3, uint32_t n, float max_dist, float min_conf, uint32_t* row, uint32_t* id_or_null,
                     float* dist2_or_null, float* plane_or_null);
/* per point the first min(k, eligible) surfels in (d2, row) order: rows[n * k], dist2[n * k] (unused slots filled as a miss); count[n] is the
 * number of ALL eligible surfels, which may exceed k (the radius count of density / outlier filters) */
int ef_query_knn(ef_ctx* ctx, const float* points3, uint32_t n, int k, float max_dist, float min_conf, uint32_t* rows, float* dist2_or_null,
                 uint32_t* count_or_null);
int ef_query_nearest_dev(ef_ctx* ctx, const float* points3_dev, uint32_t n, float max_dist, float min_conf, uint32_t* row_dev,
                         uint32_t* id_dev_or_null, float* dist2_dev_or_null, float* plane_dev_or_null);
int ef_query_knn_dev(ef_ctx* ctx, const float* points3_dev, uint32_t n, int k, float max_dist, float min_conf, uint32_t* rows_dev,
                     float* dist2_dev_or_null, uint32_t* count_dev_or_null);

/* ---- Rigid registration of a point set against the map: point-to-plane ICP on the spatial index above.  Off until first used: no register
 * call, nothing allocated, nothing run, and no frame kernel knows of it.
 *
 * T (row-major 4 x 4 double like every other pose here; NULL where allowed = identity) maps the cloud's frame into the map's world frame.
 *
 * ONE STEP (ef_register_step).  Rf, tf are T's rotation block and translation rounded to f32 once.  All per-point arithmetic is f32, one
 * rounding per operation, no contraction, in the written order.  For a point (x, y, z) with optional normal m:
 *   p'x = ((Rf00*x + Rf01*y) + Rf02*z) + tfx, likewise y, z;   m'x = (Rf00*mx + Rf01*my) + Rf02*mz, likewise y, z
 *   s   = the surfel ef_query_nearest returns for p' with max_dist, min_conf: the same eligibility, the same (d2, row) order, the same
 *         treatment of non-finite input.  A miss contributes nothing.
 *   normal gate, only with normals and min_normal_cos > -1: the pair is kept iff ((m'x*nx + m'y*ny) + m'z*nz) >= min_normal_cos, n the
 *         stored normal, not renormalised; a NaN fails the comparison and drops the pair.
 *   r   = plane(p', s) as the query defines it;   J = (nx, ny, nz, p'y*nz - p'z*ny, p'z*nx - p'x*nz, p'x*ny - p'y*nx) in f32
 *   the seven numbers are widened to double;  A += J^T J,  b -= J^T r,  e += r*r,  pairs += 1  in double.  Every product of two widened f32
 *   values is exact in double; the order of the sums is fixed by n alone (never by the index's cell size, never by timing: no
 *   floating-point atomics), so a step is reproducible bit for bit.  A is returned full and symmetric bit for bit.  points = n.
 *   row / plane (optional, n each) receive the pair that was used, or a miss as the query writes it (row 0xFFFFFFFF, plane 0); a pair the
 *   normal gate dropped is reported as a miss.
 *
 * UPDATE (ef_register_update; plain double on the host, needs neither a context nor a GPU; ef_register_cloud calls this very function).
 * Solves A xi = b by the library's 6 x 6 LDL^T with diagonal pivoting; xi = (translation, rotation) is a twist applied in the world frame.
 * T_out = exp(xi) * T (left multiplication), exp the SE(3) exponential: with th = |xi_w|, W = [xi_w]x,
 *   R = I + a W + b W^2,  V = I + b W + c W^2,  exp(xi) = [R, V xi_t; 0, 1],  a = sin th / th,  b = (1 - cos th) / th^2,  c = (1 - a) / th^2,
 *   and below th = EF_REGISTER_SMALL_ANGLE the series a = 1 - th^2/6, b = 1/2 - th^2/24, c = 1/6 - th^2/120 (their error there is under 1e-18).
 * The rotation block of the product is left as computed: it is not re-orthonormalised (its drift over EF_REGISTER_MAX_ITERATIONS updates is
 * of the order of 1e-14).  T_out's last row is 0 0 0 1.  Returns EF_OK, or EF_REG_DEGENERATE (T_out = T, xi = 0) when a pivot of the
 * factorisation is not finite and positive or xi is not finite, or EF_EINVAL for a NULL pointer or a non-finite entry of T.
 * A solution xi = 0 (b = 0 with a positive definite A) returns T itself, every entry bit for bit, without forming the product.
 *
 * THE LOOP (ef_register_cloud) is step, stop tests, update, in that order:
 *   pairs < min_pairs -> EF_REG_TOO_FEW_PAIRS with the pose reached so far;  a degenerate update -> EF_REG_DEGENERATE likewise;
 *   after an update whose |xi_t| < stop_translation and |xi_w| < stop_rotation -> one more step at the new pose for pairs / rms_last / A
 *   -> EF_REG_CONVERGED;  max_iterations updates -> the same closing step -> EF_REG_MAX_ITERATIONS.
 * status is information: the return value stays EF_OK.  rms = sqrt(e / pairs), 0 without pairs.  row / plane are those of the last step, which
 * is always taken at the returned pose.  Each iteration reads 29 doubles back (profiles/r13_register_kernel_times.txt).
 *
 * Defaults (ef_default_register_params): max_dist 0.05 m, min_conf = the context's confidence threshold (stable surfels; negative = every
 * surfel), min_normal_cos 0.5, max_iterations 30, min_pairs 32, stop_translation 1e-6 m, stop_rotation 1e-6 rad.  The stop bounds sit an order
 * of magnitude above the floor the f32 transform of the points sets on a room-sized cloud (updates of the order of 1e-7 m / 1e-7 rad once
 * converged, profiles/r13_register_accuracy.txt): lower bounds would never report EF_REG_CONVERGED.
 *
 * EF_EINVAL, before any GPU work: a NULL context, params, T_out / result / out, n > 0 with NULL points3; max_dist, min_conf and the ratio to
 * the cell as ef_query_nearest refuses them; NaN min_normal_cos; max_iterations outside 1 .. EF_REGISTER_MAX_ITERATIONS; min_pairs < 6; a
 * stop bound that is negative or not finite; a non-finite entry of T.  EF_ESTATE while the context's stream is captured.  n = 0 and an empty
 * map are valid (EF_REG_TOO_FEW_PAIRS, T_out = T_init).  The index is the query's own: built on demand, reused, made stale by the same
 * calls.  Host variants stage their arrays and synchronise; the _dev variants take DEVICE pointers for points / normals / row / plane
 * (out, T_out and result stay HOST pointers) and synchronise too, because the sums are read back. */
#define EF_REGISTER_MAX_ITERATIONS 100
#define EF_REGISTER_SMALL_ANGLE 1e-4
#define EF_REG_CONVERGED 0
#define EF_REG_MAX_ITERATIONS 1
#define EF_REG_TOO_FEW_PAIRS 2
#define EF_REG_DEGENERATE 3
typedef struct ef_register_params {
  float max_dist;          /* correspondence radius in metres */
  float min_conf;          /* as ef_query_nearest */
  float min_normal_cos;    /* used only when normals are given; <= -1 switches the gate off */
  int max_iterations;      /* 1 .. EF_REGISTER_MAX_ITERATIONS */
  int min_pairs;           /* >= 6 */
  double stop_translation; /* metres */
  double stop_rotation;    /* radians */
} ef_register_params;
typedef struct ef_register_sums {
  double A[36];            /* row-major, symmetric */
  double b[6];
  double e;
  uint32_t pairs;
  uint32_t points;
} ef_register_sums;
typedef struct ef_register_result {
  int status;              /* EF_REG_* */
  int iterations;          /* updates applied */
  uint32_t pairs;          /* at the returned pose */
  double rms_first;        /* sqrt(e / pairs) at T_init */
  double rms_last;         /* ... and at the returned pose */
  double A[36];            /* the normal matrix at the returned pose: how well each direction of motion is held */
} ef_register_result;
int ef_default_register_params(ef_ctx* ctx, ef_register_params* params);
int ef_register_step(ef_ctx* ctx, const float* points3, const float* normals3_or_null, uint32_t n, const ef_register_params* params,
                     const double* T16_or_null, ef_register_sums* out, uint32_t* row_or_null, float* plane_or_null);
int ef_register_update(const ef_register_sums* sums, const double* T16_or_null, double* T16_out, double* xi6_or_null);
int ef_register_cloud(ef_ctx* ctx, const float* points3, const float* normals3_or_null, uint32_t n, const ef_register_params* params,
                      const double* T_init16_or_null, double* T_out16, ef_register_result* result, uint32_t* row_or_null,
                      float* plane_or_null);
int ef_register_step_dev(ef_ctx* ctx, const float* points3_dev, const float* normals3_dev_or_null, uint32_t n,
                         const ef_register_params* params, const double* T16_or_null, ef_register_sums* out, uint32_t* row_dev_or_null,
                         float* plane_dev_or_null);
int ef_register_cloud_dev(ef_ctx* ctx, const float* points3_dev, const float* normals3_dev_or_null, uint32_t n,
                          const ef_register_params* params, const double* T_init16_or_null, double* T_out16, ef_register_result* result,
                          uint32_t* row_dev_or_null, float* plane_dev_or_null);

/* ---- Select, extract and erase surfels: act on a subset of the map without moving it through the host.  Off until first used: no select /
 * gather / erase call, nothing allocated, nothing run, and no frame kernel knows of it.
 *
 * "Row" is the map row at the time of the call: the row space of ef_map_download (reference download off), ef_get_surfel_ids, the index image
 * of ef_render_model and the queries.  A surfel (row of 12 floats as ef_map_download returns it) has the position (x, y, z) = floats 0 .. 2,
 * the confidence = float 3, the ID bits = float 5, the creation time = float 6, the time last seen = float 7, the radius = float 11.
 *
 * THE SELECTION.  All per-row arithmetic is f32, one rounding per operation, no contraction, in the written order.  Comparisons with NaN are
 * false.  `tests` says which of the tests below are ENABLED; the fields of a test that is not enabled are neither read nor checked.
 *   EF_SEL_BOX        Rf, tf are T_bw's rotation block and translation rounded to f32 once (T_bw maps world coordinates into the box's
 *                     frame; row-major 4 x 4 double like every other pose here):
 *                       bx = ((Rf00*x + Rf01*y) + Rf02*z) + tfx,  by = ((Rf10*x + Rf11*y) + Rf12*z) + tfy,  bz = ((Rf20*x + Rf21*y) + Rf22*z) + tfz
 *                     (the expression ef_register_step documents).  Passes iff box_min[a] <= b[a] && b[a] <= box_max[a] for a = 0, 1, 2.
 *                     Infinite bounds are allowed (a half-space, a slab).
 *   EF_SEL_CONF       conf_min <= c && c <= conf_max on the stored confidence.
 *   EF_SEL_RADIUS     radius_min <= r && r <= radius_max on the stored radius.
 *   EF_SEL_INIT_TIME  (float)init_time_min <= t && t <= (float)init_time_max on the stored creation time (a float that holds a tick).
 *   EF_SEL_LAST_TIME  (float)last_time_min <= t && t <= (float)last_time_max on the stored time last seen.
 *   EF_SEL_ID         id_min <= id && id <= id_max on the ID lane's uint32 bits.  Needs ef_set_surfel_ids on; rows created since the last
 *                     ID-consuming call are numbered first, as in every other ID-consuming call.
 *   EF_SEL_LABEL      needs ef_enable_labels on; the table is aligned to the current rows first, as in every label call.  With p the row's C
 *                     floats: best = 0, m = p[0]; for c = 1 .. C-1 in ascending order: if p[c] > m then best = c, m = p[c] (the argmax of
 *                     ef_render_labels: ties to the lowest class).  Passes iff best == label_class && m >= label_min_prob.
 * A row is SELECTED iff (every enabled test passes) XOR (EF_SEL_INVERT is set).  tests = 0 selects every row, tests = EF_SEL_INVERT none.
 * Under EF_SEL_INVERT a row that fails a test only because a comparison met a NaN IS selected: a surfel with a NaN position fails EF_SEL_BOX
 * and is therefore selected by EF_SEL_BOX | EF_SEL_INVERT.
 *
 * ef_map_select writes the first min(max_rows, total) selected rows in ASCENDING order and *count = total, the number of ALL selected rows, which
 * may exceed max_rows; rows may be NULL with max_rows 0 (a count only).  Entries of rows[] past min(max_rows, total) are left as they were.
 *
 * ef_map_gather writes n x 12 floats in ef_map_download's layout in the order of rows[]; duplicates are allowed, a row >= the map count yields
 * twelve zero words.  While IDs are on, float 5 carries the ID bits (rows created since the last ID-consuming call are numbered first).  surfels12_dev
 * is written in 16-byte words: it must be 16-byte aligned, as every ef_dev_alloc pointer is.
 *
 * ef_map_erase removes the selected rows; ef_map_erase_rows[_dev] removes the named rows: any order, duplicates and rows >= the map count are
 * ignored.  *removed (may be NULL) = the number of distinct rows actually removed.  What an erase leaves behind:
 *   the map       the kept rows in their old order (the compaction is stable), every word of them bit for bit, ID lane included;
 *   the context   the state that ef_map_upload(the kept rows) followed by ef_restore_state(tick, ef_get_pose_qt, the last processed frame) would
 *                 leave: tick, pose, trajectory, last frame and tracking statistics are unchanged, and if ef_process_frame* or ef_restore_state
 *                 has run on the context the model prediction (what the next frame is tracked against) is renewed from the edited map at the
 *                 current pose.  On a context whose map was only uploaded, only the map changes;
 *   the index     of the queries and the registration is stale and rebuilt by their next call;
 *   IDs           are never reused: the counter stays above the largest ID ever handed out, not above the largest survivor (with IDs on, an
 *                 erase numbers the new rows first like every ID-consuming call);
 *   labels        the next label call re-aligns by ID as it does after a frame's clean: kept rows keep their C floats bit for bit;
 *   the shadow buffer of ef_set_reference_download is left as it is: until the next frame a reference download still shows the unedited rows.
 * Erasing nothing (an empty selection, n = 0) is valid and still leaves the state described.  All three erase calls synchronise before and after.
 *
 * Host variants stage their arrays and synchronise.  The _dev variants of select and gather take DEVICE pointers and only enqueue on the context's
 * stream, except for what ID numbering or label alignment need and except that the first call after a call that can change the map
 * (ef_process_frame*, ef_map_upload, ef_restore_state, an erase) waits for the device once: the map count sizes the launches, as for the queries.
 *
 * EF_EINVAL, before any GPU work (the selection is checked before the context, so with a NULL context ef_last_error(NULL) names what is wrong
 * with the arguments): a NULL context, selection, count (select) or surfels12 (gather, n > 0); n > 0 or max_rows > 0 with a NULL array; unknown
 * bits in tests; with EF_SEL_BOX a non-finite entry of T_bw or a NaN bound; NaN in the range of an enabled float test; with EF_SEL_LABEL a
 * label_class outside 0 .. C-1 or a NaN label_min_prob.
 * EF_ESTATE: the context's stream is being captured; EF_SEL_ID while IDs are off or EF_SEL_LABEL while labels are off; an ID-consuming call on a
 * context whose uploaded ID lane was refused (ef_set_surfel_ids above).  The erase calls only: a context created with close_loops = 1 (its
 * sampled graph nodes, fern keyframes and pending end-of-frame record describe the unedited map); select and gather work on such contexts. */
#define EF_SEL_BOX        0x01u
#define EF_SEL_CONF       0x02u
#define EF_SEL_INIT_TIME  0x04u
#define EF_SEL_LAST_TIME  0x08u
#define EF_SEL_RADIUS     0x10u
#define EF_SEL_ID         0x20u   /* needs ef_set_surfel_ids on */
#define EF_SEL_LABEL      0x40u   /* needs ef_enable_labels on  */
#define EF_SEL_INVERT     0x100u
typedef struct ef_map_selection {
  uint32_t tests;                 /* OR of EF_SEL_*; 0 selects every row */
  double T_bw[16];                /* box frame <- world, row-major; rounded to f32 once on the host */
  float box_min[3], box_max[3];
  float conf_min, conf_max;
  int init_time_min, init_time_max;
  int last_time_min, last_time_max;
  float radius_min, radius_max;
  uint32_t id_min, id_max;
  int label_class;
  float label_min_prob;
} ef_map_selection;
/* tests 0, T_bw the identity, the box -inf .. +inf, every range covering everything (times INT_MIN .. INT_MAX, IDs 0 .. 0xFFFFFFFF), label_class 0,
 * label_min_prob -inf.  Needs neither a context nor a GPU. */
void ef_default_map_selection(ef_map_selection* sel);
int ef_map_select(ef_ctx* ctx, const ef_map_selection* sel, uint32_t* rows, uint32_t max_rows, uint32_t* count);
int ef_map_select_dev(ef_ctx* ctx, const ef_map_selection* sel, uint32_t* rows_dev, uint32_t max_rows, uint32_t* count_dev);
int ef_map_gather(ef_ctx* ctx, const uint32_t* rows, uint32_t n, float* surfels12);
int ef_map_gather_dev(ef_ctx* ctx, const uint32_t* rows_dev, uint32_t n, float* surfels12_dev);
int ef_map_erase(ef_ctx* ctx, const ef_map_selection* sel, uint32_t* removed_or_null);
int ef_map_erase_rows(ef_ctx* ctx, const uint32_t* rows, uint32_t n, uint32_t* removed_or_null);
int ef_map_erase_rows_dev(ef_ctx* ctx, const uint32_t* rows_dev, uint32_t n, uint32_t* removed_or_null);

/* ---- Insert surfels: transform a set of records, keep those the map does not already hold, append them.  Off until first used: no insert
 * call, nothing allocated, nothing run, and no frame kernel knows of it.
 *
 * A RECORD is 12 floats in ef_map_download's layout (what ef_map_download and ef_map_gather produce): position = floats 0 .. 2, confidence = 3,
 * colour = 4, ID bits = 5, creation time = 6, time last seen = 7, normal = 8 .. 10, radius = 11.  T (row-major 4 x 4 double like every other pose
 * here) maps the records' frame into the map's world frame, as in ef_register_cloud.  All per-record arithmetic is f32, one rounding per
 * operation, no contraction, in the written order.  Comparisons with NaN are false.
 *
 * TRANSFORM.  With T given, Rf, tf are its rotation block and translation rounded to f32 once, and for the position (x, y, z) and normal m:
 *   p'x = ((Rf00*x + Rf01*y) + Rf02*z) + tfx, likewise y, z;   m'x = (Rf00*mx + Rf01*my) + Rf02*mz, likewise y, z
 * (the expressions ef_register_step documents).  With T NULL nothing is computed: p' = p and m' = m bit for bit, -0 and NaN payloads included
 * (an identity T does compute: it turns -0 + 0 into +0).  Confidence, colour and radius are always copied bit for bit.
 *
 * GATE (gate = 1).  s = the row ef_query_nearest returns for p' with max_dist = min_separation and this min_conf, on the map AS IT STANDS BEFORE
 * THE CALL: the same eligibility, the same (d2, row) order, the same treatment of non-finite input.  The record is a DUPLICATE iff s is a hit and
 * (min_normal_cos <= -1 or ((m'x*nsx + m'y*nsy) + m'z*nsz) >= min_normal_cos), ns the stored normal of s, not renormalised; a NaN fails the
 * comparison, so the record is not a duplicate.  Only the NEAREST eligible surfel is asked: where the nearest is the back face of a thin wall whose
 * normal fails the test, the record is let in even if a surfel of its own side also lies inside the radius.  Records never gate one another: the
 * outcome of a record depends on the old map alone, never on n or on the records' order.  With gate = 0 no record is a duplicate and
 * min_separation, min_conf and min_normal_cos are neither read nor checked.
 *
 * OUTCOME per record i (new_row, match_row: n words each, either may be NULL):
 *   SKIPPED    p' has a non-finite coordinate:  new_row[i] = match_row[i] = 0xFFFFFFFF;
 *   DUPLICATE  new_row[i] = 0xFFFFFFFF, match_row[i] = s;
 *   INSERTED   match_row[i] = 0xFFFFFFFF, new_row[i] = count_before + (the number of inserted records before i in the input).
 * result (HOST memory in both variants) = the three counts and count_after, the map count the call leaves.
 *
 * What an insert leaves behind:
 *   the map       the old rows untouched, every word of them, followed by the inserted records in input order (the append is stable).  An inserted
 *                 row is: p' and the record's confidence; the record's colour, ZERO bits in the ID lane whatever the record held, float 6 =
 *                 (float)init_time if init_time >= 0 or the record's own under EF_INSERT_KEEP, float 7 likewise from last_time; m' and the
 *                 record's radius;
 *   IDs           with IDs on, the rows created since the last ID-consuming call are numbered BEFORE the append (as the erase does), and the next
 *                 ID-consuming call numbers the inserted rows above every ID ever handed out.  A gathered record does not bring its old ID back;
 *   the context   the state that ef_map_upload(old rows ++ inserted rows) followed by ef_restore_state(tick, ef_get_pose_qt, the last processed
 *                 frame) would leave: tick, pose, trajectory, last frame and tracking statistics are unchanged, and if ef_process_frame* or
 *                 ef_restore_state has run on the context the model prediction is renewed from the edited map at the current pose.  On a context
 *                 whose map was only uploaded, only the map changes;
 *   the index     of the queries and the registration is stale and rebuilt by their next call;
 *   labels        the next label call re-aligns by ID: old rows keep their C floats bit for bit, inserted rows get the prior 1 / C;
 *   the shadow buffer of ef_set_reference_download is left as it is.
 * Inserting nothing (n = 0, every record a duplicate or skipped) is valid and still leaves the state described.
 *
 * CAPACITY.  The number to insert is known before anything is written.  If count_before + inserted > max_surfels the call returns EF_ECAPACITY
 * and nothing has changed: map, count, prediction, the index's validity.  result still carries the three counts, with count_after =
 * count_before; match_row is written, new_row is not.
 *
 * Defaults (ef_default_insert_params): gate 1, min_separation 0.01 m, min_conf -1 (every surfel can suppress a record), min_normal_cos 0.5 (the
 * registration's default), both times the context's tick.  0.01 m is half of EF_QUERY_DEFAULT_CELL, so that a walk visits at most 27 cells: a
 * convention, not a measurement.
 *
 * Both variants synchronise before and after, like the erase calls.  ef_map_insert stages its arrays; ef_map_insert_dev takes DEVICE pointers for
 * the records and the two row arrays.  surfels12_dev is read in 16-byte words: it must be 16-byte aligned, as every ef_dev_alloc pointer is, and
 * must not lie inside the map.
 *
 * EF_EINVAL, before any GPU work (the arguments are checked before the context, so with a NULL context ef_last_error(NULL) names what is wrong
 * with them): a NULL context, params or result; n > 0 with NULL records; n above EF_INSERT_MAX_RECORDS (2^28 - 1: 12 GB of records in one
 * call); a non-finite entry of T; gate outside 0 / 1; a time below
 * EF_INSERT_KEEP; with gate = 1: min_separation, min_conf and the ratio to the query cell as ef_query_nearest refuses max_dist, min_conf and
 * max_dist / cell, or a NaN min_normal_cos; surfels12_dev not 16-byte aligned.
 * EF_ESTATE: the context's stream is being captured; a context created with close_loops = 1 (the erase's reason); with IDs on, a context whose
 * uploaded ID lane was refused (ef_set_surfel_ids above). */
#define EF_INSERT_KEEP (-1)
#define EF_INSERT_MAX_RECORDS 0x0FFFFFFFu
typedef struct ef_insert_params {
  int   gate;            /* 0: every record with a finite moved position is inserted; 1: the novelty gate above */
  float min_separation;  /* gate radius in metres: ef_query_nearest's max_dist */
  float min_conf;        /* which map surfels can suppress a record: as ef_query_nearest (negative = every surfel) */
  float min_normal_cos;  /* <= -1: no normal test */
  int   init_time;       /* >= 0: float 6 of the stored row = (float)init_time; EF_INSERT_KEEP: the record's own */
  int   last_time;       /* likewise float 7 */
} ef_insert_params;
typedef struct ef_insert_result { uint32_t inserted, duplicates, skipped, count_after; } ef_insert_result;
int ef_default_insert_params(ef_ctx* ctx, ef_insert_params* params);
int ef_map_insert(ef_ctx* ctx, const float* surfels12, uint32_t n, const double* T16_or_null, const ef_insert_params* params,
                  ef_insert_result* result, uint32_t* new_row_or_null, uint32_t* match_row_or_null);
int ef_map_insert_dev(ef_ctx* ctx, const float* surfels12_dev, uint32_t n, const double* T16_or_null, const ef_insert_params* params,
                      ef_insert_result* result, uint32_t* new_row_dev_or_null, uint32_t* match_row_dev_or_null);

/* ---- Fuse surfels: transform a set of records, merge those that match a map surfel INTO that surfel (at most one record per surfel and
 * call), optionally append the others.  What ef_map_insert throws away as a duplicate improves the map here: confidence rises, position, normal,
 * radius and colour are averaged, as a frame's fusion does for a measurement.  Off until first used: no fuse call, nothing allocated, nothing
 * run, and no frame kernel knows of it.
 *
 * Records, T, the TRANSFORM (p', m') and the arithmetic rules are those of "Insert surfels" above: f32, one rounding per operation, no
 * contraction, in the written order; comparisons with NaN are false.  The outcome is a pure function of (map, records, T, params): it depends on
 * no order of evaluation and on no sum.
 *
 * 1. MATCH.  Exactly the insert's gate, which is always on: s = the row ef_query_nearest returns for p' with max_dist = min_separation and this
 * min_conf, on the map AS IT STANDS BEFORE THE CALL.  The record is MATCHED iff s is a hit and (min_normal_cos <= -1 or
 * ((m'x*nsx + m'y*nsy) + m'z*nsz) >= min_normal_cos), ns the stored normal of s.  A record that is not matched is SKIPPED if p' has a non-finite
 * coordinate and NOVEL otherwise.  Records never match one another.  match_row[i] = s for a matched record, 0xFFFFFFFF otherwise.
 *
 * 2. ELECTION.  A matched record COMPETES iff its confidence a (float 3) satisfies a > 0 && a < +infinity; a matched record that does not (zero,
 * negative, infinite, NaN) is WEIGHTLESS: counted, and nothing else.  Among the competitors of one map row s the winner is the minimum of
 * (d2, record index): d2 = ((dx*dx + dy*dy) + dz*dz) with dx = p'x - psx and so on, ps the stored position of s (the query's own f32
 * expression; finite and non-negative, so comparing the floats is comparing their bits), and among equal d2 the LOWEST index.  The winner is
 * FUSED; every other competitor of that row is ABSORBED: counted, and nothing else.  So a surfel takes at most one record per call, and which one
 * depends on the records' order only through the tie-break.
 *
 * 3. MERGE of the FUSED record into row s, in place.  c_k = the stored confidence, (px, py, pz), colour, (nx, ny, nz), radius_s the stored
 * row; a, colour_rec, radius_rec the record's floats 3, 4, 11; p', m' the MOVED position and normal.  With avg(old, new) =
 * ((c_k*old) + (a*new)) / (c_k + a):
 *   if radius_rec < (1.0f + 0.5f) * radius_s:
 *     position  each coordinate = avg(stored, p');                    confidence = c_k + a;
 *     normal    v = (avg(nx, m'x), avg(ny, m'y), avg(nz, m'z)), dot = (vz*vz) + ((vy*vy) + (vx*vx)), rn = 1.0f / sqrtf(dot), stored normal =
 *               (vx*rn, vy*rn, vz*rn);                                radius = avg(radius_s, radius_rec);
 *     colour    a colour float c decodes to three channels: ic = (int)c (toward zero; the device's conversion where c is outside int: saturated,
 *               NaN gives 0), channel = (float)((ic >> 16) & 0xFF) / 255.0f, likewise >> 8 and >> 0.  Per channel mean = avg(stored channel,
 *               record channel), q = roundf(mean * 255.0f) (half AWAY from zero), u = (unsigned)(int)q if -2^31 <= q < 2^31, else 0x80000000 (NaN
 *               included).  rgb = (((ur << 8) + ug) << 8) + ub in 32-bit unsigned arithmetic; the stored colour = (float)(int)rgb;
 *   else only the confidence (c_k + a) changes;
 *   in both cases float 7 (time last seen) = (float)last_time, or the record's own float 7 under EF_INSERT_KEEP.
 * (The update pass of a frame's fusion, on the record instead of a measurement.)  The ID lane and the creation time (floats 5, 6) are never
 * written: the surfel keeps its stable ID, and its label row still follows it.  A surfel with c_k + a == 0 or a non-finite sum gets what the
 * expressions give.
 *
 * 4. APPEND.  With append = 1 the NOVEL records are appended in input order: the rows, new_row and count are bit for bit what ef_map_insert with
 * gate = 1 and the same min_separation, min_conf, min_normal_cos, init_time, last_time would append to the old map.  With append = 0 they are
 * only counted, and every new_row is 0xFFFFFFFF.
 *
 * OUTCOME per record i (new_row, match_row: n words each, outcome: n bytes; each may be NULL): outcome[i] is one of the EF_FUSE_* values below;
 * a NOVEL record reads EF_FUSE_INSERTED when append = 1, EF_FUSE_NOVEL when append = 0.  result (HOST memory in both variants): fused + absorbed
 * + weightless = the matched records, novel, skipped (the five add up to n), inserted = novel if append else 0, count_after = the map count the
 * call leaves.
 *
 * What a fuse leaves behind: the map as described (rows that are nobody's match_row keep every bit; so do the rows of ABSORBED-only and
 * WEIGHTLESS-only matches), and everything else as "What an insert leaves behind" says with "old rows ++ inserted rows" read as "the fused old
 * rows ++ appended rows": IDs (numbered before the call's edits; appended rows are numbered by the next ID-consuming call), the context (the
 * prediction is renewed from the edited map), the index (stale), labels (old rows keep their floats, appended rows get the prior), the shadow
 * buffer.  A call that fuses and appends nothing (n = 0, an empty map with append = 0) is valid and still leaves that state.
 *
 * CAPACITY.  Every count is known before anything is written.  If append = 1 and count_before + novel > max_surfels the call returns
 * EF_ECAPACITY and NOTHING has changed, fused rows included: map, count, prediction, the index's validity.  result carries all the counts (those
 * the call would have had), with inserted = novel and count_after = count_before; nothing is promised about the three arrays.
 *
 * Defaults (ef_default_fuse_params): the insert's (min_separation 0.01 m, min_conf -1, min_normal_cos 0.5, both times the tick), append = 1.
 *
 * Both variants synchronise before and after.  ef_map_fuse stages its arrays; ef_map_fuse_dev takes DEVICE pointers for the records and the
 * three arrays; surfels12_dev must be 16-byte aligned and must not lie inside the map.
 *
 * EF_EINVAL, before any GPU work: everything ef_map_insert refuses with gate = 1 (NULL context, params or result; n > 0 with NULL records; n above
 * EF_INSERT_MAX_RECORDS; a non-finite entry of T; a time below EF_INSERT_KEEP; min_separation, min_conf, the ratio to the query cell; a NaN
 * min_normal_cos; surfels12_dev not 16-byte aligned), and append outside 0 / 1.
 * EF_ESTATE: as ef_map_insert (a captured stream; a context created with close_loops = 1; a refused ID lane). */
#define EF_FUSE_SKIPPED    0
#define EF_FUSE_NOVEL      1
#define EF_FUSE_WEIGHTLESS 2
#define EF_FUSE_ABSORBED   3
#define EF_FUSE_FUSED      4
#define EF_FUSE_INSERTED   5
typedef struct ef_fuse_params {
  float min_separation, min_conf, min_normal_cos;  /* the match: exactly ef_insert_params' gate (the gate is always on) */
  int   append;      /* 1: records that match nothing are appended exactly as ef_map_insert would; 0: they are only counted */
  int   init_time;   /* of appended rows, as ef_insert_params */
  int   last_time;   /* of appended rows AND of fused surfels; EF_INSERT_KEEP: the record's own float 7 */
} ef_fuse_params;
typedef struct ef_fuse_result { uint32_t fused, absorbed, weightless, novel, skipped, inserted, count_after; } ef_fuse_result;
int ef_default_fuse_params(ef_ctx* ctx, ef_fuse_params* params);
int ef_map_fuse(ef_ctx* ctx, const float* surfels12, uint32_t n, const double* T16_or_null, const ef_fuse_params* params, ef_fuse_result* result,
                uint32_t* new_row_or_null, uint32_t* match_row_or_null, uint8_t* outcome_or_null);
int ef_map_fuse_dev(ef_ctx* ctx, const float* surfels12_dev, uint32_t n, const double* T16_or_null, const ef_fuse_params* params,
                    ef_fuse_result* result, uint32_t* new_row_dev_or_null, uint32_t* match_row_dev_or_null, uint8_t* outcome_dev_or_null);

/* ---- Thin the map: keep one surfel per voxel of a grid, remove the others (the voxel-grid filter).  Off until first used: no thin call,
 * nothing allocated, nothing run, and no frame kernel knows of it.
 *
 * "Row" and the layout of a surfel are those of the section "Select, extract and erase surfels": position = floats 0 .. 2, confidence = float 3,
 * time last seen = float 7.  The outcome is a pure function of the map and the arguments: it depends on no order of evaluation and on no sum.
 *
 * CELL.  inv_cell = 1.0f / cell, computed once in f32.  Per axis the cell coordinate of a position coordinate v is floor(fl(v * inv_cell)) (the
 * f32 PRODUCT with inv_cell, not a quotient by cell), clamped to -2^20 .. +2^20: the cell function of the queries' index.  Two surfels share a cell
 * iff all three coordinates agree.  Everything beyond the clamp (|v * inv_cell| >= 2^20) falls into the boundary cells: such surfels share a cell
 * however far apart they are, and therefore ONE representative.
 *
 * PARTICIPANTS.  With among NULL, every row whose position has three finite coordinates.  With a selection, the rows that are SELECTED by it
 * (the predicate of ef_map_select, unchanged, EF_SEL_INVERT included) and have a finite position.  A row that does not participate is KEPT: it is
 * neither a representative nor removed, it beats nobody and counts nowhere.
 *
 * REPRESENTATIVE.  The primary of a participant is, by keep:
 *   EF_THIN_KEEP_MAX_CONF   its confidence (float 3);
 *   EF_THIN_KEEP_NEWEST     its time last seen (float 7);
 *   EF_THIN_KEEP_FIRST      a constant.
 * Primaries are compared as f32 VALUES with two amendments that make the order total: -0 equals +0, and every NaN counts as -infinity (equal to
 * -infinity and to every other NaN).  Among the participants of one cell the representative is the one with the greatest primary; among equal
 * primaries the one with the LOWEST row.  Every other participant of the cell is REMOVED.  Hence every cell that holds a participant has exactly
 * one representative, the outcome of a row depends only on the participants of its own cell, and thinning twice with the same arguments removes
 * nothing the second time (the representatives are alone in their cells).
 *
 * ef_map_thin_select changes nothing.  It writes the rows named by `what`, EF_THIN_ROWS_REMOVED or EF_THIN_ROWS_REPRESENTATIVES, with
 * ef_map_select's conventions: the first min(max_rows, total) of them in ASCENDING order, *count = total however small max_rows is, rows may be
 * NULL with max_rows 0, entries past min(max_rows, total) are left as they were.  The removed list is what ef_map_erase_rows takes; the
 * representatives list is what ef_map_gather takes (a thinned copy of the map then leaves the device while the map stays as it is; kept
 * non-participants are not in that list).  The _dev variant takes DEVICE pointers for rows and count and only enqueues on the context's stream,
 * except for what the selection needs (ID numbering, label alignment, the count after a call that can change the map) and except that it waits
 * for the device once when the index has to be rebuilt (the map changed, or the index was last built at another cell).
 *
 * ef_map_thin removes the removed rows and leaves everything exactly as ef_map_erase_rows(the removed list) would: see "What an erase leaves
 * behind" above (the map, the context, the index, IDs, labels, the shadow buffer), with the same two synchronisations.  result (HOST memory):
 * cells = the number of representatives, removed, participants = cells + removed, count_after = the map count the call leaves.
 *
 * The index of the queries is built at the thin's cell where needed; a later query at another cell (ef_set_query_cell's) rebuilds it, as after
 * ef_set_query_cell.  No query result changes.  There is no limit on the cell's size: no box of cells is walked.
 *
 * EF_EINVAL, before any GPU work (the arguments are checked before the context, so with a NULL context ef_last_error(NULL) names what is wrong
 * with them): a NULL context, params, result or count; a cell that is not finite and positive or whose 1 / cell is not finite
 * (ef_set_query_cell's rule); keep or what outside their values; with among given, everything ef_map_select refuses for a selection;
 * max_rows > 0 with NULL rows.
 * EF_ESTATE: the context's stream is being captured; with among given, what ef_map_select answers with EF_ESTATE.  ef_map_thin only: a context
 * created with close_loops = 1 (the erase's reason; the map is unchanged); ef_map_thin_select works on such contexts. */
#define EF_THIN_KEEP_MAX_CONF 0   /* primary = confidence (pos_conf.w)            */
#define EF_THIN_KEEP_NEWEST   1   /* primary = last-seen time (col_time.w)        */
#define EF_THIN_KEEP_FIRST    2   /* primary = a constant: the lowest row wins    */
#define EF_THIN_ROWS_REMOVED         0
#define EF_THIN_ROWS_REPRESENTATIVES 1
typedef struct ef_thin_params { float cell; int keep; } ef_thin_params;
typedef struct ef_thin_result { uint32_t participants, cells, removed, count_after; } ef_thin_result;
/* cell = EF_QUERY_DEFAULT_CELL, keep = EF_THIN_KEEP_MAX_CONF */
int ef_default_thin_params(ef_ctx* ctx, ef_thin_params* params);
int ef_map_thin_select(ef_ctx* ctx, const ef_thin_params* params, const ef_map_selection* among_or_null, int what, uint32_t* rows,
                       uint32_t max_rows, uint32_t* count);
int ef_map_thin_select_dev(ef_ctx* ctx, const ef_thin_params* params, const ef_map_selection* among_or_null, int what, uint32_t* rows_dev,
                           uint32_t max_rows, uint32_t* count_dev);
int ef_map_thin(ef_ctx* ctx, const ef_thin_params* params, const ef_map_selection* among_or_null, ef_thin_result* result);

/* ---- Carve free space: remove the surfels that depth views see through (the free-space violation test of surfel and TSDF mapping).  A frame's
 * clean drops only unstable surfels; a surfel that became stable stays although the thing it stood for has moved.  Off until first used: no
 * carve call, nothing allocated, nothing run, and no frame kernel knows of it.
 *
 * "Row" and the layout of a surfel are those of the section "Select, extract and erase surfels": position (X, Y, Z) = floats 0 .. 2.  All per-row
 * arithmetic is f32, one rounding per operation, no contraction, in the written order.  Comparisons with NaN are false.  The outcome of a row is
 * a pure function of that row, the views and the parameters: it depends on no other row, on no order of evaluation and on no sum.
 *
 * VIEWS.  n views, 1 <= n <= EF_CARVE_MAX_VIEWS.  View k has T_wc = T_wc16[16 k .. 16 k + 15] (world <- camera, row-major 4 x 4 double like every
 * other pose here, rigid) and the image depth[k * height * width ..]: height x width uint16 millimetres, row-major, what ef_process_frame takes.
 * All views share one camera (width, height, fx, fy, cx, cy of the parameters).  The host forms T_cw per view in double, in this order, and then
 * rounds each of the twelve entries to f32 once: with t = (T_wc[0][3], T_wc[1][3], T_wc[2][3]),
 *   Rc[i][j] = T_wc[j][i],     tc[i] = -((T_wc[0][i]*t[0] + T_wc[1][i]*t[1]) + T_wc[2][i]*t[2])
 * (the transpose and its product with t: no quaternion, no normalisation; a T_wc that is not rigid gives what the expressions give).
 *
 * PER ROW AND VIEW.  The camera-frame point, with the box test's expression:
 *   x = ((Rc00*X + Rc01*Y) + Rc02*Z) + tcx,   y = ((Rc10*X + Rc11*Y) + Rc12*Z) + tcy,   z = ((Rc20*X + Rc21*Y) + Rc22*Z) + tcz.
 * The view SAYS NOTHING about the row in each of these cases:
 *   - z > 0 does not hold;
 *   - with uf = (fx*x)/z + cx and vf = (fy*y)/z + cy, not (uf >= 0 && uf < (float)width && vf >= 0 && vf < (float)height): compared as floats
 *     BEFORE any conversion, so that NaN, +-infinity and values beyond the int range fall out here (and uf = -0.5 does: no truncation to 0);
 *   - with u = (int)uf, v = (int)vf, the centre texel (u, v) has no data.
 * A texel d HAS DATA iff d != 0 and, with zo = (float)d / 1000.0f, min_depth <= zo && zo <= max_depth.  The WINDOW is the texels (u + a, v + b)
 * with |a| <= window and |b| <= window that lie inside the image and have data; for each of them tol = margin + (margin_quad*zo)*zo.  Then
 *   FREE       iff (z + tol) < zo holds for EVERY texel of the window, the centre included: the view measured a surface behind the surfel along
 *              every ray near it, so the ray through the surfel crossed the place where it claims a surface;
 *   SUPPORTED  iff at the centre texel neither (z + tol) < zo nor (zo + tol) < z holds: the view measured the surfel's own surface;
 *   otherwise the view says nothing: the surfel is occluded (something nearer was measured), or a depth edge runs through the window.
 * A view is never both.  Texels outside the image or without data are ignored, so at a border or beside a hole the window is smaller.
 *
 * PER ROW.  A row PARTICIPATES iff it is SELECTED by among (the predicate of ef_map_select, unchanged, EF_SEL_INVERT included; among NULL:
 * every row is) and its three position floats are finite.  free = the number of FREE views, support = the number of SUPPORTED views.  The row is
 * REMOVED iff it participates, free >= min_views, and not (protect != 0 and support > 0).  Every other row is kept: occluded, outside every
 * image, on a depth hole, not a participant.
 *
 * OUTPUTS.  votes2 (optional), 2 bytes per row of the map: {free, support}; {0, 0} for a row that does not participate.  ef_carve_result:
 * participants; observed = the participants with free + support > 0; free_space = those with free >= min_views; protected_ = the free_space rows
 * that support kept (free_space - removed); removed; count_after = the map count the call leaves.
 *
 * ef_map_carve_select changes nothing.  It writes the REMOVED rows with ef_map_select's conventions: the first min(max_rows, total) of them in
 * ASCENDING order, *count = total however small max_rows is, rows may be NULL with max_rows 0, entries past min(max_rows, total) are left as they
 * were.  The list is what ef_map_erase_rows takes.  The host variant stages the images and synchronises.  ef_map_carve_select_dev takes DEVICE
 * pointers for depth, rows, count and votes2 (T_wc16 stays a HOST pointer: it is read before the call returns) and only enqueues on the context's
 * stream, except for what the selection needs (ID numbering, label alignment, the count after a call that can change the map).
 *
 * ef_map_carve removes the removed rows and leaves everything exactly as ef_map_erase_rows(the list of ef_map_carve_select) would: see "What an
 * erase leaves behind" above (the map, the context, the index, IDs, labels, the shadow buffer), with the same two synchronisations.  Removing
 * nothing is valid.  ef_map_carve_dev takes a DEVICE pointer for depth; result is HOST memory in both.
 *
 * Defaults (ef_default_carve_params): the frame camera; min_depth 0.3 m; max_depth = the context's depth cut-off (ef_set_depth_cutoff); margin
 * 0.02 m, margin_quad 0.0025 / m (tol = 2 cm at the camera, 3 cm at 2 m, 4.25 cm at 3 m); window 1, min_views 1, protect 1.  The two margins are a
 * CHOICE, not a measurement: the quadratic term follows the way a structured-light sensor's depth noise grows with range, and nobody has fitted
 * either number to a sensor.  Give your own.
 *
 * EF_EINVAL, before any GPU work (the arguments are checked before the context, so with a NULL context ef_last_error(NULL) names what is wrong
 * with them): a NULL context, params, views, result or count; n outside 1 .. EF_CARVE_MAX_VIEWS; a NULL T_wc16 or depth; a non-finite pose entry;
 * width or height outside 1 .. 4096; non-finite intrinsics; a NaN or negative margin or margin_quad; a NaN min_depth or max_depth, or min_depth >
 * max_depth; window outside 0 .. 2; min_views outside 1 .. n; max_rows > 0 with NULL rows; with among given, everything
 * ef_map_select refuses for a selection.
 * EF_ESTATE: the context's stream is being captured; with among given, what ef_map_select answers with EF_ESTATE.  ef_map_carve[_dev] only: a
 * context created with close_loops = 1 (the erase's reason; the map is unchanged); the select variants work on such contexts. */
#define EF_CARVE_MAX_VIEWS 32
typedef struct ef_carve_params {
  int   width, height;          /* of every depth image */
  float fx, fy, cx, cy;         /* the camera all views share */
  float min_depth, max_depth;   /* metres: a texel outside has no data */
  float margin, margin_quad;    /* tol = margin + (margin_quad*zo)*zo */
  int   window;                 /* 0 .. 2: the (2 window + 1)^2 texels around the centre */
  int   min_views;              /* 1 .. n: FREE views a removed row needs */
  int   protect;                /* 1: one SUPPORTED view keeps the row */
} ef_carve_params;
typedef struct ef_carve_views {
  int n;                        /* 1 .. EF_CARVE_MAX_VIEWS */
  const double* T_wc16;         /* n x 16, HOST memory in every variant */
  const uint16_t* depth;        /* n consecutive height x width images */
} ef_carve_views;
typedef struct ef_carve_result { uint32_t participants, observed, free_space, protected_, removed, count_after; } ef_carve_result;
int ef_default_carve_params(ef_ctx* ctx, ef_carve_params* params);
int ef_map_carve_select(ef_ctx* ctx, const ef_carve_params* params, const ef_carve_views* views, const ef_map_selection* among_or_null,
                        uint32_t* rows, uint32_t max_rows, uint32_t* count, uint8_t* votes2_or_null);
int ef_map_carve_select_dev(ef_ctx* ctx, const ef_carve_params* params, const ef_carve_views* views_depth_dev,
                            const ef_map_selection* among_or_null, uint32_t* rows_dev, uint32_t max_rows, uint32_t* count_dev,
                            uint8_t* votes2_dev_or_null);
int ef_map_carve(ef_ctx* ctx, const ef_carve_params* params, const ef_carve_views* views, const ef_map_selection* among_or_null,
                 ef_carve_result* result);
int ef_map_carve_dev(ef_ctx* ctx, const ef_carve_params* params, const ef_carve_views* views_depth_dev, const ef_map_selection* among_or_null,
                     ef_carve_result* result);

/* ---- Remove outlier surfels: neighbourhood statistics of the map (the radius and the statistical outlier filters of point-cloud toolkits).  A
 * speck that became stable stands alone: no frame's clean drops it, and a thin keeps it because it is alone in its cell.  Off until first used:
 * no outlier call, nothing allocated, nothing run, and no frame kernel knows of it.
 *
 * "Row" and the layout of a surfel are those of the section "Select, extract and erase surfels": position = floats 0 .. 2, confidence = float 3.
 * All arithmetic is f32, one rounding per operation, no contraction, in the written order, except where double is named.  d2(q, t) and the rule
 * "t is ELIGIBLE for q iff conf_t > min_conf and d2 <= r2" are those of the section "Spatial index and nearest-surfel / kNN queries", with
 * r2 = radius * radius computed once in f32 on the host and the queries' rule for min_conf (negative: every surfel; NaN is refused).
 *
 * PARTICIPANTS, as in the thin.  With among NULL, every row whose position has three finite coordinates.  With a selection, the rows that are
 * SELECTED by it (the predicate of ef_map_select, unchanged, EF_SEL_INVERT included) and have a finite position.  A row that does not
 * participate is never an outlier, and its outputs are count = 0, mean_dist = +inf.
 *
 * NEIGHBOURS of the participant in row s are all rows t != s that are eligible for the query point p_s (the position of row s), whether or not
 * t participates.  Self is excluded by ROW, not by distance: a coincident surfel in another row is a neighbour at d2 = 0.  Neighbours are ordered
 * by (d2, row) ascending.  count_s = the number of ALL neighbours; it may exceed 16.
 *
 * MEAN DISTANCE.  k lies in 1 .. 16.  If count_s >= k, row s is MEASURED and, with d2_1 .. d2_k the first k neighbours' d2 in that order,
 *   mean_s = (((sqrt(d2_1) + sqrt(d2_2)) + ...) + sqrt(d2_k)) / (float)k
 * summed in neighbour order; every square root and the quotient are the CORRECTLY ROUNDED f32 operations (IEEE 754; no approximate instruction,
 * whatever the build's flags).  Otherwise row s is SPARSE and mean_s = +inf.  In EF_OUTLIER_RADIUS mode the field k is ignored, mean_dist is
 * computed with k = 1, and nothing is summed (sum = sum_sq = 0).
 *
 * SUMS, in double, pure functions of the per-row values BY ROW (they depend on no order in which anything was evaluated).  For a measured row r,
 * term1(r) = (double)mean_r and term2(r) = (double)mean_r * (double)mean_r (both exact); every other row of the map contributes +0.0.  With
 * P = EF_OUTLIER_SUM_LANES, for each of the two terms:
 *   partial[j] = ((term(j) + term(j + P)) + term(j + 2P)) + ...   for j = 0 .. P-1, rows ascending, starting from +0.0;
 *   then twelve rounds of a[i] = a[2i] + a[2i+1] over a = partial (4096 -> 2048 -> ... -> 1); the sum is a[0].
 * S1 = the sum of term1, S2 = the sum of term2, N = the number of measured rows.
 *
 * THRESHOLD, in double:  mu = S1 / N;  var = S2 / N - mu * mu, set to 0 if it is negative;  t = mu + (double)std_ratio * sqrt(var) (correctly
 * rounded);  thr = (float)t.  If N = 0, thr = +inf.  If max_mean_dist > 0, thr = max_mean_dist and the sums are only reported.  In
 * EF_OUTLIER_RADIUS mode thr = +inf.
 *
 * OUTLIERS.  EF_OUTLIER_STATISTICAL: a measured row is an outlier iff mean_s > thr, compared in f32; a sparse row is an outlier iff
 * flag_sparse != 0.  EF_OUTLIER_RADIUS: a participant is an outlier iff count_s < (uint32_t)min_neighbors.
 *
 * ef_map_neighbor_stats changes nothing.  It writes mean_dist[r] and count[r] of the rows r < min(max_rows, map count) (either array may be NULL;
 * entries past that are left as they were).  ef_map_outliers_select changes nothing.  It writes the outlier rows with ef_map_select's
 * conventions: the first min(max_rows, total) of them in ASCENDING order, *count = total however small max_rows is, rows may be NULL with
 * max_rows 0, entries past min(max_rows, total) are left as they were.  The list is what ef_map_erase_rows takes.  result (optional): sum = S1,
 * sum_sq = S2, participants, measured = N, sparse (in EF_OUTLIER_RADIUS mode both by k = 1), outliers = total, count_after = the map count
 * minus total, threshold = thr.  The _dev variants take DEVICE pointers for the arrays, count and result and only enqueue on the context's stream
 * (the threshold is formed on the device), except for what the selection needs (ID numbering, label alignment, the count after a call that can
 * change the map) and except that they wait for the device once when the index has to be rebuilt or the scratch grows.
 *
 * ef_map_remove_outliers removes the outlier rows and leaves everything exactly as ef_map_erase_rows(the list of ef_map_outliers_select) would:
 * see "What an erase leaves behind" above (the map, the context, the index, IDs, labels, the shadow buffer), with the same two synchronisations.
 * result (HOST memory, required): as above for the map as it WAS, outliers = the rows removed, count_after = the map count the call leaves.
 * Unlike the thin it is NOT idempotent: removing specks changes mu and sigma of what is left, so a second call may remove more.
 *
 * cell is the cell of the queries' index, which is built at that cell where needed; a later query at another cell (ef_set_query_cell's) rebuilds
 * it, as after ef_set_query_cell.  No result depends on it.  Defaults (ef_default_outlier_params): EF_OUTLIER_STATISTICAL, k 8, std_ratio 2,
 * max_mean_dist 0, flag_sparse 1, radius 0.03 m, min_neighbors 4, min_conf -1, cell 0.03 m (= radius, chosen by measurement among radius / 2,
 * radius and 2 radius: DESIGN.md §8i).
 *
 * EF_EINVAL, before any GPU work (the arguments are checked before the context, so with a NULL context ef_last_error(NULL) names what is wrong
 * with them): a NULL context, params, count or (ef_map_remove_outliers) result; a mode outside its two values; radius or cell not finite and
 * positive, or 1 / cell not finite; radius / cell above EF_QUERY_MAX_RATIO; k outside 1 .. 16 in EF_OUTLIER_STATISTICAL mode; min_neighbors < 0;
 * NaN min_conf or std_ratio, a negative std_ratio, a negative or NaN max_mean_dist; max_rows > 0 with NULL rows; with among given, everything
 * ef_map_select refuses for a selection.
 * EF_ESTATE: the context's stream is being captured; with among given, what ef_map_select answers with EF_ESTATE.  ef_map_remove_outliers only:
 * a context created with close_loops = 1 (the erase's reason; the map is unchanged); the select variants and the stats work on such contexts. */
#define EF_OUTLIER_RADIUS       0   /* outlier iff fewer than min_neighbors neighbours within radius      */
#define EF_OUTLIER_STATISTICAL  1   /* outlier iff mean distance to the k nearest neighbours > threshold  */
#define EF_OUTLIER_SUM_LANES 4096   /* P of the summation order above */
typedef struct ef_outlier_params {
  int mode; float radius; float cell; float min_conf;
  int min_neighbors;                 /* RADIUS */
  int k; float std_ratio; float max_mean_dist; int flag_sparse;   /* STATISTICAL */
} ef_outlier_params;
typedef struct ef_outlier_result {
  double sum, sum_sq;                /* S1, S2 above (0 in RADIUS mode) */
  uint32_t participants, measured, sparse, outliers, count_after;
  float threshold;                   /* thr above (+inf in RADIUS mode) */
} ef_outlier_result;
int ef_default_outlier_params(ef_ctx* ctx, ef_outlier_params* params);
int ef_map_neighbor_stats(ef_ctx* ctx, const ef_outlier_params* params, const ef_map_selection* among_or_null, float* mean_dist_or_null,
                          uint32_t* count_or_null, uint32_t max_rows);
int ef_map_neighbor_stats_dev(ef_ctx* ctx, const ef_outlier_params* params, const ef_map_selection* among_or_null, float* mean_dist_dev_or_null,
                              uint32_t* count_dev_or_null, uint32_t max_rows);
int ef_map_outliers_select(ef_ctx* ctx, const ef_outlier_params* params, const ef_map_selection* among_or_null, uint32_t* rows, uint32_t max_rows,
                           uint32_t* count, ef_outlier_result* result_or_null);
int ef_map_outliers_select_dev(ef_ctx* ctx, const ef_outlier_params* params, const ef_map_selection* among_or_null, uint32_t* rows_dev,
                               uint32_t max_rows, uint32_t* count_dev, ef_outlier_result* result_dev_or_null);
int ef_map_remove_outliers(ef_ctx* ctx, const ef_outlier_params* params, const ef_map_selection* among_or_null, ef_outlier_result* result);

/* ---- Connected components of the map under "closer than r" (the Euclidean cluster extraction of point-cloud toolkits).  A detached blob of a
 * few hundred surfels (a ghost a loop closure left, the far side of a carve) survives the statistical filter, because every member has k close
 * neighbours; "this component has fewer than m members" removes it.  After an erase of the floor's box the components are the objects.  Off
 * until first used: no component call, nothing allocated, nothing run, and no frame kernel knows of it.
 *
 * "Row", the layout of a surfel, d2(q, t) = ((dx * dx + dy * dy) + dz * dz) in f32 with dx = q.x - t.x (one rounding per operation, no
 * contraction, in the written order) and r2 = radius * radius computed once in f32 on the host are those of the sections "Spatial index and
 * nearest-surfel / kNN queries" and "Remove outlier surfels".  d2 is SYMMETRIC in f32: q - p and p - q differ in sign only, and the squares
 * and their sums do not see the sign, so d2(p_s, p_t) and d2(p_t, p_s) are the same bits and the graph below is undirected by construction.
 *
 * PARTICIPANTS are the thin's and the outliers'.  With among NULL, every row whose position has three finite coordinates.  With a selection, the
 * rows that are SELECTED by it (the predicate of ef_map_select, unchanged, EF_SEL_INVERT included) and have a finite position.
 * A NODE is a participant whose confidence passes the queries' rule conf > min_conf (negative min_conf: every surfel; NaN is refused;
 * comparisons with a NaN confidence are false).
 *
 * An EDGE joins two distinct nodes s != t iff d2(p_s, p_t) <= r2.  Coincident surfels in different rows are joined at d2 = 0; a row is never
 * its own neighbour; a row that is no node never carries an edge, so a surfel that is not selected (or below min_conf) does not bridge two
 * groups that are.  COMPONENTS are the connected components of that graph.  label[s] = the SMALLEST ROW of the component of s: canonical, a
 * function of the graph alone, whatever order anything was evaluated in.  size[s] = the number of nodes of that component.  A row that is no
 * node has label = EF_COMPONENT_NONE and size = 0.
 *
 * A node is REJECTED iff size < min_size or (max_size != 0 and size > max_size), otherwise ACCEPTED; all nodes of a component share the
 * verdict.  A row that is no node is neither.
 *
 * ef_component_result: nodes; components = the number of rows r with label[r] == r; largest = the greatest size (0 without nodes);
 * rejected_rows and rejected_components = the rejected nodes and their components; count_after = the map count minus rejected_rows; status =
 * 0, or non-zero if one of the device loops ran into its step bound, which no input can cause (the host variants then return EF_EHIP and
 * ef_map_remove_components removes nothing; the _dev variants can only report it here).
 *
 * ef_map_components changes nothing.  It writes label[r] and size[r] of the rows r < min(max_rows, map count) (either array may be NULL;
 * entries past that are left as they were) and the optional result; min_size and max_size only reach the result.
 * ef_map_components_select changes nothing.  what = EF_COMPONENTS_REJECTED or EF_COMPONENTS_ACCEPTED: it writes those rows with ef_map_select's
 * conventions: the first min(max_rows, total) of them in ASCENDING order, *count = total however small max_rows is, rows may be NULL with
 * max_rows 0, entries past min(max_rows, total) are left as they were.  The list is what ef_map_erase_rows and ef_map_gather take.  The
 * result does not depend on what.  The _dev variants take DEVICE pointers for the arrays, count and result and only enqueue on the context's
 * stream, except for what the selection needs (ID numbering, label alignment, the count after a call that can change the map) and except that
 * they wait for the device once when the index has to be rebuilt or the scratch grows.
 *
 * ef_map_remove_components removes the rejected rows and leaves everything exactly as ef_map_erase_rows(the EF_COMPONENTS_REJECTED list) would:
 * see "What an erase leaves behind" above, with one more synchronisation (the result is read before a row changes).  result (HOST memory,
 * required): as above for the map as it WAS, rejected_rows = the rows removed, count_after = the map count the call leaves.  Unlike the
 * outlier filters it is IDEMPOTENT: whole components go, no edge joined them to a node that stays, so every other component keeps its nodes,
 * its size and its verdict (its label's VALUE may drop with the row numbers), and a second call with the same arguments removes nothing.
 *
 * cell is the cell of the queries' index, which is built at that cell where needed; a later query at another cell rebuilds it, as after
 * ef_set_query_cell.  No result depends on it.  Defaults (ef_default_component_params): radius 0.03 m, cell 0.03 m, min_conf -1, min_size 50,
 * max_size 0 (no upper bound).
 *
 * EF_EINVAL, before any GPU work (the arguments are checked before the context, so with a NULL context ef_last_error(NULL) names what is wrong
 * with them): a NULL context, params, count or (ef_map_remove_components) result; radius or cell not finite and positive, or 1 / cell not
 * finite; radius / cell above EF_QUERY_MAX_RATIO; NaN min_conf; what outside its two values; max_rows > 0 with NULL rows; with among given,
 * everything ef_map_select refuses for a selection.
 * EF_ESTATE: the context's stream is being captured; with among given, what ef_map_select answers with EF_ESTATE.  ef_map_remove_components
 * only: a context created with close_loops = 1 (the erase's reason; the map is unchanged); the other calls work on such contexts. */
#define EF_COMPONENT_NONE 0xFFFFFFFFu   /* label of a row that is no node */
#define EF_COMPONENTS_REJECTED 0        /* the nodes of components below min_size or above max_size */
#define EF_COMPONENTS_ACCEPTED 1        /* every other node */
typedef struct ef_component_params {
  float radius; float cell; float min_conf;
  uint32_t min_size; uint32_t max_size;   /* max_size 0: no upper bound */
} ef_component_params;
typedef struct ef_component_result {
  uint32_t nodes, components, largest, rejected_rows, rejected_components, count_after, status;
} ef_component_result;
int ef_default_component_params(ef_ctx* ctx, ef_component_params* params);
int ef_map_components(ef_ctx* ctx, const ef_component_params* params, const ef_map_selection* among_or_null, uint32_t* label_or_null,
                      uint32_t* size_or_null, uint32_t max_rows, ef_component_result* result_or_null);
int ef_map_components_dev(ef_ctx* ctx, const ef_component_params* params, const ef_map_selection* among_or_null, uint32_t* label_dev_or_null,
                          uint32_t* size_dev_or_null, uint32_t max_rows, ef_component_result* result_dev_or_null);
int ef_map_components_select(ef_ctx* ctx, const ef_component_params* params, const ef_map_selection* among_or_null, int what, uint32_t* rows,
                             uint32_t max_rows, uint32_t* count, ef_component_result* result_or_null);
int ef_map_components_select_dev(ef_ctx* ctx, const ef_component_params* params, const ef_map_selection* among_or_null, int what,
                                 uint32_t* rows_dev, uint32_t max_rows, uint32_t* count_dev, ef_component_result* result_dev_or_null);
int ef_map_remove_components(ef_ctx* ctx, const ef_component_params* params, const ef_map_selection* among_or_null, ef_component_result* result);

/* ---- Segment the map into planes (the sequential RANSAC plane segmentation of point-cloud toolkits).  A reconstructed room is one connected
 * component until its floor and walls are taken out; this finds them, lists them, and removes them, so that ef_map_components then separates
 * the objects that stood on the floor.  Off until first used: no plane call, nothing allocated, nothing run, and no frame kernel knows of it.
 *
 * Up to max_planes ROUNDS k = 0, 1, ...; each finds one plane n.p + d = 0 among the participants that no earlier round claimed.  Everything
 * below is specified completely: all f32 arithmetic rounds once per operation, without contraction, in the written order; square roots and
 * quotients are the correctly rounded IEEE ones.  Every decisive quantity is an integer, and the results are the same bits on every run.
 *
 * NODES are the components' (see above): the rows selected by among (every row with among NULL) that have a finite position and
 * conf > min_conf; their number is result.nodes.  The PARTICIPANTS of round k are the nodes that rounds 0 .. k-1 did not label, in ascending
 * row order; M is their number, and participant i is the i-th of them.
 *
 * SAMPLING.  h32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 on uint32.  base = h32(seed + 0x9E3779B9 * (k + 1)).
 * Sample j in {0, 1, 2} of hypothesis h in [0, hypotheses) is participant i = ((uint64)h32(base ^ (3 h + j)) * M) >> 32.
 *
 * HYPOTHESIS.  From the three sampled positions a, b, c: u = b - a, v = c - a, cr = u x v with cr.x = u.y * v.z - u.z * v.y and so on,
 * l2 = (cr.x * cr.x + cr.y * cr.y) + cr.z * cr.z.  The hypothesis is INVALID if two of its indices coincide, or if l2 is not finite or not > 0.
 * Otherwise n = cr / sqrt(l2) (per component) and d = -((n.x * a.x + n.y * a.y) + n.z * a.z).  With an axis mode on, t = (n.x * axis.x +
 * n.y * axis.y) + n.z * axis.z; if t < 0, n and d are negated; the hypothesis is invalid unless |t| >= axis_bound (EF_PLANE_AXIS_NORMAL) or
 * |t| <= axis_bound (EF_PLANE_AXIS_INPLANE).
 *
 * SCORE.  e = ((n.x * p.x + n.y * p.y) + n.z * p.z) + d.  A participant is an INLIER of a plane iff |e| <= distance and, with normal_cos > 0,
 * also |(n.x * m.x + n.y * m.y) + n.z * m.z| >= normal_cos for its stored normal m.  A NaN fails either test.  An invalid hypothesis scores 0.
 * The WINNER has the greatest number of inliers, ties to the lowest h.  If M is 0, or the winner's count is 0 or below min_inliers, the
 * extraction ends and this round finds no plane.
 *
 * REFINEMENT (refine = 1 and the winner's count m >= 3).  With the anchor a = the winner's first sample and q = (double)p - (double)a per inlier,
 * nine sums are taken in double: q.x, q.y, q.z, and q_i * q_j for xx, xy, xz, yy, yz, zz.  Each is summed BY MAP ROW in the order of "Remove
 * outlier surfels": lane j of EF_OUTLIER_SUM_LANES adds the rows j, j + P, j + 2P, ... from +0.0, a row that is no inlier adding +0.0, then
 * twelve rounds of a[i] = a[2i] + a[2i+1].  mean = S1 / m, C_ij = S2_ij / m - mean_i * mean_j; a cyclic Jacobi eigen-decomposition of C with a
 * fixed number of sweeps in plain double (csrc/ef_plane_fit.hpp is the definition); the normal is the unit eigenvector of the smallest
 * eigenvalue lambda (ties: the lowest index), flipped so that its double dot product with the hypothesis's normal is >= 0;
 * d = -(n . (a + mean)); both are rounded to f32, thickness = (float)sqrt(max(lambda, 0)) (the RMS distance of the inliers from the plane).
 * If anything along the way is not finite, the hypothesis's plane stays.  Without refinement the FINAL plane is the hypothesis's, thickness 0.
 *
 * LABELLING.  The participants of round k that are inliers of the FINAL plane get plane[row] = k; inliers is their number.  Every other row
 * keeps EF_PLANE_NONE.
 *
 * ef_plane_model: the final plane, its inliers, the winning hypothesis's count (sampled_inliers) and index, the round's valid hypotheses and
 * participants, the thickness.  ef_plane_result: nodes; planes = the rounds that found one; on_rows = the labelled rows; off_rows = nodes -
 * on_rows; count_after = the map count minus the EF_PLANES_ON rows of `which` (ef_map_planes: of all planes).
 *
 * ef_map_planes changes nothing.  It writes plane[r] of the rows r < min(max_rows, map count) (plane may be NULL; entries past that are left
 * as they were), params->max_planes models (entries from result.planes on are all zero bytes) and the optional result.
 * ef_map_planes_select changes nothing.  what = EF_PLANES_ON: the rows labelled `which` (which = -1: labelled at all); EF_PLANES_OFF: every
 * OTHER node (which = -1: the nodes on no plane), so that for any `which` the two lists partition the nodes.  which < max_planes; a plane
 * that was not found has no rows.  The list has ef_map_select's conventions: the first min(max_rows, total) rows in ASCENDING order, *count =
 * total however small max_rows is, rows may be NULL with max_rows 0, entries past min(max_rows, total) are left as they were.  The _dev
 * variants take DEVICE pointers for the arrays, count, models and result and only enqueue on the context's stream (all rounds are enqueued
 * without a host wait), except for what the selection needs and except that they wait for the device once when the scratch grows.
 * ef_map_remove_planes removes the EF_PLANES_ON rows of `which` and leaves everything exactly as ef_map_erase_rows(that list) would: see "What
 * an erase leaves behind" above, with one more synchronisation.  result (HOST memory, required): as above for the map as it WAS; count_after
 * = the map count the call leaves.
 *
 * Defaults (ef_default_plane_params): distance 0.01 m, normal_cos 0, min_conf -1, hypotheses 1024, seed 0, max_planes 4, min_inliers 500,
 * refine 1, axis_mode EF_PLANE_AXIS_OFF, axis (0, 0, 1), axis_bound 0.95.
 *
 * EF_EINVAL, before any GPU work (the arguments are checked before the context, so with a NULL context ef_last_error(NULL) names what is wrong
 * with them): a NULL context, params, count or (ef_map_remove_planes) result; distance not finite and positive; normal_cos or axis_bound
 * outside [0, 1] or NaN; NaN min_conf; hypotheses outside 1 .. EF_PLANE_MAX_HYPOTHESES; max_planes outside 1 .. EF_PLANE_MAX_PLANES; refine
 * > 1; axis_mode outside its three values; with an axis mode on, an axis whose f32 squared norm (x * x + y * y) + z * z is outside
 * [0.99, 1.01] (it is used as given, not normalised); what outside its two values; which outside -1 .. max_planes - 1; max_rows > 0 with NULL
 * rows; with among given, everything ef_map_select refuses for a selection.
 * EF_ESTATE: the context's stream is being captured; with among given, what ef_map_select answers with EF_ESTATE.  ef_map_remove_planes only:
 * a context created with close_loops = 1 (the erase's reason; the map is unchanged); the other calls work on such contexts. */
#define EF_PLANE_NONE 0xFFFFFFFFu      /* plane[] of a row that lies on no found plane */
#define EF_PLANE_MAX_PLANES 16
#define EF_PLANE_MAX_HYPOTHESES 4096
#define EF_PLANE_AXIS_OFF 0            /* no constraint */
#define EF_PLANE_AXIS_NORMAL 1         /* |n . axis| >= axis_bound: planes perpendicular to axis (a floor, axis = up) */
#define EF_PLANE_AXIS_INPLANE 2        /* |n . axis| <= axis_bound: planes parallel to axis (walls) */
#define EF_PLANES_ON 0                 /* rows that lie on a found plane */
#define EF_PLANES_OFF 1                /* participants that lie on none */
typedef struct ef_plane_params {
  float distance;         /* inlier iff |n.p + d| <= distance */
  float normal_cos;       /* > 0: also |n . surfel normal| >= normal_cos; 0: off */
  float min_conf;         /* as ef_component_params */
  uint32_t hypotheses;    /* H per round, 1 .. EF_PLANE_MAX_HYPOTHESES */
  uint32_t seed;
  uint32_t max_planes;    /* 1 .. EF_PLANE_MAX_PLANES */
  uint32_t min_inliers;   /* a round whose best hypothesis has fewer ends the extraction */
  uint32_t refine;        /* 0 / 1: least-squares plane through the winner's inliers */
  uint32_t axis_mode;     /* EF_PLANE_AXIS_* */
  float axis[3];          /* used as given; must be unit (see EF_EINVAL) */
  float axis_bound;
} ef_plane_params;
typedef struct ef_plane_model {
  float normal[3]; float d;     /* n.p + d = 0 */
  uint32_t inliers;             /* rows labelled with this plane (final plane) */
  uint32_t sampled_inliers;     /* the winning hypothesis's count */
  uint32_t hypothesis;          /* its index h */
  uint32_t valid_hypotheses;
  uint32_t participants;        /* M of this round */
  float thickness;              /* refine: (float)sqrt(max(lambda_min, 0)); else 0 */
} ef_plane_model;
typedef struct ef_plane_result {
  uint32_t nodes, planes, on_rows, off_rows, count_after;
} ef_plane_result;
int ef_default_plane_params(ef_ctx* ctx, ef_plane_params* params);
int ef_map_planes(ef_ctx* ctx, const ef_plane_params* params, const ef_map_selection* among_or_null, uint32_t* plane_or_null, uint32_t max_rows,
                  ef_plane_model* models_or_null, ef_plane_result* result_or_null);
int ef_map_planes_dev(ef_ctx* ctx, const ef_plane_params* params, const ef_map_selection* among_or_null, uint32_t* plane_dev_or_null,
                      uint32_t max_rows, ef_plane_model* models_dev_or_null, ef_plane_result* result_dev_or_null);
int ef_map_planes_select(ef_ctx* ctx, const ef_plane_params* params, const ef_map_selection* among_or_null, int what, int which, uint32_t* rows,
                         uint32_t max_rows, uint32_t* count, ef_plane_model* models_or_null, ef_plane_result* result_or_null);
int ef_map_planes_select_dev(ef_ctx* ctx, const ef_plane_params* params, const ef_map_selection* among_or_null, int what, int which,
                             uint32_t* rows_dev, uint32_t max_rows, uint32_t* count_dev, ef_plane_model* models_dev_or_null,
                             ef_plane_result* result_dev_or_null);
int ef_map_remove_planes(ef_ctx* ctx, const ef_plane_params* params, const ef_map_selection* among_or_null, int which,
                         ef_plane_model* models_or_null, ef_plane_result* result);

/* ---- Estimate normals, curvature and spacing from the map's neighbourhoods (the PCA normal estimation of point-cloud toolkits).  Every other
 * map tool takes a surfel's normal and radius as given, and the only producer of normals is a depth frame.  This derives them from the positions
 * the map holds: for a cloud that came without normals (inserted with a zero normal and a placeholder radius), for a map whose stored normals
 * no longer describe the geometry after fuse, thin, carve or a merged session, and for the per-surfel surface variation that region growing,
 * edge extraction and smoothness-weighted thinning start from.  Off until first used: no normal call, nothing allocated, nothing run, and no
 * frame kernel knows of it.
 *
 * "Row", the layout of a surfel (position = floats 0 .. 2, confidence = float 3, normal = floats 8 .. 10, radius = float 11), d2, the rule
 * "t is ELIGIBLE for q iff conf_t > min_conf and d2 <= r2" with r2 = radius * radius computed once in f32 on the host, the PARTICIPANTS (among
 * NULL: every row with a finite position; else the rows the selection selects that have a finite position) and the NEIGHBOURS of a participant
 * (all rows t != s eligible for p_s whether or not t participates, self excluded by ROW, ordered by (d2, row) ascending, count_s = the number
 * of ALL of them) are exactly those of the section "Remove outlier surfels".  All f32 arithmetic rounds once per operation, without
 * contraction, in the written order; so does all double arithmetic.
 *
 * For a participant s, with k in 3 .. 16:
 *
 * NEIGHBOURHOOD.  c = min(count_s, k).  The USED neighbours are the first c in that order, t_1 .. t_c, with d2_1 .. d2_c.
 *
 * SPACING.  spacing_s = (((sqrt(d2_1) + sqrt(d2_2)) + ...) + sqrt(d2_c)) / (float)c, summed in neighbour order; every square root and the
 * quotient are the CORRECTLY ROUNDED f32 operations.  +inf if c = 0.  It equals mean_dist of ef_map_neighbor_stats whenever count_s >= k.
 *
 * SPARSE.  Row s is SPARSE iff count_s < (uint32_t)min_neighbors, with min_neighbors in 2 .. k.  A sparse row gets no estimate.
 *
 * MOMENTS, in double, in neighbour order.  q_j = ((double)x_j - (double)x_s, (double)y_j - (double)y_s, (double)z_j - (double)z_s) for
 * j = 1 .. c, from the f32 positions of rows t_j and s.  S[0..2] = the sums of q.x, q.y, q.z; S[3..8] = the sums of q.x * q.x, q.x * q.y,
 * q.x * q.z, q.y * q.y, q.y * q.z, q.z * q.z.  Each product is rounded once and then added to a running sum that starts at +0.0, j ascending.
 * m = c + 1: the row itself is a member of its neighbourhood and contributes exact zeros.  The anchor is the row's own position, which keeps
 * the covariance's cancellation small at any distance from the origin.
 *
 * EIGEN-DECOMPOSITION.  From S and m on, csrc/ef_plane_fit.hpp is the definition (its normal_fit; the part up to the diagonalised matrix is the
 * one ef_map_planes' refinement uses): mean = S[0..2] / m, C_ij = S2_ij / m - mean_i * mean_j, the cyclic Jacobi iteration with its fixed
 * number of sweeps over the pairs (0,1), (0,2), (1,2).  l_0, l_1, l_2 are the diagonal entries it leaves, the columns of V the eigenvectors.
 * The smallest l_i is chosen by "l_1 < l_0", then "l_2 < the smaller" (ties: the lowest index); its eigenvector is divided by its length
 * sqrt((x * x + y * y) + z * z).  The fit GIVES UP if an entry of C, a diagonal entry, the length or a component of the normal is not finite,
 * or the length is not > 0.
 *
 * ORIENTATION.  The unit vector n is negated iff (n.x * (double)hn.x + n.y * (double)hn.y) + n.z * (double)hn.z < 0 for the hint hn (f32):
 *   EF_NORMALS_KEEP_SIDE   hn = the row's stored normal.  A zero or NaN stored normal, or one exactly perpendicular to n, flips nothing.
 *   EF_NORMALS_VIEWPOINT   hn = side * (v - p_s), each component one f32 subtraction and one (exact) product with side = +1 or -1.  side = +1
 *                          orients the normals towards the viewpoint v, side = -1 away from it.  -1 is the map's own convention (a surface
 *                          seen head-on has the normal +z in the camera, Core/Shaders/geometry.glsl:59) and the default.  A surfel at the
 *                          viewpoint flips nothing.
 * The estimate is (float)n per component.  An estimate whose sign was turned is FLIPPED.
 *
 * CURVATURE (surface variation).  e_i = l_i > 0 ? l_i : 0;  sum = (e_0 + e_1) + e_2;  emin = the clamped chosen eigenvalue;
 * curvature = sum > 0 ? (float)(emin / sum) : 0.  It lies in [0, 1/3]: 0 on a plane, 1/3 for an isotropic blob.
 *
 * DEGENERATE.  A participant that is not SPARSE is DEGENERATE iff the fit gives up or !(emid > (double)line_ratio * emax), where
 * lo = e_1 < e_0 ? e_1 : e_0, hi = e_1 < e_0 ? e_0 : e_1, emax = e_2 > hi ? e_2 : hi, emid = e_2 > hi ? hi : (e_2 < lo ? lo : e_2): a
 * neighbourhood that is a line or a point has no normal.  The eigenvalues are variances: line_ratio 1e-4 means "narrower than 1 % of its
 * length".  Everything is compared in double on values that are the same bits wherever they are computed.  Every other participant that is not
 * SPARSE is ESTIMATED.
 *
 * STATUS, one byte per row: EF_NORMAL_NONE (the row takes no part), EF_NORMAL_ESTIMATED, EF_NORMAL_SPARSE, EF_NORMAL_DEGENERATE.
 * OUTPUTS by row: normal[3] = the estimate, (0, 0, 0) unless ESTIMATED; curvature, 0 unless ESTIMATED; spacing, +inf for NONE (and for a
 * participant without a neighbour); count = count_s, 0 for NONE; status.
 *
 * ef_map_normals changes nothing.  It writes the five arrays for the rows r < min(max_rows, map count) (normals3 is [rows][3]; every array may
 * be NULL; entries past that are left as they were).  ef_map_normals_select changes nothing.  what = EF_NORMAL_ESTIMATED, EF_NORMAL_SPARSE or
 * EF_NORMAL_DEGENERATE (the rows of that status), EF_NORMALS_CURVED (ESTIMATED and curvature > max_curvature, compared in f32) or
 * EF_NORMALS_FLAT (ESTIMATED and not CURVED).  The list has ef_map_select's conventions: the first min(max_rows, total) rows in ASCENDING order,
 * *count = total however small max_rows is, rows may be NULL with max_rows 0, entries past min(max_rows, total) are left as they were; it is
 * what ef_map_erase_rows and ef_map_gather take.  result (optional): participants, estimated, sparse, degenerate, flipped (the FLIPPED
 * estimates), listed = total.  The _dev variants take DEVICE pointers for the arrays, count and result and only enqueue on the context's stream,
 * except for what the selection needs (ID numbering, label alignment, the count after a call that can change the map) and except that they
 * wait for the device once when the index has to be rebuilt or the scratch grows.
 *
 * ef_map_reestimate_normals is the write-back.  For every ESTIMATED row it writes floats 8 .. 10 = the estimate and, with set_radius != 0,
 * float 11 = radius_scale * spacing (one f32 product).  Every other word of every row keeps its bits (position, confidence, colour, the ID
 * lane, both times), and a row that is not ESTIMATED keeps everything.  result (HOST memory, required): as above, listed = the rows written.
 * What a re-estimate leaves behind:
 *   the map       as described, the count unchanged;
 *   IDs           with IDs on, the rows created since the last ID-consuming call are numbered before the write, as every edit does; no ID changes;
 *   the context   the state that ef_map_upload of the edited rows followed by ef_restore_state (tick, ef_get_pose_qt, the last processed frame)
 *                 would leave: tick, pose, trajectory, last frame and tracking statistics are unchanged, and if ef_process_frame* or
 *                 ef_restore_state has run on the context the model prediction is renewed from the edited map at the current pose.  On a context
 *                 whose map was only uploaded, only the map changes;
 *   the index     of the queries and the registration counts as stale, by the rule of every edit, and is rebuilt by their next call;
 *   labels        untouched: no row moved, every row keeps its C floats;
 *   the shadow buffer of ef_set_reference_download is left as it is.
 * The call synchronises before and after, like the insert.  A call that estimates nothing is valid and still leaves that state.  In
 * EF_NORMALS_KEEP_SIDE mode without set_radius it is IDEMPOTENT bit for bit: positions do not change, so a second call forms the same n, and
 * the stored normal it is compared with is (float)n or (float)-n of the first call, whose double dot product with that n cannot be negative.
 * (With set_radius too: the radius takes no part in the estimate.)
 *
 * cell is the cell of the queries' index, which is built at that cell where needed; a later query at another cell rebuilds it, as after
 * ef_set_query_cell.  No result depends on it.  Defaults (ef_default_normal_params): radius 0.03 m, cell 0.03 m (the outlier filter's measured
 * choice for the same walk), min_conf -1, k 12, min_neighbors 5, EF_NORMALS_KEEP_SIDE, side -1, viewpoint (0, 0, 0), line_ratio 1e-4 (a
 * definition, see above, not a measurement), max_curvature 0.05 (likewise), set_radius 0, radius_scale 1.
 *
 * Not provided: a method of the C++ shim; the write-back on loop-closing contexts; normals of a point set that is not in the map (it needs an
 * index over that set: insert the set first, see accuracy.insert_cloud).  (Region growing on these estimates is the next section; smoothing of
 * the positions by moving least squares is the section "Smooth the map's positions" after it.)
 *
 * EF_EINVAL, before any GPU work (the arguments are checked before the context, so with a NULL context ef_last_error(NULL) names what is wrong
 * with them): a NULL context, params, count or (ef_map_reestimate_normals) result; radius or cell not finite and positive, or 1 / cell not
 * finite; radius / cell above EF_QUERY_MAX_RATIO; NaN min_conf; k outside 3 .. 16; min_neighbors outside 2 .. k; orientation outside its two
 * values; side not +1 or -1; in EF_NORMALS_VIEWPOINT mode a non-finite viewpoint coordinate; NaN or negative line_ratio, max_curvature or
 * radius_scale; what outside its five values; max_rows > 0 with NULL rows; with among given, everything ef_map_select refuses for a selection.
 * EF_ESTATE: the context's stream is being captured; with among given, what ef_map_select answers with EF_ESTATE.
 * ef_map_reestimate_normals only: a context created with close_loops = 1 (the erase's reason; the map is unchanged); the other calls work on
 * such contexts. */
#define EF_NORMALS_KEEP_SIDE 0     /* orientation: the side of the row's stored normal */
#define EF_NORMALS_VIEWPOINT 1     /* orientation: towards (side +1) or away from (side -1) params.viewpoint */
#define EF_NORMAL_NONE       0     /* status: the row takes no part */
#define EF_NORMAL_ESTIMATED  1     /* status, and `what`: the rows with an estimate */
#define EF_NORMAL_SPARSE     2     /* status, and `what`: fewer than min_neighbors neighbours */
#define EF_NORMAL_DEGENERATE 3     /* status, and `what`: a line or a point */
#define EF_NORMALS_CURVED    4     /* `what`: ESTIMATED and curvature > max_curvature */
#define EF_NORMALS_FLAT      5     /* `what`: ESTIMATED and not CURVED */
typedef struct ef_normal_params {
  float radius; float cell; float min_conf;
  int k;                  /* neighbours used, 3 .. 16 */
  int min_neighbors;      /* 2 .. k */
  int orientation;        /* EF_NORMALS_KEEP_SIDE / EF_NORMALS_VIEWPOINT */
  int side;               /* VIEWPOINT: +1 towards, -1 away */
  float viewpoint[3];
  float line_ratio;
  float max_curvature;    /* ef_map_normals_select: EF_NORMALS_CURVED / EF_NORMALS_FLAT */
  int set_radius;         /* ef_map_reestimate_normals: also write the radius */
  float radius_scale;
} ef_normal_params;
typedef struct ef_normal_result {
  uint32_t participants, estimated, sparse, degenerate, flipped, listed;
} ef_normal_result;
int ef_default_normal_params(ef_ctx* ctx, ef_normal_params* params);
int ef_map_normals(ef_ctx* ctx, const ef_normal_params* params, const ef_map_selection* among_or_null, float* normals3_or_null,
                   float* curvature_or_null, float* spacing_or_null, uint32_t* count_or_null, uint8_t* status_or_null, uint32_t max_rows);
int ef_map_normals_dev(ef_ctx* ctx, const ef_normal_params* params, const ef_map_selection* among_or_null, float* normals3_dev_or_null,
                       float* curvature_dev_or_null, float* spacing_dev_or_null, uint32_t* count_dev_or_null, uint8_t* status_dev_or_null,
                       uint32_t max_rows);
int ef_map_normals_select(ef_ctx* ctx, const ef_normal_params* params, const ef_map_selection* among_or_null, int what, uint32_t* rows,
                          uint32_t max_rows, uint32_t* count, ef_normal_result* result_or_null);
int ef_map_normals_select_dev(ef_ctx* ctx, const ef_normal_params* params, const ef_map_selection* among_or_null, int what, uint32_t* rows_dev,
                              uint32_t max_rows, uint32_t* count_dev, ef_normal_result* result_dev_or_null);
int ef_map_reestimate_normals(ef_ctx* ctx, const ef_normal_params* params, const ef_map_selection* among_or_null, ef_normal_result* result);

/* ---- Segment the map into smooth regions (the smoothness-constrained region growing of point-cloud toolkits).  ef_map_components separates
 * objects only once they are detached, and ef_map_planes takes out what is flat; this splits a CONNECTED map along its creases: the faces of a
 * box, a cylinder from the table it stands on, the two sides of a thin wall.  Textbook region growing is sequential, and its result depends on
 * the order of its seeds.  The formulation here is order-free, a function of the graph alone, whatever order anything was evaluated in: the
 * low-curvature surfels (CORES) form regions as the connected components of "close and smooth", and the crease surfels (BORDERS) are attached to
 * the region of their nearest smooth core and never bridge two regions.  Off until first used: no region call, nothing allocated, nothing run,
 * and no frame kernel knows of it.
 *
 * "Row", the layout of a surfel, d2 (symmetric in f32), r2 = radius * radius computed once in f32 on the host, the PARTICIPANTS, the rule
 * "ELIGIBLE", the NEIGHBOURS of a participant and the whole estimate (NEIGHBOURHOOD, MOMENTS, EIGEN-DECOMPOSITION, ORIENTATION, CURVATURE,
 * SPARSE, DEGENERATE, STATUS) are exactly those of the sections "Connected components of the map" and "Estimate normals, curvature and spacing
 * from the map's neighbourhoods".  All f32 arithmetic rounds once per operation, without contraction, in the written order.
 *
 * ESTIMATE.  Every participant gets the estimate of ef_map_normals with this call's radius, cell, min_conf, k, min_neighbors and line_ratio and
 * the orientation EF_NORMALS_KEEP_SIDE.  The neighbours of the estimate are the normals' neighbours: all rows eligible for the participant,
 * whether they participate or not.
 *
 * NODE.  A participant with conf > min_conf (a NaN confidence compares false) whose status is EF_NORMAL_ESTIMATED.  SPARSE, DEGENERATE and
 * non-participating rows are not nodes: they carry no edge and attach nowhere.
 *
 * THE NORMAL n_s of a node.  normal_source = EF_REGIONS_ESTIMATED: the (float)n estimate.  EF_REGIONS_STORED: floats 8 .. 10 of the row as they
 * are, not renormalised (the curvature, and with it core / border, is the estimate's in both cases).
 *
 * SMOOTH(s, t).  dot = (n_s.x * n_t.x + n_s.y * n_t.y) + n_s.z * n_t.z in f32.  The rule is dot >= min_normal_cos; with two_sided != 0 it is
 * fabsf(dot) >= min_normal_cos.  A NaN compares false (a NaN stored normal is smooth with nothing; a zero one only for min_normal_cos <= 0).
 * The products commute, so dot is the same bits from either end and the graph is undirected by construction, like d2.  Signed is the default:
 * a map's normals are oriented by the sensor, and the two sides of a thin wall must not merge.
 *
 * CORE / BORDER.  A node is a CORE iff curvature <= max_curvature, compared in f32.  Every other node is a BORDER.
 *
 * EDGE.  Two distinct cores s != t are joined iff d2(p_s, p_t) <= r2 and SMOOTH(s, t).  REGIONS are the connected components of the cores under
 * these edges.  label = the SMALLEST CORE ROW of the region.  Smoothness is pairwise, between neighbours, never against a seed: a cylinder's
 * side is one region although its normals turn all the way round.
 *
 * ATTACH (attach_borders != 0).  For a border b take the cores t with d2(p_b, p_t) <= r2 and SMOOTH(b, t), ordered by (d2, row) ascending.  b
 * joins the region of the first of them: label[b] = that region's label.  If there is none, or if attach_borders == 0, the border is
 * UNASSIGNED and its label is EF_REGION_NONE.  A border never carries an edge: two regions that touch only through borders stay two.
 *
 * SIZE.  size[s] = the cores plus the attached borders of the region of s.  A row without a region (no node, or UNASSIGNED) has
 * label = EF_REGION_NONE and size = 0.  kind[s] = EF_REGION_KIND_CORE, EF_REGION_KIND_BORDER, or EF_REGION_KIND_NONE for a row that is no node.
 *
 * VERDICT.  A node with a region is REJECTED iff size < min_size or (max_size != 0 and size > max_size), otherwise ACCEPTED; all rows of a
 * region share the verdict.  A row without a region is neither.
 *
 * THE FOUR LISTS (what).  EF_REGIONS_REJECTED, EF_REGIONS_ACCEPTED: the nodes with that verdict.  EF_REGIONS_UNASSIGNED: the borders without a
 * region.  EF_REGIONS_BORDERS: every border node, attached or not: the crease lines.
 *
 * ef_region_result: nodes; cores; borders (nodes = cores + borders); attached and unassigned (borders = attached + unassigned); regions = the
 * number of core rows r with label[r] == r; largest = the greatest size (0 without regions); rejected_rows and rejected_regions = the rejected
 * nodes and their regions; listed = the number of rows of the list `what` (ef_map_regions, which takes no what: of EF_REGIONS_REJECTED);
 * count_after = the map count minus listed, which is the count ef_map_remove_regions with that what leaves; status = 0, or non-zero if one of
 * the device loops ran into its step bound, which no input can cause (the host variants then return EF_EHIP and ef_map_remove_regions removes
 * nothing; the _dev variants can only report it here).  But for listed and count_after the result does not depend on what.
 *
 * ef_map_regions changes nothing.  It writes label[r], size[r] and kind[r] of the rows r < min(max_rows, map count) (each array may be NULL;
 * entries past that are left as they were) and the optional result.  ef_map_regions_select changes nothing.  It writes the list `what` with
 * ef_map_select's conventions: the first min(max_rows, total) rows in ASCENDING order, *count = total however small max_rows is, rows may be
 * NULL with max_rows 0, entries past min(max_rows, total) are left as they were.  The list is what ef_map_erase_rows and ef_map_gather take.
 * The _dev variants take DEVICE pointers for the arrays, count and result and only enqueue on the context's stream, except for what the
 * selection needs (ID numbering, label alignment, the count after a call that can change the map) and except that they wait for the device once
 * when the index has to be rebuilt or the scratch grows.
 *
 * ef_map_remove_regions removes the rows of the list `what` and leaves everything exactly as ef_map_erase_rows(that list) would: see "What an
 * erase leaves behind" above, with one more synchronisation (the result is read before a row changes).  result (HOST memory, required): as
 * above for the map as it WAS, listed = the rows removed, count_after = the map count the call leaves.  Unlike ef_map_remove_components it is
 * NOT IDEMPOTENT: a removed row was a neighbour of rows that stay, so their neighbourhoods, and with them their normals, curvatures, kinds and
 * edges, are different in a second call, which may list rows again.
 *
 * cell is the cell of the queries' index, which is built at that cell where needed; a later query at another cell rebuilds it, as after
 * ef_set_query_cell.  No result depends on it.  Defaults (ef_default_region_params): radius 0.03 m, cell 0.03 m, min_conf -1, k 12,
 * min_neighbors 5, line_ratio 1e-4, EF_REGIONS_ESTIMATED, two_sided 0, min_normal_cos 0.9659258 (the cosine of 15 degrees: a definition, not
 * a measurement), max_curvature 0.05 (the normals' default), attach_borders 1, min_size 50, max_size 0 (no upper bound).
 *
 * Not provided: a model per region (a plane, a cylinder: ef_map_planes fits planes); writing the region labels into the label table of
 * ef_enable_labels; a method of the C++ shim.
 *
 * EF_EINVAL, before any GPU work (the arguments are checked before the context, so with a NULL context ef_last_error(NULL) names what is wrong
 * with them): a NULL context, params, count or (ef_map_remove_regions) result; radius or cell not finite and positive, or 1 / cell not finite;
 * radius / cell above EF_QUERY_MAX_RATIO; NaN min_conf; k outside 3 .. 16; min_neighbors outside 2 .. k; NaN or negative line_ratio or
 * max_curvature; NaN min_normal_cos; normal_source outside its two values; what outside its four values; max_rows > 0 with NULL rows; with
 * among given, everything ef_map_select refuses for a selection.
 * EF_ESTATE: the context's stream is being captured; with among given, what ef_map_select answers with EF_ESTATE.  ef_map_remove_regions only:
 * a context created with close_loops = 1 (the erase's reason; the map is unchanged); the other calls work on such contexts. */
#define EF_REGION_NONE 0xFFFFFFFFu   /* label of a row without a region */
#define EF_REGION_KIND_NONE   0      /* kind: the row is no node */
#define EF_REGION_KIND_CORE   1      /* kind: a node with curvature <= max_curvature */
#define EF_REGION_KIND_BORDER 2      /* kind: every other node */
#define EF_REGIONS_ESTIMATED 0       /* normal_source: the estimate */
#define EF_REGIONS_STORED    1       /* normal_source: the row's stored normal */
#define EF_REGIONS_REJECTED   0      /* what: the nodes of regions below min_size or above max_size */
#define EF_REGIONS_ACCEPTED   1      /* what: every other node with a region */
#define EF_REGIONS_UNASSIGNED 2      /* what: the borders without a region */
#define EF_REGIONS_BORDERS    3      /* what: every border node */
typedef struct ef_region_params {
  float radius; float cell; float min_conf;
  int k;                  /* the estimate: neighbours used, 3 .. 16 */
  int min_neighbors;      /* the estimate: 2 .. k */
  float line_ratio;       /* the estimate */
  int normal_source;      /* EF_REGIONS_ESTIMATED / EF_REGIONS_STORED */
  int two_sided;          /* non-zero: |dot| is compared */
  float min_normal_cos;
  float max_curvature;
  int attach_borders;     /* non-zero: borders join the region of their nearest smooth core */
  uint32_t min_size; uint32_t max_size;   /* max_size 0: no upper bound */
} ef_region_params;
typedef struct ef_region_result {
  uint32_t nodes, cores, borders, attached, unassigned, regions, largest, rejected_rows, rejected_regions, listed, count_after, status;
} ef_region_result;
int ef_default_region_params(ef_ctx* ctx, ef_region_params* params);
int ef_map_regions(ef_ctx* ctx, const ef_region_params* params, const ef_map_selection* among_or_null, uint32_t* label_or_null,
                   uint32_t* size_or_null, uint8_t* kind_or_null, uint32_t max_rows, ef_region_result* result_or_null);
int ef_map_regions_dev(ef_ctx* ctx, const ef_region_params* params, const ef_map_selection* among_or_null, uint32_t* label_dev_or_null,
                       uint32_t* size_dev_or_null, uint8_t* kind_dev_or_null, uint32_t max_rows, ef_region_result* result_dev_or_null);
int ef_map_regions_select(ef_ctx* ctx, const ef_region_params* params, const ef_map_selection* among_or_null, int what, uint32_t* rows,
                          uint32_t max_rows, uint32_t* count, ef_region_result* result_or_null);
int ef_map_regions_select_dev(ef_ctx* ctx, const ef_region_params* params, const ef_map_selection* among_or_null, int what, uint32_t* rows_dev,
                              uint32_t max_rows, uint32_t* count_dev, ef_region_result* result_dev_or_null);
int ef_map_remove_regions(ef_ctx* ctx, const ef_region_params* params, const ef_map_selection* among_or_null, int what, ef_region_result* result);

/* ---- Smooth the map's positions (the moving-least-squares projection of point-cloud toolkits, plane fits only).  The cleaning tools remove
 * surfels and the analysis tools read them; none reduces the noise in the positions themselves.  A merged second session, an inserted cloud
 * (accuracy.insert_cloud) or a thinned map keeps its sensor noise, and every later normal, plane or region estimate is computed on it.  This
 * fits a weighted plane to each surfel's neighbourhood and moves the surfel onto it, along the plane's normal only, several times if asked,
 * without leaving the device.  Off until first used: no smooth call, nothing allocated, nothing run, and no frame kernel knows of it.
 *
 * "Row", the layout of a surfel, d2 (the queries' expression: dx = q.x - p.x, ..., (dx * dx + dy * dy) + dz * dz in f32), r2 = radius * radius
 * computed once in f32 on the host, the PARTICIPANTS, the rule "ELIGIBLE", the NEIGHBOURS of a participant, count_s, c = min(count_s, k), the
 * USED neighbours t_1 .. t_c in (d2, row) order and SPARSE (count_s < (uint32_t)min_neighbors) are exactly those of the section "Estimate
 * normals, curvature and spacing from the map's neighbourhoods".  All f32 arithmetic rounds once per operation, without contraction, in the
 * written order; so does all double arithmetic.
 *
 * NEIGHBOURHOODS.  They are taken ONCE, from the map's own positions P^0, and stay fixed for the whole call: the same rows t_1 .. t_c in the
 * same order in every iteration, however far anything moves.  A row that does not participate and a SPARSE row never move; they still serve
 * as neighbours, at their fixed positions.
 *
 * ITERATION i = 1 .. iterations reads P^(i-1) and writes P^i, every row (nothing is updated in place: a row's fit never sees a position of the
 * same iteration).  For a participant s that is not SPARSE, with p = P^(i-1)_s:
 *   d2_j       = d2(p, P^(i-1)_{t_j}) in f32.  For i = 1 these are the list's own bits.
 *   WEIGHT     w_j, a double.  EF_SMOOTH_UNIFORM: w_j = 1.0.  EF_SMOOTH_COMPACT: u = 1.0 - (double)d2_j / (double)r2, then
 *              w_j = u > 0.0 ? u * u : 0.0: a neighbour that drifted past the radius counts for nothing, and a NaN takes 0.  With
 *              normal_gate != 0, after that: w_j = 0.0 unless dot >= min_normal_cos, where dot is SMOOTH's expression of the section "Segment
 *              the map into smooth regions" in f32, (n_s.x * n_t.x + n_s.y * n_t.y) + n_s.z * n_t.z, on the STORED normals (floats 8 .. 10) of
 *              rows s and t_j as the map holds them; they do not change during the call.  A NaN compares false: the weight is 0.
 *   DIFFERENCE q_j = ((double)x_{t_j} - (double)p.x, ...) per component, from the f32 positions of P^(i-1).
 *   SUMS       in double, j ascending.  a = w_j * q.x, b = w_j * q.y, g = w_j * q.z;  S[0..2] += a, b, g;  S[3..8] += a * q.x, a * q.y,
 *              a * q.z, b * q.y, b * q.z, g * q.z;  W = W + w_j.  Every product is rounded once and then added.  Every S starts at +0.0 and
 *              W at 1.0: the row itself is a member of its neighbourhood with the weight 1 and contributes exact zeros to S.  With
 *              EF_SMOOTH_UNIFORM and no gate these are the normals' S bit for bit, and W == (double)(c + 1).
 *   FIT        csrc/ef_plane_fit.hpp is the definition (its smooth_fit): the text of the normals' EIGEN-DECOMPOSITION with the divisor W in
 *              place of (double)m (mean = S[0..2] / W, C_ij = S2_ij / W - mean_i * mean_j); its "fewer than three members" test is on c + 1;
 *              then the normals' choice of the eigenvector, its normalisation and the ORIENTATION EF_NORMALS_KEEP_SIDE (the hint is the row's
 *              stored normal), the same finiteness checks, the CURVATURE and the DEGENERATE test with line_ratio.  The fit of the iteration
 *              is ESTIMATED, with the unit normal n and the mean in double and the curvature in f32, or it is not.
 *   PROJECTION only for an ESTIMATED fit.  t = (n.x * mean.x + n.y * mean.y) + n.z * mean.z: the signed distance from p to the fitted plane
 *              along n.  s = (double)strength * t.  If s > (double)max_shift then s = (double)max_shift, else if s < -(double)max_shift then
 *              s = -(double)max_shift; either sets the row's CLAMPED bit, which stays set for the rest of the call.  p'.x = (float)((double)p.x +
 *              s * n.x), likewise y and z.  If a component of p' is not finite, the row keeps p and this iteration's verdict is DEGENERATE (a
 *              CLAMPED bit the iteration set stays).  Otherwise P^i_s = p' and the verdict is SMOOTHED.
 *   OTHERWISE  a row whose fit is not ESTIMATED keeps p for this iteration, with the verdict DEGENERATE; a later iteration fits it again.
 * A surfel moves along its plane's normal only: the sampling pattern does not contract, and a flat region's border does not creep inwards as
 * it does under Laplacian smoothing.
 *
 * STATUS, one byte per row: EF_SMOOTH_NONE (the row takes no part), EF_SMOOTH_SPARSE, and for every other participant the LAST iteration's
 * verdict, EF_SMOOTH_SMOOTHED or EF_SMOOTH_DEGENERATE.
 * OUTPUTS by row after the last iteration I: position[3] = P^I, the map's own bits for a row that never moved; normal[3] = (float)n per
 * component and curvature of the last iteration's fit, zeros unless the status is SMOOTHED; shift = the CORRECTLY ROUNDED f32 square root of
 * d2(P^I_s, P^0_s) for a SMOOTHED or DEGENERATE row and 0 for every other row (NONE and SPARSE rows never move; a NONE row may have no finite
 * position to measure from); count = count_s, 0 for NONE; status.
 * RESULT: participants, smoothed, sparse, degenerate = the status counts (participants = their sum); clamped = the rows with the CLAMPED bit;
 * moved = the rows with shift > 0; largest_shift = the greatest shift (0 without any); listed (below).
 *
 * ef_map_smooth changes nothing.  It writes the six arrays for the rows r < min(max_rows, map count) (position3 and normal3 are [rows][3];
 * every array may be NULL; entries past that are left as they were) and the optional result with listed = 0.  ef_map_smooth_select changes
 * nothing.  what = EF_SMOOTH_SMOOTHED, EF_SMOOTH_SPARSE or EF_SMOOTH_DEGENERATE (the rows of that status), EF_SMOOTH_CLAMPED (the rows with
 * the CLAMPED bit) or EF_SMOOTH_SHIFTED (shift > shift_threshold, compared in f32).  The list has ef_map_select's conventions: the first
 * min(max_rows, total) rows in ASCENDING order, *count = total however small max_rows is, rows may be NULL with max_rows 0, entries past
 * min(max_rows, total) are left as they were; it is what ef_map_erase_rows and ef_map_gather take.  result (optional): as above, listed =
 * total.  The _dev variants take DEVICE pointers for the arrays, count and result and only enqueue on the context's stream, except for what
 * the selection needs (ID numbering, label alignment, the count after a call that can change the map) and except that they wait for the
 * device once when the index has to be rebuilt or the scratch grows.
 *
 * ef_map_smooth_apply is the write-back.  For every participant it writes floats 0 .. 2 = P^I (the same bits for a row that did not move)
 * and, with set_normal != 0, floats 8 .. 10 = the last iteration's normal for the rows whose status is SMOOTHED.  Every other word of every
 * row keeps its bits (confidence, colour, the ID lane, both times, the radius; the normal without set_normal), and a row that takes no part
 * keeps everything.  result (HOST memory, required): as above, listed = moved.  All counts are read back before a row is written.
 * What a write-back leaves behind:
 *   the map       as described, the count unchanged;
 *   IDs           with IDs on, the rows created since the last ID-consuming call are numbered before the write, as every edit does; no ID changes;
 *   the context   the state that ef_map_upload of the edited rows followed by ef_restore_state (tick, ef_get_pose_qt, the last processed frame)
 *                 would leave: tick, pose, trajectory, last frame and tracking statistics are unchanged, and if ef_process_frame* or
 *                 ef_restore_state has run on the context the model prediction is renewed from the edited map at the current pose.  On a context
 *                 whose map was only uploaded, only the map changes;
 *   the index     of the queries and the registration is stale, here in earnest (positions moved), and is rebuilt by their next call;
 *   labels        untouched: no row moved to another row, every row keeps its C floats;
 *   the shadow buffer of ef_set_reference_download is left as it is.
 * The call synchronises before and after, like the insert.  A call that moves nothing is valid and still leaves that state.  It is NOT
 * idempotent: a second call fits the moved positions.
 *
 * cell is the cell of the queries' index, which is built at that cell where needed; a later query at another cell rebuilds it, as after
 * ef_set_query_cell.  No result depends on it.  Defaults (ef_default_smooth_params): radius 0.03 m, cell 0.03 m, min_conf -1, k 12,
 * min_neighbors 5 (the normals' defaults), iterations 1, EF_SMOOTH_COMPACT, normal_gate 0, min_normal_cos 0.9, strength 1, max_shift =
 * radius, line_ratio 1e-4, set_normal 0, shift_threshold 0.  These defaults are definitions, not measurements.
 *
 * Not provided: polynomial surfaces (the fit is a plane); tangential (Laplacian) motion; upsampling; smoothing of colour or radius; a method
 * of the C++ shim; the write-back on loop-closing contexts.
 *
 * EF_EINVAL, before any GPU work (the arguments are checked before the context, so with a NULL context ef_last_error(NULL) names what is wrong
 * with them): a NULL context, params, count or (ef_map_smooth_apply) result; radius or cell not finite and positive, or 1 / cell not finite;
 * radius / cell above EF_QUERY_MAX_RATIO; NaN min_conf; k outside 3 .. 16; min_neighbors outside 2 .. k; iterations outside 1 .. 16;
 * weighting outside its two values; normal_gate not 0 or 1; NaN min_normal_cos; strength not in (0, 1]; max_shift not > 0 (+inf is allowed: no
 * bound); NaN or negative line_ratio or shift_threshold; what outside its five values; max_rows > 0 with NULL rows; with among given,
 * everything ef_map_select refuses for a selection.
 * EF_ESTATE: the context's stream is being captured; with among given, what ef_map_select answers with EF_ESTATE.  ef_map_smooth_apply only:
 * a context created with close_loops = 1 (the erase's reason; the map is unchanged); the other calls work on such contexts. */
#define EF_SMOOTH_UNIFORM    0     /* weighting: every used neighbour counts 1 */
#define EF_SMOOTH_COMPACT    1     /* weighting: (1 - d2 / r2)^2, 0 from the radius on */
#define EF_SMOOTH_NONE       0     /* status: the row takes no part */
#define EF_SMOOTH_SMOOTHED   1     /* status, and `what`: the last iteration moved the row onto its plane */
#define EF_SMOOTH_SPARSE     2     /* status, and `what`: fewer than min_neighbors neighbours */
#define EF_SMOOTH_DEGENERATE 3     /* status, and `what`: the last iteration found no plane */
#define EF_SMOOTH_CLAMPED    4     /* `what`: a step was cut at max_shift */
#define EF_SMOOTH_SHIFTED    5     /* `what`: shift > shift_threshold */
typedef struct ef_smooth_params {
  float radius; float cell; float min_conf;
  int k;                  /* neighbours used, 3 .. 16 */
  int min_neighbors;      /* 2 .. k */
  int iterations;         /* 1 .. 16 */
  int weighting;          /* EF_SMOOTH_UNIFORM / EF_SMOOTH_COMPACT */
  int normal_gate;        /* 1: a neighbour counts only if its stored normal agrees with the row's */
  float min_normal_cos;   /* the gate's bound */
  float strength;         /* the share of the distance to the plane a step covers, (0, 1] */
  float max_shift;        /* the longest step, > 0 (+inf: no bound) */
  float line_ratio;
  int set_normal;         /* ef_map_smooth_apply: also write the last iteration's normal */
  float shift_threshold;  /* ef_map_smooth_select: EF_SMOOTH_SHIFTED */
} ef_smooth_params;
typedef struct ef_smooth_result {
  uint32_t participants, smoothed, sparse, degenerate, clamped, moved, listed;
  float largest_shift;
} ef_smooth_result;
int ef_default_smooth_params(ef_ctx* ctx, ef_smooth_params* params);
int ef_map_smooth(ef_ctx* ctx, const ef_smooth_params* params, const ef_map_selection* among_or_null, float* position3_or_null,
                  float* normal3_or_null, float* curvature_or_null, float* shift_or_null, uint32_t* count_or_null, uint8_t* status_or_null,
                  uint32_t max_rows, ef_smooth_result* result_or_null);
int ef_map_smooth_dev(ef_ctx* ctx, const ef_smooth_params* params, const ef_map_selection* among_or_null, float* position3_dev_or_null,
                      float* normal3_dev_or_null, float* curvature_dev_or_null, float* shift_dev_or_null, uint32_t* count_dev_or_null,
                      uint8_t* status_dev_or_null, uint32_t max_rows, ef_smooth_result* result_dev_or_null);
int ef_map_smooth_select(ef_ctx* ctx, const ef_smooth_params* params, const ef_map_selection* among_or_null, int what, uint32_t* rows,
                         uint32_t max_rows, uint32_t* count, ef_smooth_result* result_or_null);
int ef_map_smooth_select_dev(ef_ctx* ctx, const ef_smooth_params* params, const ef_map_selection* among_or_null, int what, uint32_t* rows_dev,
                             uint32_t max_rows, uint32_t* count_dev, ef_smooth_result* result_dev_or_null);
int ef_map_smooth_apply(ef_ctx* ctx, const ef_smooth_params* params, const ef_map_selection* among_or_null, ef_smooth_result* result);

/* ---- Find the map's boundaries (the boundary estimation by the angle criterion of point-cloud toolkits).  The tools above clean, thin, carve,
 * label, segment, re-estimate and smooth a map; this says WHERE THE MAP ENDS: the rim of the scanned surface and the rims of the holes in it,
 * which are the frontiers a reconstruction looks at next and the places a merged or carved map is still missing.  A surfel is on the boundary
 * if, seen along its normal, its neighbours leave an angular gap wider than a threshold; the boundary surfels are strung into LOOPS.  Off until
 * first used: no boundary call, nothing allocated, nothing run, and no frame kernel knows of it.  It changes no map and takes no part in a frame.
 *
 * "Row", the layout of a surfel, d2, ELIGIBLE, the PARTICIPANTS (among), the NEIGHBOURS of a participant with their (d2, row) order, count_s,
 * c = min(count_s, k), the USED neighbours t_1 .. t_c and SPARSE (count_s < (uint32_t)min_neighbors) are exactly those of the section "Estimate
 * normals, curvature and spacing".  All double arithmetic rounds once per operation, in the written order, without contraction; |v| is exact.
 * From FRAME to GAP, csrc/ef_boundary_gap.hpp is the definition (its boundary_gap); what follows restates it.
 *
 * For a participant s that is not SPARSE, with the used neighbours in SLOTS 1 .. c in neighbour order:
 *
 * NORMAL m_s (three f32).
 *   EF_BOUNDARY_STORED      floats 8 .. 10 of the row as they are (any length).
 *   EF_BOUNDARY_ESTIMATED   the (float)n estimate of ef_map_normals with this call's radius, cell, min_conf, k, min_neighbors and line_ratio and
 *                           the orientation EF_NORMALS_KEEP_SIDE.  A row whose estimate is SPARSE or DEGENERATE has that status here.
 *
 * FRAME, in double.  a = ((double)m.x, (double)m.y, (double)m.z);  nn = (a.x * a.x + a.y * a.y) + a.z * a.z.  The row is DEGENERATE unless nn is
 * finite and > 0.  h = (a.x / sqrt(nn), a.y / sqrt(nn), a.z / sqrt(nn)) with the correctly rounded square root.  i0 = the index of the smallest
 * |h_i|, chosen by "|h_1| < |h_0|", then "|h_2| < the smaller" (ties: the lowest index); e = the unit vector of axis i0.  e1 = e x h and
 * e2 = h x e1, both by the one formula u x v = (u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x) with e's exact zeros and ones
 * as doubles (so a component of e1 may be either zero).  No further normalisation: |e1| = |e2| = sqrt(1 - h_i0^2) >= sqrt(2 / 3) up to
 * rounding, and the two axes scale every direction alike, which no angle sees.
 *
 * PROJECTION.  q_j = ((double)x_j - (double)x_s, (double)y_j - (double)y_s, (double)z_j - (double)z_s) from the f32 positions of rows t_j and s
 * (the q_j of the normals' MOMENTS).  x_j = (q.x * e1.x + q.y * e1.y) + q.z * e1.z;  y_j = (q.x * e2.x + q.y * e2.y) + q.z * e2.z.  The used
 * neighbour in slot j is a DIRECTION iff x_j and y_j are finite and |x_j| + |y_j| > 0.  m_s = the number of directions.  The row is DEGENERATE if
 * m_s = 0 (every used neighbour lies along the normal, or on the row itself).
 *
 * TURN(j, i) for the directions in slots j != i: a monotone measure in [0, 4] of the counter-clockwise angle from j to i that needs divisions
 * only (1 = 90 degrees, 2 = 180, 3 = 270).  d = x_j * x_i + y_j * y_i;  c = x_j * y_i - y_j * x_i;  s = |d| + |c|.
 *   s is zero or not finite:   t = 0
 *   else d >= 0 and c >= 0:    t = c / s
 *   else d < 0:                t = 2 - c / s
 *   else:                      t = 4 + c / s
 * then, if t == 0 and i < j, t = 4.  c is EXACTLY antisymmetric in IEEE arithmetic (the products commute and a - b = -(b - a)) and d is
 * symmetric; the definition relies on it: TURN(j, i) and TURN(i, j) see the same |c| and d, so two directions agree on whether they coincide,
 * and of a group of coincident directions only the highest slot looks past the group (the others' gap is 0).
 *
 * GAP.  g_j starts at 4 and is replaced by every TURN(j, i) < g_j over the directions i != j, i ascending (4 with no other direction).  G_s
 * starts at +0.0 and is replaced by every g_j > G_s over the directions j, j ascending.  gap_s = (float)G_s.  The row is BOUNDARY iff
 * G_s > (double)max_gap; otherwise it is INTERIOR.  On a regular grid seen along its normal with the eight surrounding surfels as neighbours,
 * an inner surfel has G = 0.5, one on a straight edge 2, a convex corner 3 and the concave corner of a hole 1.
 *
 * STATUS, one byte per row: EF_BOUNDARY_NONE (the row takes no part), EF_BOUNDARY_INTERIOR, EF_BOUNDARY_BOUNDARY, EF_BOUNDARY_SPARSE,
 * EF_BOUNDARY_DEGENERATE.  SPARSE is decided first, then DEGENERATE, then the verdict.
 * OUTPUTS by row: gap = gap_s, 0 unless INTERIOR or BOUNDARY; count = count_s, 0 for NONE; status; the loop's label and size.
 *
 * LOOPS are the connected components of the section "Connected components of the map", unchanged, of the graph whose NODES are the BOUNDARY
 * rows that are nodes by that section's rule (so a BOUNDARY row with conf <= min_conf is in no loop) and whose radius is this call's radius.
 * label = the SMALLEST ROW of the loop, size = the number of its nodes; min_size / max_size give ACCEPTED / REJECTED as there.  Every row that
 * is in no loop has label = EF_COMPONENT_NONE and size = 0.
 *
 * max_gap is in TURN units, finite and in (0, 4).  The default 1.0 is a right angle, the toolkits' default: a definition, not a measurement.
 * ef_boundary_gap_from_angle (host only, no context, no GPU) gives the TURN from the direction (1, 0) to (cos a, sin a) for an angle a in
 * (0, 2 pi): with n = the whole quarter turns in a and b = a - n (pi / 2), *gap = n + sin b / (sin b + cos b) in double, which is exact at the
 * quarter turns.  Nothing above depends on it or on libm.
 *
 * ef_boundary_result: participants, interior, boundary, sparse, degenerate (they add up to participants); loops = the number of loops,
 * accepted = the ACCEPTED ones among them, largest = the greatest size (0 without loops); listed = the list's total (0 for ef_map_boundaries);
 * status = the union-find's word of ef_component_result, always 0 (the host variants return EF_EHIP otherwise).
 *
 * ef_map_boundaries changes nothing.  It writes the five arrays for the rows r < min(max_rows, map count) (every array may be NULL; entries
 * past that are left as they were) and the optional result.  ef_map_boundaries_select changes nothing.  what = EF_BOUNDARY_INTERIOR,
 * EF_BOUNDARY_BOUNDARY, EF_BOUNDARY_SPARSE or EF_BOUNDARY_DEGENERATE (the rows of that status), EF_BOUNDARY_LOOPS_ACCEPTED or
 * EF_BOUNDARY_LOOPS_REJECTED (the nodes of those loops).  The list has ef_map_select's conventions: the first min(max_rows, total) rows in
 * ASCENDING order, *count = total however small max_rows is, rows may be NULL with max_rows 0, entries past min(max_rows, total) are left as
 * they were; it is what ef_map_erase_rows and ef_map_gather take.  The _dev variants take DEVICE pointers for the arrays, count and result and
 * only enqueue on the context's stream, except for what the selection needs (ID numbering, label alignment, the count after a call that can
 * change the map) and except that they wait for the device once when the index has to be rebuilt or the scratch grows.
 *
 * cell is the cell of the queries' index, which is built at that cell where needed; a later query at another cell rebuilds it, as after
 * ef_set_query_cell.  No result depends on it.  Defaults (ef_default_boundary_params): radius 0.03 m, cell 0.03 m, min_conf -1, k 12,
 * min_neighbors 5 (the normals' defaults), EF_BOUNDARY_STORED, line_ratio 1e-4, max_gap 1, min_size 1, max_size 0 (no upper bound).
 *
 * Not provided: a write-back (nothing of the result is a field of a surfel); a remove call (ef_map_erase_rows takes the lists); the order of
 * a loop's rows along the loop; a method of the C++ shim.
 *
 * EF_EINVAL, before any GPU work (the arguments are checked before the context, so with a NULL context ef_last_error(NULL) names what is wrong
 * with them): a NULL context, params or count; radius or cell not finite and positive, or 1 / cell not finite; radius / cell above
 * EF_QUERY_MAX_RATIO; NaN min_conf; k outside 3 .. 16; min_neighbors outside 2 .. k; normal_source outside its two values; NaN or negative
 * line_ratio; max_gap not finite or not in (0, 4); what outside its six values; max_rows > 0 with NULL rows; with among given, everything
 * ef_map_select refuses for a selection.  ef_boundary_gap_from_angle: a NULL gap, an angle that is not inside (0, 2 pi).
 * EF_ESTATE: the context's stream is being captured; with among given, what ef_map_select answers with EF_ESTATE.  All calls work on contexts
 * created with close_loops = 1. */
#define EF_BOUNDARY_STORED         0     /* normal_source: the row's stored normal */
#define EF_BOUNDARY_ESTIMATED      1     /* normal_source: ef_map_normals' estimate */
#define EF_BOUNDARY_NONE           0     /* status: the row takes no part */
#define EF_BOUNDARY_INTERIOR       1     /* status, and `what`: no gap wider than max_gap */
#define EF_BOUNDARY_BOUNDARY       2     /* status, and `what`: a gap wider than max_gap */
#define EF_BOUNDARY_SPARSE         3     /* status, and `what`: fewer than min_neighbors neighbours */
#define EF_BOUNDARY_DEGENERATE     4     /* status, and `what`: no normal, or no neighbour off the normal */
#define EF_BOUNDARY_LOOPS_ACCEPTED 5     /* `what`: the nodes of the loops within min_size .. max_size */
#define EF_BOUNDARY_LOOPS_REJECTED 6     /* `what`: the nodes of the other loops */
typedef struct ef_boundary_params {
  float radius; float cell; float min_conf;
  int k;                  /* neighbours used, 3 .. 16 */
  int min_neighbors;      /* 2 .. k */
  int normal_source;      /* EF_BOUNDARY_STORED / EF_BOUNDARY_ESTIMATED */
  float line_ratio;       /* EF_BOUNDARY_ESTIMATED: the estimate's */
  float max_gap;          /* TURN units, (0, 4) */
  uint32_t min_size; uint32_t max_size;   /* of a loop; max_size 0: no upper bound */
} ef_boundary_params;
typedef struct ef_boundary_result {
  uint32_t participants, interior, boundary, sparse, degenerate, loops, accepted, largest, listed, status;
} ef_boundary_result;
int ef_default_boundary_params(ef_ctx* ctx, ef_boundary_params* params);
int ef_boundary_gap_from_angle(double radians, double* gap);
int ef_map_boundaries(ef_ctx* ctx, const ef_boundary_params* params, const ef_map_selection* among_or_null, float* gap_or_null,
                      uint32_t* count_or_null, uint8_t* status_or_null, uint32_t* label_or_null, uint32_t* size_or_null, uint32_t max_rows,
                      ef_boundary_result* result_or_null);
int ef_map_boundaries_dev(ef_ctx* ctx, const ef_boundary_params* params, const ef_map_selection* among_or_null, float* gap_dev_or_null,
                          uint32_t* count_dev_or_null, uint8_t* status_dev_or_null, uint32_t* label_dev_or_null, uint32_t* size_dev_or_null,
                          uint32_t max_rows, ef_boundary_result* result_dev_or_null);
int ef_map_boundaries_select(ef_ctx* ctx, const ef_boundary_params* params, const ef_map_selection* among_or_null, int what, uint32_t* rows,
                             uint32_t max_rows, uint32_t* count, ef_boundary_result* result_or_null);
int ef_map_boundaries_select_dev(ef_ctx* ctx, const ef_boundary_params* params, const ef_map_selection* among_or_null, int what,
                                 uint32_t* rows_dev, uint32_t max_rows, uint32_t* count_dev, ef_boundary_result* result_dev_or_null);

/* named internal images, copied to HOST (synchronises); for tests and for a front-end's drawing code */
enum ef_image {
  EF_IMG_DEPTH_FILTERED = 0,      /* u16  */
  EF_IMG_DEPTH_METRIC,            /* f32  */
  EF_IMG_DEPTH_METRIC_FILTERED,   /* f32  */
  EF_IMG_PREDICT_IMAGE,           /* u8x4 IndexMap::imageTex   */
  EF_IMG_PREDICT_VERTEX,          /* f32x4 IndexMap::vertexTex */
  EF_IMG_PREDICT_NORMAL,          /* f32x4 IndexMap::normalTex */
  EF_IMG_PREDICT_TIME,            /* u16  IndexMap::timeTex    */
  EF_IMG_FILL_IMAGE,              /* u8x4 FillIn::imageTexture */
  EF_IMG_FILL_VERTEX,             /* f32x4 */
  EF_IMG_FILL_NORMAL,             /* f32x4 */
  EF_IMG_INDEX,                   /* u32  IndexMap::indexTex   */
  EF_IMG_VERT_CONF,               /* f32x4 */
  EF_IMG_COLOR_TIME,              /* f32x4 */
  EF_IMG_NORM_RAD,                /* f32x4 */
  EF_IMG_OLD_IMAGE,               /* u8x4 IndexMap::oldImageTex  (INACTIVE prediction; close_loops contexts only) */
  EF_IMG_OLD_VERTEX,              /* f32x4 IndexMap::oldVertexTex */
  EF_IMG_OLD_NORMAL,              /* f32x4 IndexMap::oldNormalTex */
  EF_IMG_OLD_TIME                 /* u16  IndexMap::oldTimeTex   */
};
int ef_get_image(ef_ctx* ctx, int which, void* host_dst, size_t bytes);
/* Resize::image / vertex / time (Core/Shaders/Resize.cpp:50-159): the predicted, fill-in or inactive-prediction image `which`
 * downsampled NEAREST by an integer factor on the device ((W/factor) x (H/factor) elements copied to the host): what the fern
 * database encodes (factor 8, Ferns.cpp:31-36,78-116) and what the constraint sampling reads (factor 20).  Synchronises. */
int ef_get_image_resized(ef_ctx* ctx, int which, int factor, void* host_dst, size_t bytes);
/* tracker pyramids (RGBDOdometry private state) for kernel-level parity tests:
 * which: 0 vmap_curr 1 nmap_curr 2 vmap_g_prev 3 nmap_g_prev 4 lastDepth 5 nextDepth 6 lastImage
 *        7 nextImage 8 lastNextImage 9 dIdx 10 dIdy 11 depth_tmp
 *        12 rgbMask (u8: the frame-invariant half of residualKernel's gates, 1 = the iterations revisit the pixel)
 *        13 corres (u32 packed photometric correspondence of the last iteration: bit 31 valid | (diff + 255) << 22 | v0 << 11 | u0)
 * nextDepth is lastDepth on the frame-to-model tracker (quirk Q1).
 * ef_get_tracker_buffer_of: tracker 0 = frameToModel (what ef_get_tracker_buffer reads), 1 = modelToModel (close_loops contexts only:
 * EF_ESTATE otherwise; its nextDepth is a buffer of its own and its depth_tmp is never written) */
int ef_get_tracker_buffer(ef_ctx* ctx, int which, int level, void* host_dst, size_t bytes);
int ef_get_tracker_buffer_of(ef_ctx* ctx, int tracker, int which, int level, void* host_dst, size_t bytes);

/* per-stage GPU time of the last ef_process_frame (hipEvent pairs; names follow the reference's
 * TICK/TOCK sites, Core/Utils/Stopwatch.h): fills up to max entries, returns count in *n */
typedef struct ef_timing { const char* name; float ms; } ef_timing;
int ef_enable_timing(ef_ctx* ctx, int on);
int ef_get_timings(ef_ctx* ctx, ef_timing* out, int max, int* n);

/* Sampling of the dominant kernel (the level-0 icpStep+rgbStep normal-equation kernel) every `every_n_frames`-th frame (0 = off;
 * resets the samples): the sampled launches go through hipExtLaunchKernelGGL with a start and a stop event, which receive the
 * DISPATCH's own begin / end timestamps -- the duration rocprofv3 --kernel-trace reports for the same launch, no marker packets
 * in between.  ef_get_kernel_timing synchronises and returns the average launch duration, the number of sampled launches and the
 * algorithmic bytes one launch must move (bytes_per_launch_survey: SURVEY.md 8d's narrower numerator) --
 * bench.py's roofline leg. */
typedef struct ef_kernel_time {
  const char* name; float avg_us; int launches; double bytes_per_launch; double bytes_per_launch_survey;
} ef_kernel_time;
int ef_kernel_timing(ef_ctx* ctx, int every_n_frames);
int ef_get_kernel_timing(ef_ctx* ctx, ef_kernel_time* out);
/* same sampling (switched on by ef_kernel_timing) of the IndexMap point splat: k_index_splat of the frame's first predictIndices */
int ef_get_splat_timing(ef_ctx* ctx, ef_kernel_time* out);
/* same sampling of the persistent tracker launch (k_track_fast: the whole of RGBDOdometry::getIncrementalTransformation, RGBDOdometry.cpp:259-553,
 * as one launch); launches = 0 while the launch-per-step script runs (ef_set_persistent_tracker(ctx, 0), rgbOnly, graph replay) */
int ef_get_tracker_timing(ef_ctx* ctx, ef_kernel_time* out);

/* Persistent tracker launches (the default: RGBDOdometry::getIncrementalTransformation, RGBDOdometry.cpp:259-553, as one launch of 256 co-resident
 * workgroups) that found part of the chip taken by other work and ran on one workgroup instead: same results, ~25x the tracking time, nothing for
 * the caller to do — a server that sees the count grow is sharing the GPU with something that holds CUs for milliseconds.  Synchronises. */
int ef_get_tracker_fallbacks(ef_ctx* ctx, int* count);
/* Which launches the frame-to-model tracker's last RGBDOdometry::getIncrementalTransformation ran (all zero before the first tracked frame).
 * script: 0 = one launch per step, 1 = the whole call as one persistent launch, 2 = the launch of the small levels, then one launch per
 * remaining step (ef_set_persistent_tracker; graph replay and rgbOnly run script 0 whatever was asked).  n_iter: Gauss-Newton iterations of the
 * call; n_small: how many of them ran inside script 2's launch; levels: the pyramid level of each iteration inside the one launch (script 1:
 * all n_iter, script 2: the first n_small; 0 otherwise), two bits each, the first iteration lowest.  res_bytes: dynamic LDS of script 1's launch
 * (its levels' resident pixel data; 0 = every level streams); res_budget: what the device allows for it (0 = not asked yet, or none).
 * Reads host state only: enqueues and synchronises nothing, and answers whatever the stream is doing. */
typedef struct ef_tracker_plan {
  int script, n_small, n_iter;
  unsigned long long levels;
  unsigned res_bytes, res_budget;
} ef_tracker_plan;
int ef_get_tracker_plan(ef_ctx* ctx, ef_tracker_plan* out);
/* developer instrumentation for the test of that path: `workgroups` workgroups that each fill one CU spin for `microseconds` on a stream of their own */
int ef_debug_occupy(ef_ctx* ctx, int workgroups, int microseconds);
/* developer instrumentation: lanes that share one query of ef_query_nearest / ef_query_knn (1, 8; nearest also 16, 64; 0 = the default: 16 for nearest, 1 for kNN).  Results do not
 * depend on it; tools/query_times.py measures the choices */
int ef_debug_query_lanes(ef_ctx* ctx, int lanes);
/* test hook: raises the sticky "a persistent tracker launch gave up waiting" flag of the frame tracker, as a wait that timed out after admission
 * would.  From then on every persistent launch of the context returns at once; the frame whose tracker saw the flag hands it to the host, the
 * NEXT ef_process_frame[_dev] (class ElasticFusion::processFrame: throws) returns EF_EHIP without having enqueued anything, and so does
 * ef_synchronize.  Results since the flag was raised are invalid. */
int ef_debug_inject_tracker_abort(ef_ctx* ctx);

/* developer instrumentation: the 16 wall_clock64() (100 MHz) stamps the last tracking solve left in the device state;
 * all zero unless the library was built with -DEF_STAGE_CLOCKS (EF_HIPCC_FLAGS=-DEF_STAGE_CLOCKS python -m elasticfusion_amd.build) */
int ef_debug_clocks(ef_ctx* ctx, unsigned long long* out16);
/* developer instrumentation of the persistent tracker launch (zeros unless the library was built with -DEF_STAGE_CLOCKS): 32 sums
 * of 10 ns ticks per phase since the last call; tools/fast_clocks.py (reference-order builds: tools/small_clocks.py) names them */
int ef_debug_small_clocks(ef_ctx* ctx, unsigned long long* out32);

/* ---- device memory helpers (so that a non-HIP host can drive the operator tier) ---- */
int ef_dev_alloc(void** dev, size_t bytes);
int ef_dev_free(void* dev);
int ef_dev_upload(void* dev, const void* host, size_t bytes);
int ef_dev_download(void* host, const void* dev, size_t bytes);
int ef_dev_memset(void* dev, int value, size_t bytes);
int ef_dev_sync(void);
/* box calibration for benchmarks (GPU boxes of one pool differ by 10-20 %): average time per launch of 200 back-to-back launches of an EMPTY
 * kernel and of a kernel that copies 16 MiB with 16-byte accesses (16 MiB read + 16 MiB written), on `stream` (a hipStream_t, 0 = null stream) */
int ef_dev_calibrate(void* stream, float* empty_us, float* stream16mb_us);
int ef_device_count(int* n);
int ef_set_device(int device);

/* ---- operator tier: tracking (Core/Cuda/cudafuncs.cuh:61-169). All pointers are DEVICE pointers,
 * work runs on `stream` (hipStream_t, NULL = default stream) and is synchronous only where the
 * reference returns host results (icp/rgb/so3 steps, rgb residual). ---- */
typedef struct ef_intr { float fx, fy, cx, cy; } ef_intr;   /* CameraModel, types.cuh:88-96 */

int ef_op_pyr_down(const uint16_t* src, int src_cols, int src_rows, uint16_t* dst, void* stream);             /* pyrDown */
int ef_op_create_vmap(const ef_intr* intr, const uint16_t* depth, int cols, int rows, float depth_cutoff,
                      float* vmap, void* stream);                                                              /* createVMap */
int ef_op_create_nmap(const float* vmap, int cols, int rows, float* nmap, void* stream);                       /* createNMap */
int ef_op_transform_maps(const float* vmap_src, const float* nmap_src, int cols, int rows, const float* R9,
                         const float* t3, float* vmap_dst, float* nmap_dst, void* stream);                      /* tranformMaps */
int ef_op_copy_maps(const float* vmap_src_f4, const float* nmap_src_f4, int cols, int rows, float* vmaps_tmp,
                    float* vmap_dst, float* nmap_dst, void* stream);                                            /* copyMaps */
int ef_op_resize_vmap(const float* in, int src_cols, int src_rows, float* out, void* stream);                  /* resizeVMap */
int ef_op_resize_nmap(const float* in, int src_cols, int src_rows, float* out, void* stream);                  /* resizeNMap */
int ef_op_pyr_down_gauss_f(const float* src, int src_cols, int src_rows, float* dst, void* stream);            /* pyrDownGaussF */
int ef_op_pyr_down_uchar_gauss(const uint8_t* src, int src_cols, int src_rows, uint8_t* dst, void* stream);    /* pyrDownUcharGauss */
int ef_op_vertices_to_depth(const float* vmaps_tmp, int cols, int rows, float cutoff, float* dst, void* stream); /* verticesToDepth */
int ef_op_image_bgr_to_intensity(const uint8_t* rgba, int cols, int rows, uint8_t* dst, void* stream);         /* imageBGRToIntensity */
int ef_op_compute_derivative_images(const uint8_t* src, int cols, int rows, int16_t* dx, int16_t* dy, void* stream); /* computeDerivativeImages */
int ef_op_project_to_point_cloud(const float* depth, int cols, int rows, const ef_intr* intr_level0, int level,
                                 float* cloud_f3, void* stream);                                                /* projectToPointCloud */
/* icpStep: host outputs A[36] row-major symmetric, b[6], residual[2] = {sum r^2, inliers} */
int ef_op_icp_step(const float* Rcurr9, const float* tcurr3, const float* vmap_curr, const float* nmap_curr,
                   const float* Rprev_inv9, const float* tprev3, const ef_intr* intr, const float* vmap_g_prev,
                   const float* nmap_g_prev, float dist_thres, float angle_thres, int cols, int rows,
                   float* A_host36, float* b_host6, float* residual_host2, void* stream);
/* computeRgbResidual: corres_img is W*H 16-byte DataTerm records (types.cuh:81-86) */
int ef_op_compute_rgb_residual(float min_scale, const int16_t* dIdx, const int16_t* dIdy, const float* last_depth,
                               const float* next_depth, const uint8_t* last_image, const uint8_t* next_image,
                               void* corres_img, float max_depth_delta, const float* kt3, const float* krkinv9,
                               int cols, int rows, int* sigma_sum_host, int* count_host, void* stream);
int ef_op_rgb_step(const void* corres_img, float sigma, const float* cloud_f3, float fx, float fy,
                   const int16_t* dIdx, const int16_t* dIdy, float sobel_scale, int cols, int rows,
                   float* A_host36, float* b_host6, void* stream);
int ef_op_so3_step(const uint8_t* last_image, const uint8_t* next_image, const float* image_basis9,
                   const float* kinv9, const float* krlr9, int cols, int rows, float* A_host9, float* b_host3,
                   float* residual_host2, void* stream);

/* The frame tier's two most heavily fused input launches on caller-owned DEVICE buffers, for parity tests against the composition of
 * reference operators each stands for.  No behaviour of a frame depends on these two entries.
 * ef_op_model_maps: the shipped k_model_maps (copyMaps -> resizeVMap / resizeNMap x2 -> tranformMaps x3, verticesToDepth and the model's
 * level-0 intensity in one launch, RGBDOdometry.cpp:171-239), or -- joint != 0 -- the model-map half of k_frame_inputs, whose grid also
 * carries the depth pre-processing tiles of a raw frame (filtered / metric / metric_filtered / next0 come back as well).
 * The source of the maps is the prediction or the fill-in: !(dense_count / dense_samples > 0.75) reads the fill-in
 * (ElasticFusion.cpp:256-268,304-305); tally != 0: the count is first taken from pred_image's (cols / 20) x (rows / 20) sample texels
 * (20 a + 10, 20 b + 10), and *dense_count_left receives it.  camera_frame != 0: copyMaps + resize only (initICP on predicted maps).
 * cols and rows are multiples of 4.  vmap / nmap: 3 planes per level (levels 0-2); outputs keep what they held where the launch does
 * not write (quirk Q3: y / z planes of an invalid texel of levels 1-2).  Synchronises. */
typedef struct ef_model_maps_op {
  int cols, rows;
  const float *pred_vertex, *pred_normal, *fill_vertex, *fill_normal;   /* 4 floats per texel */
  const uint8_t *pred_image, *fill_image;                               /* rgba, or both NULL: last0 is not written */
  float R[9], t[3];                                                     /* T_wc as floats (RGBDOdometry.cpp:192-193) */
  float max_depth_rgb;                                                  /* RGBDOdometry.cpp:42 */
  int camera_frame, force_fill_image, tally;
  unsigned dense_count;
  int dense_samples;
  float* vmap[3];
  float* nmap[3];
  float* depth0;                                                        /* lastDepth[0] (camera_frame: nextDepth[0]) */
  uint8_t* last0;                                                       /* lastImage[0] */
  int joint;
  const uint16_t* raw;                                                  /* joint: the frame's raw depth and packed rgb */
  const uint8_t* rgb3;
  float depth_cut;
  uint16_t* filtered;
  float* metric;
  float* metric_filtered;
  uint8_t* next0;                                                       /* nextImage[0] */
} ef_model_maps_op;
int ef_op_model_maps(const ef_model_maps_op* args, unsigned* dense_count_left, void* stream);
/* ef_op_sobel_mask: k_sobel_levels on a caller's nextImage / nextDepth pyramids (arrays of 3 device pointers, level l is
 * (cols >> l) x (rows >> l)): computeDerivativeImages of every level, the frame-invariant half of residualKernel's gates
 * (reduce.cu:631-667; minScale = 1600, 576, 64) as one byte per pixel, and the packed correspondences reset to 0.  Synchronises. */
int ef_op_sobel_mask(const uint8_t* const* next_image3, const float* const* next_depth3, int cols, int rows, int16_t* const* dIdx3,
                     int16_t* const* dIdy3, uint8_t* const* mask3, uint32_t* const* corres3, void* stream);

/* The tracking driver's small linear algebra (Eigen / Sophus arithmetic of RGBDOdometry.cpp:356,526-534,566-570,
 * OdometryProvider.h:34-96, ElasticFusion.cpp:371-374) as the DEVICE evaluates it, host vectors in and out
 * (<= 64 doubles each) -- for parity tests against the oracle's efo_ldlt6 / efo_polar3 / ... */
enum ef_linalg_op {
  EF_LINALG_LDLT6 = 0,        /* in A[36] b[6]              -> x[6]   Eigen::LDLT solve, double            */
  EF_LINALG_LDLT3F,           /* in A[9] b[3] (as doubles)  -> x[3]   Eigen::LDLT solve, float             */
  EF_LINALG_POLAR3,           /* in A[9]                    -> R[9]   JacobiSVD U V^T                      */
  EF_LINALG_RODRIGUES,        /* in v[3]                    -> R[9]   OdometryProvider::rodrigues          */
  EF_LINALG_SE3_INVERSE,      /* in T[16]                   -> T^-1[16] Sophus::SE3d::inverse().matrix()    */
  EF_LINALG_SE3_LOG_NORM,     /* in T[16]                   -> |log(T)| Sophus::SE3d::log().norm()          */
  EF_LINALG_SCALAR,           /* in a, b -> sqrt(a), a/b, sin(a), cos(a), atan2(a,b) (fp64 device math)     */
  EF_LINALG_LDLT6_WAVE,       /* as EF_LINALG_LDLT6, through the earlier one-element-per-lane wavefront version, kept for tests */
  EF_LINALG_LDLT6_EVERY_LANE, /* as EF_LINALG_LDLT6, through the whole-matrix-per-lane version the update step runs  */
  EF_LINALG_MAT_TO_QUAT,      /* in R[9]                    -> q[4] Eigen::Quaternion(Matrix3) xyzw, q[4] after Sophus' setRotationMatrix */
  EF_LINALG_SE3_MUL,          /* in Ta[16] Tb[16]           -> q[4] t[3] of Sophus::SE3d Ta * Tb            */
  EF_LINALG_SE3_CASTF,        /* in T[16]                   -> T.cast<float>().matrix()[16], widened        */
  EF_LINALG_SE3_INVERSE_F,    /* in T[16]                   -> T.inverse().matrix().cast<float>()[16], widened */
  EF_LINALG_M4_AFFINE_INVERSE,/* in M[16] (last row 0 0 0 1) -> M^-1[16]                                    */
  EF_LINALG_LDLT_PIVOTS,      /* in A[36]                   -> d[6] the pivots of EF_LINALG_LDLT6, in elimination order */
  EF_LINALG_LU_INVERSE6       /* in A[36]                   -> A^-1[36] Eigen::PartialPivLU inverse (getCovariance) */
};
int ef_op_linalg(int which, const double* in_host, int n_in, double* out_host, int n_out);

/* The Gauss-Newton update step between two reductions (RGBDOdometry.cpp:440-551 + OdometryProvider.h:73-96) as the tracker's kernels run
 * it, on caller-supplied state: one workgroup, no image.  ef_gn_state is what one update hands to the next. */
typedef struct ef_gn_state {
  float Rcurr[9], tcurr[3];
  double resultRt[16];
  float krkinv[9], kt[3];     /* K R K^-1, K t of the coming iteration */
  float lastRGBErrorLevel;    /* rgbOnly early-exit bookkeeping */
  int rgb_broken;
} ef_gn_state;
typedef struct ef_gn_update_args {
  float sums[58];             /* the 29 + 29 members of JtJJtrSE3 (ICP, RGB; types.cuh:98-143) */
  ef_gn_state prev;
  float Rprev[9], tprev[3];
  int count, sigma;           /* {count, sum diff^2} of the residual pass */
  int icp, rgb, rgb_only;
  float icp_weight;
  ef_intr knext;              /* intrinsics of the coming iteration's level */
  int level_changes;          /* the coming iteration runs at another level */
  int split_tail;             /* 1: the step's two tails on two wavefronts side by side, as the persistent launch runs them */
} ef_gn_update_args;
/* lastA36, lastb6, stats4 = {lastICPError, lastICPCount, lastRGBError, lastRGBCount} are in/out: a step that takes the rgbOnly break
 * leaves them as they are */
int ef_op_gn_update(const ef_gn_update_args* in, ef_gn_state* next, double* lastA36, double* lastb6, float* stats4);
/* The end of getIncrementalTransformation on one lane (0.3 m guard, re-orthonormalisation, RGBDOdometry.cpp:555-570), the float
 * matrices of the map passes, the velocity weighting (ElasticFusion.cpp:369-383) and the logged pose, on caller-supplied state */
typedef struct ef_track_end_out {
  double q[4], t[3];
  double logged[16];
  float T_cw[16], pose_f[16], R_wc_f[9], t_wc_f[3];
  float weighting;
} ef_track_end_out;
int ef_op_track_end_tail(const float* Rcurr9, const float* tcurr3, const float* Rprev9, const float* tprev3, const double* q_prev4,
                         const double* t_prev3, int rgb, float weight_multiplier, ef_track_end_out* out);

/* ---- operator tier: pre-processing and surfel map (the reference's GLSL passes) ---- */
typedef struct ef_cam { int cols, rows; float fx, fy, cx, cy; } ef_cam;

int ef_op_filter_depth(const uint16_t* raw, int cols, int rows, float max_d, uint16_t* filtered, void* stream);   /* depth_bilateral.frag */
int ef_op_metricise_depth(const uint16_t* in, int cols, int rows, float max_d, float* out, void* stream);         /* depth_metric.frag */
/* vertex_feedback x2 + init_unstable: returns the number of seeded surfels in *count_host */
int ef_op_seed_map(const ef_cam* cam, const uint8_t* rgb, const float* depth_metric, const float* depth_metric_filtered,
                   int time, float max_depth, float* surfels_aos, uint32_t* count_host, void* stream);
/* IndexMap::predictIndices: surfels_aos = count x 12 floats */
int ef_op_predict_indices(const ef_cam* cam, const double* T_wc16, int time, const float* surfels_aos, uint32_t count,
                          float max_depth, int time_delta, uint32_t* index_map, float* vert_conf, float* color_time,
                          float* norm_rad, void* stream);
/* IndexMap::combinedPredict (ACTIVE) */
int ef_op_combined_predict(const ef_cam* cam, const double* T_wc16, const float* surfels_aos, uint32_t count,
                           float max_depth, float conf_threshold, int time, int max_time, int time_delta,
                           uint8_t* image_rgba, float* vertex, float* normal, uint16_t* time_map, void* stream);
/* IndexMap::synthesizeDepth (splat.vert + depth_splat.frag, IndexMap.cpp:395-476): float depth, 0 = nothing drawn */
int ef_op_synthesize_depth(const ef_cam* cam, const double* T_wc16, const float* surfels_aos, uint32_t count,
                           float max_depth, float conf_threshold, int time, int max_time, int time_delta,
                           float* depth, void* stream);
/* FillIn::{vertex,normal,image} */
int ef_op_fill_in(const ef_cam* cam, const uint8_t* image_rgba, const float* vertex, const float* normal,
                  const uint16_t* depth_filtered, const uint8_t* rgb, int passthrough, int passthrough_image,
                  uint8_t* fill_image, float* fill_vertex, float* fill_normal, void* stream);
/* Resize::image + denseEnough -> *dense_host in {0,1} */
int ef_op_dense_enough(const ef_cam* cam, const uint8_t* image_rgba, int* dense_host, void* stream);
/* GlobalModel::fuse: surfels updated in place; new_unstable gets the tagged candidates in draw order */
int ef_op_fuse(const ef_cam* cam, const double* T_wc16, int time, const uint8_t* rgb, const float* depth_metric,
               const float* depth_metric_filtered, const uint32_t* index_map, const float* vert_conf,
               const float* color_time, const float* norm_rad, float max_depth, float weighting, float* surfels_aos,
               uint32_t count, float* new_unstable_aos, uint32_t* new_count_host, void* stream);
/* GlobalModel::clean (no deformation graph) */
int ef_op_clean(const ef_cam* cam, const double* T_wc16, int time, const uint32_t* index_map, const float* vert_conf,
                const float* color_time, const float* norm_rad, float conf_threshold, int time_delta, float max_depth,
                const float* surfels_aos, uint32_t count, const float* new_unstable_aos, uint32_t new_count,
                float* surfels_out_aos, uint32_t* out_count_host, void* stream);
/* GlobalModel::clean with the deformation graph applied to every kept surfel (copy_unstable.vert:128-322):
 * graph = nodes x 16 floats sorted by time {position 3, rotation 9 column-major, translation 3, time} (device pointer), the
 * content of the reference's node texture (GlobalModel.cpp:540-546); depth = ef_op_synthesize_depth image (device, read
 * unless is_fern).  nodes == 0 is ef_op_clean. */
int ef_op_clean_deform(const ef_cam* cam, const double* T_wc16, int time, const uint32_t* index_map, const float* vert_conf,
                       const float* color_time, const float* norm_rad, float conf_threshold, int time_delta, float max_depth,
                       const float* surfels_aos, uint32_t count, const float* new_unstable_aos, uint32_t new_count,
                       const float* graph, int nodes, const float* depth, int is_fern, float* surfels_out_aos,
                       uint32_t* out_count_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EF_HIP_H_ */
