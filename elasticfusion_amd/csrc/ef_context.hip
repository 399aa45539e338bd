// libefusion_hip: the context and the C ABI of include/ef_hip.h.  This file holds struct ef_ctx, what every part of the host code shares,
// the translation unit's kernels, create / destroy and the setters; the frame, its loop closures and the getters are included below
// (ef_host_closures.inc, ef_host_frame.inc, ef_host_inspect.inc), the map operations at the end.
// The frame script follows ElasticFusion::processFrame (Core/ElasticFusion.cpp:270-607) for the open-loop
// configuration; every stage is only ENQUEUED on the context's stream — pose, surfel count, fill-in
// decision and fusion weight all live in a device-resident state block, so a frame costs zero
// host<->device round trips (the reference has ~70 blocking ones).
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdio.h>
#include <string.h>
#include <limits>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ef_hip.h"
#include "ef_linalg_dev.hpp"
#include "ef_solve_dev.hpp"
#include "ef_map.hpp"
#include "ef_deform_solver.hpp"
#include "ef_track.hpp"

// (the time-stamp log's push_back, kept out of line: the library has always exported this name, and its exported names are compared commit to commit)
template void std::vector<int64_t>::push_back(const int64_t&);

namespace {

thread_local std::string g_create_error;

struct StageTimer {
  const char* name;
  hipEvent_t a, b;
  bool used;
};

// A device buffer that grows on demand (reserve, beside dev_alloc).  No growth policy: the caller asks for the size it wants, slack included.
struct DevBuf {
  uint8_t* p = nullptr;
  size_t bytes = 0;
  int reserve(ef_ctx* c, size_t need, const char* what, bool* grew = nullptr);
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <class T>
  T* as() const { return (T*)p; }
};
// Hands out consecutive sub-ranges of a DevBuf from its base on, each aligned to `align` bytes (a power of two; hipMalloc's base is aligned far
// beyond any used here).  It checks no size: the caller has reserved what it carves.
struct Carver {
  uint8_t* at;
  explicit Carver(const DevBuf& b) : at(b.p) {}
  template <class T>
  T* take(size_t count, size_t align = alignof(T)) {
    at = (uint8_t*)(((uintptr_t)at + align - 1) & ~(uintptr_t)(align - 1));
    T* r = (T*)at;
    at += count * sizeof(T);
    return r;
  }
  // {chunk counts | chunk offsets | 4 words} of a SelectScratch for `rows` rows; returns the 4 words (the scan's total).  The flag bytes are
  // the caller's to place: several sets may share them, or share these words.
  static size_t chunks(size_t rows) { return (size_t)efm::select_chunks((unsigned)rows) + 1; }
  static size_t scan_bytes(size_t rows) { return (2 * chunks(rows) + 4) * sizeof(uint32_t); }
  uint32_t* scan_words(size_t rows, efm::SelectScratch* sc, size_t align = alignof(uint32_t)) {
    const size_t k = chunks(rows);
    sc->chunk_count = take<uint32_t>(k, align);
    sc->chunk_offset = take<uint32_t>(k);
    return take<uint32_t>(4);
  }
};

// The five images of one frame.  A context holds two sets (ef_ctx::img / img_alt) and swaps them at the head of every frame.
struct FrameImages {
  uint8_t* rgb = nullptr;
  uint16_t *depth_raw = nullptr, *depth_filtered = nullptr;
  float *depth_metric = nullptr, *depth_metric_filtered = nullptr;
};
// One slot of the host-pointer frames' ring (ef_process_frame): a pinned staging pair, its device landing pair, the upload's event
struct RingSlot {
  uint8_t *h_rgb = nullptr, *d_rgb = nullptr;
  uint16_t *h_depth = nullptr, *d_depth = nullptr;
  hipEvent_t ev_h2d = nullptr;
};
// HIP-event sampling of one kernel (ef_kernel_timing): the start / stop events the launch code records through `probe`, created on first use
struct KernelSampler {
  std::vector<hipEvent_t> start, stop;
  eft::KernelProbe probe{nullptr, nullptr, 0, 0};
  int create(ef_ctx* c, int capacity);           // nothing when the events exist
  int average_us(ef_ctx* c, float* us) const;    // waits for the stream; over probe.used samples, 0 when there is none
  void release() {
    for (auto e : start) (void)hipEventDestroy(e);
    for (auto e : stop) (void)hipEventDestroy(e);
    *this = KernelSampler{};
  }
};

}  // namespace

struct ef_ctx {
  ef_config cfg;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string err;
  efm::Cam cam;
  eft::Intr intr;
  const float maxDepthProcessed = 20.0f;  // ElasticFusion.cpp:83
  // frame images, and a second set of the five: frame k+1's input stage (copy, bilateral filter, frame pyramids) runs on
  // in_stream while frame k is still being fused on `stream`, so the two frames must not share these buffers
  FrameImages img, img_alt;
  hipStream_t in_stream = nullptr;
  hipEvent_t ev_input_done = nullptr, ev_track_done = nullptr;
  hipEvent_t ev_frame_done[2] = {nullptr, nullptr};   // end of the frame that last used each set of frame images
  int frame_parity = 0;
  int overlap_mode = 1;          // ef_set_input_overlap: 1 = whole input stage after the previous tracker; 2 = copy + bilateral filter already during it
  bool overlap = false;
  bool events_live = false;      // the previous frame recorded ev_track_done (and, in mode 2, ev_frame_done): see process_frame
  // host-pointer frames (ef_process_frame, the reference's processFrame signature): a ring of pinned staging pairs and device landing pairs; the
  // upload runs on copy_stream, the frame script reads the landing pair in place (round 6)
  static constexpr int RING = 3;
  RingSlot ring[RING];
  hipStream_t copy_stream = nullptr;
  unsigned host_seq = 0;           // host-pointer frames submitted so far
  unsigned mark_value = 0;         // what this frame's prediction writes into *h_consumed (host_seq + 1; 0: nothing)
  unsigned* h_consumed = nullptr;  // host-mapped: 1 + the index of the last host-pointer frame whose input images the GPU has finished reading
  unsigned* d_consumed = nullptr;
  unsigned* h_abort = nullptr;   // 4 words of host-mapped pinned memory: k_track_end copies a tracker instance's sticky abort flag here (d_abort: the device alias)
  unsigned* d_abort = nullptr;
  // tracker
  eft::Pyramid pyr{};
  eft::TrackState* st = nullptr;
  // model prediction
  efm::IndexMaps im{};
  efm::PredictMaps pm{};
  efm::FillMaps fm{};
  unsigned long long* zbuf = nullptr;
  // Round 9: a frame that fuses does not resolve its two predictIndices into `im` — the association and the keep-test of clean() tap the keys
  // (efm::KeyedIndex), each predictIndices on a z-buffer of its own: zbuf_assoc is cleared by the frame's clean(), zbuf_clean keeps the second
  // splat's keys until the NEXT fusing frame's association clears it.  Until then `im` can be had from them (im_materialise, on the first
  // ef_get_image of one of the four): im_pending says `im` is stale, im_map which of maps[] the keys' ids name (the buffer clean() read, left
  // alone until the next clean() writes it) and im_T16 (device) holds the frame's T_cw.
  unsigned long long* zbuf_assoc = nullptr;
  unsigned long long* zbuf_clean = nullptr;
  float* im_T16 = nullptr;
  bool im_pending = false;
  int im_map = 0;
  // global model
  efm::SurfelSoA maps[2]{};
  int cur = 0;
  // ef_set_reference_download: the reference's vbos[renderSource] after a frame (GlobalModel.cpp:521,667,693: what its update pass
  // wrote, never overwritten by clean) — the buffer GlobalModel::downloadMap and savePly actually read (quirk Q14)
  efm::SurfelSoA shadow{};
  bool reference_download = false;
  uint32_t capacity = 0;
  uint32_t* winner = nullptr;
  efm::Candidates cand{};
  efm::CompactScratch cs{};
  int* overflow = nullptr;
  // trajectory (device log + host timestamps)
  double* traj = nullptr;  // 16 doubles per frame
  int traj_cap = 0;
  std::vector<int64_t> stamps;
  int tick = 1;
  std::vector<void*> allocs;
  // denseEnough()'s tally (ElasticFusion.cpp:256-268): taken by the model-map workgroups of the next tracked frame from the predicted image
  // (eft::ModelMapsArgs::tally_image) instead of one atomic per sample from the prediction's resolve pass
  // (set at ef_create: up to 1 024 samples — 640 x 480 has 768: the resolve pass 13.5 -> 10.3 us, 2072 -> 2091 frames/s; at 1280 x 960, 3 072
  // samples, every model-map workgroup reading them all costs more than the atomics, which hide behind that size's 139 MB: 1029 against 1034,
  // profiles/r08o_*, r08p_*)
  bool tally_by_consumer = false;
  bool tally_pending = false;
  // timing
  bool timing = false;
  std::vector<StageTimer> timers;
  // deformation graph to be applied by the next frame's clean() (ef_set_deformation): the device half of loop closure
  float* graph_dev = nullptr;
  int graph_nodes = 0, graph_is_fern = 0;
  float* synth_depth = nullptr;
  float* rays = nullptr;           // efm::build_ray_table: the ray of every pixel (float4, column-major), for the surface splat
  // local loop closure, front half (ElasticFusion.cpp:447-527): a second tracker instance registers the view of the INACTIVE
  // part of the model against the ACTIVE one; buffers exist only when cfg.close_loops is set
  int icp_count_thresh = 35000;            // ElasticFusion.h:44-46
  float icp_err_thresh = 5e-05f, cov_thresh = 1e-05f;
  int deforms = 0;
  const float* bil_table = nullptr;        // efm::bilateral_table() of this context's device, asked once at ef_create
  eft::Pyramid pyr2{};                     // RGBDOdometry modelToModel (ElasticFusion.h:280)
  eft::TrackState* st2 = nullptr;
  efm::PredictMaps old{};                  // IndexMap's oldImage/oldVertex/oldNormal/oldTime textures (IndexMap.h:114-128)
  float* cons_dev = nullptr;               // (W/20) x (H/20) x {x, y, z, inactive time}
  float* h_cons = nullptr;                 // pinned
  eft::TrackState* h_states = nullptr;     // pinned: [0] frame-to-model, [1] model-to-model / fern tracker, [2] frame-to-model at the end of the frame
  ef_loop_solver solver = nullptr;
  void* solver_user = nullptr;
  bool builtin_solver = false;             // ef_use_builtin_loop_solver: efd::solve_local where Deformation::constrain stands
  int64_t last_deform_time = 0;            // Deformation::lastDeformTime (Deformation.cpp:31,199-201)
  float* nodes_dev = nullptr;              // sampled graph nodes (Deformation::sampleGraphModel), 1024 x 4 + count
  std::vector<float> h_nodes;
  ef_local_loop loop{};
  std::vector<double> loop_constraints;    // n x 8
  std::vector<float> loop_graph;
  // global loop closure (ElasticFusion.cpp:392-445, 588-589, 609-618; ef_enable_global_closure): the host-side closure object (fern
  // database, relative constraints, trajectory; ef_ferns.hip), the 1/8-resolution fill-in views it works on, and a third tracker
  // instance at 1/8 resolution for the fern-to-view registration (Ferns.cpp:243-258: RGBDOdometry rgbd(w / 8, h / 8, ...))
  ef_closure* closure = nullptr;
  ef_global_loop gloop{};
  std::string fern_tracker_error;          // first HIP error inside the fern tracker callback (it cannot return one)
  int fern_w = 0, fern_h = 0;
  uchar4* view_img_dev = nullptr;          // Resize::image / vertex (x2) of the fill-in maps, factor 8
  float4* view_vert_dev = nullptr;
  float4* view_norm_dev = nullptr;
  uint8_t* h_view = nullptr;               // pinned: image | vertices | normals
  eft::Pyramid pyr3{};
  eft::TrackState* st3 = nullptr;
  eft::Intr intr3{};
  float4* fern_maps_dev = nullptr;         // fern vertices | fern normals | view vertices | view normals (+ a zero image)
  float* h_nodes_pinned = nullptr;         // graph nodes sampled at the end of the previous frame (Deformation::sampleGraphModel, :593)
  // fern coding on the device (k_fern_codes): the table, the codes of the view just coded (num bytes, padded to 512, + their count),
  // pinned landing zones for the mid-frame codes and for the END-of-frame record (codes, view, pose, nodes), which is only looked at
  // at the next frame's first synchronisation (Ferns::addFrame's verdict matters to nobody before the next findFrame)
  int* fern_table_dev = nullptr;
  int fern_num = 0, fern_table_version = -1;
  uint8_t* fern_codes_dev = nullptr;       // FERN_CODES_BYTES
  uint8_t* h_codes = nullptr;              // pinned, mid-frame
  uint8_t* h_codes_end = nullptr;          // pinned, end of frame
  uint8_t* h_view_end = nullptr;           // pinned, end of frame: image | vertices | normals
  hipEvent_t ev_end_record = nullptr;
  bool end_pending = false, end_lost = false;
  int end_tick = 0;
  int n_nodes_host = 0;
  double h_pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  // relocalisation (ef_set_relocalisation; ElasticFusion.h:283-286,311-312)
  bool reloc = false, lost = false, last_frame_recovery = false, tracking_ok = true;
  int tracking_count = 0;
  eft::TrackState h_reloc{};               // the frame-to-model tracker's state as read back for the verdict
  // hipGraph replay of the tracker (BASELINE.json configs[4]): the ~70 launches of getIncrementalTransformation are
  // captured once per pyramid parity (the SO(3) reference / frame intensity buffers swap every frame) and replayed
  bool use_graph = false;
  bool track_only = false;       // ef_set_track_only: odometry on a frozen map (BASELINE.json configs[4])
  bool no_resident = false;      // ef_set_resident_levels(ctx, 0): the persistent tracker launch streams every level's pixel data (round 5's kernel; A/B)
  bool fused_step = false;       // ef_set_fused_step: level-0 update step inside the correspondence-search launch
  int persistent = 1;            // ef_set_persistent_tracker: 1 = the whole tracker as one persistent launch of 256 workgroups, 0 = one launch per step,
                                 // 2 = (reference-order builds) round 3's launch of the small levels on 128 workgroups
  struct TrackGraph { hipGraphExec_t exec = nullptr; const void* key = nullptr; eft::TrackParams tp{}; eft::TrackTail tail{}; eft::TrackerPlan plan{}; };
  TrackGraph tgraph[2];
  // HIP-event sampling (ef_kernel_timing) of the dominant kernel (level 0 of the launch-per-step script), of the IndexMap point splat
  // (k_index_splat of the first predictIndices of a frame) and of the persistent tracker launch
  int ktime_every = 0;
  KernelSampler sample_step, sample_splat, sample_all;
  hipStream_t debug_stream = nullptr;          // ef_debug_occupy
  // Host-pointer entry points of the map operations (ef_host_*.inc): the ONE device landing area their host arguments are staged through, grown
  // on demand, freed by ef_destroy.  Each call lays its own bytes out in it.  What makes one area enough:
  //  - a host-pointer entry point reserves `stage` at most once, before it enqueues anything that reads or writes it;
  //  - it never calls another host-pointer entry point (the _dev tier and the helpers below it take device pointers);
  //  - it ends with hipStreamSynchronize(stream) on success, so nothing of it is in flight when the next one starts;
  //  - after an early error return the next user's copies are ordered behind the leftovers on the same stream, and a reserve that grows
  //    synchronises before it frees.
  DevBuf stage;
  // ef_render_model: its own z-buffer (never the frame's), allocated on first use, grown on demand, freed by ef_destroy
  struct RenderState { DevBuf zbuf; } render;
  // stable surfel IDs and labels (ef_set_surfel_ids / ef_enable_labels; kernels in ef_labels.inc).  ids_state (device, kept for the context's
  // lifetime once allocated): [0] the next ID, [1] the shape flag of ids_check, [2 + k] the row count of label alignment k.  The table and
  // the ID list it was aligned to exist twice (ping-pong, cur the live half), rows rows each, grown on demand.  known is
  // the map count as of known_frames frames (stamps.size()): an upper bound of the count needs no device round trip.
  struct LabelState {
    bool ids_on = false, ids_bad = false;
    unsigned* ids_state = nullptr;
    int C = 0, cur = 0;
    float* tab[2] = {};
    uint32_t* ids[2] = {};
    size_t rows = 0, bound = 0;
    size_t known = 0, known_frames = 0, ev_frames = 0;
    unsigned* count_h = nullptr;           // pinned: the count each label call leaves behind, valid once ev has completed
    hipEvent_t ev = nullptr;
    bool ev_pending = false;
    DevBuf index;                          // the view's index image
  } labels;
  // spatial index and nearest / kNN queries (ef_query_nearest / ef_query_knn; kernels in ef_query.inc).  map_gen counts the calls that can
  // change the map's rows or positions; the index is rebuilt when it or the cell size differs from what the index was built for.
  uint64_t map_gen = 1;
  struct QueryState {
    uint64_t gen = 0;
    float cell = EF_QUERY_DEFAULT_CELL, built_cell = 0.f;
    int lanes = 0;                         // lanes per query; 0 = the measured choice: 16 for nearest, 1 for kNN (ef_debug_query_lanes)
    DevBuf sorted, rows;                   // the cell-sorted copy {x, y, z, conf} and each record's map row: grown together
    DevBuf cells;                          // buckets (ends after the build) followed by the scan's tile sums
    uint32_t nb = 0, n = 0;
  } query;
  // registration against the map (ef_register_step / ef_register_cloud; kernels in ef_register.inc): grown by the first call, freed with the context
  struct RegisterState {
    DevBuf slabs;                          // the workgroups' slabs followed by the step's 32 sums
    double* sums_h = nullptr;              // pinned: the 32 sums of a step
  } reg;
  // select / gather / erase (ef_map_select, ef_map_gather, ef_map_erase; kernels in ef_select.inc): scratch of their own (never c->cs: clean()
  // owns its halves), grown by the first call, freed with the context.  count is the map count as of map_gen == gen.
  struct SelectState {
    DevBuf scratch;                        // chunk counts | chunk offsets | 4 words (the total) | one flag byte per row
    size_t rows = 0;
    uint64_t gen = 0;
    uint32_t count = 0;
  } sel;
  // insert (ef_map_insert; kernels in ef_insert.inc): scratch of its own, sized by the records of a call (which may outnumber the map's capacity),
  // grown by the first call, freed with the context
  struct InsertState {
    DevBuf scratch;                        // chunk counts | chunk offsets | 4 words (the total) | one flag byte per record
    size_t rows = 0;
  } ins;
  // thin (ef_map_thin, ef_map_thin_select; kernels in ef_thin.inc): scratch of its own, sized by the map's rows, grown by the first call, freed
  // with the context
  struct ThinState {
    DevBuf scratch;                        // chunk counts | chunk offsets | 4 words (totals) | participant bytes | representative bytes
    size_t rows = 0;
  } thin;
  // carve (ef_map_carve, ef_map_carve_select; kernel in ef_carve.inc): scratch of its own, sized by the map's rows, grown by the first call,
  // freed with the context
  struct CarveState {
    DevBuf scratch;                        // 4 x {chunk counts | chunk offsets | 4 words}: the selection's and the three tallies | participant bytes
    size_t rows = 0;
  } carve;
  // outliers (ef_map_neighbor_stats, ef_map_outliers_select, ef_map_remove_outliers; kernels in ef_outlier.inc): scratch of its own, sized by
  // the map's rows, grown by the first call, freed with the context
  struct OutlierState {
    DevBuf scratch;                        // the result | the lanes' partial sums and tallies | {mean, count} per row | chunk counts | chunk offsets | 4 words | participant bytes
    size_t rows = 0;
  } outlier;
  // components (ef_map_components, ef_map_components_select, ef_map_remove_components; kernels in ef_components.inc): scratch of its own, sized
  // by the map's rows, grown by the first call, freed with the context
  struct ComponentState {
    DevBuf scratch;                        // the result | parent, label, members per row | chunk counts | chunk offsets | 4 words | node bytes
    size_t rows = 0;
  } components;
  // planes (ef_map_planes, ef_map_planes_select, ef_map_remove_planes; kernels in ef_planes.inc): scratch of its own, sized by the map's rows,
  // grown by the first call, freed with the context
  struct PlaneState {
    DevBuf scratch;                        // result, round state, models | hypotheses, counts | partial sums | label, compacted rows | scan words | node and participant bytes (plane_scratch)
    size_t rows = 0;
  } planes;
  // normals (ef_map_normals, ef_map_normals_select, ef_map_reestimate_normals; kernels in ef_normals.inc): scratch of its own, sized by the map's
  // rows, grown by the first call, freed with the context
  struct NormalState {
    DevBuf scratch;                        // the result | {normal, curvature} per row | {spacing, count} per row | chunk counts | chunk offsets | 4 words | status bytes
    size_t rows = 0;
  } normals;
  // regions (ef_map_regions, ef_map_regions_select, ef_map_remove_regions; kernels in ef_regions.inc and the normals' join): scratch of its own,
  // sized by the map's rows, grown by the first call, freed with the context.  The normals' scratch is not touched
  struct RegionState {
    DevBuf scratch;                        // the result | {normal, curvature}, the stored-normal word, {spacing, count} per row | parent, attach, label, members per row | chunk counts | chunk offsets | 4 words | status bytes | kind bytes
    size_t rows = 0;
  } regions;
  // smoothing (ef_map_smooth, ef_map_smooth_select, ef_map_smooth_apply; kernels in ef_smooth.inc): scratch of its own, sized by the map's rows and
  // by the list's slots K (4 / 8 / 16 for the k in use), grown by the first call and by a call with more of either, freed with the context
  struct SmoothState {
    DevBuf scratch;                        // the result | two position buffers and {normal, curvature} per row | K list slots per row | count, shift per row | chunk counts | chunk offsets | 4 words | status bytes
    size_t rows = 0;
    int slots = 0;
  } smooth;
  // boundaries (ef_map_boundaries, ef_map_boundaries_select; kernels in ef_boundary.inc, the normals' join and the components' union-find):
  // scratch of its own, sized by the map's rows, grown by the first call, freed with the context.  The normals' and the components' scratch are
  // not touched
  struct BoundaryState {
    DevBuf scratch;                        // the two results | {normal, curvature}, {spacing, count}, {gap, count} per row | parent, label, members per row | chunk counts | chunk offsets | 4 words | selection / normal-status / node bytes | status bytes
    size_t rows = 0;
  } boundary;
  // fuse (ef_map_fuse; kernels in ef_fuse.inc) beside the insert's scratch, which its gate and append use: the election's keys (one per map row),
  // match_row and the outcome bytes (one each per record), and the two counts' words (FuseScratch / fuse_scratch in ef_host_insert.inc, beside
  // append_run, which carves it).  Grown by the first call, freed with the context
  struct FuseState {
    DevBuf scratch;
  } fuse;
};

namespace {

#define EF_HIP(ctx, expr)                                                                       \
  do {                                                                                          \
    hipError_t _e = (expr);                                                                     \
    if (_e != hipSuccess) {                                                                     \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(_e);                           \
      return EF_EHIP;                                                                           \
    }                                                                                           \
  } while (0)

// Every entry point that takes a context runs on the CONTEXT's device, whatever device is current on the calling thread
// (two contexts on two GPUs in one process, or a context used from a thread that never called hipSetDevice), and
// leaves the thread's current device as it found it.
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  explicit DeviceGuard(const ef_ctx* c) {
    if (c && hipGetDevice(&prev) == hipSuccess && prev != c->cfg.device) switched = hipSetDevice(c->cfg.device) == hipSuccess;
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

template <typename T>
int dev_alloc(ef_ctx* c, T** p, size_t n, int fill = 0) {
  void* q = nullptr;
  hipError_t e = hipMalloc(&q, n * sizeof(T));
  if (e != hipSuccess) {
    c->err = std::string("hipMalloc: ") + hipGetErrorString(e);
    return EF_ENOMEM;
  }
  e = hipMemsetAsync(q, fill, n * sizeof(T), c->stream);
  if (e != hipSuccess) {
    c->err = std::string("hipMemset: ") + hipGetErrorString(e);
    return EF_EHIP;
  }
  c->allocs.push_back(q);
  *p = (T*)q;
  return EF_OK;
}
#define EF_ALLOC(c, p, n, ...)                                   \
  do {                                                           \
    int _r = dev_alloc((c), &(p), (size_t)(n), ##__VA_ARGS__);   \
    if (_r != EF_OK) return _r;                                  \
  } while (0)
#define EF_TRY(call) do { const int _r = (call); if (_r != EF_OK) return _r; } while (0)
// Nothing when `need` bytes are there; else the stream is waited for (work still queued may use the old buffer), the old buffer freed and a
// new one allocated, its contents undefined.  A failed allocation leaves the buffer empty.
int DevBuf::reserve(ef_ctx* c, size_t need, const char* what, bool* grew) {
  if (grew) *grew = false;
  if (need <= bytes) return EF_OK;
  EF_HIP(c, hipStreamSynchronize(c->stream));
  release();
  hipError_t e = hipMalloc((void**)&p, need);
  if (e != hipSuccess) { p = nullptr; c->err = std::string("hipMalloc (") + what + "): " + hipGetErrorString(e); return EF_ENOMEM; }
  bytes = need;
  if (grew) *grew = true;
  return EF_OK;
}

// scalar per-frame bookkeeping kernels -----------------------------------------------------------
__global__ void k_init_state(eft::TrackState* st, int dense_samples, int pixels) {
  if (threadIdx.x != 0) return;
  st->dense_count = 0;
  st->dense_samples = dense_samples;
  st->map_counts[0] = st->map_counts[1] = 0;
  // RGBDOdometry's constructor (RGBDOdometry.cpp:31-36): errors 0, counts width * height until a step overwrites them
  st->lastICPError = st->lastRGBError = st->lastSO3Error = 0.f;
  st->lastICPCount = st->lastRGBCount = st->lastSO3Count = (float)pixels;
}
// API boundary: the frame tier's column-major index maps are handed out in the reference's row-major order
template <typename T>
__global__ void k_to_rowmajor(const T* __restrict__ src, int cols, int rows, T* __restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cols * rows) return;
  const int y = i / cols, x = i - y * cols;
  dst[i] = src[x * rows + y];
}
// Resize::{image,vertex,time} (Resize.cpp:50-159): NEAREST downsample, destination (a, b) <- source texel (f a + f/2, f b + f/2)
template <typename T>
__global__ void k_resize_nearest(const T* __restrict__ src, int cols, int dw, int dh, int factor, T* __restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= dw * dh) return;
  const int b = i / dw, a = i - b * dw;
  dst[i] = src[(size_t)(b * factor + factor / 2) * cols + (a * factor + factor / 2)];
}
// Ferns.cpp:97-118 / :186-208 on the device: the 4-bit code of every fern on the view Resize::image / Resize::vertex would produce
// (NEAREST, texel (f x + f / 2, f y + f / 2) of the full-resolution fill-in maps), 255 where the depth is not positive, and the number
// of valid codes behind them.  One workgroup of FERN_CODES_PAD threads; table6 rows {x, y, r, g, b, d}.
constexpr int FERN_CODES_PAD = 512, FERN_CODES_BYTES = FERN_CODES_PAD + 16;
__global__ void __launch_bounds__(FERN_CODES_PAD) k_fern_codes(const uchar4* __restrict__ image, const float4* __restrict__ vertex, int cols, int factor,
                                                              const int* __restrict__ table6, int num, uint8_t* __restrict__ codes) {
  __shared__ int wsum[FERN_CODES_PAD / 64];
  const int i = threadIdx.x;
  uint8_t code = 255;
  int good = 0;
  if (i < num) {
    const int x = table6[i * 6], y = table6[i * 6 + 1];
    const size_t texel = (size_t)(y * factor + factor / 2) * cols + (x * factor + factor / 2);
    const float z = vertex[texel].z;
    if (z > 0) {
      const uchar4 p = image[texel];
      code = (uint8_t)((p.x > table6[i * 6 + 2]) << 3 | (p.y > table6[i * 6 + 3]) << 2 | (p.z > table6[i * 6 + 4]) << 1 | ((int)(z * 1000.0f) > table6[i * 6 + 5]));
      good = 1;
    }
  }
  codes[i] = code;
  for (int off = 32; off > 0; off >>= 1) good += __shfl_down(good, off, 64);
  if ((i & 63) == 0) wsum[i >> 6] = good;
  __syncthreads();
  if (i == 0) {
    int g = 0;
    for (int w = 0; w < FERN_CODES_PAD / 64; ++w) g += wsum[w];
    *(int*)(codes + FERN_CODES_PAD) = g;
  }
}
__global__ void k_set_count(unsigned* count_dev, unsigned v) {
  if (threadIdx.x == 0) *count_dev = v;
}

void timer_begin(ef_ctx* c, const char* name) {
  if (!c->timing) return;
  for (auto& t : c->timers)
    if (t.name == name || !strcmp(t.name, name)) { (void)hipEventRecord(t.a, c->stream); t.used = true; return; }
  StageTimer t{name, nullptr, nullptr, true};
  (void)hipEventCreate(&t.a);
  (void)hipEventCreate(&t.b);
  (void)hipEventRecord(t.a, c->stream);
  c->timers.push_back(t);
}
void timer_end(ef_ctx* c, const char* name) {
  if (!c->timing) return;
  for (auto& t : c->timers)
    if (!strcmp(t.name, name)) { (void)hipEventRecord(t.b, c->stream); return; }
}

int grow_trajectory(ef_ctx* c) {
  double* bigger = nullptr;
  EF_HIP(c, hipStreamSynchronize(c->stream));
  hipError_t e = hipMalloc((void**)&bigger, (size_t)c->traj_cap * 2 * 16 * sizeof(double));
  if (e != hipSuccess) { c->err = std::string("hipMalloc (trajectory log): ") + hipGetErrorString(e); return EF_ENOMEM; }
  e = hipMemcpy(bigger, c->traj, (size_t)c->traj_cap * 16 * sizeof(double), hipMemcpyDeviceToDevice);
  if (e != hipSuccess) { (void)hipFree(bigger); c->err = std::string("hipMemcpy (trajectory log): ") + hipGetErrorString(e); return EF_EHIP; }
  for (auto& p : c->allocs)
    if (p == (void*)c->traj) p = bigger;
  (void)hipFree(c->traj);
  c->traj = bigger;
  c->traj_cap *= 2;
  return EF_OK;
}


void pose_of_state(const eft::TrackState& h, double* T16) {
  efl::SE3 T;
  for (int i = 0; i < 4; ++i) T.q[i] = h.q[i];
  for (int i = 0; i < 3; ++i) T.t[i] = h.t[i];
  efl::se3_matrix(T, T16);
}
// a tracker instance's state as it stands once everything enqueued so far has run: one copy, one synchronisation
int read_state(ef_ctx* c, const eft::TrackState* dev, eft::TrackState* h) {
  EF_HIP(c, hipMemcpyAsync(h, dev, sizeof(*h), hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  return EF_OK;
}
// what every tracker call of a context shares; the caller sets rgbOnly, pyramid, fastOdom, so3 and icpWeight (and the empty-model pair)
eft::TrackParams track_params(const ef_ctx* c) {
  eft::TrackParams tp;
  tp.persistent = c->persistent;
  tp.fused_step = c->fused_step ? 1 : 0;
  tp.no_resident = c->no_resident ? 1 : 0;
  tp.distThres = 0.10f;                                   // RGBDOdometry.h:41
  tp.angleThres = sinf(20.f * 3.14159254f / 180.f);       // RGBDOdometry.h:42
  return tp;
}
// the captured tracker graphs hold the script and the knobs they were captured with
void drop_track_graphs(ef_ctx* c) {
  for (auto& g : c->tgraph)
    if (g.exec) { (void)hipGraphExecDestroy(g.exec); g.exec = nullptr; }
}
// a deformation graph (nodes x 16 floats, host) into graph_dev, waited for: the source is free on return; graph_nodes / graph_is_fern are the caller's
int upload_graph(ef_ctx* c, const float* graph16, int nodes) {
  EF_HIP(c, hipMemcpyAsync(c->graph_dev, graph16, (size_t)nodes * 16 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  return EF_OK;
}
// one RGBDOdometry instance's buffers (zero-filled: the stale y/z planes of quirk Q3 are then deterministic), `partials` last.  The
// frame-to-model tracker's nextDepth IS its lastDepth (quirk Q1); the model-to-model and the fern tracker have one of their own.
int alloc_pyramid(ef_ctx* c, eft::Pyramid& p, int w, int h, bool alias_next_depth) {
  p.width = w;
  p.height = h;
  for (int i = 0; i < eft::NUM_PYRS; ++i) {
    const size_t n = (size_t)(w >> i) * (h >> i);
    EF_ALLOC(c, p.depth_tmp[i], n);
    EF_ALLOC(c, p.vmap_curr[i], 3 * n);
    EF_ALLOC(c, p.nmap_curr[i], 3 * n);
    EF_ALLOC(c, p.vmap_g_prev[i], 3 * n);
    EF_ALLOC(c, p.nmap_g_prev[i], 3 * n);
    EF_ALLOC(c, p.lastDepth[i], n);
    if (alias_next_depth) p.nextDepth[i] = p.lastDepth[i];
    else EF_ALLOC(c, p.nextDepth[i], n);
    EF_ALLOC(c, p.lastImage[i], n);
    EF_ALLOC(c, p.nextImage[i], n);
    EF_ALLOC(c, p.lastNextImage[i], n);
    EF_ALLOC(c, p.dIdx[i], n);
    EF_ALLOC(c, p.dIdy[i], n);
    EF_ALLOC(c, p.corres[i], n);
    EF_ALLOC(c, p.rgbMask[i], n);
  }
  EF_ALLOC(c, p.partials, (size_t)eft::PARTIAL_ALLOC_FLOATS);
  return EF_OK;
}
int KernelSampler::create(ef_ctx* c, int capacity) {
  if (!start.empty()) return EF_OK;
  start.resize(capacity);
  stop.resize(capacity);
  for (int i = 0; i < capacity; ++i) {
    EF_HIP(c, hipEventCreate(&start[i]));
    EF_HIP(c, hipEventCreate(&stop[i]));
  }
  probe = eft::KernelProbe{start.data(), stop.data(), capacity, 0};
  return EF_OK;
}
int KernelSampler::average_us(ef_ctx* c, float* us) const {
  EF_HIP(c, hipStreamSynchronize(c->stream));
  double total_ms = 0;
  for (int i = 0; i < probe.used; ++i) {
    float ms = 0;
    EF_HIP(c, hipEventElapsedTime(&ms, start[i], stop[i]));
    total_ms += ms;
  }
  *us = probe.used ? (float)(1e3 * total_ms / probe.used) : 0.f;
  return EF_OK;
}

}  // namespace

// What a frame runs: its loop closures, then the frame itself (each may use what stands above it)
#include "ef_host_closures.inc"
#include "ef_host_frame.inc"

namespace {

int ctx_init(ef_ctx* c) {
  const ef_config& g = c->cfg;
  const int W = g.width, H = g.height;
  const size_t P = (size_t)W * H;
  hipStream_t s = c->stream;
  for (FrameImages* f : {&c->img, &c->img_alt}) {
    EF_ALLOC(c, f->rgb, P * 3);
    EF_ALLOC(c, f->depth_raw, P);
    EF_ALLOC(c, f->depth_filtered, P);
    EF_ALLOC(c, f->depth_metric, P);
    EF_ALLOC(c, f->depth_metric_filtered, P);
  }
  EF_HIP(c, hipStreamCreateWithFlags(&c->in_stream, hipStreamNonBlocking));
  for (auto& e : c->ev_frame_done) EF_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  EF_HIP(c, hipEventCreateWithFlags(&c->ev_input_done, hipEventDisableTiming));
  EF_HIP(c, hipEventCreateWithFlags(&c->ev_track_done, hipEventDisableTiming));
  EF_HIP(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
  for (RingSlot& r : c->ring) {
    EF_HIP(c, hipEventCreateWithFlags(&r.ev_h2d, hipEventDisableTiming));
    EF_HIP(c, hipHostMalloc((void**)&r.h_rgb, P * 3));
    EF_HIP(c, hipHostMalloc((void**)&r.h_depth, P * 2));
    EF_ALLOC(c, r.d_rgb, P * 3);
    EF_ALLOC(c, r.d_depth, P);
  }
  EF_HIP(c, hipHostMalloc((void**)&c->h_consumed, sizeof(unsigned), hipHostMallocMapped));
  *c->h_consumed = 0u;
  EF_HIP(c, hipHostGetDevicePointer((void**)&c->d_consumed, c->h_consumed, 0));
  EF_HIP(c, hipHostMalloc((void**)&c->h_abort, 4 * sizeof(unsigned), hipHostMallocMapped));
  memset(c->h_abort, 0, 4 * sizeof(unsigned));
  EF_HIP(c, hipHostGetDevicePointer((void**)&c->d_abort, c->h_abort, 0));
  // tracker pyramids (zero-filled: the stale y/z planes of quirk Q3 are then deterministic)
  EF_TRY(alloc_pyramid(c, c->pyr, W, H, true));
  EF_ALLOC(c, c->st, 1);
  // prediction images
  EF_ALLOC(c, c->im.index, P);
  EF_ALLOC(c, c->im.vert_conf, P);
  EF_ALLOC(c, c->im.color_time, P);
  EF_ALLOC(c, c->im.norm_rad, P);
  c->im.colmajor = 1;
  EF_ALLOC(c, c->pm.image, P);
  EF_ALLOC(c, c->pm.vertex, P);
  EF_ALLOC(c, c->pm.normal, P);
  EF_ALLOC(c, c->pm.time, P);
  EF_ALLOC(c, c->fm.image, P);
  EF_ALLOC(c, c->fm.vertex, P);
  EF_ALLOC(c, c->fm.normal, P);
  EF_ALLOC(c, c->zbuf, P, 0xFF);
  EF_ALLOC(c, c->zbuf_assoc, P, 0xFF);
  EF_ALLOC(c, c->zbuf_clean, P, 0xFF);
  EF_ALLOC(c, c->im_T16, 16);
  EF_ALLOC(c, c->graph_dev, 1024 * 16);     // GlobalModel::MAX_NODES x 16 (GlobalModel.cpp:24)
  EF_ALLOC(c, c->synth_depth, P);
  EF_ALLOC(c, c->rays, P * 4);
  EF_ALLOC(c, c->overflow, 1);
  // global model
  c->capacity = g.max_surfels;
  for (int k = 0; k < 2; ++k) {
    EF_ALLOC(c, c->maps[k].pos_conf, c->capacity);
    EF_ALLOC(c, c->maps[k].col_time, c->capacity);
    EF_ALLOC(c, c->maps[k].nrm_rad, c->capacity);
  }
  EF_ALLOC(c, c->winner, c->capacity, 0xFF);
  c->cand.n = (W / 2) * (H / 2);
  EF_ALLOC(c, c->cand.pos_conf, c->cand.n);
  EF_ALLOC(c, c->cand.col_time, c->cand.n);
  EF_ALLOC(c, c->cand.nrm_rad, c->cand.n);
  EF_ALLOC(c, c->cand.best, c->cand.n);
  c->cs.max_chunks = (int)((c->capacity + (size_t)c->cand.n + 2 * P) / efm::CLEAN_ROW + 8);
  EF_ALLOC(c, c->cs.flags, (size_t)c->capacity + c->cand.n + 2 * P);
  EF_ALLOC(c, c->cs.chunk_count, c->cs.max_chunks);
  EF_ALLOC(c, c->cs.chunk_offset, c->cs.max_chunks);
  EF_ALLOC(c, c->cs.totals, 8);
  c->cs.max_groups = c->cs.max_chunks / efm::CLEAN_GROUP + 2;
  EF_ALLOC(c, c->cs.group_sum, 2 * (size_t)c->cs.max_groups * efm::CLEAN_GSTRIDE);   // (zero-filled: what the first clean() expects of its half)
  if (g.close_loops) {
    EF_TRY(alloc_pyramid(c, c->pyr2, W, H, false));
    EF_ALLOC(c, c->st2, 1);
    EF_ALLOC(c, c->old.image, P);
    EF_ALLOC(c, c->old.vertex, P);
    EF_ALLOC(c, c->old.normal, P);
    EF_ALLOC(c, c->old.time, P);
    EF_ALLOC(c, c->cons_dev, (size_t)(W / 20) * (H / 20) * 4 + 4);
    EF_ALLOC(c, c->nodes_dev, (size_t)1024 * 4 + 4);
    EF_HIP(c, hipHostMalloc((void**)&c->h_cons, ((size_t)(W / 20) * (H / 20) * 4 + 4) * sizeof(float)));
    EF_HIP(c, hipHostMalloc((void**)&c->h_states, 3 * sizeof(eft::TrackState)));
    hipLaunchKernelGGL(k_init_state, dim3(1), dim3(64), 0, s, c->st2, (W / 20) * (H / 20), W * H);
  }
  c->traj_cap = 1 << 10;   // doubled on demand (grow_trajectory)
  EF_ALLOC(c, c->traj, (size_t)c->traj_cap * 16);
  // T_wc = identity (ElasticFusion.h: T_wc_curr default) -> publish the float matrices
  hipLaunchKernelGGL(k_init_state, dim3(1), dim3(64), 0, s, c->st, (W / 20) * (H / 20), W * H);
  c->tally_by_consumer = (W / 20) * (H / 20) <= 1024;
  efm::build_ray_table(c->cam, c->rays, s);
  const double I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  eft::pose_injected(c->st, I16, false, 1.0f, false, nullptr, 0, s);
  eft::pose_injected(c->st, I16, true, 1.0f, false, nullptr, 0, s);   // previous pose = identity too
  EF_HIP(c, hipStreamSynchronize(s));
  return EF_OK;
}

void ctx_free(ef_ctx* c) {
  if (c->in_stream) (void)hipStreamSynchronize(c->in_stream);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->stream) eft::persistent_chain_forget(c->stream);   // (a borrowed stream may be destroyed by its owner right after this call)
  if (c->in_stream) (void)hipStreamDestroy(c->in_stream);
  for (hipEvent_t e : {c->ev_input_done, c->ev_track_done, c->ev_frame_done[0], c->ev_frame_done[1]})
    if (e) (void)hipEventDestroy(e);
  for (void* p : c->allocs) (void)hipFree(p);
  if (c->h_abort) (void)hipHostFree(c->h_abort);
  if (c->copy_stream) { (void)hipStreamSynchronize(c->copy_stream); (void)hipStreamDestroy(c->copy_stream); }
  for (RingSlot& r : c->ring) {
    if (r.ev_h2d) (void)hipEventDestroy(r.ev_h2d);
    if (r.h_rgb) (void)hipHostFree(r.h_rgb);
    if (r.h_depth) (void)hipHostFree(r.h_depth);
  }
  for (void* p : {(void*)c->h_consumed, (void*)c->h_cons, (void*)c->h_states, (void*)c->h_view, (void*)c->h_view_end, (void*)c->h_codes, (void*)c->h_codes_end})
    if (p) (void)hipHostFree(p);
  if (c->ev_end_record) (void)hipEventDestroy(c->ev_end_record);
  if (c->h_nodes_pinned) (void)hipHostFree(c->h_nodes_pinned);
  if (c->closure) ef_closure_destroy(c->closure);
  for (auto& t : c->timers) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
  for (KernelSampler* k : {&c->sample_step, &c->sample_all, &c->sample_splat}) k->release();
  drop_track_graphs(c);
  if (c->debug_stream) { (void)hipStreamSynchronize(c->debug_stream); (void)hipStreamDestroy(c->debug_stream); }
  for (DevBuf* b : {&c->stage, &c->render.zbuf, &c->labels.index, &c->query.sorted, &c->query.rows, &c->query.cells, &c->reg.slabs, &c->sel.scratch, &c->ins.scratch, &c->thin.scratch, &c->carve.scratch, &c->outlier.scratch, &c->components.scratch, &c->planes.scratch, &c->normals.scratch, &c->regions.scratch, &c->smooth.scratch, &c->boundary.scratch, &c->fuse.scratch})
    b->release();
  for (int k = 0; k < 2; ++k) {
    if (c->labels.tab[k]) (void)hipFree(c->labels.tab[k]);
    if (c->labels.ids[k]) (void)hipFree(c->labels.ids[k]);
  }
  if (c->labels.ids_state) (void)hipFree(c->labels.ids_state);
  if (c->labels.count_h) (void)hipHostFree(c->labels.count_h);
  if (c->labels.ev) (void)hipEventDestroy(c->labels.ev);
  if (c->reg.sums_h) (void)hipHostFree(c->reg.sums_h);
  if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
}

// ---- what the map's download / upload and the map operations (ef_host_*.inc) share ----
// never inside a capture: a map operation recorded into a graph would be replayed with every frame
int capture_check(ef_ctx* c, const char* fn) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  EF_HIP(c, hipStreamIsCapturing(c->stream, &cs));
  if (cs != hipStreamCaptureStatusNone) { c->err = std::string(fn) + ": the context's stream is being captured"; return EF_ESTATE; }
  return EF_OK;
}
int read_count(ef_ctx* c, uint32_t* n) {
  EF_HIP(c, hipMemcpyAsync(n, &c->st->map_counts[c->cur], sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  return EF_OK;
}
// the two float pose matrices derived from a double T_wc
void pose_mats(const double* T16, float* Tcw_host, float* pose_host) {
  const efl::SE3 T = efl::se3_from_matrix(T16);
  efl::se3_inverse_matrix_f(T, Tcw_host);
  efl::se3_castf_matrix(T, pose_host);
}
// T (row-major 4 x 4 doubles) as the f32 rotation and translation the map kernels take: every entry rounded once
void pose_Rt(const double* T, float* R, float* t) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) R[i * 3 + j] = (float)T[i * 4 + j];
    t[i] = (float)T[i * 4 + 3];
  }
}
bool finite16(const double* T) {
  for (int i = 0; i < 16; ++i)
    if (!std::isfinite(T[i])) return false;
  return true;
}
// the lazy numbering every ID-consuming call starts with
int ids_prepare(ef_ctx* c, const char* fn) {
  if (c->labels.ids_bad) {
    c->err = std::string(fn) + ": the uploaded map's ID lane (float 5 of each surfel) is not a strictly increasing non-zero prefix followed by "
             "a zero suffix, or numbering that suffix above its largest ID and above every ID handed out so far would pass 0xFFFFFFFE: the "
             "numbering would wrap";
    return EF_ESTATE;
  }
  efm::ids_assign(c->maps[c->cur], &c->st->map_counts[c->cur], c->labels.ids_state, c->stream);
  EF_HIP(c, hipGetLastError());
  return EF_OK;
}
// ef_map_upload with IDs on: the uploaded lane is kept when its shape is valid (the counter then continues above its largest ID, ids_assign);
// any other shape, and a lane whose zero suffix cannot be numbered from there without leaving uint32 (the numbering would wrap to 0 or below the
// prefix), is remembered and refused by the next ID-consuming call.  Labels restart from the prior.
int ids_uploaded(ef_ctx* c, uint32_t count) {
  EF_HIP(c, hipMemsetAsync(c->labels.ids_state + 1, 0, sizeof(unsigned), c->stream));
  efm::ids_check(c->maps[c->cur], count, c->labels.ids_state, c->labels.ids_state + 1, c->stream);
  EF_HIP(c, hipGetLastError());
  unsigned flag = 0;
  EF_HIP(c, hipMemcpyAsync(&flag, c->labels.ids_state + 1, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  c->labels.ids_bad = flag != 0;
  if (c->labels.C) {
    EF_HIP(c, hipMemsetAsync(c->labels.ids_state + 2 + c->labels.cur, 0, sizeof(unsigned), c->stream));
    c->labels.known = count;
    c->labels.known_frames = c->stamps.size();
    c->labels.ev_pending = false;
  }
  return EF_OK;
}

}  // namespace

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

void ef_default_config(ef_config* cfg) {
  memset(cfg, 0, sizeof(*cfg));
  cfg->width = 640; cfg->height = 480;                          // MainController.cpp:37
  cfg->fx = 528; cfg->fy = 528; cfg->cx = 320; cfg->cy = 240;   // MainController.cpp:42
  cfg->time_delta = 2147483647 / 2;                             // -o, MainController.cpp:179-183
  cfg->confidence = 10.0f;                                      // MainController.cpp:69
  cfg->depth_cut = 3.0f;                                        // MainController.cpp:70
  cfg->icp_weight = 10.0f;                                      // MainController.cpp:71
  cfg->fast_odom = 0; cfg->so3 = 1; cfg->frame_to_frame_rgb = 0; cfg->pyramid = 1; cfg->rgb_only = 0;
  cfg->close_loops = 0;
  cfg->max_surfels = 4u * 1024u * 1024u;
  cfg->device = 0;
  cfg->stream = nullptr;
}

int ef_create(const ef_config* cfg, ef_ctx** out) {
  if (!cfg || !out) { g_create_error = "null argument"; return EF_EINVAL; }
  if (cfg->width <= 0 || cfg->height <= 0 || (cfg->width % 4) || (cfg->height % 4) || cfg->fx <= 0 || cfg->fy <= 0) {
    g_create_error = "width/height must be positive multiples of 4 and focal lengths positive";
    return EF_EINVAL;
  }
  if ((size_t)cfg->max_surfels < (size_t)cfg->width * cfg->height) { g_create_error = "max_surfels must be >= width*height"; return EF_EINVAL; }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0) {
    g_create_error = std::string("no HIP device: ") + hipGetErrorString(e);
    return EF_EHIP;
  }
  if (cfg->device < 0 || cfg->device >= ndev) { g_create_error = "bad device ordinal"; return EF_EINVAL; }
  ef_ctx* c = new ef_ctx();
  c->cfg = *cfg;
  DeviceGuard dg_(c);   // the context's device for the allocations below; the caller's current device is restored on return
  {
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != cfg->device) { g_create_error = "hipSetDevice failed"; delete c; return EF_EHIP; }
  }
  c->cam = efm::Cam{cfg->width, cfg->height, cfg->fx, cfg->fy, cfg->cx, cfg->cy};
  c->intr = eft::Intr{cfg->fx, cfg->fy, cfg->cx, cfg->cy};
  {
    // the persistent tracker launch needs its workgroups resident together, one per CU (fast order: 256, the reference-order launch of
    // the small levels: 128): on a device (or a partition of one: CPX mode exposes 32 CUs) that cannot hold them the per-step script is
    // the default; ef_set_persistent_tracker can still ask for it (the fast order's launch then falls back to one workgroup every frame)
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->device) != hipSuccess) cus = 0;
    if (cus < 256) {
#ifdef EF_FAST_ORDER
      c->persistent = 0;
#else
      c->persistent = cus >= eft::PT_WGS ? 2 : 0;   // round 3's launch of the small levels needs 128 co-resident workgroups
#endif
    }
  }
  if (cfg->stream) {
    c->stream = (hipStream_t)cfg->stream;
  } else {
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { g_create_error = std::string("hipStreamCreate: ") + hipGetErrorString(e); delete c; return EF_EHIP; }
    c->own_stream = true;
  }
  c->bil_table = efm::bilateral_table();
  if (!c->bil_table) {   // the depth filter's weight table of this device (built once per process and device, here at the latest)
    g_create_error = "bilateral weight table: allocation or launch failed";
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return EF_EHIP;
  }
  const int r = ctx_init(c);
  if (r != EF_OK) {
    g_create_error = c->err;
    ctx_free(c);
    delete c;
    return r;
  }
  *out = c;
  return EF_OK;
}

void ef_destroy(ef_ctx* c) {
  if (!c) return;
  DeviceGuard dg_(c);
  ctx_free(c);
  delete c;
}
const char* ef_last_error(const ef_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }
void* ef_stream(ef_ctx* c) { return c ? (void*)c->stream : nullptr; }
static int check_capacity(ef_ctx* c);
int ef_synchronize(ef_ctx* c) {
  if (!c) return EF_EINVAL;
  DeviceGuard dg_(c);
  EF_HIP(c, hipStreamSynchronize(c->stream));
  {
    const int rf = flush_end_record(c);
    if (rf != EF_OK) return rf;
  }
  for (const eft::Pyramid* p : {&c->pyr, &c->pyr2, &c->pyr3}) {
    const int a = eft::tracker_aborted(*p, c->stream);
    if (a != 0) {
      c->err = a > 0 ? "a persistent tracker launch timed out waiting for another workgroup AFTER its whole grid had reported in (with the fast "
                       "order this is a protocol failure, not a busy chip: a chip partly taken is handled by the one-workgroup fallback, "
                       "ef_get_tracker_fallbacks): results since then are invalid; recreate the context, or run it with "
                       "ef_set_persistent_tracker(ctx, 0)"
                     : "hipMemcpy (tracker status)";
      return EF_EHIP;
    }
  }
  return check_capacity(c);
}

// The input stream restricted to every n-th CU (hipExtStreamCreateWithCUMask; n <= 1: the whole chip): the next frame's bilateral filter —
// the one ALU-bound kernel of a frame — then runs beside the previous frame's fusion and prediction on a quarter of the chip instead of
// flooding every CU the latency-bound map kernels are trying to run on.
int ef_set_input_cu_mask(ef_ctx* c, int one_in_n) {
  if (!c || one_in_n < 0 || one_in_n > 32) return EF_EINVAL;
  DeviceGuard dg_(c);
  EF_HIP(c, hipStreamSynchronize(c->stream));
  if (c->in_stream) { EF_HIP(c, hipStreamSynchronize(c->in_stream)); EF_HIP(c, hipStreamDestroy(c->in_stream)); c->in_stream = nullptr; }
  if (one_in_n <= 1) {
    EF_HIP(c, hipStreamCreateWithFlags(&c->in_stream, hipStreamNonBlocking));
    return EF_OK;
  }
  int cus = 0;
  EF_HIP(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->cfg.device));
  std::vector<uint32_t> mask((size_t)(cus + 31) / 32, 0u);
  for (int i = 0; i < cus; i += one_in_n) mask[(size_t)i / 32] |= 1u << (i % 32);
  EF_HIP(c, hipExtStreamCreateWithCUMask(&c->in_stream, (uint32_t)mask.size(), mask.data()));
  return EF_OK;
}
int ef_set_input_overlap(ef_ctx* c, int on) {
  if (!c || on < 0 || on > 2) return EF_EINVAL;
  c->overlap = on != 0;
  c->overlap_mode = on == 2 ? 2 : 1;
  c->events_live = false;   // (the next overlapped frame joins the streams on the host: the events of the other mode were not recorded)
  return EF_OK;
}
int ef_set_deformation(ef_ctx* c, const float* graph, int nodes, int is_fern) {
  if (!c || nodes < 0 || (nodes > 0 && !graph)) return EF_EINVAL;
  DeviceGuard dg_(c);
  if (nodes >= 1024) { c->err = "ef_set_deformation: at most 1023 nodes (GlobalModel::MAX_NODES)"; return EF_EINVAL; }
  if (nodes > 0) EF_TRY(upload_graph(c, graph, nodes));   // (waited for: the caller's buffer is borrowed for the call only)
  c->graph_nodes = nodes;
  c->graph_is_fern = is_fern != 0;
  return EF_OK;
}
int ef_set_loop_thresholds(ef_ctx* c, int icp_count_thresh, float icp_err_thresh, float cov_thresh) {
  if (!c) return EF_EINVAL;
  c->icp_count_thresh = icp_count_thresh; c->icp_err_thresh = icp_err_thresh; c->cov_thresh = cov_thresh;
  return EF_OK;
}
int ef_set_loop_solver(ef_ctx* c, ef_loop_solver fn, void* user) {
  if (!c) return EF_EINVAL;
  if (!c->cfg.close_loops) { c->err = "ef_set_loop_solver: the context was created with close_loops = 0"; return EF_ESTATE; }
  c->solver = fn; c->solver_user = user;
  return EF_OK;
}
int ef_use_builtin_loop_solver(ef_ctx* c, int on) {
  if (!c) return EF_EINVAL;
  if (!c->cfg.close_loops) { c->err = "ef_use_builtin_loop_solver: the context was created with close_loops = 0"; return EF_ESTATE; }
  c->builtin_solver = on != 0;
  return EF_OK;
}
int ef_solve_local_deformation(const float* nodes4, int n_nodes, const double* constraints8, int n_constraints, int64_t src_time,
                               int64_t last_deform_time, float* graph16_out, float* error_out, float* mean_constraint_error_out) {
  if (!nodes4 || !constraints8 || !graph16_out || n_nodes < 0 || n_nodes > 1023 || n_constraints < 0) return EF_EINVAL;
  const efd::Result r = efd::solve_local(nodes4, n_nodes, constraints8, n_constraints, (uint64_t)src_time, (uint64_t)last_deform_time, graph16_out);
  if (error_out) *error_out = r.error;
  if (mean_constraint_error_out) *mean_constraint_error_out = r.meanConsErr;
  return r.ok ? EF_OK : EF_ESTATE;
}
int ef_solve_deformation(const float* nodes4, int n_nodes, const ef_graph_constraint* constraints, int n_constraints, int fern_match,
                         int64_t last_deform_time, double* poses16, const int64_t* pose_times, int n_poses, float* graph16_out, float* error_out,
                         float* mean_constraint_error_out, ef_graph_constraint* new_relative_out, int* n_new_relative_out) {
  return ef_solve_deformation_gated(nodes4, n_nodes, constraints, n_constraints, fern_match, last_deform_time, poses16, pose_times, n_poses, graph16_out,
                                    error_out, mean_constraint_error_out, new_relative_out, n_new_relative_out, nullptr);
}
int ef_solve_deformation_gated(const float* nodes4, int n_nodes, const ef_graph_constraint* constraints, int n_constraints, int fern_match,
                               int64_t last_deform_time, double* poses16, const int64_t* pose_times, int n_poses, float* graph16_out, float* error_out,
                               float* mean_constraint_error_out, ef_graph_constraint* new_relative_out, int* n_new_relative_out, const float* gates3) {
  if (!nodes4 || !constraints || !graph16_out || n_nodes < 0 || n_nodes > 1023 || n_constraints < 0 || n_poses < 0 || (n_poses > 0 && (!poses16 || !pose_times)))
    return EF_EINVAL;
  std::vector<efd::Constraint> cons((size_t)n_constraints);
  for (int i = 0; i < n_constraints; ++i) {
    const ef_graph_constraint& c = constraints[i];
    cons[i] = efd::Constraint{{c.src[0], c.src[1], c.src[2]}, {c.target[0], c.target[1], c.target[2]}, (uint64_t)c.src_time, (uint64_t)c.target_time,
                              c.relative != 0, c.pin != 0};
  }
  efd::Result r{false, 0, 0.f, 0.f};
  std::vector<efd::Constraint> rel;
  const efd::Gates gates = gates3 ? efd::Gates{gates3[0], gates3[1], gates3[2]} : efd::Gates();
  const bool updated = efd::constrain(nodes4, n_nodes, cons.data(), n_constraints, fern_match != 0, (uint64_t)last_deform_time, poses16, pose_times, n_poses,
                                      graph16_out, &r, new_relative_out ? &rel : nullptr, gates);
  if (n_new_relative_out) *n_new_relative_out = (int)rel.size();
  for (size_t i = 0; new_relative_out && i < rel.size(); ++i) {
    ef_graph_constraint& o = new_relative_out[i];
    for (int k = 0; k < 3; ++k) { o.src[k] = rel[i].src[k]; o.target[k] = rel[i].target[k]; }
    o.src_time = (int64_t)rel[i].srcTime; o.target_time = (int64_t)rel[i].targetTime; o.relative = 1; o.pin = 0;
  }
  if (error_out) *error_out = r.error;
  if (mean_constraint_error_out) *mean_constraint_error_out = r.meanConsErr;
  return updated ? EF_OK : EF_ESTATE;
}
int ef_enable_global_closure(ef_ctx* c, int num_ferns, float photo_thresh, float fern_thresh, unsigned seed) {
  if (!c || num_ferns < 50) return EF_EINVAL;
  if (num_ferns > FERN_CODES_PAD) { c->err = "ef_enable_global_closure: at most 512 ferns"; return EF_EINVAL; }   // (every refusal before the first allocation)
  DeviceGuard dg_(c);
  if (!c->cfg.close_loops) { c->err = "ef_enable_global_closure: the context was created with close_loops = 0"; return EF_ESTATE; }
  if (c->closure) { c->err = "ef_enable_global_closure: already enabled"; return EF_ESTATE; }
  const int W = c->cam.cols, H = c->cam.rows;
  if ((W / 8) % 4 || (H / 8) % 4 || W % 8 || H % 8) { c->err = "ef_enable_global_closure: width and height must be multiples of 32"; return EF_EINVAL; }
  c->fern_w = W / 8;
  c->fern_h = H / 8;
  const size_t n = (size_t)c->fern_w * c->fern_h;
  EF_ALLOC(c, c->view_img_dev, n);
  EF_ALLOC(c, c->view_vert_dev, n);
  EF_ALLOC(c, c->view_norm_dev, n);
  EF_ALLOC(c, c->fern_maps_dev, 5 * n);   // 4 maps + a zero image (the 1/8 tracker never reads colour: icpWeight = 100)
  EF_HIP(c, hipHostMalloc((void**)&c->h_view, n * 36));
  EF_HIP(c, hipHostMalloc((void**)&c->h_view_end, n * 36));
  EF_HIP(c, hipHostMalloc((void**)&c->h_codes, FERN_CODES_BYTES));
  EF_HIP(c, hipHostMalloc((void**)&c->h_codes_end, FERN_CODES_BYTES));
  c->fern_num = num_ferns;
  EF_ALLOC(c, c->fern_table_dev, (size_t)num_ferns * 6);
  EF_ALLOC(c, c->fern_codes_dev, (size_t)FERN_CODES_BYTES);
  EF_HIP(c, hipEventCreateWithFlags(&c->ev_end_record, hipEventDisableTiming));
  EF_HIP(c, hipHostMalloc((void**)&c->h_nodes_pinned, ((size_t)1024 * 4 + 4) * sizeof(float)));
  memset(c->h_nodes_pinned, 0, ((size_t)1024 * 4 + 4) * sizeof(float));
  c->intr3 = eft::Intr{c->cfg.fx / 8, c->cfg.fy / 8, c->cfg.cx / 8, c->cfg.cy / 8};   // Ferns.cpp:31-36
  EF_TRY(alloc_pyramid(c, c->pyr3, c->fern_w, c->fern_h, false));
  EF_ALLOC(c, c->st3, 1);
  hipLaunchKernelGGL(k_init_state, dim3(1), dim3(64), 0, c->stream, c->st3, 1, c->fern_w * c->fern_h);
  EF_HIP(c, hipStreamSynchronize(c->stream));
  memset(&c->gloop, 0, sizeof(c->gloop));
  c->gloop.closest = -1;
  c->closure = ef_closure_create(num_ferns, c->cfg.depth_cut, photo_thresh, fern_thresh, W, H, c->cfg.fx, c->cfg.fy, c->cfg.cx, c->cfg.cy, seed);
  if (!c->closure) { c->err = "ef_closure_create failed"; return EF_ENOMEM; }
  return EF_OK;
}
int ef_set_relocalisation(ef_ctx* c, int on) {
  if (!c) return EF_EINVAL;
  c->reloc = on != 0;
  if (!c->reloc) { c->lost = false; c->last_frame_recovery = false; c->tracking_count = 0; c->tracking_ok = true; }
  return EF_OK;
}
int ef_set_graph_replay(ef_ctx* c, int on) { if (!c) return EF_EINVAL; c->use_graph = on != 0; return EF_OK; }
int ef_set_fused_step(ef_ctx* c, int on) {
  if (!c) return EF_EINVAL;
  c->fused_step = on != 0;
  drop_track_graphs(c);
  return EF_OK;
}
int ef_set_track_only(ef_ctx* c, int on) { if (!c) return EF_EINVAL; c->track_only = on != 0; return EF_OK; }
int ef_set_resident_levels(ef_ctx* c, int on) { if (!c) return EF_EINVAL; c->no_resident = on == 0; return EF_OK; }
int ef_set_persistent_tracker(ef_ctx* c, int on) {
  if (!c) return EF_EINVAL;
  c->persistent = on < 0 ? 0 : (on > 2 ? 1 : on);
#ifdef EF_FAST_ORDER
  if (c->persistent == 2) c->persistent = 1;   // (the fast order has no launch of the small levels: 2 means 1 there, also to process_frame's overlap rule)
#endif
  drop_track_graphs(c);   // they hold the other script
  return EF_OK;
}
int ef_set_tick(ef_ctx* c, int tick) { if (!c) return EF_EINVAL; c->tick = tick; return EF_OK; }
// developer instrumentation (tests/test_gpu_fallback.py): `workgroups` workgroups of 1024 threads and 128 registers per lane — each fills the
// register file of a whole CU — spin for `microseconds` on a stream of their own: the chip is partly taken, as by another process
__global__ void __launch_bounds__(1024) k_debug_occupy(unsigned long long ticks, unsigned* started) {
  asm volatile("v_mov_b32 v127, 0" ::: "v127");
  if (threadIdx.x == 0) __hip_atomic_fetch_add(started, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  const unsigned long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
}
int ef_debug_occupy(ef_ctx* c, int workgroups, int microseconds) {
  if (!c || workgroups < 1 || workgroups > 1024 || microseconds < 1 || microseconds > 2000000) return EF_EINVAL;
  DeviceGuard dg_(c);
  // (a stream of ANOTHER priority: the runtime multiplexes the streams of a process onto a few hardware queues, and a spinner that sits in the
  // queue the compute or the copy stream maps to holds up the frame itself — what the spinners stand for, another process, has queues of its own)
  if (!c->debug_stream) {
    int lo = 0, hi = 0;
    EF_HIP(c, hipDeviceGetStreamPriorityRange(&lo, &hi));
    EF_HIP(c, hipStreamCreateWithPriority(&c->debug_stream, hipStreamNonBlocking, hi));
  }
  // The call returns once every spinner IS resident (they report in through a host-mapped word): a spinner needs a whole idle CU, and since round 6
  // the frame script leaves no bubble in which one could slip in — enqueued right before a frame, the spinners would start behind it and the
  // test would exercise nothing.  The compute stream is drained first so that they find the chip idle.
  EF_HIP(c, hipStreamSynchronize(c->stream));
  c->h_abort[3] = 0u;
  hipLaunchKernelGGL(k_debug_occupy, dim3(workgroups), dim3(1024), 0, c->debug_stream, (unsigned long long)microseconds * 100ull, c->d_abort + 3);
  EF_HIP(c, hipGetLastError());
  volatile unsigned* started = c->h_abort + 3;
  for (int spin = 0; spin < 2000000 && *started < (unsigned)workgroups; ++spin) std::this_thread::yield();
  if (*started < (unsigned)workgroups) { c->err = "ef_debug_occupy: the spinners did not become resident"; return EF_EHIP; }
  return EF_OK;
}
// clean() clamps the new surfel count to the capacity and raises a device flag (the reference's fixed 3072 x 3072 vertex
// buffer simply overflows, GlobalModel.cpp:22-24).  The flag is a WARNING: ef_synchronize reports it once (EF_ECAPACITY) and
// clears it; the clamped map stays readable (ef_map_count / ef_map_download / ef_save_ply proceed with the clamped count).
static int check_capacity(ef_ctx* c) {
  int flag = 0;
  EF_HIP(c, hipMemcpyAsync(&flag, c->overflow, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  EF_HIP(c, hipStreamSynchronize(c->stream));
  if (flag) {
    EF_HIP(c, hipMemsetAsync(c->overflow, 0, sizeof(int), c->stream));
    c->err = "surfel capacity exceeded (ef_config.max_surfels = " + std::to_string(c->capacity) + "): the newest surfels were dropped";
    return EF_ECAPACITY;
  }
  return EF_OK;
}
int ef_set_reference_download(ef_ctx* c, int on) {
  if (!c) return EF_EINVAL;
  DeviceGuard dg_(c);
  if (on && !c->shadow.pos_conf) {   // zero-filled like the reference's vertex buffers (GlobalModel.cpp:72-75)
    EF_ALLOC(c, c->shadow.pos_conf, c->capacity);
    EF_ALLOC(c, c->shadow.col_time, c->capacity);
    EF_ALLOC(c, c->shadow.nrm_rad, c->capacity);
  }
  c->reference_download = on != 0;
  return EF_OK;
}
int ef_map_upload(ef_ctx* c, const float* surfels, uint32_t count) {
  if (!c || (!surfels && count)) return EF_EINVAL;
  DeviceGuard dg_(c);
  if (count > c->capacity) { c->err = "ef_map_upload: count exceeds max_surfels"; return EF_ECAPACITY; }
  ++c->map_gen;
  float* tmp = nullptr;
  if (count) {
    EF_HIP(c, hipMalloc((void**)&tmp, (size_t)count * 48));
    hipError_t e = hipMemcpyAsync(tmp, surfels, (size_t)count * 48, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
      efm::aos_to_soa(tmp, count, c->maps[c->cur], c->stream);
      e = hipStreamSynchronize(c->stream);
    }
    (void)hipFree(tmp);
    EF_HIP(c, e);
  }
  hipLaunchKernelGGL(k_set_count, dim3(1), dim3(64), 0, c->stream, &c->st->map_counts[c->cur], count);
  if (c->labels.ids_on) return ids_uploaded(c, count);
  return EF_OK;
}
// Resume from a checkpoint (include/ef_hip.h): the end-of-frame state of the frame `rgb_prev` / `depth_prev` was, on the uploaded map
int ef_restore_state(ef_ctx* c, int tick, const double* q4_t3, const uint8_t* rgb_prev, const uint16_t* depth_prev) {
  if (!c || !q4_t3 || !rgb_prev || !depth_prev || tick < 2) return EF_EINVAL;
  DeviceGuard dg_(c);
  ++c->map_gen;
  hipStream_t s = c->stream;
  const int W = c->cam.cols, H = c->cam.rows;
  if (c->closure) {
    // the fern database and the pose graph are not part of a checkpoint: a record still pending from before the restore belongs to the OLD
    // replay and goes where it was headed before tick and pose change under it
    const int fr = flush_end_record(c);
    if (fr != EF_OK) return fr;
  }
  EF_HIP(c, hipMemcpyAsync(c->img.rgb, rgb_prev, (size_t)W * H * 3, hipMemcpyHostToDevice, s));
  EF_HIP(c, hipMemcpyAsync(c->img.depth_raw, depth_prev, (size_t)W * H * 2, hipMemcpyHostToDevice, s));
  EF_HIP(c, hipStreamSynchronize(s));   // the caller's buffers are pageable and only borrowed
  if (!efm::preprocess_depth(c->img.depth_raw, W, H, c->cfg.depth_cut, c->img.depth_filtered, c->img.depth_metric, c->img.depth_metric_filtered, s, 0u, nullptr,
                             nullptr, nullptr, c->bil_table)) {
    c->err = "bilateral weight table missing on this device";
    return EF_EHIP;
  }
  // the frame's intensity pyramid where the next frame's SO(3) pre-alignment looks for it (lastNextImage: initFirstRGB's target and,
  // after every tracked frame, the swapped-in nextImage, RGBDOdometry.cpp:246-257,284-288)
  eft::init_first_rgb(c->pyr, c->img.rgb, s);
  efl::SE3 T;
  for (int i = 0; i < 4; ++i) T.q[i] = q4_t3[i];
  for (int i = 0; i < 3; ++i) T.t[i] = q4_t3[4 + i];
  eft::pose_restored(c->st, T.q, T.t, s);
  c->tick = tick;
  c->lost = c->last_frame_recovery = false;
  c->tracking_ok = true;
  c->tracking_count = 0;
  c->graph_nodes = 0;
  const int r = do_predict(c);
  EF_HIP(c, hipGetLastError());
  return r;
}
int ef_set_rgb_only(ef_ctx* c, int v) { if (!c) return EF_EINVAL; c->cfg.rgb_only = v; return EF_OK; }
int ef_set_icp_weight(ef_ctx* c, float v) { if (!c) return EF_EINVAL; c->cfg.icp_weight = v; return EF_OK; }
int ef_set_pyramid(ef_ctx* c, int v) { if (!c) return EF_EINVAL; c->cfg.pyramid = v; return EF_OK; }
int ef_set_fast_odom(ef_ctx* c, int v) { if (!c) return EF_EINVAL; c->cfg.fast_odom = v; return EF_OK; }
int ef_set_so3(ef_ctx* c, int v) { if (!c) return EF_EINVAL; c->cfg.so3 = v; return EF_OK; }
int ef_set_frame_to_frame_rgb(ef_ctx* c, int v) { if (!c) return EF_EINVAL; c->cfg.frame_to_frame_rgb = v; return EF_OK; }
int ef_set_confidence_threshold(ef_ctx* c, float v) { if (!c) return EF_EINVAL; c->cfg.confidence = v; return EF_OK; }
int ef_set_depth_cutoff(ef_ctx* c, float v) { if (!c) return EF_EINVAL; c->cfg.depth_cut = v; return EF_OK; }

}  // extern "C"

// Looking at a context: getters, timers, kernel sampling, debug hooks
#include "ef_host_inspect.inc"


// The map operations' host code, one file beside each kernel file of ef_map_kernels.hip, in dependency order (each may use what the ones before it define)
#include "ef_host_ops.inc"
#include "ef_host_render.inc"
#include "ef_host_labels.inc"
#include "ef_host_query.inc"
#include "ef_host_register.inc"
#include "ef_host_select.inc"
#include "ef_host_insert.inc"
#include "ef_host_thin.inc"
#include "ef_host_carve.inc"
#include "ef_host_outlier.inc"
#include "ef_host_components.inc"
#include "ef_host_planes.inc"
#include "ef_host_normals.inc"
#include "ef_host_regions.inc"
#include "ef_host_smooth.inc"
#include "ef_host_boundary.inc"
#include "ef_host_fuse.inc"
