// Map side of libefusion_hip: depth pre-processing and surfel-map maintenance as HIP compute.
// Replaces the reference's GLSL transform-feedback / FBO passes (Core/IndexMap.cpp, Core/GlobalModel.cpp,
// Core/Shaders/{ComputePack,FillIn,FeedbackBuffer,Resize}.cpp and their shaders): no GL, no interop.
//
// HBM layout: surfels are three float4 streams (SoA) {x,y,z,conf} {colour,0,initTime,lastTime}
// {nx,ny,nz,radius}: every per-surfel pass issues perfectly coalesced 16-byte loads, and passes that
// cull on position/time never touch the normal stream.  The 48-byte AoS records of the reference
// (Core/Shaders/Vertex.cpp:21-41) exist only at the download / upload boundary.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ef_track.hpp"

namespace efm {

struct Cam { int cols, rows; float fx, fy, cx, cy; };

struct SurfelSoA {
  float4* pos_conf;
  float4* col_time;
  float4* nrm_rad;
};

constexpr unsigned long long ZBUF_EMPTY = 0xFFFFFFFFFFFFFFFFull;
constexpr unsigned WINNER_EMPTY = 0xFFFFFFFFu;
constexpr int CHUNK = 1024;  // elements per compaction chunk (256 threads x 4) of the seeding / candidate passes
constexpr int CLEAN_ROW = 256; // elements per compaction chunk of clean(): one per thread

// per-pixel model prediction products
struct IndexMaps {   // IndexMap::predictIndices outputs (IndexMap.h:74-88)
  uint32_t* index;
  float4* vert_conf;
  float4* color_time;
  float4* norm_rad;
  // Storage order of the four images (and of the z-buffer they are resolved from).  The frame tier keeps them
  // COLUMN-major (texel (x, y) at x * rows + y): surfels are created in column-major pixel order (the reference's draw
  // order, FeedbackBuffer.cpp:44-52) and move little between frames, so consecutive surfel ids project to vertically
  // adjacent pixels — with this layout the per-surfel taps of clean() and the per-pixel gathers of the resolve pass
  // touch consecutive addresses instead of one cache line per lane.  The operator tier passes row-major host images.
  int colmajor = 0;
};
__host__ __device__ inline int im_texel(const IndexMaps& im, const Cam& cam, int px, int py) {
  return im.colmajor ? px * cam.rows + py : py * cam.cols + px;
}
// The z-buffer of a predict_indices(..., resolve = false) standing in for the four images it was not resolved into (round 9).  A texel's key
// holds the winner's id and the exact float of its depth (= vert_conf.z); fuse() and clean() test the depth first, so they read 8 bytes per
// texel, and for the texels behind that gate gather the winner's two surfel rows and redo the resolve's arithmetic (index_texel_* in
// ef_map_kernels.hip: the expressions k_index_resolve evaluates, on the same inputs).  Nobody returns these keys to ZBUF_EMPTY on reading
// them (a consumer's neighbours read the texel too): the buffer is cleared by a later launch that is given it as `zclear` (fuse, clean).
struct KeyedIndex {
  const unsigned long long* keys;   // same storage order as IndexMaps::colmajor says
  const float* T_cw16_dev;          // the pose the splat projected with
  SurfelSoA map;                    // the rows the keys' ids name, as they stood when the splat ran (or as the splat's merge left them)
};
struct PredictMaps { // IndexMap::combinedPredict outputs (IndexMap.h:98-112)
  uchar4* image;
  float4* vertex;
  float4* normal;
  uint16_t* time;
};
struct FillMaps {    // FillIn textures (FillIn.h)
  uchar4* image;
  float4* vertex;
  float4* normal;
};
// association products of one frame: one slot per fused pixel (W/2 x H/2, quirk Q12), in draw order
struct Candidates {
  float4* pos_conf;
  float4* col_time;   // .w tag: -1 matched, -2 new unstable, 0 not emitted
  float4* nrm_rad;
  uint32_t* best;     // surfel id chosen by the association (tag -1)
  int n;              // (W/2)*(H/2)
};
struct CompactScratch {
  uint8_t* flags;          // capacity + n_candidates (or 2 x pixels for seeding)
  uint32_t* chunk_count;   // per chunk
  uint32_t* chunk_offset;  // exclusive scan
  uint32_t* totals;        // small scratch (>= 4 u32)
  int max_chunks;
  // clean() without its scan launch (round 6): kept elements per GROUP of CLEAN_GROUP rows, added up by k_clean_flags (integer atomics: exact
  // in any order) and read by k_clean_scatter, whose workgroups find their row's offset themselves.  Two halves of max_groups words: a call
  // adds into half `flip` and zeroes the other one for the call after it (clean() owns `flip`: it toggles it at entry).  Null: the scan launch.
  // One sum per 128-byte line (CLEAN_GSTRIDE words apart): with the sums side by side every row's atomic of a frame queued on one or two lines
  // (k_clean_flags 16.9 -> 20.9 us, profiles/r08a_bench_kernel_stats.csv).
  uint32_t* group_sum = nullptr;
  int max_groups = 0;
  int flip = 0;
};
constexpr int CLEAN_GROUP = 32;     // rows per group of CompactScratch::group_sum
constexpr int CLEAN_GSTRIDE = 32;   // words between two group sums

// ---- pre-processing (ComputePack FILTER / METRIC / METRIC_FILTERED, ElasticFusion.cpp:655-673) ----
// the bilateral filter's weight table of the current device (built on first use, synchronously; null on a HIP error).  ef_create asks
// for it so that no later call — possibly inside a stream capture — is the first
const float* bilateral_table();
bool filter_depth(const uint16_t* raw, int cols, int rows, float maxD, uint16_t* filtered, hipStream_t s);   // false: no weight table on this device
void metricise_depth(const uint16_t* in, int cols, int rows, float maxD, float* out, hipStream_t s);
// fused: bilateral + both metric conversions in one pass over the raw depth
// extra_lds: unused dynamic LDS bytes added to the launch = an occupancy cap for when the kernel shares the GPU
// rgb3 given: the frame's level-0 intensity image (next0) and, with rgb_keep, a copy of the colour image are written by the same launch
// table: bilateral_table()'s pointer when the caller holds it (null: asked here); returns false when the device has no table
bool preprocess_depth(const uint16_t* raw, int cols, int rows, float maxD, uint16_t* filtered, float* metric,
                      float* metric_filtered, hipStream_t s, unsigned extra_lds = 0, const uint8_t* rgb3 = nullptr, uint8_t* next0 = nullptr,
                      uint8_t* rgb_keep = nullptr, const float* table = nullptr);

// ---- layout conversion at the API boundary ----
void aos_to_soa(const float* aos, uint32_t count, SurfelSoA soa, hipStream_t s);
void soa_to_aos(SurfelSoA soa, uint32_t count, float* aos, hipStream_t s);
// dst[0, *count_dev) = src[0, *count_dev): the full-map copy the reference's update pass makes into its second vertex buffer
// (GlobalModel.cpp:458-524); only used to reproduce GlobalModel::downloadMap's buffer choice (ef_set_reference_download)
void copy_map(SurfelSoA src, const unsigned* count_dev, SurfelSoA dst, hipStream_t s);

// ---- first frame (vertex_feedback x2 + init_unstable) ----
void seed_map(const Cam& cam, const uint8_t* rgb3, const float* depth_metric, const float* depth_metric_filtered, int time,
              float maxDepth, SurfelSoA out, unsigned* count_dev, const CompactScratch& cs, hipStream_t s);

// ---- model prediction ----
// T_cw16_dev: device pointer to the float 4x4 T_wc^-1; count_dev: device surfel count
void predict_indices(const Cam& cam, const float* T_cw16_dev, int time, SurfelSoA map, const unsigned* count_dev, float maxDepth,
                     int timeDelta, unsigned long long* zbuf, IndexMaps out, hipStream_t s, eft::KernelProbe* probe = nullptr,
                     // merge_cand / merge_winner given (behind fuse(..., defer_merge = true)): the update pass of the fusion rides on this splat
                     const struct Candidates* merge_cand = nullptr, const uint32_t* merge_winner = nullptr,
                     // resolve false: only the splat — `out` is not written (its colmajor still names the z-buffer's order) and the keys stay in
                     // zbuf for a KeyedIndex consumer; the caller has the buffer cleared by a later launch
                     bool resolve = true);
// the resolve launch of predict_indices on its own, from keys a splat left behind; the z-buffer is left as it is
void resolve_indices(const Cam& cam, const float* T_cw16_dev, SurfelSoA map, const unsigned long long* zbuf, IndexMaps out, hipStream_t s);
void combined_predict(const Cam& cam, const float* T_cw16_dev, SurfelSoA map, const unsigned* count_dev, float maxDepth,
                      float confThreshold, int time, int maxTime, int timeDelta, unsigned long long* zbuf, PredictMaps out,
                      // optional fused fill-in + denseEnough sampling (null fill.image => skipped)
                      FillMaps fill, const uint16_t* depth_filtered, const uint8_t* rgb3, bool passthroughImage,
                      unsigned* dense_counter, hipStream_t s,
                      // optional: *nonempty_flag = nonempty_value when the view shows at least one surfel (the caller stamps a fresh value per use)
                      unsigned* nonempty_flag = nullptr, unsigned nonempty_value = 0,
                      // optional: *consumed_mark = consumed_value (system scope, e.g. host-mapped memory) as soon as the splat launch starts, i.e. once
                      // everything enqueued before it has finished
                      unsigned* consumed_mark = nullptr, unsigned consumed_value = 0,
                      // optional: build_ray_table's table for this camera (cols x rows float4, column-major): the splat loads a fragment's ray instead of
                      // evaluating it — the same value
                      const float* rays4 = nullptr);
void build_ray_table(const Cam& cam, float* rays4, hipStream_t s);
// IndexMap::synthesizeDepth (splat.vert + depth_splat.frag): float depth of the nearest splat per pixel, 0 = none
void synthesize_depth(const Cam& cam, const float* T_cw16_dev, SurfelSoA map, const unsigned* count_dev, float maxDepth,
                      float confThreshold, int time, int maxTime, int timeDelta, unsigned long long* zbuf, float* depth, hipStream_t s,
                      const float* rays4 = nullptr);
void fill_in(const Cam& cam, PredictMaps pred, const uint16_t* depth_filtered, const uint8_t* rgb3, bool passthrough,
             bool passthroughImage, FillMaps out, hipStream_t s);
// counts the (W/20)x(H/20) sample texels with r,g,b > 0 into *counter (Resize::image + denseEnough)
void dense_count(const Cam& cam, const uchar4* image, unsigned* counter, hipStream_t s);

// ---- fusion ----
// pose_f16_dev: float T_wc (cast<float>().matrix()); weighting_dev: device float
void fuse(const Cam& cam, const float* pose_f16_dev, int time, const uint8_t* rgb3, const float* depth_metric,
          const float* depth_metric_filtered, IndexMaps im, float maxDepth, const float* weighting_dev, SurfelSoA map,
          const unsigned* count_dev, Candidates cand, uint32_t* winner, hipStream_t s, bool defer_merge = false,
          // keyed given: the association taps the z-buffer instead of im's images (im.colmajor still read); zclear (or null): cols x rows keys
          // of ANOTHER z-buffer that the association's launch returns to ZBUF_EMPTY
          const KeyedIndex* keyed = nullptr, unsigned long long* zclear = nullptr);
// deformation graph handed to clean() after a loop closure (copy_unstable.vert:128-322): nodes x 16 floats sorted by time
// {position 3, rotation 9 column-major, translation 3, time}; depth = synthesize_depth image (read unless is_fern)
struct Deformation {
  const float* graph_dev;
  int nodes;
  const float* depth_dev;
  int is_fern;
  float max_depth;
};
// clean + append; writes the compacted map to `out` and the new count (clamped to capacity) to *count_out_dev
void clean(const Cam& cam, const float* T_cw16_dev, int time, IndexMaps im, float confThreshold, int timeDelta, SurfelSoA map,
           const unsigned* count_dev, Candidates cand, uint32_t* winner, SurfelSoA out, unsigned* count_out_dev, uint32_t capacity,
           CompactScratch& cs, int* overflow_flag, hipStream_t s, const Deformation* deform = nullptr,
           // keyed given (no deformation): the keep-test taps the z-buffer instead of im's images; zclear (or null): cols x rows keys of ANOTHER
           // z-buffer that the scatter launch returns to ZBUF_EMPTY; T_keep16_dev (or null): receives a copy of the 16 floats at T_cw16_dev
           const KeyedIndex* keyed = nullptr, unsigned long long* zclear = nullptr, float* T_keep16_dev = nullptr);
// Deformation::sampleGraphModel: nodes {x, y, z, initTime} = every `stride`-th surfel (5000 in the reference); *n_out = node count
void sample_graph(SurfelSoA map, const unsigned* count_dev, int stride, int max_nodes, float* out4, unsigned* n_out, hipStream_t s);
// candidates -> AoS "newUnstable" list in draw order (operator tier / tests)
void candidates_to_aos(Candidates cand, float* aos, unsigned* count_dev, const CompactScratch& cs, hipStream_t s);

// ---- GlobalModel::renderPointCloud, headless (ef_render.inc; ef_render_model of include/ef_hip.h) ----
struct RenderArgs {
  Cam cam;
  float Tcw[16];   // float T_wc^-1, row-major (pose_mats)
  float maxDepth, threshold;
  int drawUnstable, colorType, drawWindow, time, timeDelta;
};
struct RenderOut {   // row-major images; a null pointer is not written
  uchar4* rgba;
  float* depth;
  float4* vertex;
  float4* normal;
  uint32_t* index;
};
// zbuf: cols x rows keys, all ZBUF_EMPTY on entry and on return
void render_model(const RenderArgs& a, SurfelSoA map, const unsigned* count_dev, unsigned long long* zbuf, RenderOut out, hipStream_t s);

// ---- stable surfel IDs and label fusion (ef_labels.inc; ef_set_surfel_ids / ef_enable_labels of include/ef_hip.h) ----
// state[0]: the next ID to hand out.  One workgroup numbers the zero suffix of the ID lane (col_time.y as uint32).
void ids_assign(SurfelSoA map, const unsigned* count_dev, unsigned* state, hipStream_t s);
// *flag |= 1 unless the lane of rows [0, n) is a strictly increasing non-zero prefix followed by a zero suffix, |= 2 when numbering that suffix
// from max(*counter, largest ID + 1) would not stay below 0xFFFFFFFF (counter = state of ids_assign)
void ids_check(SurfelSoA map, unsigned n, const unsigned* counter, unsigned* flag, hipStream_t s);
// max_rows: an upper bound of *count_dev (sizes the grid only)
void ids_zero(SurfelSoA map, const unsigned* count_dev, unsigned max_rows, hipStream_t s);
void ids_gather(SurfelSoA map, unsigned n, uint32_t* out, hipStream_t s);
struct LabelAlign {
  SurfelSoA map;
  const unsigned* count_dev;
  const uint32_t* ids_in;   // the previous alignment's IDs (*n_in of them, sorted) and their rows
  const float* tab_in;
  const unsigned* n_in;
  uint32_t* ids_out;        // the current rows' IDs and rows; *n_out = *count_dev
  float* tab_out;
  unsigned* n_out;
  int C;
  float prior;              // 1 / C
};
struct LabelFuse {
  SurfelSoA map;
  const unsigned* count_dev;
  Cam cam;
  float Tcw[16];            // float T_wc^-1, row-major (pose_mats), as the render takes it
  const uint32_t* index;    // the view's index image (render_model), row-major
  const float* probs;       // C x rows x cols
  float* tab;
  int C;
};
void labels_align(const LabelAlign& a, unsigned max_rows, hipStream_t s);
void labels_fuse(const LabelFuse& f, unsigned max_rows, hipStream_t s);
void labels_gather(const uint32_t* index, int P, const float* tab, int C, int32_t* label, float* prob, hipStream_t s);

// ---- spatial index and nearest / kNN queries (ef_query.inc; ef_query_nearest / ef_query_knn of include/ef_hip.h) ----
struct QueryArgs {
  SurfelSoA map;            // the live map: normal and ID of a winner
  const float4* sorted;     // the index: {x, y, z, conf} sorted by bucket, rows[] the map row of each record
  const uint32_t* rows;
  const uint32_t* cells;    // cells[b]: the END of bucket b in sorted[] (its start is cells[b - 1], 0 for b = 0)
  unsigned mask;            // buckets - 1 (a power of two)
  unsigned n_sorted;        // records in the index (0: every query misses)
  float inv_cell;           // 1 / cell, the float the build used
  const float* points;      // n x 3
  unsigned n;
  int k;                    // slots per query in row / dist2
  float max_dist, r2, min_conf;
  uint32_t* row;            // n x k
  float* dist2;             // n x k or null
  uint32_t* id;             // n or null (k = 1 only)
  float* plane;             // n or null (k = 1 only)
  uint32_t* count;          // n or null
};
constexpr int QUERY_MAX_RATIO = 16;   // max_dist / cell the query accepts: its box is at most (2 ratio + 3)^3 cells
unsigned query_buckets(unsigned n);   // a power of two >= 1024
void query_build(SurfelSoA map, unsigned n, float inv_cell, unsigned nb, uint32_t* cells, uint32_t* tile_sum, float4* sorted, uint32_t* rows,
                 hipStream_t s);
// k 1 .. 16; lanes per query 1, 8 (k = 1: also 16, 64), 0 = the default (16 for k = 1, else 1)
void query_run(const QueryArgs& a, int k, int lanes, hipStream_t s);

// ---- point-to-plane registration of a point set against the map (ef_register.inc; ef_register_step / ef_register_cloud of include/ef_hip.h) ----
constexpr int REGISTER_SLOTS = 32;          // doubles per slab: 21 upper-triangle entries of A (row-major), 6 of b, e, pairs, 3 unused
// Slabs (= workgroups) of one step at most: 6 per CU, so that every wave of the launch is resident at once (the kernel fits 7 waves per SIMD).
// A group's points are assigned statically (the order of the sums must not depend on timing), so workgroups that have to wait for a slot run
// behind a chip that is already draining: 2048 took 1.29 times as long as 1536 at 1 M points, 1792 1.37, 1024 1.18 times
// (profiles/r13_register_kernel_times.txt).
constexpr int REGISTER_MAX_BLOCKS = 1536;
struct RegisterArgs {
  QueryArgs q;              // the index, the radius and min_conf; q.points = the cloud (n x 3), q.row / q.plane = per-point outputs or null
  const float* normals;     // n x 3 or null
  float R[9], t[3];         // the pose rounded to f32 once (row-major rotation block, translation)
  float min_normal_cos;
  int gate;                 // the normal gate is on (normals given and min_normal_cos > -1)
  double* slabs;            // REGISTER_MAX_BLOCKS x REGISTER_SLOTS
  double* sums;             // REGISTER_SLOTS: the fixed-order sum of the slabs
};
unsigned register_blocks(unsigned n);   // workgroups (= slabs) of a step over n points: a function of n alone
void register_step(const RegisterArgs& a, hipStream_t s);

// ---- select, extract and erase surfels (ef_select.inc; ef_map_select / ef_map_gather / ef_map_erase of include/ef_hip.h) ----
constexpr unsigned SEL_BOX = 0x01u, SEL_CONF = 0x02u, SEL_INIT_TIME = 0x04u, SEL_LAST_TIME = 0x08u, SEL_RADIUS = 0x10u, SEL_ID = 0x20u,
                   SEL_LABEL = 0x40u;   // EF_SEL_* without EF_SEL_INVERT (SelectArgs::invert)
struct SelectArgs {
  SurfelSoA map;
  unsigned n;               // rows of the map (the host knows the count: it sizes the grid)
  unsigned tests;           // OR of SEL_*
  unsigned invert;
  float R[9], t[3];         // T_bw rounded to f32 once (row-major rotation block, translation)
  float box_min[3], box_max[3];
  float conf_min, conf_max;
  float init_min, init_max, last_min, last_max;   // the int bounds converted to float once
  float radius_min, radius_max;
  unsigned id_min, id_max;
  const float* tab;         // the aligned label table [rows][C] (SEL_LABEL only)
  int C, label_class;
  float label_min_prob;
};
struct SelectScratch {
  uint8_t* flags;           // one byte per row
  uint32_t* chunk_count;    // per chunk of 256 rows
  uint32_t* chunk_offset;   // their exclusive scan
};
unsigned select_chunks(unsigned n);
// flags of the selected rows, their per-chunk counts and offsets; *total = the number selected
void select_flags(const SelectArgs& a, const SelectScratch& sc, uint32_t* total, hipStream_t s);
// counts, offsets and *total of the rows whose flag in sc.flags differs from `flip` (k_select_count + the scan; n = 0: the scan alone writes 0)
void flags_count(const SelectScratch& sc, unsigned n, unsigned flip, uint32_t* total, hipStream_t s);
// flags = 1 for the named rows (< n; duplicates harmless); counts, offsets and *total of the rows whose flag differs from `flip`
void select_mark_rows(const uint32_t* rows, unsigned n_rows, unsigned n, unsigned flip, const SelectScratch& sc, uint32_t* total, hipStream_t s);
// the flagged rows in ascending order, the first max_rows of them
void select_rows(const SelectScratch& sc, unsigned n, uint32_t* rows, unsigned max_rows, hipStream_t s);
// dst = the rows of src whose flag differs from `flip`, in their old order (all three streams as data)
void select_compact(const SelectScratch& sc, unsigned n, unsigned flip, SurfelSoA src, SurfelSoA dst, hipStream_t s);
// out: n_rows x 12 floats in the download's layout, in the order of rows[]; a row >= n gives twelve zero words
void map_gather(SurfelSoA map, unsigned n, const uint32_t* rows, unsigned n_rows, float* out, hipStream_t s);

// ---- insert surfels (ef_insert.inc; ef_map_insert of include/ef_hip.h) ----
constexpr int INSERT_KEEP = -1;   // EF_INSERT_KEEP
struct InsertArgs {
  QueryArgs q;              // gate only: the index of the OLD map, max_dist / r2 = the separation, min_conf (points, n, k and the outputs unused)
  const float4* rec;        // n records of three 16-byte words {x, y, z, conf} {colour, ID bits, initTime, lastTime} {nx, ny, nz, radius}
  unsigned n;
  int moved;                // T given: R, t below are applied; 0: position and normal are copied
  float R[9], t[3];         // T rounded to f32 once (row-major rotation block, translation)
  int gate;
  float min_normal_cos;     // gate only; <= -1: no normal test
  int init_time, last_time; // >= 0: stored as (float); INSERT_KEEP: the record's own
  unsigned count_before;    // the scatter's first row
  uint8_t* flags;           // one byte per record: 1 = insert
  uint8_t* dup;             // gate only, one byte per record: 1 = duplicate (a record with neither byte set was skipped)
  const uint32_t* chunk_offset;   // of the scatter: the exclusive scan of the flags' counts per SELECT_ROW records
  uint32_t* match_row;      // n or null (written by the gate)
  uint32_t* new_row;        // n or null (written by the scatter)
};
// flags (and match_row) of the n records, their per-chunk counts into sc.chunk_count, offsets into sc.chunk_offset and *total = records to insert;
// with the gate on also a.dup and, through dup_sc (whose flags are a.dup), *dup_total = duplicates (gate off: neither is touched)
void insert_gate(const InsertArgs& a, const SelectScratch& sc, uint32_t* total, const SelectScratch& dup_sc, uint32_t* dup_total, hipStream_t s);
// the flagged records appended to dst at a.count_before in input order (a.chunk_offset = sc.chunk_offset of insert_gate), and new_row
void insert_scatter(const InsertArgs& a, SurfelSoA dst, hipStream_t s);

// ---- thin the map to one surfel per voxel (ef_thin.inc; ef_map_thin of include/ef_hip.h) ----
constexpr int THIN_KEEP_MAX_CONF = 0, THIN_KEEP_NEWEST = 1, THIN_KEEP_FIRST = 2;   // EF_THIN_KEEP_*
struct ThinArgs {
  QueryArgs q;              // the index built at the thin's cell (sorted, rows, cells, mask, n_sorted, inv_cell) and the live map (NEWEST: col_time)
  unsigned n;               // rows of the map: the length of the byte arrays below
  int keep;                 // THIN_KEEP_*
  const uint8_t* part;      // one byte per row, non-zero = the row passes the selection; null: every row does
  uint8_t* removed;         // one byte per row, zero on entry: 1 is stored for every removed row; or null
  uint8_t* rep;             // likewise for every representative; or null
};
// one wave per bucket of the index: nothing is launched for an empty index
void thin_flags(const ThinArgs& a, hipStream_t s);

// ---- carve free space: flag the surfels that depth views see through (ef_carve.inc; ef_map_carve of include/ef_hip.h) ----
constexpr int CARVE_MAX_VIEWS = 32;   // EF_CARVE_MAX_VIEWS
struct CarveArgs {
  const float4* pos_conf;   // the map's {x, y, z, conf} stream: the only map stream the carve reads
  unsigned n;               // rows of the map: the length of the byte arrays below
  const uint8_t* part;      // one byte per row, non-zero = the row passes the selection; null: every row does
  const uint16_t* depth;    // n_views consecutive height x width images of millimetres (2-byte aligned, no more)
  int n_views;
  int width, height;
  float fx, fy, cx, cy;
  float min_depth, max_depth, margin, margin_quad;
  int window, min_views, protect;
  uint8_t* removed;         // one byte per row: 1 = removed, 0 = kept (every row is written)
  uint8_t* votes;           // two bytes per row {free, support}; or null
  uint32_t* tally;          // 3 x tally_stride words: per chunk of SELECT_ROW rows the participants, the observed and the free-space rows; or null
  unsigned tally_stride;
  float Tcw[CARVE_MAX_VIEWS][12];   // per view the rows {Rc i0, Rc i1, Rc i2, tc i} of T_cw, each entry rounded to f32 once; it travels in the
                                    // kernel's argument segment and is read with scalar loads (uniform across the launch)
};
// one lane per row; nothing is launched for an empty map
void carve_flags(const CarveArgs& a, hipStream_t s);
// offsets and *total of per-chunk counts that a kernel has already written into sc.chunk_count (the scan select_flags and flags_count end with)
void chunk_totals(const SelectScratch& sc, unsigned n, uint32_t* total, hipStream_t s);

// ---- remove outlier surfels: neighbourhood statistics of the map (ef_outlier.inc; ef_map_remove_outliers of include/ef_hip.h) ----
constexpr int OUTLIER_RADIUS = 0, OUTLIER_STATISTICAL = 1;   // EF_OUTLIER_*
constexpr int OUTLIER_SUM_LANES = 4096;                      // EF_OUTLIER_SUM_LANES
struct OutlierResult {      // ef_outlier_result, field for field (ef_host_outlier.inc asserts the layout)
  double sum, sum_sq;
  uint32_t participants, measured, sparse, outliers, count_after;
  float threshold;
};
struct OutlierArgs {
  QueryArgs q;              // the index built at the call's cell and the live map; max_dist = radius, r2, min_conf (points, n, k, outputs unused)
  unsigned n;               // rows of the map: the length of the per-row arrays below
  int mode;                 // OUTLIER_*
  int k;                    // neighbours of the mean: 1 .. 16 (1 in RADIUS mode)
  unsigned min_neighbors;
  int flag_sparse;
  float std_ratio, max_mean_dist;
  const uint8_t* part_in;   // one byte per row, non-zero = the row passes the selection (may be `part` itself); null: every row does
  uint8_t* part;            // one byte per row: 1 = participant (selected and finite); every row is written by the join
  uint2* stat;              // per row {bits of mean_dist, count}; every row is written by the join
  double* partial;          // 2 x OUTLIER_SUM_LANES: the lanes' partial sums of term1 and term2
  uint32_t* tally;          // 3 x OUTLIER_SUM_LANES: the lanes' participants, measured and sparse rows
  OutlierResult* res;       // the call's result on the device; its threshold is what the flags compare with
};
// stat and part of every row: one lane per record of the index, in index order; nothing is launched for an empty map
void outlier_join(const OutlierArgs& a, hipStream_t s);
// the fixed-order sums, the counts and the threshold into *a.res (outliers and count_after are outlier_tally's)
void outlier_reduce(const OutlierArgs& a, hipStream_t s);
// flags[row] = 1 for every outlier, 0 for every other row (every row is written)
void outlier_flags(const OutlierArgs& a, uint8_t* flags, hipStream_t s);
// res->outliers = *total, res->count_after = n - *total; then *copy_to = *res unless copy_to is null
void outlier_tally(const OutlierArgs& a, const uint32_t* total, OutlierResult* copy_to, hipStream_t s);
// mean[r] / count[r] of the rows r < min(rows, n) from stat (either may be null)
void outlier_split(const OutlierArgs& a, float* mean, uint32_t* count, unsigned rows, hipStream_t s);

// ---- connected components of the map under "closer than r" (ef_components.inc; ef_map_components of include/ef_hip.h) ----
constexpr unsigned COMPONENT_NONE = 0xFFFFFFFFu;                    // EF_COMPONENT_NONE
constexpr int COMPONENTS_REJECTED = 0, COMPONENTS_ACCEPTED = 1;     // EF_COMPONENTS_*
struct ComponentResult {    // ef_component_result, field for field (ef_host_components.inc asserts the layout)
  uint32_t nodes, components, largest, rejected_rows, rejected_components, count_after, status;
};
struct ComponentArgs {
  QueryArgs q;              // the index built at the call's cell and the live map; max_dist = radius, r2, min_conf (points, n, k, outputs unused)
  unsigned n;               // rows of the map: the length of the per-row arrays below
  unsigned min_size, max_size;
  const uint8_t* sel;       // one byte per row, non-zero = the row passes the selection (may be `node` itself); null: every row does
  uint8_t* node;            // one byte per row: 1 = node (selected, finite, conf > min_conf); every row is written by component_hook
  uint32_t* parent;         // the union-find's word per row (ef_unionfind.hpp); COMPONENT_NONE for a row that is no node
  uint32_t* label;          // per row the smallest row of its component, COMPONENT_NONE for a row that is no node
  uint32_t* members;        // members[l] = nodes of the component labelled l (0 at every row that is no label)
  ComponentResult* res;     // the call's result on the device, zeroed by component_hook's caller; status != 0: a loop cap tripped
};
// node, parent and members of every row, the link to the smallest lower neighbour, then every edge's union (one lane per record of the index, in
// index order), with pointer-jumping passes after each of the two (nothing for an empty map)
void component_hook(const ComponentArgs& a, hipStream_t s);
// label and members; then nodes, components, largest, rejected_rows, rejected_components into *a.res and, unless flags is null,
// flags[row] = 1 for every rejected (what = COMPONENTS_REJECTED) or accepted (COMPONENTS_ACCEPTED) node, 0 for every other row
void component_label(const ComponentArgs& a, int what, uint8_t* flags, hipStream_t s);
// res->count_after = n - res->rejected_rows; then *copy_to = *res unless copy_to is null
void component_tally(const ComponentArgs& a, ComponentResult* copy_to, hipStream_t s);
// label[r] / size[r] of the rows r < min(rows, n) (either may be null)
void component_split(const ComponentArgs& a, uint32_t* label, uint32_t* size, unsigned rows, hipStream_t s);

// ---- segment the map into planes by sequential RANSAC (ef_planes.inc; ef_map_planes of include/ef_hip.h) ----
constexpr unsigned PLANE_NONE = 0xFFFFFFFFu;                        // EF_PLANE_NONE
constexpr int PLANE_MAX_PLANES = 16, PLANE_MAX_HYPOTHESES = 4096;   // EF_PLANE_MAX_*
constexpr int PLANE_AXIS_OFF = 0, PLANE_AXIS_NORMAL = 1, PLANE_AXIS_INPLANE = 2;   // EF_PLANE_AXIS_*
constexpr int PLANES_ON = 0, PLANES_OFF = 1;                        // EF_PLANES_*
constexpr int PLANE_CHUNK = 2048;                                   // compacted participants per workgroup of the scoring kernel
struct PlaneModel {         // ef_plane_model, field for field (ef_host_planes.inc asserts the layout)
  float normal[3], d;
  uint32_t inliers, sampled_inliers, hypothesis, valid_hypotheses, participants;
  float thickness;
};
struct PlaneResult {        // ef_plane_result, field for field
  uint32_t nodes, planes, on_rows, off_rows, count_after;
};
struct PlaneRound {         // what one round's kernels hand to the next ones, on the device
  uint32_t done;            // non-zero: the extraction has ended; every later kernel of the call returns at once
  uint32_t count, h, valid, M;   // the winner's count and index, the round's valid hypotheses and participants
  float hn[3], hd;          // the winning hypothesis
  float a[3];               // its first sample: the anchor of the refinement
  float n[3], d;            // the final plane: what the labels are tested against
};
struct PlaneArgs {
  SurfelSoA map;
  unsigned n;               // rows of the map: the length of the per-row arrays below
  float distance, normal_cos, min_conf;
  unsigned H, seed, max_planes, min_inliers, refine;
  int axis_mode;
  float axis[3], axis_bound;
  const uint8_t* sel;       // one byte per row, non-zero = the row passes the selection (may be `node` itself); null: every row does
  uint8_t* node;            // one byte per row: 1 = node (selected, finite, conf > min_conf); every row is written by plane_init
  uint8_t* part;            // one byte per row: 1 = participant of the current round (a node no earlier round labelled); = sc.flags
  uint32_t* label;          // per row the plane's index, PLANE_NONE for every other row
  SelectScratch sc;         // the participants' bytes, their chunk counts and offsets
  uint32_t* M;              // the current round's number of participants (the scan's total)
  float4* cpos;             // the participants' {x, y, z, conf}, compacted in ascending row order
  float4* cnrm;             // their {nx, ny, nz, radius} (normal_cos > 0 only)
  float4* hyp;              // H hypotheses {n, d}; an invalid one is four NaNs (it then scores 0 by itself)
  uint32_t* hyp_a;          // H: the compacted index of each hypothesis's first sample
  uint32_t* counts;         // H inlier counts
  double* partial;          // 9 x OUTLIER_SUM_LANES: the lanes' partial sums of the refinement
  PlaneRound* st;
  PlaneModel* models;       // PLANE_MAX_PLANES, zeroed by the caller
  PlaneResult* res;         // zeroed by the caller
};
// node and label of every row (nothing for an empty map)
void plane_init(const PlaneArgs& a, hipStream_t s);
// round k: participants, compaction, hypotheses, scores, the pick, the refinement, the labels.  Grids are sized by a.n; the kernels read the
// round's M and the done word from device memory, so nothing here waits for the device
void plane_round(const PlaneArgs& a, unsigned k, hipStream_t s);
// flags[row] = 1 for the rows of the list (what = PLANES_ON: labelled `which`, any plane for which < 0; PLANES_OFF: every other node), 0 for
// every other row (every row is written; flags null: nothing), then res->off_rows and res->count_after = n - the PLANES_ON rows of `which`
void plane_finish(const PlaneArgs& a, int what, int which, uint8_t* flags, hipStream_t s);
// label[r] of the rows r < min(rows, n), the max_planes models and the result (each may be null)
void plane_split(const PlaneArgs& a, uint32_t* label, unsigned rows, PlaneModel* models, PlaneResult* res, hipStream_t s);

// ---- estimate normals, curvature and spacing from the map's neighbourhoods (ef_normals.inc; ef_map_normals of include/ef_hip.h) ----
constexpr int NORMALS_KEEP_SIDE = 0, NORMALS_VIEWPOINT = 1;                                   // EF_NORMALS_KEEP_SIDE / _VIEWPOINT
constexpr unsigned NORMAL_NONE = 0, NORMAL_ESTIMATED = 1, NORMAL_SPARSE = 2, NORMAL_DEGENERATE = 3;   // EF_NORMAL_*: the status byte
constexpr int NORMALS_CURVED = 4, NORMALS_FLAT = 5;                                           // EF_NORMALS_*: `what` beside the three statuses
constexpr unsigned NORMAL_STATUS_MASK = 3u, NORMAL_FLIPPED = 4u;   // the scratch's byte: the status, and the bit of an estimate the orientation turned
struct NormalResult {       // ef_normal_result, field for field (ef_host_normals.inc asserts the layout)
  uint32_t participants, estimated, sparse, degenerate, flipped, listed;
};
struct NormalArgs {
  QueryArgs q;              // the index built at the call's cell and the live map; max_dist = radius, r2, min_conf (points, n, k, outputs unused)
  unsigned n;               // rows of the map: the length of the per-row arrays below
  int k;                    // neighbours used: 3 .. 16
  unsigned min_neighbors;
  int orientation;          // NORMALS_*
  float side;               // +1 / -1 (VIEWPOINT)
  float view[3];
  float line_ratio, max_curvature;
  int set_radius;
  float radius_scale;
  const uint8_t* part_in;   // one byte per row, non-zero = the row passes the selection (may be `status` itself); null: every row does
  float4* est;              // per row {normal, curvature}; every row is written by the join
  uint2* stat;              // per row {bits of spacing, count}; every row is written by the join
  uint8_t* status;          // per row NORMAL_* | NORMAL_FLIPPED; every row is written by the join
  NormalResult* res;        // the call's result on the device
};
// est, stat and status of every row: one lane per record of the index, in index order; nothing is launched for an empty map
void normal_join(const NormalArgs& a, hipStream_t s);
// flags[row] = 1 for the rows `what` names, 0 for every other row (every row is written)
void normal_flags(const NormalArgs& a, int what, uint8_t* flags, hipStream_t s);
// *a.res (zeroed here first) from the status bytes, listed = *total (0 with total null); then *copy_to = *res unless copy_to is null
void normal_tally(const NormalArgs& a, const uint32_t* total, NormalResult* copy_to, hipStream_t s);
// the optional per-row outputs of the rows r < min(rows, n) from the packed words (each may be null)
void normal_split(const NormalArgs& a, float* normals3, float* curvature, float* spacing, uint32_t* count, uint8_t* status, unsigned rows,
                  hipStream_t s);
// the write-back: floats 8 .. 10 (and 11 with set_radius) of every ESTIMATED row of a.q.map, in place
void normal_apply(const NormalArgs& a, hipStream_t s);

// ---- segment the map into smooth regions (ef_regions.inc; ef_map_regions of include/ef_hip.h) ----
constexpr unsigned REGION_NONE = 0xFFFFFFFFu;                                                 // EF_REGION_NONE
constexpr unsigned REGION_KIND_NONE = 0, REGION_KIND_CORE = 1, REGION_KIND_BORDER = 2;        // EF_REGION_KIND_*: the kind byte
constexpr int REGIONS_ESTIMATED = 0, REGIONS_STORED = 1;                                      // EF_REGIONS_ESTIMATED / _STORED: normal_source
constexpr int REGIONS_REJECTED = 0, REGIONS_ACCEPTED = 1, REGIONS_UNASSIGNED = 2, REGIONS_BORDERS = 3;   // EF_REGIONS_*: `what`
struct RegionResult {       // ef_region_result, field for field (ef_host_regions.inc asserts the layout)
  uint32_t nodes, cores, borders, attached, unassigned, regions, largest, rejected_rows, rejected_regions, listed, count_after, status;
};
struct RegionArgs {
  NormalArgs nrm;           // the estimate's arguments and outputs (normal_join, unchanged): q, n, est, stat, status by row
  float min_normal_cos, max_curvature;
  int two_sided, normal_source, attach_borders;
  unsigned min_size, max_size;
  const float4* nw;         // per row {n_s, curvature}: nrm.est itself (REGIONS_ESTIMATED) or `stored`, which region_init fills (REGIONS_STORED)
  float4* stored;
  uint8_t* kind;            // one byte per row: REGION_KIND_*; every row is written by region_init
  uint32_t* parent;         // the union-find's word per row (ef_unionfind.hpp); REGION_NONE for a row that is no core
  uint32_t* attach;         // per row the core a border joins, REGION_NONE for every other row and for a border without one
  uint32_t* label;          // per row the smallest core row of its region, REGION_NONE for a row without a region
  uint32_t* members;        // members[l] = cores and attached borders of the region labelled l (0 at every row that is no label)
  RegionResult* res;        // the call's result on the device, zeroed by region_hook's caller; status != 0: a loop cap tripped
};
// kind, parent, attach and members of every row (and `stored`), the link to the smallest lower smooth core neighbour, then every core edge's
// union (one lane per record of the index, in index order), with pointer-jumping passes after each of the two, then the borders' attachment
// (attach_borders != 0 only).  a.nrm's join has been enqueued before.  Nothing for an empty map
void region_hook(const RegionArgs& a, hipStream_t s);
// label and members; then the result's counts but count_after and, unless flags is null, flags[row] = 1 for the rows of the list `what`
// (REGIONS_*), 0 for every other row; res->listed = the number of those rows whether or not flags is null
void region_label(const RegionArgs& a, int what, uint8_t* flags, hipStream_t s);
// res->count_after = n - res->listed; then *copy_to = *res unless copy_to is null
void region_tally(const RegionArgs& a, RegionResult* copy_to, hipStream_t s);
// label[r] / size[r] / kind[r] of the rows r < min(rows, n) (each may be null)
void region_split(const RegionArgs& a, uint32_t* label, uint32_t* size, uint8_t* kind, unsigned rows, hipStream_t s);

// ---- smooth the map's positions by moving least squares (ef_smooth.inc; ef_map_smooth of include/ef_hip.h) ----
constexpr int SMOOTH_UNIFORM = 0, SMOOTH_COMPACT = 1;                                         // EF_SMOOTH_UNIFORM / _COMPACT: weighting
constexpr unsigned SMOOTH_NONE = 0, SMOOTH_SMOOTHED = 1, SMOOTH_SPARSE = 2, SMOOTH_DEGENERATE = 3;   // EF_SMOOTH_*: the status byte
constexpr int SMOOTH_CLAMPED = 4, SMOOTH_SHIFTED = 5;                                         // EF_SMOOTH_*: `what` beside the three statuses
constexpr unsigned SMOOTH_STATUS_MASK = 3u, SMOOTH_CLAMPED_BIT = 4u;   // the scratch's byte: the status, and the sticky bit of a row whose step was clamped
struct SmoothResult {       // ef_smooth_result, field for field (ef_host_smooth.inc asserts the layout)
  uint32_t participants, smoothed, sparse, degenerate, clamped, moved, listed;
  float largest_shift;
};
struct SmoothArgs {
  QueryArgs q;              // the index built at the call's cell and the live map; max_dist = radius, r2, min_conf (points, n, k, outputs unused)
  unsigned n;               // rows of the map: the length of the per-row arrays below
  int k;                    // neighbours used: 3 .. 16
  unsigned min_neighbors;
  int iterations;           // 1 .. 16
  int weighting;            // SMOOTH_UNIFORM / SMOOTH_COMPACT
  int gate;                 // non-zero: a neighbour counts only if its stored normal agrees with the row's
  float min_normal_cos, strength, max_shift, line_ratio, shift_threshold;
  int set_normal;
  const uint8_t* part_in;   // one byte per row, non-zero = the row passes the selection (may be `status` itself); null: every row does
  unsigned stride;          // rows between two slots of nbr
  uint32_t* nbr;            // slot-major: nbr[j * stride + row] = the row's j-th used neighbour, the row itself from slot c on; slots 0 .. k - 1
  uint32_t* count;          // per row count_s (0 for a row that takes no part); every row is written by smooth_neighbours
  uint8_t* status;          // per row SMOOTH_* | SMOOTH_CLAMPED_BIT: NONE / SPARSE / SMOOTHED (= "is fitted") after smooth_neighbours, the last verdict after a step
  float4* buf[2];           // the ping-pong positions {x, y, z, conf}: iteration i writes buf[(i - 1) & 1]
  float4* est;              // per row {normal, curvature} of the last step; every row is written by every step
  float* shift;             // per row; every row is written by smooth_finish
  SmoothResult* res;        // the call's result on the device
};
// the positions after the last iteration
inline const float4* smooth_final(const SmoothArgs& a) { return a.buf[(a.iterations - 1) & 1]; }
// count, status and the neighbour list of every row: one lane per record of the index, in index order; nothing is launched for an empty map
void smooth_neighbours(const SmoothArgs& a, hipStream_t s);
// iteration i (1 ..): one lane per row reads the list, gathers from the iteration's input (the map for i = 1, buf[i & 1] after) and writes
// buf[(i - 1) & 1], est and status of every row
void smooth_step(const SmoothArgs& a, int i, hipStream_t s);
// shift[] of every row from the last iteration's positions and the map's
void smooth_finish(const SmoothArgs& a, hipStream_t s);
// flags[row] = 1 for the rows `what` names, 0 for every other row (every row is written)
void smooth_flags(const SmoothArgs& a, int what, uint8_t* flags, hipStream_t s);
// *a.res (zeroed here first) from status and shift, listed = *total (0 with total null); then *copy_to = *res unless copy_to is null
void smooth_tally(const SmoothArgs& a, const uint32_t* total, SmoothResult* copy_to, hipStream_t s);
// the optional per-row outputs of the rows r < min(rows, n) (each may be null)
void smooth_split(const SmoothArgs& a, float* position3, float* normal3, float* curvature, float* shift, uint32_t* count, uint8_t* status,
                  unsigned rows, hipStream_t s);
// the write-back: floats 0 .. 2 of every participant of a.q.map, and floats 8 .. 10 of the SMOOTHED rows with set_normal, in place
void smooth_apply(const SmoothArgs& a, hipStream_t s);

// ---- find the map's boundaries by the angle criterion (ef_boundary.inc; ef_map_boundaries of include/ef_hip.h) ----
constexpr int BOUNDARY_STORED = 0, BOUNDARY_ESTIMATED = 1;                                    // EF_BOUNDARY_STORED / _ESTIMATED: normal_source
constexpr unsigned BOUNDARY_NONE = 0, BOUNDARY_INTERIOR = 1, BOUNDARY_BOUNDARY = 2, BOUNDARY_SPARSE = 3, BOUNDARY_DEGENERATE = 4;   // EF_BOUNDARY_*: the status byte
constexpr int BOUNDARY_LOOPS_ACCEPTED = 5, BOUNDARY_LOOPS_REJECTED = 6;                       // EF_BOUNDARY_LOOPS_*: `what` beside the four verdicts
struct BoundaryResult {     // ef_boundary_result, field for field (ef_host_boundary.inc asserts the layout)
  uint32_t participants, interior, boundary, sparse, degenerate, loops, accepted, largest, listed, status;
};
struct BoundaryArgs {
  QueryArgs q;              // the index built at the call's cell and the live map; max_dist = radius, r2, min_conf (points, n, k, outputs unused)
  unsigned n;               // rows of the map: the length of the per-row arrays below
  int k;                    // neighbours used: 3 .. 16
  unsigned min_neighbors;
  int normal_source;        // BOUNDARY_*
  float max_gap;
  const uint8_t* part_in;   // STORED: one byte per row, non-zero = the row passes the selection; null: every row does
  NormalArgs nrm;           // ESTIMATED: the estimate's arguments and outputs (normal_join, unchanged, enqueued before the join)
  const float4* nest;       // ESTIMATED: nrm.est
  const uint8_t* nstatus;   // ESTIMATED: nrm.status (NORMAL_NONE at every row that takes no part)
  uint2* stat;              // per row {bits of gap, count}; every row is written by the join
  uint8_t* status;          // per row BOUNDARY_*; every row is written by the join
  ComponentArgs loops;      // the loops: component_hook / component_label, unchanged, with sel = node = the BOUNDARY byte of every row
  BoundaryResult* res;      // the call's result on the device
};
// stat and status of every row: one lane per record of the index, in index order; nothing is launched for an empty map
void boundary_join(const BoundaryArgs& a, hipStream_t s);
// flags[row] = 1 for the rows whose status is `what`, 0 for every other row (every row is written)
void boundary_flags(const BoundaryArgs& a, unsigned what, uint8_t* flags, hipStream_t s);
// *a.res (zeroed by the caller) from the status bytes and *a.loops.res, listed = *total (0 with total null); then *copy_to = *res unless
// copy_to is null
void boundary_tally(const BoundaryArgs& a, const uint32_t* total, BoundaryResult* copy_to, hipStream_t s);
// the optional per-row outputs of the rows r < min(rows, n) (each may be null)
void boundary_split(const BoundaryArgs& a, float* gap, uint32_t* count, uint8_t* status, uint32_t* label, uint32_t* size, unsigned rows,
                    hipStream_t s);

// ---- fuse surfels into the map (ef_fuse.inc; ef_map_fuse of include/ef_hip.h) ----
constexpr unsigned long long FUSE_KEY_EMPTY = 0xFFFFFFFFFFFFFFFFull;
constexpr unsigned FUSE_SKIPPED = 0, FUSE_NOVEL = 1, FUSE_WEIGHTLESS = 2, FUSE_ABSORBED = 3, FUSE_FUSED = 4, FUSE_INSERTED = 5;   // EF_FUSE_*
struct MapFuseArgs {
  InsertArgs ins;           // what insert_gate was given and wrote: rec, n, the transform, last_time, count_before (= the rows of the old map),
                            // q.map (the live map), flags, dup and match_row (never null here)
  unsigned long long* key;  // one per row of the old map, FUSE_KEY_EMPTY before the election: (d2 bits << 32) | record index of the row's winner
  int append;
  uint8_t* outcome;         // one byte per record (never null here): FUSE_*
};
// the election: key[s] = the minimum over the competitors of row s
void fuse_pick(const MapFuseArgs& a, hipStream_t s);
// outcome[] of every record; nothing else is written
void fuse_outcome(const MapFuseArgs& a, hipStream_t s);
// the records whose outcome is FUSE_FUSED merged into their rows, in place
void fuse_apply(const MapFuseArgs& a, hipStream_t s);

}  // namespace efm
