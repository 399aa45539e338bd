// Smooth regions of the map: the connected components of the low-curvature surfels under "close and smooth", the crease surfels attached to the
// region of their nearest smooth core (ef_map_regions / ef_map_regions_select / ef_map_remove_regions, include/ef_hip.h; DESIGN.md §8m).
// Included at the end of ef_map_kernels.hip, after ef_normals.inc.  It uses the query's index and its cell walk (ef_query.inc: query_visit with
// the self exclusion), the normals' join (ef_normals.inc: normal_join, called unchanged by the host into the regions' own scratch), the
// union-find of ef_unionfind.hpp with the components' device operations and pointer-jumping kernel (ef_components.inc: UfDevice, k_comp_jump,
// used where they stand) and the selection's flag -> count -> scan -> list chain (ef_select.inc) unchanged.  No frame kernel reads or writes
// anything here.
//   init      k_region_init: the kind byte from the join's status byte, the confidence and the curvature; parent[r] = r for a core and NONE
//             otherwise, attach[r] = NONE, members[r] = 0; with REGIONS_STORED the word {stored normal, curvature} per row, so that every later
//             kernel reads ONE per-row word {n_s, curvature} whatever the source.
//   first     k_region_first: parent[s] = the smallest lower smooth core neighbour of the core s.  No atomics (k_comp_first's reason).
//   jump      k_comp_jump, a few passes after `first` and after `hook`.
//   hook      k_region_hook: k_comp_hook's shape, one lane per record in index order.  For a candidate in a LOWER row inside the radius the lane
//             reads the candidate's kind byte; only for a core does it gather the candidate's 16-byte word by row, form the f32 dot and unite.
//             The atomic discipline is the components': relaxed agent-scope loads, compare-and-swap / minimum writes, nobody waits.
//   attach    k_region_attach: one lane per record, working for borders only: the same walk keeps the best (d2, row) among the smooth cores in
//             registers and writes attach[b].  No atomics: a lane writes its own word.
//   label     k_region_label (the next launch: plain loads see everything): a core walks to its root, a border walks from attach[b];
//             members[label] += 1, added up inside the wave first.
//   finish    k_region_finish: the list's byte per row and the result's counts (integer atomics, exact in any order); k_region_tally,
//             k_region_split as the components'.  Lists and the removal are flags_count / select_rows / the erase, unchanged.
namespace {

constexpr int REGION_FINISH_BLOCKS = 1024;   // k_region_finish strides the rows: at most this many workgroups add to the result's words

// SMOOTH(s, t) of the header: the f32 dot in the written bracketing (the products commute: the same bits from either end); a NaN compares false
__device__ __forceinline__ bool region_smooth(const RegionArgs& A, const float4& a, const float4& b) {
  const float dot = (a.x * b.x + a.y * b.y) + a.z * b.z;
  return (A.two_sided ? fabsf(dot) : dot) >= A.min_normal_cos;
}

__global__ void __launch_bounds__(BLK) k_region_init(const RegionArgs A) {
  const unsigned r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= A.nrm.n) return;
  const float4 e = A.nrm.est[r];
  const bool node = (A.nrm.status[r] & NORMAL_STATUS_MASK) == NORMAL_ESTIMATED && A.nrm.q.map.pos_conf[r].w > A.nrm.q.min_conf;
  const bool core = node && e.w <= A.max_curvature;
  A.kind[r] = (uint8_t)(core ? REGION_KIND_CORE : node ? REGION_KIND_BORDER : REGION_KIND_NONE);
  A.parent[r] = core ? r : REGION_NONE;
  A.attach[r] = REGION_NONE;
  A.members[r] = 0u;
  if (A.normal_source == REGIONS_STORED) {
    const float4 m = A.nrm.q.map.nrm_rad[r];
    A.stored[r] = make_float4(m.x, m.y, m.z, e.w);
  }
}

// Every core's word = the smallest of its lower smooth core neighbours (its own row without one).  Each of these links is an edge, and
// parent < self, so this is a valid forest of the union-find before the hook starts; no atomics: a lane writes its own word and reads nobody's.
__global__ void __launch_bounds__(BLK) k_region_first(const RegionArgs A) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned n_rec = min(A.nrm.q.cells[A.nrm.q.mask], A.nrm.n);
  if (t >= n_rec) return;
  const float4 q = A.nrm.q.sorted[t];
  const unsigned row = A.nrm.q.rows[t];
  if (row >= A.nrm.n || A.kind[row] != REGION_KIND_CORE) return;
  const float4 mine = A.nw[row];
  unsigned low = row;
  query_visit<1, true>(A.nrm.q, q.x, q.y, q.z, 0u, t, [&](float, unsigned k) {
    const unsigned r = A.nrm.q.rows[k];
    if (r >= low || A.kind[r] != REGION_KIND_CORE) return;
    if (region_smooth(A, mine, A.nw[r])) low = r;
  });
  A.parent[row] = low;
}

__global__ void __launch_bounds__(BLK) k_region_hook(const RegionArgs A) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned n_rec = min(A.nrm.q.cells[A.nrm.q.mask], A.nrm.n);   // the records of the index: the end of its last bucket
  if (t >= n_rec) return;
  const float4 q = A.nrm.q.sorted[t];
  const unsigned row = A.nrm.q.rows[t];
  if (row >= A.nrm.n || A.kind[row] != REGION_KIND_CORE) return;
  const float4 mine = A.nw[row];
  const unsigned cap = A.nrm.n + 64u;
  unsigned cur = row;   // a row of this lane's set that the last union left nearest the root
  bool ok = true;
  query_visit<1, true>(A.nrm.q, q.x, q.y, q.z, 0u, t, [&](float, unsigned k) {
    const unsigned r = A.nrm.q.rows[k];
    if (r >= row || !ok) return;
    if (A.kind[r] != REGION_KIND_CORE) return;          // one byte first: the 16-byte gather below is paid for cores only
    if (!region_smooth(A, mine, A.nw[r])) return;
    ok = uf_union<UfDevice>(A.parent, cur, r, cap, &cur);
  });
  if (!ok) atomicOr(&A.res->status, 1u);
}

__global__ void __launch_bounds__(BLK) k_region_attach(const RegionArgs A) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned n_rec = min(A.nrm.q.cells[A.nrm.q.mask], A.nrm.n);
  if (t >= n_rec) return;
  const float4 q = A.nrm.q.sorted[t];
  const unsigned row = A.nrm.q.rows[t];
  if (row >= A.nrm.n || A.kind[row] != REGION_KIND_BORDER) return;
  const float4 mine = A.nw[row];
  float bd = __builtin_inff();
  unsigned br = REGION_NONE;
  query_visit<1, true>(A.nrm.q, q.x, q.y, q.z, 0u, t, [&](float d2, unsigned k) {
    const unsigned r = A.nrm.q.rows[k];
    if (r >= A.nrm.n || !query_less(d2, r, bd, br)) return;
    if (A.kind[r] != REGION_KIND_CORE) return;
    if (!region_smooth(A, mine, A.nw[r])) return;
    bd = d2;
    br = r;
  });
  A.attach[row] = br;
}

__global__ void __launch_bounds__(BLK) k_region_label(const RegionArgs A) {
  const unsigned r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= A.nrm.n) return;
  const unsigned kind = A.kind[r];
  unsigned at = kind == REGION_KIND_CORE ? r : kind == REGION_KIND_BORDER ? A.attach[r] : REGION_NONE;
  unsigned x = REGION_NONE;
  if (at < A.nrm.n) {
    const unsigned cap = A.nrm.n + 64u;
    x = A.parent[at];
    for (unsigned steps = 0; x < at; ++steps) {   // (x == at: the root)
      if (steps > cap) { atomicOr(&A.res->status, 2u); break; }
      at = x;
      x = A.parent[at];
    }
    if (x >= A.nrm.n) {   // (a word that is no row: only a logic error puts one there; status says so)
      x = REGION_NONE;
      atomicOr(&A.res->status, 4u);
    }
  }
  A.label[r] = x;
  // members[label] += 1, the lanes of a wave that share a label first added up among themselves (k_comp_label's reason and form)
  unsigned long long todo = __ballot(x != REGION_NONE);
  while (todo) {
    const unsigned lead = (unsigned)__ffsll((long long)todo) - 1u;
    const unsigned lx = __shfl(x, (int)lead);
    const unsigned long long same = __ballot(x == lx) & todo;
    if ((threadIdx.x & 63u) == lead) atomicAdd(&A.members[lx], (unsigned)__popcll(same));
    todo &= ~same;
  }
}

__global__ void __launch_bounds__(BLK) k_region_finish(const RegionArgs A, int what, uint8_t* __restrict__ flags) {
  // nodes, cores, borders, attached, unassigned, regions, largest, rejected_rows, rejected_regions, listed: the result's first ten words
  __shared__ unsigned tot[10];
  if (threadIdx.x < 10) tot[threadIdx.x] = 0u;
  __syncthreads();
  unsigned c[10] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  for (unsigned r = blockIdx.x * blockDim.x + threadIdx.x; r < A.nrm.n; r += gridDim.x * blockDim.x) {
    const unsigned kind = A.kind[r], l = A.label[r];
    const bool node = kind != REGION_KIND_NONE, border = kind == REGION_KIND_BORDER, has = l != REGION_NONE;
    const unsigned size = has ? A.members[l] : 0u;
    const bool rejected = has && (size < A.min_size || (A.max_size != 0u && size > A.max_size));
    const bool unassigned = node && !has;
    const bool listed = what == REGIONS_REJECTED ? rejected : what == REGIONS_ACCEPTED ? (has && !rejected) : what == REGIONS_UNASSIGNED ? unassigned : border;
    if (flags) flags[r] = listed ? 1 : 0;
    c[0] += node;
    c[1] += kind == REGION_KIND_CORE;
    c[2] += border;
    c[3] += border && has;
    c[4] += unassigned;
    if (has && l == r) {
      ++c[5];
      c[6] = max(c[6], size);
      c[8] += rejected;
    }
    c[7] += rejected;
    c[9] += listed;
  }
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    if (!c[i]) continue;
    if (i == 6) atomicMax(&tot[i], c[i]);
    else atomicAdd(&tot[i], c[i]);
  }
  __syncthreads();
  if (threadIdx.x >= 10 || !tot[threadIdx.x]) return;
  uint32_t* word = &A.res->nodes + threadIdx.x;   // (RegionResult is twelve consecutive words: ef_host_regions.inc asserts the layout)
  if (threadIdx.x == 6) atomicMax(word, tot[6]);
  else atomicAdd(word, tot[threadIdx.x]);
}

__global__ void k_region_tally(RegionResult* res, unsigned n, RegionResult* copy_to) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  RegionResult r = *res;
  r.count_after = n - r.listed;
  *res = r;
  if (copy_to) *copy_to = r;
}

__global__ void __launch_bounds__(BLK) k_region_split(const uint32_t* __restrict__ label_in, const uint32_t* __restrict__ members,
                                                      const uint8_t* __restrict__ kind_in, unsigned rows, uint32_t* __restrict__ label,
                                                      uint32_t* __restrict__ size, uint8_t* __restrict__ kind) {
  const unsigned r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const unsigned l = label_in[r];
  if (label) label[r] = l;
  if (size) size[r] = l != REGION_NONE ? members[l] : 0u;
  if (kind) kind[r] = kind_in[r];
}

}  // namespace

void region_hook(const RegionArgs& a, hipStream_t s) {
  if (!a.nrm.n) return;
  const dim3 g(ceil_div((int)a.nrm.n, BLK)), b(BLK);
  int passes = 2;   // about log8(n) + 2, as component_hook's (speed only: k_region_label walks what is left)
  for (unsigned m = 1; m < a.nrm.n; m *= 8) ++passes;
  hipLaunchKernelGGL(k_region_init, g, b, 0, s, a);
  hipLaunchKernelGGL(k_region_first, g, b, 0, s, a);
  for (int i = 0; i < passes; ++i) hipLaunchKernelGGL(k_comp_jump, g, b, 0, s, a.parent, a.nrm.n);
  hipLaunchKernelGGL(k_region_hook, g, b, 0, s, a);
  for (int i = 0; i < passes; ++i) hipLaunchKernelGGL(k_comp_jump, g, b, 0, s, a.parent, a.nrm.n);
  if (a.attach_borders) hipLaunchKernelGGL(k_region_attach, g, b, 0, s, a);
}
void region_label(const RegionArgs& a, int what, uint8_t* flags, hipStream_t s) {
  if (!a.nrm.n) return;
  const int g = ceil_div((int)a.nrm.n, BLK);
  hipLaunchKernelGGL(k_region_label, dim3(g), dim3(BLK), 0, s, a);
  hipLaunchKernelGGL(k_region_finish, dim3(min(g, REGION_FINISH_BLOCKS)), dim3(BLK), 0, s, a, what, flags);
}
void region_tally(const RegionArgs& a, RegionResult* copy_to, hipStream_t s) {
  hipLaunchKernelGGL(k_region_tally, dim3(1), dim3(64), 0, s, a.res, a.nrm.n, copy_to);
}
void region_split(const RegionArgs& a, uint32_t* label, uint32_t* size, uint8_t* kind, unsigned rows, hipStream_t s) {
  rows = rows < a.nrm.n ? rows : a.nrm.n;
  if (rows && (label || size || kind))
    hipLaunchKernelGGL(k_region_split, dim3(ceil_div((int)rows, BLK)), dim3(BLK), 0, s, (const uint32_t*)a.label, (const uint32_t*)a.members,
                       (const uint8_t*)a.kind, rows, label, size, kind);
}
