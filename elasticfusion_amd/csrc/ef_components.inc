// Connected components of the map under "closer than r" (ef_map_components / ef_map_components_select / ef_map_remove_components,
// include/ef_hip.h; DESIGN.md §8j).  Included at the end of ef_map_kernels.hip, after ef_outlier.inc.  It uses the query's index and its cell
// walk (ef_query.inc: query_visit with the self exclusion), the union-find of ef_unionfind.hpp and the selection's flag -> count -> scan ->
// list chain (ef_select.inc) unchanged.  No frame kernel reads or writes anything here.
//   init      k_comp_init: the node byte, parent[r] = r for a node and NONE otherwise, members[r] = 0.
//   first     k_comp_first: the same self-join with a trivial visitor: parent[s] = the smallest lower neighbour node of s.  No atomics.  Without
//             it the hook starts from singletons and builds chains thousands of links deep (measured: DESIGN.md §8j).
//   jump      k_comp_jump, a few passes after `first` and after `hook`: pointer jumping with plain loads and stores, between launches that
//             unite, never beside one.
//   hook      k_comp_hook: the self-join of the map on its own index, one lane per record in index order (as k_outlier_join).  For every
//             eligible candidate in a LOWER row (an edge is symmetric: the lane of its greater end sees it) the lane unites the two rows'
//             sets.  ONE launch, whatever the components' diameters.  Inside it every read of parent is a relaxed agent-scope atomic load and
//             every write an agent-scope compare-and-swap or minimum: a CU's L1 is never refreshed and the XCDs' L2s are not coherent, and no
//             result depends on how fresh a load is (ef_unionfind.hpp).  Nothing is handed from one workgroup to another: nobody waits, spins
//             or polls, and the next launch is the only consumer.
//   label     k_comp_label (the next launch: plain loads see everything): label[r] = the root of r, one integer atomicAdd on members[label].
//   finish    k_comp_finish: the reject / accept byte per row and the result's counts (integer atomics, exact in any order).
//             Lists and the removal are flags_count / select_rows / the erase, unchanged.
namespace {

constexpr int COMP_FINISH_BLOCKS = 1024;   // k_comp_finish strides the rows: at most this many workgroups add to the result's five words

struct UfDevice {   // the union-find's atomic operations on the device (ef_unionfind.hpp)
  static __device__ __forceinline__ uint32_t load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ __forceinline__ uint32_t cas(uint32_t* p, uint32_t expect, uint32_t want) { return atomicCAS(p, expect, want); }
  static __device__ __forceinline__ void lower(uint32_t* p, uint32_t v) { atomicMin(p, v); }
};

__global__ void __launch_bounds__(BLK) k_comp_init(const ComponentArgs A) {
  const unsigned r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= A.n) return;
  const float4 p = A.q.map.pos_conf[r];
  const bool node = (!A.sel || A.sel[r] != 0) && query_finite3(p.x, p.y, p.z) && p.w > A.q.min_conf;
  A.node[r] = node ? 1 : 0;
  A.parent[r] = node ? r : COMPONENT_NONE;
  A.members[r] = 0u;
}

// Every node's word = the smallest of its lower neighbour nodes (its own row without one).  Each of these links is an edge, and parent < self,
// so this is a valid forest of the union-find before the hook starts; no atomics: a lane writes its own word and reads nobody's.
__global__ void __launch_bounds__(BLK) k_comp_first(const ComponentArgs A) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned n_rec = min(A.q.cells[A.q.mask], A.n);
  if (t >= n_rec) return;
  const float4 q = A.q.sorted[t];
  const unsigned row = A.q.rows[t];
  if (row >= A.n || !A.node[row]) return;
  unsigned low = row;
  query_visit<1, true>(A.q, q.x, q.y, q.z, 0u, t, [&](float, unsigned k) {
    const unsigned r = A.q.rows[k];
    if (r < low && A.node[r]) low = r;
  });
  A.parent[row] = low;
}

// Pointer jumping between the launches that unite: parent[r] = up to its eighth ancestor as this lane's plain loads show it.  Any value read,
// old or new, is an ancestor below the row it was read from, and words only decrease, so a pass can only shorten chains (a chain of depth d
// is at most ceil(d / 2) deep afterwards, usually d / 8); no result depends on how many passes ran: k_comp_label walks what is left.
__global__ void __launch_bounds__(BLK) k_comp_jump(uint32_t* __restrict__ parent, unsigned n) {
  const unsigned r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const unsigned p0 = parent[r];
  if (p0 >= r) return;   // a root, or a row that is no node
  unsigned p = p0;
#pragma unroll 1
  for (int i = 0; i < 7; ++i) {
    const unsigned q = parent[p];   // (p < r < n)
    if (q >= p) break;
    p = q;
  }
  if (p != p0) parent[r] = p;
}

__global__ void __launch_bounds__(BLK) k_comp_hook(const ComponentArgs A) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned n_rec = min(A.q.cells[A.q.mask], A.n);   // the records of the index: the end of its last bucket
  if (t >= n_rec) return;
  const float4 q = A.q.sorted[t];
  const unsigned row = A.q.rows[t];
  if (row >= A.n || !A.node[row]) return;
  const unsigned cap = A.n + 64u;
  unsigned cur = row;   // a row of this lane's set that the last union left nearest the root
  bool ok = true;
  query_visit<1, true>(A.q, q.x, q.y, q.z, 0u, t, [&](float, unsigned k) {
    const unsigned r = A.q.rows[k];
    if (r >= row || !ok) return;
    if (!A.node[r]) return;   // (without a selection the walk's own tests are the node rule already; the byte does not rely on the index's copy)
    ok = uf_union<UfDevice>(A.parent, cur, r, cap, &cur);
  });
  if (!ok) atomicOr(&A.res->status, 1u);
}

__global__ void __launch_bounds__(BLK) k_comp_label(const ComponentArgs A) {
  const unsigned r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= A.n) return;
  unsigned x = A.parent[r];
  if (x != COMPONENT_NONE) {
    const unsigned cap = A.n + 64u;
    unsigned steps = 0;
    for (unsigned at = r; x < at; ++steps) {   // (x == at: the root)
      if (steps > cap) { atomicOr(&A.res->status, 2u); break; }
      at = x;
      x = A.parent[at];
    }
    if (x >= A.n) x = COMPONENT_NONE;   // (a word that is no row: only a logic error puts one there; status says so)
  }
  A.label[r] = x;
  // members[label] += 1, the lanes of a wave that share a label first added up among themselves: a component of a million rows is a million
  // adds to ONE word otherwise, and one word takes about 88 adds per microsecond (measured: 13.05 ms of this kernel on 1.15 M rows)
  unsigned long long todo = __ballot(x != COMPONENT_NONE);
  while (todo) {
    const unsigned lead = (unsigned)__ffsll((long long)todo) - 1u;
    const unsigned lx = __shfl(x, (int)lead);
    const unsigned long long same = __ballot(x == lx) & todo;
    if ((threadIdx.x & 63u) == lead) atomicAdd(&A.members[lx], (unsigned)__popcll(same));
    todo &= ~same;
  }
}

__global__ void __launch_bounds__(BLK) k_comp_finish(const ComponentArgs A, int what, uint8_t* __restrict__ flags) {
  __shared__ unsigned tot[5];   // nodes, components, largest, rejected_rows, rejected_components
  if (threadIdx.x < 5) tot[threadIdx.x] = 0u;
  __syncthreads();
  unsigned nodes = 0, comps = 0, largest = 0, rej_rows = 0, rej_comps = 0;
  for (unsigned r = blockIdx.x * blockDim.x + threadIdx.x; r < A.n; r += gridDim.x * blockDim.x) {
    const unsigned l = A.label[r];
    const bool node = l != COMPONENT_NONE;
    const unsigned size = node ? A.members[l] : 0u;
    const bool rejected = node && (size < A.min_size || (A.max_size != 0u && size > A.max_size));
    if (flags) flags[r] = (what == COMPONENTS_REJECTED ? rejected : (node && !rejected)) ? 1 : 0;
    nodes += node;
    rej_rows += rejected;
    if (l == r) {
      ++comps;
      rej_comps += rejected;
      largest = max(largest, size);
    }
  }
  if (nodes) atomicAdd(&tot[0], nodes);
  if (comps) { atomicAdd(&tot[1], comps); atomicMax(&tot[2], largest); }
  if (rej_rows) atomicAdd(&tot[3], rej_rows);
  if (rej_comps) atomicAdd(&tot[4], rej_comps);
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (tot[0]) atomicAdd(&A.res->nodes, tot[0]);
  if (tot[1]) { atomicAdd(&A.res->components, tot[1]); atomicMax(&A.res->largest, tot[2]); }
  if (tot[3]) atomicAdd(&A.res->rejected_rows, tot[3]);
  if (tot[4]) atomicAdd(&A.res->rejected_components, tot[4]);
}

__global__ void k_comp_tally(ComponentResult* res, unsigned n, ComponentResult* copy_to) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  ComponentResult r = *res;
  r.count_after = n - r.rejected_rows;
  *res = r;
  if (copy_to) *copy_to = r;
}

__global__ void __launch_bounds__(BLK) k_comp_split(const uint32_t* __restrict__ label_in, const uint32_t* __restrict__ members, unsigned rows,
                                                    uint32_t* __restrict__ label, uint32_t* __restrict__ size) {
  const unsigned r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const unsigned l = label_in[r];
  if (label) label[r] = l;
  if (size) size[r] = l != COMPONENT_NONE ? members[l] : 0u;
}

}  // namespace

void component_hook(const ComponentArgs& a, hipStream_t s) {
  if (!a.n) return;
  const dim3 g(ceil_div((int)a.n, BLK)), b(BLK);
  int passes = 2;   // about log8(n) + 2: enough to flatten what the links below leave on the maps measured (DESIGN.md §8j); speed only
  for (unsigned m = 1; m < a.n; m *= 8) ++passes;
  hipLaunchKernelGGL(k_comp_init, g, b, 0, s, a);
  hipLaunchKernelGGL(k_comp_first, g, b, 0, s, a);
  for (int i = 0; i < passes; ++i) hipLaunchKernelGGL(k_comp_jump, g, b, 0, s, a.parent, a.n);
  hipLaunchKernelGGL(k_comp_hook, g, b, 0, s, a);
  for (int i = 0; i < passes; ++i) hipLaunchKernelGGL(k_comp_jump, g, b, 0, s, a.parent, a.n);
}
void component_label(const ComponentArgs& a, int what, uint8_t* flags, hipStream_t s) {
  if (!a.n) return;
  const int g = ceil_div((int)a.n, BLK);
  hipLaunchKernelGGL(k_comp_label, dim3(g), dim3(BLK), 0, s, a);
  hipLaunchKernelGGL(k_comp_finish, dim3(min(g, COMP_FINISH_BLOCKS)), dim3(BLK), 0, s, a, what, flags);
}
void component_tally(const ComponentArgs& a, ComponentResult* copy_to, hipStream_t s) {
  hipLaunchKernelGGL(k_comp_tally, dim3(1), dim3(64), 0, s, a.res, a.n, copy_to);
}
void component_split(const ComponentArgs& a, uint32_t* label, uint32_t* size, unsigned rows, hipStream_t s) {
  rows = rows < a.n ? rows : a.n;
  if (rows && (label || size))
    hipLaunchKernelGGL(k_comp_split, dim3(ceil_div((int)rows, BLK)), dim3(BLK), 0, s, (const uint32_t*)a.label, (const uint32_t*)a.members, rows, label, size);
}
