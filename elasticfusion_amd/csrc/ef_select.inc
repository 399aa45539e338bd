// Select, extract and erase surfels (ef_map_select / ef_map_gather / ef_map_erase, include/ef_hip.h; DESIGN.md §8d).
// Included at the end of ef_map_kernels.hip, after ef_register.inc.  No frame kernel reads or writes anything here.
//   select    k_select_flags (one predicate over the streams an enabled test needs: one byte per row, one count per SELECT_ROW rows),
//             k_scan_chunks (the compaction passes' multi-launch scan: one workgroup, trips bounded by the chunk count), then
//             k_select_rows (the ascending row list) or k_select_compact (the erase's stable scatter of the three streams).
//   rows      k_select_mark_rows scatters a 1 into the flag of every named row, k_select_count counts per chunk.
//   gather    k_map_gather: three lanes per row, one float4 each, so that the 48-byte records are one contiguous run of the output.
// Nothing waits for another workgroup, every loop is bounded by the row count, and there are no atomics: the counts are wave ballots.
namespace {

constexpr int SELECT_ROW = BLK;        // rows per chunk: one per thread
constexpr int SELECT_LDS_FLOATS = 4096;   // label floats staged per step of the LABEL test (16 KiB)

// the calling lane's rank among the lanes of `mask` below it
__device__ __forceinline__ unsigned select_rank(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}
// the workgroup's number of set flags (every thread gets it) and, in `before`, the number in the threads below the caller
__device__ __forceinline__ unsigned select_block_rank(bool f, unsigned* lds, unsigned& before) {
  const unsigned long long m = __ballot(f);
  const unsigned w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[w] = (unsigned)__popcll(m);
  __syncthreads();
  unsigned base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < BLK / 64; ++i) {
    const unsigned s = lds[i];
    if ((unsigned)i < w) base += s;
    tot += s;
  }
  before = base + select_rank(m);
  return tot;
}

// flags[i] = row i is selected (every enabled test passes, XOR invert); chunk_count[c] = selected rows of chunk c.  The test set is uniform:
// a BOX-only selection reads the position stream alone.
__global__ void __launch_bounds__(BLK) k_select_flags(const SelectArgs A, uint8_t* __restrict__ flags, uint32_t* __restrict__ chunk_count) {
  __shared__ unsigned lds[BLK / 64];
  __shared__ float s_tab[SELECT_LDS_FLOATS];
  __shared__ uint8_t s_label[BLK];
  const unsigned r0 = blockIdx.x * SELECT_ROW, i = r0 + threadIdx.x;
  const bool live = i < A.n;
  bool pass = true;
  if (live) {
    if (A.tests & (SEL_BOX | SEL_CONF)) {
      const float4 p = A.map.pos_conf[i];
      if (A.tests & SEL_BOX) {
        const float bx = ((A.R[0] * p.x + A.R[1] * p.y) + A.R[2] * p.z) + A.t[0];
        const float by = ((A.R[3] * p.x + A.R[4] * p.y) + A.R[5] * p.z) + A.t[1];
        const float bz = ((A.R[6] * p.x + A.R[7] * p.y) + A.R[8] * p.z) + A.t[2];
        pass = pass && A.box_min[0] <= bx && bx <= A.box_max[0] && A.box_min[1] <= by && by <= A.box_max[1] && A.box_min[2] <= bz &&
               bz <= A.box_max[2];
      }
      if (A.tests & SEL_CONF) pass = pass && A.conf_min <= p.w && p.w <= A.conf_max;
    }
    if (A.tests & (SEL_INIT_TIME | SEL_LAST_TIME | SEL_ID)) {
      const float4 ct = A.map.col_time[i];
      if (A.tests & SEL_INIT_TIME) pass = pass && A.init_min <= ct.z && ct.z <= A.init_max;
      if (A.tests & SEL_LAST_TIME) pass = pass && A.last_min <= ct.w && ct.w <= A.last_max;
      if (A.tests & SEL_ID) {
        const unsigned id = __float_as_uint(ct.y);
        pass = pass && A.id_min <= id && id <= A.id_max;
      }
    }
    if (A.tests & SEL_RADIUS) {
      const float r = A.map.nrm_rad[i].w;
      pass = pass && A.radius_min <= r && r <= A.radius_max;
    }
  }
  if (A.tests & SEL_LABEL) {
    // The chunk's rows x C floats are one contiguous run of the table: staged through LDS `step` rows at a time by consecutive lanes on
    // consecutive floats (stride C + 1 in LDS when C is even: the per-row walk below then spreads over the banks), then one lane per row
    // takes the argmax (ties to the lowest class: a later class wins only when strictly greater).
    const unsigned C = (unsigned)A.C, rows = min((unsigned)SELECT_ROW, A.n - r0);
    const unsigned stride = C | 1u;
    const unsigned step = max(1u, min((unsigned)SELECT_ROW, (unsigned)SELECT_LDS_FLOATS / stride));
    const float invC = 1.0f / (float)C;
    for (unsigned b = 0; b < rows; b += step) {
      const unsigned nr = min(step, rows - b), nf = nr * C;
      const float* src = A.tab + ((size_t)r0 + b) * C;
      for (unsigned f = threadIdx.x; f < nf; f += BLK) {
        unsigned rr = (unsigned)((float)f * invC);   // f < 2^16: off by at most one
        if (rr * C > f) --rr;
        else if ((rr + 1) * C <= f) ++rr;
        s_tab[rr * stride + (f - rr * C)] = src[f];
      }
      __syncthreads();
      if (threadIdx.x < nr) {
        const float* row = s_tab + threadIdx.x * stride;
        unsigned best = 0;
        float bp = row[0];
        for (unsigned c = 1; c < C; ++c) {
          const float v = row[c];
          if (v > bp) { bp = v; best = c; }
        }
        s_label[b + threadIdx.x] = (best == (unsigned)A.label_class && bp >= A.label_min_prob) ? 1 : 0;
      }
      __syncthreads();
    }
    if (live) pass = pass && s_label[threadIdx.x] != 0;
  }
  const bool sel = live && (pass != (A.invert != 0));
  if (live) flags[i] = sel ? 1 : 0;
  unsigned before;
  const unsigned tot = select_block_rank(sel, lds, before);
  if (threadIdx.x == 0) chunk_count[blockIdx.x] = tot;
}

// flags (zeroed by the caller) of the named rows; duplicates store the same byte twice, rows >= n are skipped
__global__ void __launch_bounds__(BLK) k_select_mark_rows(const uint32_t* __restrict__ rows, unsigned n_rows, unsigned n, uint8_t* __restrict__ flags) {
  for (unsigned k = blockIdx.x * blockDim.x + threadIdx.x; k < n_rows; k += gridDim.x * blockDim.x) {
    const uint32_t r = rows[k];
    if (r < n) flags[r] = 1;
  }
}
// chunk_count[c] = rows of chunk c whose flag differs from `flip`
__global__ void __launch_bounds__(BLK) k_select_count(const uint8_t* __restrict__ flags, unsigned n, unsigned flip, uint32_t* __restrict__ chunk_count) {
  __shared__ unsigned lds[BLK / 64];
  const unsigned i = blockIdx.x * SELECT_ROW + threadIdx.x;
  const bool f = i < n && (unsigned)flags[i] != flip;
  unsigned before;
  const unsigned tot = select_block_rank(f, lds, before);
  if (threadIdx.x == 0) chunk_count[blockIdx.x] = tot;
}

// the selected rows in ascending order, the first max_rows of them
__global__ void __launch_bounds__(BLK) k_select_rows(const uint8_t* __restrict__ flags, const uint32_t* __restrict__ chunk_offset, unsigned n,
                                                     uint32_t* __restrict__ rows, unsigned max_rows) {
  __shared__ unsigned lds[BLK / 64];
  const unsigned i = blockIdx.x * SELECT_ROW + threadIdx.x;
  const bool f = i < n && flags[i] != 0;
  unsigned before;
  select_block_rank(f, lds, before);
  const unsigned pos = chunk_offset[blockIdx.x] + before;
  if (f && pos < max_rows) rows[pos] = i;
}

// the erase: rows whose flag differs from `flip` move to dst in their old order, all three streams as data (the ID lane with them)
__global__ void __launch_bounds__(BLK) k_select_compact(const uint8_t* __restrict__ flags, unsigned flip, const uint32_t* __restrict__ chunk_offset,
                                                        unsigned n, SurfelSoA src, SurfelSoA dst) {
  __shared__ unsigned lds[BLK / 64];
  const unsigned i = blockIdx.x * SELECT_ROW + threadIdx.x;
  const bool f = i < n && (unsigned)flags[i] != flip;
  unsigned before;
  select_block_rank(f, lds, before);
  if (!f) return;
  const unsigned pos = chunk_offset[blockIdx.x] + before;   // pos <= i < n: inside both buffers
  dst.pos_conf[pos] = src.pos_conf[i];
  dst.col_time[pos] = src.col_time[i];
  dst.nrm_rad[pos] = src.nrm_rad[i];
}

// out4[3 k + part] = stream `part` of row rows[k]: consecutive lanes write consecutive 16-byte words; a row >= n gives zeros
__global__ void __launch_bounds__(BLK) k_map_gather(SurfelSoA map, unsigned n, const uint32_t* __restrict__ rows, unsigned n_rows,
                                                    float4* __restrict__ out4) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)n_rows * 3) return;
  const unsigned k = (unsigned)(t / 3), part = (unsigned)(t - (size_t)k * 3);
  const uint32_t r = rows[k];
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (r < n) v = part == 0 ? map.pos_conf[r] : part == 1 ? map.col_time[r] : map.nrm_rad[r];
  out4[t] = v;
}

}  // namespace

unsigned select_chunks(unsigned n) { return (n + SELECT_ROW - 1) / SELECT_ROW; }

// the scan of the chunk counts: offsets, and the total into *total (and, clamped to capacity — it never exceeds it — into *count_out)
static void select_scan(const SelectScratch& sc, unsigned n, uint32_t* total, unsigned* count_out, uint32_t capacity, hipStream_t s) {
  hipLaunchKernelGGL(k_scan_chunks, dim3(1), dim3(1024), 0, s, (const uint32_t*)sc.chunk_count, (const unsigned*)nullptr, n, sc.chunk_offset, total,
                     count_out, capacity, (int*)nullptr, (unsigned)SELECT_ROW);
}

void select_flags(const SelectArgs& a, const SelectScratch& sc, uint32_t* total, hipStream_t s) {
  // (n = 0: the scan alone writes the total 0)
  if (a.n) hipLaunchKernelGGL(k_select_flags, dim3(select_chunks(a.n)), dim3(BLK), 0, s, a, sc.flags, sc.chunk_count);
  select_scan(sc, a.n, total, nullptr, 0u, s);
}
void flags_count(const SelectScratch& sc, unsigned n, unsigned flip, uint32_t* total, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_select_count, dim3(select_chunks(n)), dim3(BLK), 0, s, (const uint8_t*)sc.flags, n, flip, sc.chunk_count);
  select_scan(sc, n, total, nullptr, 0u, s);
}
void select_mark_rows(const uint32_t* rows, unsigned n_rows, unsigned n, unsigned flip, const SelectScratch& sc, uint32_t* total, hipStream_t s) {
  if (n) {
    (void)hipMemsetAsync(sc.flags, 0, n, s);
    const unsigned g = (unsigned)min(((size_t)n_rows + BLK - 1) / BLK, (size_t)8192);
    if (n_rows) hipLaunchKernelGGL(k_select_mark_rows, dim3(g), dim3(BLK), 0, s, rows, n_rows, n, sc.flags);
  }
  flags_count(sc, n, flip, total, s);
}
void select_rows(const SelectScratch& sc, unsigned n, uint32_t* rows, unsigned max_rows, hipStream_t s) {
  if (n && max_rows)
    hipLaunchKernelGGL(k_select_rows, dim3(select_chunks(n)), dim3(BLK), 0, s, (const uint8_t*)sc.flags, (const uint32_t*)sc.chunk_offset, n, rows, max_rows);
}
void select_compact(const SelectScratch& sc, unsigned n, unsigned flip, SurfelSoA src, SurfelSoA dst, hipStream_t s) {
  if (n)
    hipLaunchKernelGGL(k_select_compact, dim3(select_chunks(n)), dim3(BLK), 0, s, (const uint8_t*)sc.flags, flip, (const uint32_t*)sc.chunk_offset, n, src, dst);
}
void map_gather(SurfelSoA map, unsigned n, const uint32_t* rows, unsigned n_rows, float* out, hipStream_t s) {
  if (!n_rows) return;
  const size_t groups = ((size_t)n_rows * 3 + BLK - 1) / BLK;
  hipLaunchKernelGGL(k_map_gather, dim3((unsigned)groups), dim3(BLK), 0, s, map, n, rows, n_rows, (float4*)out);
}
