// Stable surfel IDs and per-surfel label fusion (ef_set_surfel_ids / ef_enable_labels / ef_fuse_labels, include/ef_hip.h; DESIGN.md §8a).
// Included at the end of ef_map_kernels.hip, after ef_render.inc.  No frame kernel reads or writes anything here:
//   the ID lane   the colour stream's unused .y ({colour, 0, initTime, lastTime}, init_unstable.vert:33) holds a uint32 ID as raw bits.  Every
//                 frame kernel creates surfels with .y = 0 and moves the float4 as data (fusion's merge, clean's deform and scatter, the
//                 layout conversions), and the map stays in creation order, so the lane is always a strictly increasing non-zero prefix
//                 followed by a zero suffix: the rows created since the last ID-consuming call.
//   the table     float [rows][C] in map row order, re-aligned lazily to the current rows by ID (both ID lists sorted), ping-pong.
namespace {

constexpr unsigned LABEL_NONE = 0xFFFFFFFFu;

__device__ __forceinline__ unsigned* id_lane(SurfelSoA map) { return reinterpret_cast<unsigned*>(map.col_time) + 1; }   // 4 words apart

// First index of [lo, hi) where pred is false, pred being true on a prefix (hi when it holds everywhere).  Called by a whole wave with uniform
// arguments; every lane returns the same index.  64 probes per step: log64 of the range in dependent loads instead of log2.
template <class Pred>
__device__ __forceinline__ unsigned wave_partition_point(unsigned lo, unsigned hi, Pred pred) {
  const unsigned k = threadIdx.x & 63;
  while (lo < hi) {
    const unsigned step = (hi - lo + 63) / 64;
    const unsigned p = lo + k * step;
    const bool t = p < hi && pred(p);
    const unsigned K = (unsigned)__popcll(__ballot(t));
    if (K == 0) break;                            // pred(lo) is false
    const unsigned nhi = min(hi, lo + K * step);  // probe K lies past the prefix (or past hi)
    lo = lo + (K - 1) * step + 1;
    hi = nhi;
  }
  return lo;
}

// One workgroup: find the zero suffix of the ID lane and number it from the counter st[0] (continued past the largest ID present: an upload may
// bring larger ones).  Wave 0 searches; the numbering is one store per new row.
__global__ void __launch_bounds__(1024) k_ids_assign(SurfelSoA map, const unsigned* __restrict__ count_dev, unsigned* st) {
  __shared__ unsigned s_start, s_base;
  const unsigned n = *count_dev;
  unsigned* lane = id_lane(map);
  if (threadIdx.x < 64) {
    const unsigned start = wave_partition_point(0u, n, [&](unsigned p) { return lane[(size_t)p * 4] != 0u; });
    if (threadIdx.x == 0) {
      unsigned base = st[0];
      if (start > 0) base = max(base, lane[(size_t)(start - 1) * 4] + 1u);
      s_start = start;
      s_base = base;
      st[0] = base + (n - start);
    }
  }
  __syncthreads();
  const unsigned start = s_start, base = s_base;
  for (unsigned i = start + threadIdx.x; i < n; i += blockDim.x) lane[(size_t)i * 4] = base + (i - start);
}

// the whole lane after an upload: *flag |= 1 unless it is a strictly increasing non-zero prefix followed by a zero suffix, |= 2 when
// k_ids_assign's numbering of that suffix, from max(*counter, largest ID + 1), would not stay below 0xFFFFFFFF with the counter it leaves
// (past it the numbering wraps: an ID of 0, or IDs below the prefix)
__global__ void k_ids_check(SurfelSoA map, unsigned n, const unsigned* __restrict__ counter, unsigned* flag) {
  const unsigned* lane = id_lane(map);
  unsigned bad = 0u;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const unsigned a = lane[(size_t)i * 4], b = i + 1 < n ? lane[(size_t)(i + 1) * 4] : 0u;
    if (b != 0u && (a == 0u || b <= a)) bad |= 1u;
    // the row the numbering starts behind: the last of the prefix, or (an all-zero lane, seen from row 0) none
    if (b == 0u && (a != 0u || i == 0u)) {
      const unsigned long long next = *counter;
      const unsigned long long base = a != 0u ? max(next, a + 1ull) : next;
      const unsigned suffix = a != 0u ? n - 1u - i : n;
      if (base + suffix > 0xFFFFFFFFull) bad |= 2u;
    }
  }
  if (bad) atomicOr(flag, bad);
}

__global__ void k_ids_zero(SurfelSoA map, const unsigned* __restrict__ count_dev) {
  const unsigned n = *count_dev;
  unsigned* lane = id_lane(map);
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) lane[(size_t)i * 4] = 0u;
}

__global__ void k_ids_gather(SurfelSoA map, unsigned n, uint32_t* __restrict__ out) {
  const unsigned* lane = id_lane(map);
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = lane[(size_t)i * 4];
}

// Re-alignment, LABEL_TILE rows per workgroup step: every row looks its ID up in the previous alignment's ID list (wave 0 / wave 1 bound the
// tile's range of that list with 64-way searches, each thread then bisects only inside it), then the tile's rows x C floats are written as one
// flat run: consecutive lanes, consecutive floats of the destination; the source floats are consecutive within every run of surviving rows.
constexpr int LABEL_TILE = 256;
__global__ void __launch_bounds__(LABEL_TILE) k_labels_align(const LabelAlign A) {
  __shared__ unsigned s_src[LABEL_TILE];
  __shared__ unsigned s_lo, s_hi;
  const unsigned n = *A.count_dev, np = *A.n_in;
  const unsigned C = (unsigned)A.C;
  const float invC = 1.0f / (float)C;
  const unsigned* lane = id_lane(A.map);
  for (unsigned r0 = blockIdx.x * LABEL_TILE; r0 < n; r0 += gridDim.x * LABEL_TILE) {
    const unsigned r1 = min(n, r0 + LABEL_TILE), r = r0 + threadIdx.x;
    const unsigned id = r < r1 ? lane[(size_t)r * 4] : 0u;
    if (r < r1) A.ids_out[r] = id;
    const unsigned wave = threadIdx.x >> 6;
    if (wave == 0) {
      const unsigned key = lane[(size_t)r0 * 4];
      const unsigned lo = wave_partition_point(0u, np, [&](unsigned p) { return A.ids_in[p] < key; });
      if (threadIdx.x == 0) s_lo = lo;
    } else if (wave == 1) {
      const unsigned key = lane[(size_t)(r1 - 1) * 4];
      const unsigned hi = wave_partition_point(0u, np, [&](unsigned p) { return A.ids_in[p] <= key; });
      if (threadIdx.x == 64) s_hi = hi;
    }
    __syncthreads();
    unsigned src = LABEL_NONE;
    if (r < r1) {
      unsigned a = s_lo, b = s_hi;
      while (a < b) {
        const unsigned m = a + (b - a) / 2;
        if (A.ids_in[m] < id) a = m + 1; else b = m;
      }
      if (a < s_hi && A.ids_in[a] == id) src = a;
    }
    s_src[threadIdx.x] = src;
    __syncthreads();
    const unsigned nf = (r1 - r0) * C;
    float* dst = A.tab_out + (size_t)r0 * C;
    for (unsigned f = threadIdx.x; f < nf; f += LABEL_TILE) {
      unsigned rr = (unsigned)((float)f * invC);   // f < 2^16: off by at most one
      if (rr * C > f) --rr;
      else if ((rr + 1) * C <= f) ++rr;
      const unsigned s = s_src[rr];
      dst[f] = s == LABEL_NONE ? A.prior : A.tab_in[(size_t)s * C + (f - rr * C)];
    }
    __syncthreads();
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *A.n_out = n;
}

// One observation per surfel (SemanticFusion's projection): the row's pixel is floor of its projected centre, and it is observed when the view's
// index image shows that very row there.  p_c <- p_c o_c / sum_c p_c o_c (ascending c), kept only for a finite positive sum.  No atomics: a row is
// only ever touched by its own lane.
__global__ void __launch_bounds__(BLK) k_labels_fuse(const LabelFuse F) {
  const rt34 T = rt34_load16(F.Tcw);
  const Cam& cam = F.cam;
  const unsigned n = *F.count_dev;
  const size_t P = (size_t)cam.cols * cam.rows;
  for (unsigned s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
    const float4 pc = F.map.pos_conf[s];
    const f3 p = xform(T, f3{pc.x, pc.y, pc.z});
    if (!(p.z > 0.f)) continue;
    const float uf = floorf(((cam.fx * p.x) / p.z) + cam.cx), vf = floorf(((cam.fy * p.y) / p.z) + cam.cy);
    if (!(uf >= 0.f && uf < (float)cam.cols && vf >= 0.f && vf < (float)cam.rows)) continue;
    const size_t pix = (size_t)vf * cam.cols + (size_t)uf;
    if (F.index[pix] != s) continue;
    const float* o = F.probs + pix;
    float* row = F.tab + (size_t)s * F.C;
    float Z = 0.f;
    for (int c = 0; c < F.C; ++c) Z = Z + row[c] * o[(size_t)c * P];
    if (!(Z > 0.f && Z <= 3.402823466e38f)) continue;
    for (int c = 0; c < F.C; ++c) row[c] = (row[c] * o[(size_t)c * P]) / Z;
  }
}

// per pixel of an index image: argmax of the row it shows (ties to the lower class) and that maximum; -1 / 0 where nothing is drawn
__global__ void __launch_bounds__(BLK) k_labels_gather(const uint32_t* __restrict__ index, int P, const float* __restrict__ tab, int C,
                                                       int32_t* __restrict__ label, float* __restrict__ prob) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  const uint32_t s = index[i];
  int best = -1;
  float bp = 0.f;
  if (s != 0xFFFFFFFFu) {
    const float* row = tab + (size_t)s * C;
    best = 0;
    bp = row[0];
    for (int c = 1; c < C; ++c) {
      const float v = row[c];
      if (v > bp) { bp = v; best = c; }
    }
  }
  if (label) label[i] = best;
  if (prob) prob[i] = bp;
}

}  // namespace

void ids_assign(SurfelSoA map, const unsigned* count_dev, unsigned* state, hipStream_t s) {
  hipLaunchKernelGGL(k_ids_assign, dim3(1), dim3(1024), 0, s, map, count_dev, state);
}
void ids_check(SurfelSoA map, unsigned n, const unsigned* counter, unsigned* flag, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_ids_check, dim3(min(ceil_div((int)n, BLK), 4096)), dim3(BLK), 0, s, map, n, counter, flag);
}
void ids_zero(SurfelSoA map, const unsigned* count_dev, unsigned max_rows, hipStream_t s) {
  hipLaunchKernelGGL(k_ids_zero, dim3(max(1, min(ceil_div((int)max_rows, BLK), 4096))), dim3(BLK), 0, s, map, count_dev);
}
void ids_gather(SurfelSoA map, unsigned n, uint32_t* out, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_ids_gather, dim3(min(ceil_div((int)n, BLK), 4096)), dim3(BLK), 0, s, map, n, out);
}
void labels_align(const LabelAlign& a, unsigned max_rows, hipStream_t s) {
  hipLaunchKernelGGL(k_labels_align, dim3(max(1, min(ceil_div((int)max_rows, LABEL_TILE), 8192))), dim3(LABEL_TILE), 0, s, a);
}
void labels_fuse(const LabelFuse& f, unsigned max_rows, hipStream_t s) {
  hipLaunchKernelGGL(k_labels_fuse, dim3(max(1, min(ceil_div((int)max_rows, BLK), 8192))), dim3(BLK), 0, s, f);
}
void labels_gather(const uint32_t* index, int P, const float* tab, int C, int32_t* label, float* prob, hipStream_t s) {
  hipLaunchKernelGGL(k_labels_gather, dim3(ceil_div(P, BLK)), dim3(BLK), 0, s, index, P, tab, C, label, prob);
}
