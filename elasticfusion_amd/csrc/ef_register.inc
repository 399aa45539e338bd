// Point-to-plane registration of a point set against the map: one step = transform, nearest-surfel search and the sums of the normal
// equations in one launch (ef_register_step / ef_register_cloud, include/ef_hip.h; DESIGN.md §8c).  Included at the end of
// ef_map_kernels.hip, after ef_query.inc, whose index and cell walk (query_walk) it uses.  No frame kernel reads or writes anything here.
//   k_register          16 lanes share a point (the query's measured choice).  After the group's butterfly every lane holds the winner, so the
//                       29 quantities of a pair (21 upper-triangle entries of J^T J, 6 of -J^T r, r^2, 1) are dealt out over the group: lane l
//                       owns slots l and l + 16 and adds one exact double product per slot and point.  A group takes points group,
//                       group + groups, ... ; at the end the four groups of a wave are added (two xor steps), the four waves of a workgroup
//                       through LDS in wave order, and the workgroup writes one slab of REGISTER_SLOTS doubles.
//   k_register_reduce   one workgroup adds the slabs in a fixed order.
// No floating-point atomics anywhere: which point goes to which lane, and every order of addition, is a function of n alone, so the sums of a
// step are the same bits on every run and for every cell size of the index.
namespace {

// what slot s multiplies: codes 0 .. 5 = J[code], 6 = r, 7 = -r, 8 = 1, 9 = 0
__device__ __forceinline__ void register_slot(int s, int& a, int& b) {
  a = 9;
  b = 9;
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = i; j < 6; ++j) {
      if (k == s) { a = i; b = j; }
      ++k;
    }
  }
  if (s >= 21 && s < 27) { a = s - 21; b = 7; }   // b -= J r
  if (s == 27) { a = 6; b = 6; }                  // e += r r
  if (s == 28) { a = 8; b = 8; }                  // pairs += 1
}
__device__ __forceinline__ float register_pick(int code, const float (&J)[6], float r) {
  float v = 0.f;
  v = code == 0 ? J[0] : v;
  v = code == 1 ? J[1] : v;
  v = code == 2 ? J[2] : v;
  v = code == 3 ? J[3] : v;
  v = code == 4 ? J[4] : v;
  v = code == 5 ? J[5] : v;
  v = code == 6 ? r : v;
  v = code == 7 ? -r : v;
  v = code == 8 ? 1.0f : v;
  return v;
}

template <int L>
__global__ void __launch_bounds__(BLK) k_register(const RegisterArgs A) {
  static_assert(2 * L == REGISTER_SLOTS && 64 % L == 0, "a group of L lanes owns the slots l and l + L");
  __shared__ double lds[BLK / 64][REGISTER_SLOTS];
  const unsigned sub = threadIdx.x % L;
  const unsigned long long group = ((unsigned long long)blockIdx.x * BLK + threadIdx.x) / L, groups = (unsigned long long)gridDim.x * (BLK / L);
  int a0, b0, a1, b1;
  register_slot((int)sub, a0, b0);
  register_slot((int)sub + L, a1, b1);
  double acc0 = 0.0, acc1 = 0.0;
  for (unsigned long long base = 0; base < A.q.n; base += groups) {   // the same trip count for every lane: all of a wave take part in the shuffles
    const unsigned long long qi = base + group;
    const bool live = qi < A.q.n;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (live) {
      const float x = A.q.points[qi * 3], y = A.q.points[qi * 3 + 1], z = A.q.points[qi * 3 + 2];
      qx = ((A.R[0] * x + A.R[1] * y) + A.R[2] * z) + A.t[0];
      qy = ((A.R[3] * x + A.R[4] * y) + A.R[5] * z) + A.t[1];
      qz = ((A.R[6] * x + A.R[7] * y) + A.R[8] * z) + A.t[2];
    }
    float bd[1] = {__builtin_inff()};
    unsigned br[1] = {QUERY_NONE};
    unsigned cnt = 0;
    if (live) query_walk<L, 1>(A.q, qx, qy, qz, sub, bd, br, cnt);
    float d = bd[0];
    unsigned r = br[0];
#pragma unroll
    for (int m = 1; m < L; m <<= 1) {
      const float od = __shfl_xor(d, m, L);
      const unsigned orow = __shfl_xor(r, m, L);
      if (query_less(od, orow, d, r)) { d = od; r = orow; }
    }
    // every lane of the group now holds the winner and evaluates the pair (the same loads, served once per group)
    bool hit = r != QUERY_NONE;
    float J[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float res = 0.f;
    if (hit) {
      const float4 p = A.q.map.pos_conf[r], nr = A.q.map.nrm_rad[r];
      if (A.gate) {
        const float mx = A.normals[qi * 3], my = A.normals[qi * 3 + 1], mz = A.normals[qi * 3 + 2];
        const float tx = (A.R[0] * mx + A.R[1] * my) + A.R[2] * mz;
        const float ty = (A.R[3] * mx + A.R[4] * my) + A.R[5] * mz;
        const float tz = (A.R[6] * mx + A.R[7] * my) + A.R[8] * mz;
        hit = ((tx * nr.x + ty * nr.y) + tz * nr.z) >= A.min_normal_cos;   // NaN: dropped
      }
      if (hit) {
        res = (((qx - p.x) * nr.x + (qy - p.y) * nr.y) + (qz - p.z) * nr.z);
        J[0] = nr.x;
        J[1] = nr.y;
        J[2] = nr.z;
        J[3] = qy * nr.z - qz * nr.y;
        J[4] = qz * nr.x - qx * nr.z;
        J[5] = qx * nr.y - qy * nr.x;
      }
    }
    if (live && sub == 0) {
      if (A.q.row) A.q.row[qi] = hit ? r : QUERY_NONE;
      if (A.q.plane) A.q.plane[qi] = res;
    }
    if (hit) {   // the product of two widened f32 values is exact in double
      acc0 += (double)register_pick(a0, J, res) * (double)register_pick(b0, J, res);
      acc1 += (double)register_pick(a1, J, res) * (double)register_pick(b1, J, res);
    }
  }
  // the wave's groups (a + b = b + a: both partners of a step hold the same bits), then the workgroup's waves in wave order
#pragma unroll
  for (int m = L; m < 64; m <<= 1) {
    acc0 += __shfl_xor(acc0, m, 64);
    acc1 += __shfl_xor(acc1, m, 64);
  }
  const unsigned wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  if (lane < L) {
    lds[wave][lane] = acc0;
    lds[wave][lane + L] = acc1;
  }
  __syncthreads();
  if (threadIdx.x < REGISTER_SLOTS) {
    double s = lds[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < BLK / 64; ++w) s += lds[w][threadIdx.x];
    A.slabs[(size_t)blockIdx.x * REGISTER_SLOTS + threadIdx.x] = s;
  }
}

// thread t adds the slabs t / 32, t / 32 + 8, ... of slot t % 32 in ascending order; the eight partial sums are then added in ascending order
__global__ void __launch_bounds__(BLK) k_register_reduce(const double* __restrict__ slabs, unsigned nb, double* __restrict__ sums) {
  constexpr int PARTS = BLK / REGISTER_SLOTS;
  __shared__ double lds[PARTS][REGISTER_SLOTS];
  const unsigned slot = threadIdx.x % REGISTER_SLOTS, part = threadIdx.x / REGISTER_SLOTS;
  double s = 0.0;
  for (unsigned b = part; b < nb; b += PARTS) s += slabs[(size_t)b * REGISTER_SLOTS + slot];
  lds[part][slot] = s;
  __syncthreads();
  if (threadIdx.x < REGISTER_SLOTS) {
    double v = lds[0][threadIdx.x];
#pragma unroll
    for (int p = 1; p < PARTS; ++p) v += lds[p][threadIdx.x];
    sums[threadIdx.x] = v;
  }
}

}  // namespace

unsigned register_blocks(unsigned n) {
  const unsigned per = BLK / 16;
  const unsigned long long want = ((unsigned long long)n + per - 1) / per;
  return (unsigned)(want < (unsigned long long)REGISTER_MAX_BLOCKS ? want : (unsigned long long)REGISTER_MAX_BLOCKS);
}

// n = 0: no slab, the reduction writes zeros
void register_step(const RegisterArgs& a, hipStream_t s) {
  const unsigned nb = register_blocks(a.q.n);
  if (nb) hipLaunchKernelGGL((k_register<16>), dim3(nb), dim3(BLK), 0, s, a);
  hipLaunchKernelGGL(k_register_reduce, dim3(1), dim3(BLK), 0, s, (const double*)a.slabs, nb, a.sums);
}
