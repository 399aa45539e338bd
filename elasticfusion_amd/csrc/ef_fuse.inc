// Fuse surfels into the map (ef_map_fuse, include/ef_hip.h; DESIGN.md §8g).  Included at the end of ef_map_kernels.hip, after ef_insert.inc, whose
// gate (k_insert_gate: the match), transform (insert_move_pos / insert_move_nrm) and scatter (the append) it uses unchanged; the selection's
// flags_count (ef_select.inc: k_select_count + k_scan_chunks) counts the outcome bytes.  No frame kernel reads or writes anything here.
//   pick      k_fuse_pick: one lane per record.  A matched record whose confidence competes forms the query's d2 against the stored position of
//             its row and takes part in the election: atomicMin on key[row] of (d2 bits << 32) | record index, the z-buffer's idiom.  d2 is
//             finite and non-negative, so its bits order as the floats do; the minimum of a set does not depend on the order of the atomics.
//   outcome   k_fuse_outcome: one lane per record, one byte each.  The competitor that finds its own index in the low word of key[row] is FUSED.
//             Nothing of the map is written: the host reads the counts back (and can still refuse the call) before a row changes.
//   apply     k_fuse_apply: one lane per record; the FUSED record is the only writer of its row: three 16-byte words of the row and of the
//             record in, update.vert's weighted average (merge_surfel's arithmetic, header point 3), two or three words out.
// The pick reads pos_conf of rows the apply of the same call writes, and the outcome needs every pick finished: three launches.
// Every kernel is a single bounded pass, nothing waits for another workgroup, the election is the one atomic (an integer one), and every index
// written is bounded by the old count (key, the rows) or by n (outcome).
namespace {

__device__ __forceinline__ bool fuse_competes(float a) { return a > 0.0f && a < __builtin_inff(); }   // (NaN: neither comparison holds)

__global__ void __launch_bounds__(BLK) k_fuse_pick(const MapFuseArgs A) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.ins.n || !A.ins.dup[i]) return;
  const unsigned s = A.ins.match_row[i];
  if (s >= A.ins.count_before) return;   // (a duplicate's row is a row of the old map; the bound keeps a broken gate from writing outside key[])
  const float4 u = A.ins.rec[(size_t)i * 3];
  if (!fuse_competes(u.w)) return;
  const float4 p = insert_move_pos(A.ins, u), ps = A.ins.q.map.pos_conf[s];
  const float dx = p.x - ps.x, dy = p.y - ps.y, dz = p.z - ps.z;
  const float d2 = ((dx * dx + dy * dy) + dz * dz);   // the query's expression on the query's inputs: the d2 that made s the match
  atomicMin(&A.key[s], ((unsigned long long)__float_as_uint(d2) << 32) | i);
}

__global__ void __launch_bounds__(BLK) k_fuse_outcome(const MapFuseArgs A) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.ins.n) return;
  unsigned o;
  if (A.ins.dup[i]) {
    const unsigned s = A.ins.match_row[i];
    if (s >= A.ins.count_before || !fuse_competes(A.ins.rec[(size_t)i * 3].w)) o = FUSE_WEIGHTLESS;
    else o = (unsigned)A.key[s] == i ? FUSE_FUSED : FUSE_ABSORBED;
  } else {
    o = A.ins.flags[i] ? (A.append ? FUSE_INSERTED : FUSE_NOVEL) : FUSE_SKIPPED;
  }
  A.outcome[i] = (uint8_t)o;
}

__global__ void __launch_bounds__(BLK) k_fuse_apply(const MapFuseArgs A) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.ins.n || A.outcome[i] != FUSE_FUSED) return;
  const unsigned id = A.ins.match_row[i];
  const SurfelSoA& map = A.ins.q.map;
  const float4 ucol = A.ins.rec[(size_t)i * 3 + 1];
  const float4 u = insert_move_pos(A.ins, A.ins.rec[(size_t)i * 3]), un = insert_move_nrm(A.ins, A.ins.rec[(size_t)i * 3 + 2]);
  float4 s = map.pos_conf[id], sc = map.col_time[id];
  // merge_surfel, with the record in the candidate's place (and the normalisation's dot product written out: no multiply-add in any build)
  const float c_k = s.w, a = u.w, ftime = A.ins.last_time != INSERT_KEEP ? (float)A.ins.last_time : ucol.w;
  float4 sn = map.nrm_rad[id];
  if (un.w < (1.0f + 0.5f) * sn.w) {
    s.x = ((c_k * s.x) + (a * u.x)) / (c_k + a);
    s.y = ((c_k * s.y) + (a * u.y)) / (c_k + a);
    s.z = ((c_k * s.z) + (a * u.z)) / (c_k + a);
    s.w = c_k + a;
    const f3 oldCol = decodeColor(sc.x), newCol = decodeColor(ucol.x);
    const f3 avg{((c_k * oldCol.x) + (a * newCol.x)) / (c_k + a), ((c_k * oldCol.y) + (a * newCol.y)) / (c_k + a),
                 ((c_k * oldCol.z) + (a * newCol.z)) / (c_k + a)};
    sc.x = encodeColorMerged(avg);
    sc.w = ftime;
    const float nx = ((c_k * sn.x) + (a * un.x)) / (c_k + a), ny = ((c_k * sn.y) + (a * un.y)) / (c_k + a),
                nz = ((c_k * sn.z) + (a * un.z)) / (c_k + a), nw = ((c_k * sn.w) + (a * un.w)) / (c_k + a);
    const float rn = 1.0f / sqrtf((nz * nz) + ((ny * ny) + (nx * nx)));
    map.pos_conf[id] = s;
    map.col_time[id] = sc;
    map.nrm_rad[id] = make_float4(nx * rn, ny * rn, nz * rn, nw);
  } else {
    s.w = c_k + a;
    sc.w = ftime;
    map.pos_conf[id] = s;
    map.col_time[id] = sc;
  }
}

}  // namespace

void fuse_pick(const MapFuseArgs& a, hipStream_t s) {
  if (a.ins.n) hipLaunchKernelGGL(k_fuse_pick, dim3((a.ins.n + BLK - 1) / BLK), dim3(BLK), 0, s, a);
}
void fuse_outcome(const MapFuseArgs& a, hipStream_t s) {
  if (a.ins.n) hipLaunchKernelGGL(k_fuse_outcome, dim3((a.ins.n + BLK - 1) / BLK), dim3(BLK), 0, s, a);
}
void fuse_apply(const MapFuseArgs& a, hipStream_t s) {
  if (a.ins.n) hipLaunchKernelGGL(k_fuse_apply, dim3((a.ins.n + BLK - 1) / BLK), dim3(BLK), 0, s, a);
}
