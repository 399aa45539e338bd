// The depth pre-processing of a frame (G1 + G2: bilateral filter, both metric conversions; round 6: + the frame's level-0 intensity image) as a
// device function of one workgroup tile — included by ef_map_kernels.hip (k_preprocess: the operator tier and the frames that are not tracked) and
// by ef_track_kernels.hip (k_frame_inputs: the tracked frames' launch, which carries the model maps too).  Included inside a namespace.
__device__ __forceinline__ float metric_px(unsigned value, unsigned maxv) {
  return (value > maxv || value < 300U) ? 0.0f : (float)value / 1000.0f;
}
// Bilateral filter, the fast path (round 5: the weights come from a table).  The arithmetic of bilateral_px is kept operation for
// operation (the filtered depth must be the oracle's, bit for bit); what changes is how it is fed and issued:
//   * the weight of a tap, ef_expf(-(S + d * d * c)), depends on two small integers only: its squared distance dx^2 + dy^2 (27 distinct
//     values in the 13 x 13 window) and |d| = |value - tmp| (depths are integers; beyond |d| = 395 the argument is below -87 and the weight is
//     exactly +0 for every S).  A 27 x 400 table of these weights, each entry evaluated ONCE with the very expression of bilateral_px
//     (k_bilateral_table: bit-identical by construction; rounds 1-4 evaluated 169 polynomial exps per pixel, 43 us of ALU), lives in HBM per
//     device (43 KB) and is copied into LDS by every workgroup; a tap is then a subtraction, a clamp, a conversion and an LDS look-up;
//   * the 76 x 20 neighbourhood of a 64 x 8 pixel tile is staged once in LDS as float (169 global loads per pixel -> 1);
//   * every lane filters TWO pixels (rows y and y + 4); both loops fully unrolled, so the table row of a tap is an immediate offset;
//   * taps outside the image read a sentinel far away from every depth: their |d| clamps to a zero column of the table, and
//     x + sentinel * 0 == x exactly, so the two sums see the same sequence of non-trivial additions in the same order as the clipped
//     loops of depth_bilateral.frag:49-72.
typedef float float2v __attribute__((ext_vector_type(2)));
// Round 6: a lane's two pixels are horizontal NEIGHBOURS (x = 2 lane, 2 lane + 1): the two tile values of a tap are adjacent in LDS — one
// 8-byte read straight into the register pair the packed arithmetic wants (four rows apart they arrived in two registers of two different
// reads and were paired with a v_mov each: 315 of the kernel's 2 300 VALU instructions) — and the outputs of a lane are adjacent too.
constexpr int PRE_TW = 128, PRE_TH = 4, PRE_R = 6, PRE_LW = PRE_TW + 2 * PRE_R + 4 /* rows of 576 bytes: 16-byte aligned */, PRE_LH = PRE_TH + 2 * PRE_R;
constexpr int BIL_ROWS = 27, BIL_COLS = 400, BIL_ZERO = 396;   // columns >= BIL_ZERO hold +0 (|d| >= 396: 396^2 * 0.000555556 > 87)
constexpr float BIL_OUTSIDE = 1.0e6f;                            // sentinel of a tap outside the image
struct BilRows {   // (|dy|, |dx|) -> first float of the table row of dx^2 + dy^2
  int distinct[BIL_ROWS];
  int base[PRE_R + 1][PRE_R + 1];
  constexpr BilRows() : distinct{}, base{} {
    int n = 0;
    for (int s2 = 0; s2 <= 2 * PRE_R * PRE_R; ++s2) {
      bool hit = false;
      for (int a = 0; a <= PRE_R; ++a)
        for (int b = 0; b <= PRE_R; ++b)
          if (a * a + b * b == s2) { hit = true; base[a][b] = n * BIL_COLS; }
      if (hit) distinct[n++] = s2;
    }
  }
};
constexpr BilRows BIL{};
static_assert(BIL.distinct[BIL_ROWS - 1] == 2 * PRE_R * PRE_R && BIL.base[PRE_R][PRE_R] == (BIL_ROWS - 1) * BIL_COLS, "27 distinct squared distances");
// One tile of the filter (a 256-thread workgroup: dim3(64, 4)); bx, by: the tile's position in the grid of ceil(cols / PRE_TW) x ceil(rows / PRE_TH)
// tiles.  A device function, so that the frame script can run it inside a launch that also carries other work (k_frame_inputs,
// ef_track_kernels.hip) as well as a launch of its own (k_preprocess).
template <bool WITH_METRIC>
__device__ __forceinline__ void preprocess_tile(int bx, int by, const uint16_t* __restrict__ raw, int cols, int rows, unsigned maxv,
                                                const float* __restrict__ table, uint16_t* __restrict__ filtered, float* __restrict__ metric,
                                                float* __restrict__ metric_filtered, const uint8_t* __restrict__ rgb3, uint8_t* __restrict__ next0,
                                                uint8_t* __restrict__ rgb_keep) {
  __shared__ __attribute__((aligned(16))) float tab[BIL_ROWS * BIL_COLS];
  __shared__ float tile[PRE_LH][PRE_LW];
  const int x0 = bx * PRE_TW, y0 = by * PRE_TH;
  const int tx = threadIdx.x, ty = threadIdx.y, t = ty * 64 + tx;
  {
    const float4* src = (const float4*)table;
    float4* dst = (float4*)tab;
#pragma unroll
    for (int i = 0; i < (BIL_ROWS * BIL_COLS / 4 + 255) / 256; ++i) {
      const int q = t + i * 256;
      if (q < BIL_ROWS * BIL_COLS / 4) dst[q] = src[q];
    }
  }
  constexpr int LWU = PRE_TW + 2 * PRE_R;   // columns of the tile that are filled
  for (int i = t; i < PRE_LH * LWU; i += 256) {
    const int ly = i / LWU, lx = i - ly * LWU;
    const int gx = x0 + lx - PRE_R, gy = y0 + ly - PRE_R;
    // (4 x the depth: |4 value - 4 tmp|, clamped, IS the byte offset of the tap's weight in its table row — no shift per look-up; exact: depths are
    // integers below 2^16)
    tile[ly][lx] = 4.0f * ((gx >= 0 && gx < cols && gy >= 0 && gy < rows) ? (float)raw[gy * cols + gx] : BIL_OUTSIDE);
  }
  __syncthreads();
  const int xa = x0 + 2 * tx, xb = xa + 1, y = y0 + ty;
  if (xa >= cols || y >= rows) return;
  const bool in_a = true, in_b = xb < cols;
  if (rgb3) {   // the frame's level-0 intensity image and the context's copy of the colours ride along (see above)
    const int xs[2] = {xa, xb};
    const bool ins[2] = {in_a, in_b};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if (!ins[q]) continue;
      const size_t i = (size_t)y * cols + xs[q];
      const uint8_t r = rgb3[i * 3], g = rgb3[i * 3 + 1], b = rgb3[i * 3 + 2];
      next0[i] = intensity_of((float)r, (float)g, (float)b);
      if (rgb_keep) { rgb_keep[i * 3] = r; rgb_keep[i * 3 + 1] = g; rgb_keep[i * 3 + 2] = b; }
    }
  }
  const float2v value4 = {tile[ty + PRE_R][2 * tx + PRE_R], tile[ty + PRE_R][2 * tx + 1 + PRE_R]};
  const float2v value = value4 * 0.25f;
  const unsigned va = (unsigned)value.x, vb = in_b ? (unsigned)value.y : 0u;
  const bool gate_a = !(va > maxv || va < 300U), gate_b = in_b && !(vb > maxv || vb < 300U);
  float2v sum1 = (float2v)(0.0f), sum2 = (float2v)(0.0f);
  if (gate_a || gate_b) {
#pragma unroll
    for (int dy = -PRE_R; dy <= PRE_R; ++dy) {
#pragma unroll
      for (int dx = -PRE_R; dx <= PRE_R; ++dx) {
        const float* row = tab + BIL.base[dy < 0 ? -dy : dy][dx < 0 ? -dx : dx];   // (an immediate once both loops are unrolled)
        const float2v tmp4 = {tile[ty + PRE_R + dy][2 * tx + PRE_R + dx], tile[ty + PRE_R + dy][2 * tx + 1 + PRE_R + dx]};
        const float2v d4 = value4 - tmp4;   // 4 (value - tmp), exactly
        const int ia = (int)fminf(fabsf(d4.x), 4.0f * BIL_ZERO), ib = (int)fminf(fabsf(d4.y), 4.0f * BIL_ZERO);   // byte offsets
        const float2v w = {*(const float*)((const char*)row + ia), *(const float*)((const char*)row + ib)};
        // sum1 is carried as 4 x the shader's sum: (4 tmp) * w and the additions of such products are 4 x the unscaled ones BIT FOR BIT (a power of
        // two commutes with rounding while nothing is subnormal or overflows: 300 <= tmp < 2^16, w = 0 or >= e^-87 > FLT_MIN, every term >= 0),
        // so one multiplication by 0.25 behind the loop replaces 169 inside it
        sum1 = sum1 + tmp4 * w;
        sum2 = sum2 + w;
      }
    }
  }
  sum1 = sum1 * 0.25f;
  {
    const uint16_t f = gate_a ? (uint16_t)(unsigned)roundf(sum1.x / sum2.x) : (uint16_t)0;
    filtered[y * cols + xa] = f;
    if (WITH_METRIC) { metric[y * cols + xa] = metric_px(va, maxv); metric_filtered[y * cols + xa] = metric_px(f, maxv); }
  }
  if (in_b) {
    const uint16_t f = gate_b ? (uint16_t)(unsigned)roundf(sum1.y / sum2.y) : (uint16_t)0;
    filtered[y * cols + xb] = f;
    if (WITH_METRIC) { metric[y * cols + xb] = metric_px(vb, maxv); metric_filtered[y * cols + xb] = metric_px(f, maxv); }
  }
}
