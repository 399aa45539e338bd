// GlobalModel::renderPointCloud (GlobalModel.cpp:286-350, draw_global_surface.{vert,geom,frag}) restated headless: the live map drawn from any
// pinhole camera and pose into plain images (ef_render_model, include/ef_hip.h).  Included at the end of ef_map_kernels.hip, beside the surface
// splat whose geometry it reuses unchanged (make_sprite / pixel_ray / sprite_fragment_ray: the footprint, the ray / disc intersection, the N3
// clamp, no sprite whose centre leaves the image).  What differs from the frame's prediction, and why these are kernels of their own
// (DESIGN.md §8):
//   selection   conf > threshold || drawUnstable (draw_global_surface.vert:44), and 0 <= z <= maxDepth; no time-window cull
//   depth test  key zkey(z, id) for a stable surfel, zkey(fl32(z + radius), id) for an unstable one: the reference pushes unstable fragments back
//               by their radius (draw_global_surface.frag:35-41) in GL window depth, which a renderer without a projection matrix does not have;
//               the same intent in camera metres.  The depth / vertex outputs carry the real intersection z.
//   shading     draw_global_surface.geom:49-79 per surfel, in f32
namespace {

// make_sprite with every prediction-only cull neutral: conf >= -inf, no time window (a colour / time stream of zeros: 0 - 0 > inf is false)
__device__ __forceinline__ Sprite render_sprite(const Cam& cam, const rt34& T, float4 pc, float4 nr, float maxDepth) {
  return make_sprite(cam, T, pc, make_float4(0.f, 0.f, 0.f, 0.f), nr, maxDepth, -INFINITY, 0.f, INFINITY, INFINITY);
}
// roundf(clamp(c, 0, 1) * 255), NaN -> 0
__device__ __forceinline__ uint8_t render_u8(float c) {
  if (!(c >= 0.f)) return 0;
  return (uint8_t)roundf(fminf(c, 1.f) * 255.0f);
}
// draw_global_surface.geom:49-79: n is the stored world normal (not renormalised), s = |dot(n, (1, 1, 1))|.  GLSL leaves max() of a NaN open;
// this is fmaxf's (the other operand): drawTimes at time 1 divides by zero.
__device__ __forceinline__ uchar4 render_shade(const RenderArgs& a, float4 ct, float4 nr) {
  const float s = fabsf((nr.x + nr.y) + nr.z);
  f3 c;
  if (a.colorType == 1) {
    c = f3{nr.x, nr.y, nr.z};
  } else if (a.colorType == 2) {
    c = decodeColor(ct.x);
  } else if (a.colorType == 3) {
    const float ratio = 2.0f * (ct.z - 1.0f) / ((float)a.time - 1.0f);
    const float r = fmaxf(0.f, 1.0f - ratio), g = fmaxf(0.f, ratio - 1.0f);
    const float m = s + 0.1f;
    c = f3{r * m, g * m, ((1.0f - r) - g) * m};
  } else {
    const float l = 0.5f * s + 0.1f;
    c = f3{l, l, l};
  }
  if (a.drawWindow && (float)a.time - ct.w > (float)a.timeDelta) c = f3{c.x * 0.25f, c.y * 0.25f, c.z * 0.25f};
  return make_uchar4(render_u8(c.x), render_u8(c.y), render_u8(c.z), 255);
}

// k_surface_splat's loop (SPLAT_LANES lanes per surfel, column-major z-buffer, one global 64-bit atomicMin per fragment) with the render's
// selection and depth key.  Without UNSTABLE a surfel's confidence decides before its normal stream is loaded; the colour stream is never read.
template <bool UNSTABLE>
__global__ void __launch_bounds__(BLK) k_render_splat(const RenderArgs a, SurfelSoA map, const unsigned* __restrict__ count_dev,
                                                       unsigned long long* zbuf) {
  const rt34 T = rt34_load16(a.Tcw);
  const Cam& cam = a.cam;
  const unsigned count = *count_dev;
  const unsigned sub = threadIdx.x % SPLAT_LANES;
  const unsigned stride = gridDim.x * blockDim.x / SPLAT_LANES;
  for (unsigned id = (blockIdx.x * blockDim.x + threadIdx.x) / SPLAT_LANES; id < count; id += stride) {
    const float4 pc = map.pos_conf[id];
    const bool stable = pc.w > a.threshold;
    if (!UNSTABLE && !stable) continue;
    const float4 nr = map.nrm_rad[id];
    const Sprite S = render_sprite(cam, T, pc, nr, a.maxDepth);
    if (!S.ok) continue;
    const int px0 = max(0, (int)ceilf(S.u - S.hs - 0.5f)), px1 = min(cam.cols - 1, (int)ceilf(S.u + S.hs - 0.5f) - 1);
    const int py0 = max(0, (int)ceilf(S.v - S.hs - 0.5f)), py1 = min(cam.rows - 1, (int)ceilf(S.v + S.hs - 0.5f) - 1);
    const int hgt = py1 - py0 + 1, nfrag = (px1 - px0 + 1) * hgt;
    const float psn = dot(S.p, S.n);
    for (int f = (int)sub; f < nfrag; f += SPLAT_LANES) {
      const int fx = f / hgt, py = py0 + (f - fx * hgt), px = px0 + fx;
      float z;
      if (!sprite_fragment_ray(S.p, S.n, S.rad, psn, pixel_ray(cam, px, py), z)) continue;
      if (z != z) continue;
      atomicMin(&zbuf[px * cam.rows + py], zkey(stable ? z : z + S.rad, id));
    }
  }
}

// k_surface_resolve's walk (16 x 16 pixel tiles, a wavefront on an 8 x 8 block going down the columns): z re-derived from the winning surfel with
// the splat's operations, only the requested outputs written, the z-buffer returned to ZBUF_EMPTY
__global__ void __launch_bounds__(BLK) k_render_resolve(const RenderArgs a, SurfelSoA map, unsigned long long* zbuf, RenderOut out) {
  const Cam& cam = a.cam;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int px = blockIdx.x * 16 + (wave & 1) * 8 + (lane >> 3), py = blockIdx.y * 16 + (wave >> 1) * 8 + (lane & 7);
  if (px >= cam.cols || py >= cam.rows) return;
  const size_t pi = (size_t)py * cam.cols + px, zi = (size_t)px * cam.rows + py;
  const unsigned long long key = zbuf[zi];
  uchar4 im = make_uchar4(0, 0, 0, 0);
  float4 vt = make_float4(0, 0, 0, 0), nm = make_float4(0, 0, 0, 0);
  uint32_t idx = 0xFFFFFFFFu;
  if (key != ZBUF_EMPTY) {
    zbuf[zi] = ZBUF_EMPTY;
    idx = (uint32_t)key;
    const rt34 T = rt34_load16(a.Tcw);
    const float4 pc = map.pos_conf[idx], nr = map.nrm_rad[idx];
    const Sprite S = render_sprite(cam, T, pc, nr, a.maxDepth);
    float z = 0.f;
    sprite_fragment(cam, S, px, py, z);  // same operations as the splat => same bits
    const float fcx = (float)px + 0.5f, fcy = (float)py + 0.5f;
    vt = make_float4((fcx - cam.cx) * z * (1.f / cam.fx), (fcy - cam.cy) * z * (1.f / cam.fy), z, pc.w);
    nm = make_float4(S.n.x, S.n.y, S.n.z, nr.w);
    if (out.rgba) im = render_shade(a, map.col_time[idx], nr);
  }
  if (out.rgba) out.rgba[pi] = im;
  if (out.depth) out.depth[pi] = vt.z;
  if (out.vertex) out.vertex[pi] = vt;
  if (out.normal) out.normal[pi] = nm;
  if (out.index) out.index[pi] = idx;
}

}  // namespace

void render_model(const RenderArgs& a, SurfelSoA map, const unsigned* count_dev, unsigned long long* zbuf, RenderOut out, hipStream_t s) {
  if (a.drawUnstable)
    hipLaunchKernelGGL(k_render_splat<true>, dim3(SPLAT_GRID), dim3(BLK), 0, s, a, map, count_dev, zbuf);
  else
    hipLaunchKernelGGL(k_render_splat<false>, dim3(SPLAT_GRID), dim3(BLK), 0, s, a, map, count_dev, zbuf);
  hipLaunchKernelGGL(k_render_resolve, dim3(ceil_div(a.cam.cols, 16), ceil_div(a.cam.rows, 16)), dim3(BLK), 0, s, a, map, zbuf, out);
}
