// Per-pixel noise inputs of a StyleGAN synthesis layer on NHWC fp32 maps (include/bgan.h "noise inputs"): the kernels behind
// layers.NoiseInjection in the generator -- forward (add + LeakyReLU) and the gradient of the one learned strength.  Data is [R, C]:
// R = B * H * W rows (pixels) of C contiguous channels; noise is [R], one value per pixel, broadcast over the channels; strength is
// one float in device memory (a trainable variable: a replayed step program reads its current value).
//
//   forward   y[r, c] = LeakyReLU(x[r, c] + t_r),  t_r = strength[0] * noise[r] rounded to fp32 once, then added (two roundings:
//             the build's -ffp-contract=off).  Pure streaming, no LDS; every element is read once and written once by the same
//             lane, so y may alias x on every route.
//   gradient  dstrength[0] = beta * old + scale * sum_r noise[r] * (sum_c dz[r, c]).  A row's channel sum is each lane's units in
//             index order, then rowwise.h's group_sum butterfly; a lane adds its rows' noise[r] * sum in visit order; a workgroup
//             folds its lanes with reduce.h's block_sum and leaves ONE partial; a second launch of one wave adds the partials in
//             lane_sum_partials' order and ends with a fixed shuffle.  No atomics, two launches, dz read once: two runs give the
//             same bits.
//
// Routes (bg_noise_route reports the ones a C takes): csrc/rowwise.h's, with float4 units only where C % 4 == 0 AND every matrix of
// the call is 16-byte aligned; anything else, a misaligned view included, goes by single floats: no call is refused for its
// alignment.  On the chunked routes (C > 1024, or C > 256 by single floats) a workgroup handles its own chunk of 64 units of a row
// and nothing else: neither kernel needs a statistic of the whole row before it writes, so no row is swept twice.
#include "common.h"
#include "reduce.h"
#include "rowwise.h"

namespace {

using namespace bg::rowwise;

__device__ __forceinline__ float lrelu(float x, float alpha) { return x > 0.f ? x : alpha * x; }

template <int VEC, int NV, bool LOOP>
__global__ __launch_bounds__(kT) void noise_add_kernel(const float* x, const float* __restrict__ noise, const float* __restrict__ strength,
                                                       float* y, Geo g, float alpha) {
  ROWWISE_POS_SETUP();
  (void)Cf;
  const float s = strength[0];
  for (size_t rg = blockIdx.x; rg < groups; rg += gridDim.x) {
    ROWWISE_ROW_SETUP();
    const float t = q.row_ok ? s * noise[q.row] : 0.f;
    const Tile<VEC, NV> v = load_tile<VEC, NV>(x, q, base);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      if (!unit_ok(q, base, j)) continue;
      float o[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) o[e] = lrelu(v.v[j][e] + t, alpha);
      store_unit<VEC>(y, q.unit0 + base + j * q.L + q.sub, o);
    }
  }
}

// part[blockIdx.y * gridDim.x + blockIdx.x] = the workgroup's sum of noise[r] * (its units' sum of dz[r, :])
template <int VEC, int NV, bool LOOP>
__global__ __launch_bounds__(kT) void noise_grad_kernel(const float* __restrict__ dz, const float* __restrict__ noise, float* __restrict__ part,
                                                        Geo g) {
  __shared__ float red[kWaves];
  ROWWISE_POS_SETUP();
  (void)Cf;
  float acc = 0.f;
  for (size_t rg = blockIdx.x; rg < groups; rg += gridDim.x) {
    ROWWISE_ROW_SETUP();
    const Tile<VEC, NV> v = load_tile<VEC, NV>(dz, q, base);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
      for (int e = 0; e < VEC; ++e) s += v.v[j][e];
    s = group_sum(s, q.L);
    if (q.row_ok && q.sub == 0) acc += noise[q.row] * s;
  }
  const float tot = bg::block_sum(acc, red);
  if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = tot;
}

// one wave: out[0] = beta * out[0] + scale * sum of the partials (beta == 0: the old value is not read)
__global__ __launch_bounds__(64) void noise_grad_finish_kernel(const float* __restrict__ part, int nblk, float* out, float beta, float scale) {
  float s = bg::lane_sum_partials(part, nblk, 1, 0, 1, 0);
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (threadIdx.x == 0) {
    float v = scale * s;
    if (beta != 0.f) v += beta * out[0];
    out[0] = v;
  }
}

inline bool al(const void* p) { return bg::aligned16(p); }
inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

inline size_t grad_blocks(int R, const Route& t) {
  const dim3 grid = grid_for(R, t);
  return (size_t)grid.x * grid.y;
}

}  // namespace

extern "C" {

int bg_noise_route(int C, int* out) {
  BG_REQUIRE(out, BG_ERR_NULL, "bg_noise_route: null pointer");
  BG_REQUIRE(C > 0, BG_ERR_BAD_SHAPE, "bg_noise_route: C=%d", C);
  for (int k = 0; k < 2; ++k) {
    const Route t = route_for(C, k == 0);
    out[4 * k + 0] = t.vec;
    out[4 * k + 1] = 1 << t.lg;
    out[4 * k + 2] = t.nv;
    out[4 * k + 3] = t.chunks;
  }
  return BG_OK;
}

int bg_noise_add_f32(const float* x, const float* noise, const float* strength, float* y, int R, int C, float lrelu_alpha, void* stream) {
  BG_REQUIRE(x && noise && strength && y, BG_ERR_NULL, "bg_noise_add_f32: null pointer");
  BG_REQUIRE(R > 0 && C > 0, BG_ERR_BAD_SHAPE, "bg_noise_add_f32: R=%d C=%d", R, C);
  BG_REQUIRE(al4(x) && al4(noise) && al4(strength) && al4(y), BG_ERR_BAD_ALIGNMENT, "bg_noise_add_f32: pointers must be 4-byte aligned");
  const Route t = route_for(C, al(x) && al(y));
  bg::Launch L(stream, "noise_add", 0, 8.0 * R * C + 4.0 * R);
  const dim3 grid = grid_for(R, t);
  for_route(t, [&](auto lanes) {
    using Rt = decltype(lanes);
    bg::launch(noise_add_kernel<Rt::VEC, Rt::NV, Rt::LOOP>, grid, dim3(kT), 0, L.s, x, noise, strength, y, geo_for(R, C, t), lrelu_alpha);
  });
  return L.done("noise_add_kernel");
}

size_t bg_noise_grad_workspace_bytes(int R, int C) {
  if (R <= 0 || C <= 0) return 0;
  return sizeof(float) * std::max(grad_blocks(R, route_for(C, true)), grad_blocks(R, route_for(C, false)));
}

int bg_noise_grad_f32(const float* dz, const float* noise, float* dstrength, int R, int C, void* ws, float beta, float scale, void* stream) {
  BG_REQUIRE(dz && noise && dstrength && ws, BG_ERR_NULL, "bg_noise_grad_f32: null pointer");
  BG_REQUIRE(R > 0 && C > 0, BG_ERR_BAD_SHAPE, "bg_noise_grad_f32: R=%d C=%d", R, C);
  BG_REQUIRE(al4(dz) && al4(noise) && al4(dstrength) && al4(ws), BG_ERR_BAD_ALIGNMENT, "bg_noise_grad_f32: pointers must be 4-byte aligned");
  const Route t = route_for(C, al(dz));
  const dim3 grid = grid_for(R, t);
  float* part = static_cast<float*>(ws);
  {
    bg::Launch L(stream, "noise_grad", 0, 4.0 * R * C + 4.0 * R);
    for_route(t, [&](auto lanes) {
      using Rt = decltype(lanes);
      bg::launch(noise_grad_kernel<Rt::VEC, Rt::NV, Rt::LOOP>, grid, dim3(kT), 0, L.s, dz, noise, part, geo_for(R, C, t));
    });
    const int rc = L.done("noise_grad_kernel");
    if (rc != BG_OK) return rc;
  }
  bg::Launch L(stream, "noise_grad_finish", 0, 4.0 * grid.x * grid.y);
  bg::launch(noise_grad_finish_kernel, dim3(1), dim3(64), 0, L.s, (const float*)part, (int)(grid.x * grid.y), dstrength, beta, scale);
  return L.done("noise_grad_finish_kernel");
}

}  // extern "C"
