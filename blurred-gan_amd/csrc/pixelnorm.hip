// Pixel normalisation over the channel axis of NHWC fp32 maps and of latent vectors (include/bgan.h "pixel normalisation"): the
// kernels behind layers.PixelNormalization in the generator -- forward (LeakyReLU + PixelNorm) and backward (through both).  Data is
// [R, C]: R rows of C contiguous channels; the one statistic is a mean over ONE row, so rows are independent and the kernels are
// pure streaming.  No parameters, no column sums, no workspace, no LDS, no atomics: two runs give the same bits.
//
// Per row, with the mean over the row's C channels:  a = LeakyReLU(x),  r = 1 / sqrt(mean(a^2) + eps)  (saved by the forward where
// a backward follows),  y = a * r;  the Jacobian of a -> y is r * (I - y y^T / C), and r > 0 gives sign(y) = sign(x): the backward
// reads LeakyReLU's branch from the stored output and never sees x.
//
// Routes (bg_pixelnorm_route reports the ones a C takes): csrc/rowwise.h's, with float4 units only where C % 4 == 0 AND every
// matrix of the call is 16-byte aligned; anything else, a misaligned view included, goes by single floats: no call is refused for
// its alignment.  Up to 256 units a row is read ONCE and stays in registers between its sum and its use, so the output may alias
// the source it replaces there (x and the incoming gradient carry no __restrict__).
#include "common.h"
#include "rowwise.h"

namespace {

using namespace bg::rowwise;

__device__ __forceinline__ float lrelu(float x, float alpha) { return x > 0.f ? x : alpha * x; }

// y = a * r with a = LeakyReLU(x), r = 1 / sqrt(mean(a^2) + eps); saves r where rs != NULL.  (A unit that does not exist is zeros
// and adds nothing to the sum of squares.)
template <int VEC, int NV, bool LOOP>
__global__ __launch_bounds__(kT) void pn_fwd_kernel(const float* x, float* y, Geo g, float eps, float alpha, float* __restrict__ rs) {
  ROWWISE_POS_SETUP();
  for (size_t rg = blockIdx.x; rg < groups; rg += gridDim.x) {
    ROWWISE_ROW_SETUP();
    Tile<VEC, NV> t = load_tile<VEC, NV>(x, q, base);
    float s = 0.f;
    if constexpr (!LOOP) {
#pragma unroll
      for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          t.v[j][e] = lrelu(t.v[j][e], alpha);
          s = fmaf(t.v[j][e], t.v[j][e], s);
        }
    } else {
      for (int b = 0; b < g.U; b += 64 * NV) {
        const Tile<VEC, NV> c = load_tile<VEC, NV>(x, q, b);
#pragma unroll
        for (int j = 0; j < NV; ++j)
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            const float a = lrelu(c.v[j][e], alpha);
            s = fmaf(a, a, s);
          }
      }
#pragma unroll
      for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e) t.v[j][e] = lrelu(t.v[j][e], alpha);
    }
    const float r = 1.f / sqrtf(group_sum(s, q.L) / Cf + eps);
    if (rs != nullptr && q.row_ok && q.sub == 0 && base == 0) rs[q.row] = r;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      if (!unit_ok(q, base, j)) continue;
      float o[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) o[e] = t.v[j][e] * r;
      store_unit<VEC>(y, q.unit0 + base + j * q.L + q.sub, o);
    }
  }
}

// dz = LeakyReLU' * r * (g - y * mean(g * y)), LeakyReLU' = y > 0 ? 1 : alpha (bg_mul_grad's comparison)
template <int VEC, int NV, bool LOOP>
__global__ __launch_bounds__(kT) void pn_bwd_kernel(const float* gr, const float* __restrict__ y, const float* __restrict__ rs, float* dz,
                                                    Geo g, float alpha) {
  ROWWISE_POS_SETUP();
  for (size_t rg = blockIdx.x; rg < groups; rg += gridDim.x) {
    ROWWISE_ROW_SETUP();
    const float r = q.row_ok ? rs[q.row] : 0.f;
    const Tile<VEC, NV> tg = load_tile<VEC, NV>(gr, q, base), ty = load_tile<VEC, NV>(y, q, base);
    float s = 0.f;
    if constexpr (!LOOP) {
#pragma unroll
      for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e) s = fmaf(tg.v[j][e], ty.v[j][e], s);
    } else {
      for (int b = 0; b < g.U; b += 64 * NV) {
        const Tile<VEC, NV> cg = load_tile<VEC, NV>(gr, q, b), cy = load_tile<VEC, NV>(y, q, b);
#pragma unroll
        for (int j = 0; j < NV; ++j)
#pragma unroll
          for (int e = 0; e < VEC; ++e) s = fmaf(cg.v[j][e], cy.v[j][e], s);
      }
    }
    const float m = group_sum(s, q.L) / Cf;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      if (!unit_ok(q, base, j)) continue;
      float o[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const float f = ty.v[j][e] > 0.f ? 1.f : alpha;
        o[e] = f * (r * (tg.v[j][e] - ty.v[j][e] * m));
      }
      store_unit<VEC>(dz, q.unit0 + base + j * q.L + q.sub, o);
    }
  }
}

inline bool al(const void* p) { return bg::aligned16(p); }
inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }      // NULL counts as aligned

}  // namespace

extern "C" {

int bg_pixelnorm_route(int C, int* out) {
  BG_REQUIRE(out, BG_ERR_NULL, "bg_pixelnorm_route: null pointer");
  BG_REQUIRE(C > 0, BG_ERR_BAD_SHAPE, "bg_pixelnorm_route: C=%d", C);
  for (int k = 0; k < 2; ++k) {
    const Route t = route_for(C, k == 0);
    out[4 * k + 0] = t.vec;
    out[4 * k + 1] = 1 << t.lg;
    out[4 * k + 2] = t.nv;
    out[4 * k + 3] = t.chunks;
  }
  return BG_OK;
}

int bg_pixelnorm_fwd_f32(const float* x, float* y, float* r, int R, int C, float eps, float lrelu_alpha, void* stream) {
  BG_REQUIRE(x && y, BG_ERR_NULL, "bg_pixelnorm_fwd_f32: null pointer");
  BG_REQUIRE(R > 0 && C > 0 && eps > 0.f, BG_ERR_BAD_SHAPE, "bg_pixelnorm_fwd_f32: R=%d C=%d eps=%g", R, C, (double)eps);
  BG_REQUIRE(al4(x) && al4(y) && al4(r), BG_ERR_BAD_ALIGNMENT, "bg_pixelnorm_fwd_f32: pointers must be 4-byte aligned");
  const Route t = route_for(C, al(x) && al(y));
  BG_REQUIRE(t.chunks == 1 || y != x, BG_ERR_UNSUPPORTED,
             "bg_pixelnorm_fwd_f32: y may alias x on the register routes only (C=%d is swept in %d chunks)", C, t.chunks);
  bg::Launch L(stream, "pixelnorm_fwd", 0, 8.0 * R * C + (r ? 4.0 * R : 0.0));
  const dim3 grid = grid_for(R, t);
  for_route(t, [&](auto lanes) {
    using Rt = decltype(lanes);
    bg::launch(pn_fwd_kernel<Rt::VEC, Rt::NV, Rt::LOOP>, grid, dim3(kT), 0, L.s, x, y, geo_for(R, C, t), eps, lrelu_alpha, r);
  });
  return L.done("pn_fwd_kernel");
}

int bg_pixelnorm_bwd_f32(const float* g, const float* y, const float* r, float* dz, int R, int C, float lrelu_alpha, void* stream) {
  BG_REQUIRE(g && y && r && dz, BG_ERR_NULL, "bg_pixelnorm_bwd_f32: null pointer");
  BG_REQUIRE(R > 0 && C > 0, BG_ERR_BAD_SHAPE, "bg_pixelnorm_bwd_f32: R=%d C=%d", R, C);
  BG_REQUIRE(al4(g) && al4(y) && al4(r) && al4(dz), BG_ERR_BAD_ALIGNMENT, "bg_pixelnorm_bwd_f32: pointers must be 4-byte aligned");
  const Route t = route_for(C, al(g) && al(y) && al(dz));
  BG_REQUIRE(dz != y, BG_ERR_UNSUPPORTED, "bg_pixelnorm_bwd_f32: dz must not alias y");
  BG_REQUIRE(t.chunks == 1 || dz != g, BG_ERR_UNSUPPORTED,
             "bg_pixelnorm_bwd_f32: dz may alias g on the register routes only (C=%d is swept in %d chunks)", C, t.chunks);
  bg::Launch L(stream, "pixelnorm_bwd", 0, 12.0 * R * C + 4.0 * R);
  const dim3 grid = grid_for(R, t);
  for_route(t, [&](auto lanes) {
    using Rt = decltype(lanes);
    bg::launch(pn_bwd_kernel<Rt::VEC, Rt::NV, Rt::LOOP>, grid, dim3(kT), 0, L.s, g, y, r, dz, geo_for(R, C, t), lrelu_alpha);
  });
  return L.done("pn_bwd_kernel");
}

}  // extern "C"
