// 2x nearest-neighbour upsampling and 2x2 sum pooling over NHWC fp32 maps (include/bgan.h "resampling"): the two linear,
// parameter-free operators behind layers.UpSampling2D and layers.AveragePooling2D.  Each is the transpose of the other, so the
// pair serves forward, backward and the gradient penalty's linearised forward of both layers (scale 1 or 0.25).  The upsample
// optionally applies bg_mul_grad_f32's factor to what it writes: the pooling layer's backward then lands as the dz of the
// conv + LeakyReLU (+ Dropout) stage below it in one pass instead of a store and a full-resolution read-modify-write.
// Pure streaming: one thread owns one low-resolution pixel's channel quad (float4 route, C % 4 == 0) or one low-resolution
// element (scalar route, any other C), in a grid-stride loop; size_t indices throughout.
#include "common.h"
#include <algorithm>

namespace {

constexpr int kT = 256;

// bg_mul_grad_f32's factor (misc.hip mul_grad_kernel), operation for operation
__device__ inline float grad_factor(float r, bool has_keep, unsigned k, float alpha, float gscale) {
  float f = r > 0.f ? 1.f : alpha;
  if (has_keep) f = k ? f * gscale : 0.f;
  return f;
}

// Unit index u of the low-resolution map [B, H, W, CU] -> index of the top-left of its 2x2 block in [B, 2H, 2W, CU]
// (CU = channel units per pixel: C / 4 float4s or C floats).  The other three lie at + CU, + 2W*CU and + 2W*CU + CU.
__device__ inline size_t hi_index(size_t u, size_t H, size_t W, size_t CU) {
  const size_t c = u % CU, p = u / CU;
  const size_t j = p % W, t = p / W;
  const size_t i = t % H, b = t / H;
  return ((b * 2 * H + 2 * i) * 2 * W + 2 * j) * CU + c;
}

template <bool FUSED>
__global__ __launch_bounds__(kT) void upsample2x_v4_kernel(const float4* __restrict__ x, float4* __restrict__ y, size_t units, size_t H,
                                                           size_t W, size_t C4, float scale, const float4* __restrict__ ref,
                                                           const uint32_t* __restrict__ keep, float alpha, float gscale) {
  const size_t row = 2 * W * C4;
  for (size_t u = (size_t)blockIdx.x * kT + threadIdx.x; u < units; u += (size_t)gridDim.x * kT) {
    float4 v = x[u];
    v.x = scale * v.x;
    v.y = scale * v.y;
    v.z = scale * v.z;
    v.w = scale * v.w;
    const size_t o = hi_index(u, H, W, C4);
    const size_t at[4] = {o, o + C4, o + row, o + row + C4};
    if constexpr (FUSED) {
      float4 r[4];
      uint32_t k[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int q = 0; q < 4; ++q) r[q] = ref[at[q]];
      if (keep) {
#pragma unroll
        for (int q = 0; q < 4; ++q) k[q] = keep[at[q]];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float4 w;
        w.x = v.x * grad_factor(r[q].x, keep != nullptr, k[q] & 0xffu, alpha, gscale);
        w.y = v.y * grad_factor(r[q].y, keep != nullptr, (k[q] >> 8) & 0xffu, alpha, gscale);
        w.z = v.z * grad_factor(r[q].z, keep != nullptr, (k[q] >> 16) & 0xffu, alpha, gscale);
        w.w = v.w * grad_factor(r[q].w, keep != nullptr, k[q] >> 24, alpha, gscale);
        y[at[q]] = w;
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) y[at[q]] = v;
    }
  }
}

template <bool FUSED>
__global__ __launch_bounds__(kT) void upsample2x_s_kernel(const float* __restrict__ x, float* __restrict__ y, size_t units, size_t H,
                                                          size_t W, size_t C, float scale, const float* __restrict__ ref,
                                                          const uint8_t* __restrict__ keep, float alpha, float gscale) {
  const size_t row = 2 * W * C;
  for (size_t u = (size_t)blockIdx.x * kT + threadIdx.x; u < units; u += (size_t)gridDim.x * kT) {
    const float v = scale * x[u];
    const size_t o = hi_index(u, H, W, C);
    const size_t at[4] = {o, o + C, o + row, o + row + C};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if constexpr (FUSED)
        y[at[q]] = v * grad_factor(ref[at[q]], keep != nullptr, keep ? keep[at[q]] : 0u, alpha, gscale);
      else
        y[at[q]] = v;
    }
  }
}

// y = scale * ((x00 + x01) + (x10 + x11)): the order is part of the contract (bit-reproducible against the same expression)
__global__ __launch_bounds__(kT) void pool2x_sum_v4_kernel(const float4* __restrict__ x, float4* __restrict__ y, size_t units, size_t H,
                                                           size_t W, size_t C4, float scale) {
  const size_t row = 2 * W * C4;
  for (size_t u = (size_t)blockIdx.x * kT + threadIdx.x; u < units; u += (size_t)gridDim.x * kT) {
    const size_t o = hi_index(u, H, W, C4);
    const float4 a = x[o], b = x[o + C4], c = x[o + row], d = x[o + row + C4];
    float4 s;
    s.x = scale * ((a.x + b.x) + (c.x + d.x));
    s.y = scale * ((a.y + b.y) + (c.y + d.y));
    s.z = scale * ((a.z + b.z) + (c.z + d.z));
    s.w = scale * ((a.w + b.w) + (c.w + d.w));
    y[u] = s;
  }
}

__global__ __launch_bounds__(kT) void pool2x_sum_s_kernel(const float* __restrict__ x, float* __restrict__ y, size_t units, size_t H,
                                                          size_t W, size_t C, float scale) {
  const size_t row = 2 * W * C;
  for (size_t u = (size_t)blockIdx.x * kT + threadIdx.x; u < units; u += (size_t)gridDim.x * kT) {
    const size_t o = hi_index(u, H, W, C);
    y[u] = scale * ((x[o] + x[o + C]) + (x[o + row] + x[o + row + C]));
  }
}

}  // namespace

extern "C" {

int bg_upsample2x_nhwc_f32(const float* x, float* y, int B, int H, int W, int C, float scale, const float* ref, const uint8_t* keep,
                           float alpha, float grad_scale, void* stream) {
  BG_REQUIRE(x && y, BG_ERR_NULL, "bg_upsample2x_nhwc_f32: null pointer");
  BG_REQUIRE(ref || !keep, BG_ERR_NULL, "bg_upsample2x_nhwc_f32: keep needs ref");
  BG_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, BG_ERR_BAD_SHAPE, "bg_upsample2x_nhwc_f32: B=%d H=%d W=%d C=%d", B, H, W, C);
  const bool v4 = C % 4 == 0;
  BG_REQUIRE(!v4 || (bg::aligned16(x) && bg::aligned16(y) && bg::aligned16(ref) && bg::aligned16(keep)), BG_ERR_BAD_ALIGNMENT,
             "bg_upsample2x_nhwc_f32: pointers must be 16-byte aligned when C %% 4 == 0");
  const size_t n = (size_t)B * H * W * C, units = v4 ? n / 4 : n, CU = v4 ? C / 4 : C;
  bg::Launch L(stream, ref ? "upsample2x_mul_grad" : "upsample2x", 0, (20.0 + (ref ? 16.0 : 0.0) + (keep ? 4.0 : 0.0)) * n);
  const dim3 grid(bg::grid_cap(units, kT)), block(kT);
  if (v4) {
    const float4* x4 = reinterpret_cast<const float4*>(x);
    const float4* r4 = reinterpret_cast<const float4*>(ref);
    const uint32_t* k4 = reinterpret_cast<const uint32_t*>(keep);
    float4* y4 = reinterpret_cast<float4*>(y);
    if (ref)
      bg::launch(upsample2x_v4_kernel<true>, grid, block, 0, L.s, x4, y4, units, (size_t)H, (size_t)W, CU, scale, r4, k4, alpha, grad_scale);
    else
      bg::launch(upsample2x_v4_kernel<false>, grid, block, 0, L.s, x4, y4, units, (size_t)H, (size_t)W, CU, scale, r4, k4, alpha, grad_scale);
  } else {
    if (ref)
      bg::launch(upsample2x_s_kernel<true>, grid, block, 0, L.s, x, y, units, (size_t)H, (size_t)W, CU, scale, ref, keep, alpha, grad_scale);
    else
      bg::launch(upsample2x_s_kernel<false>, grid, block, 0, L.s, x, y, units, (size_t)H, (size_t)W, CU, scale, ref, keep, alpha, grad_scale);
  }
  return L.done("upsample2x_kernel");
}

int bg_pool2x_sum_nhwc_f32(const float* x, float* y, int B, int H, int W, int C, float scale, void* stream) {
  BG_REQUIRE(x && y, BG_ERR_NULL, "bg_pool2x_sum_nhwc_f32: null pointer");
  BG_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, BG_ERR_BAD_SHAPE, "bg_pool2x_sum_nhwc_f32: B=%d H=%d W=%d C=%d", B, H, W, C);
  const bool v4 = C % 4 == 0;
  BG_REQUIRE(!v4 || (bg::aligned16(x) && bg::aligned16(y)), BG_ERR_BAD_ALIGNMENT,
             "bg_pool2x_sum_nhwc_f32: pointers must be 16-byte aligned when C %% 4 == 0");
  const size_t n = (size_t)B * H * W * C, units = v4 ? n / 4 : n, CU = v4 ? C / 4 : C;
  bg::Launch L(stream, "pool2x_sum", 0, 20.0 * n);
  const dim3 grid(bg::grid_cap(units, kT)), block(kT);
  if (v4)
    bg::launch(pool2x_sum_v4_kernel, grid, block, 0, L.s, reinterpret_cast<const float4*>(x), reinterpret_cast<float4*>(y), units, (size_t)H,
               (size_t)W, CU, scale);
  else
    bg::launch(pool2x_sum_s_kernel, grid, block, 0, L.s, x, y, units, (size_t)H, (size_t)W, CU, scale);
  return L.done("pool2x_sum_kernel");
}

}  // extern "C"
