// FIR-filtered 2x resampling over NHWC fp32 maps (include/bgan.h "resampling"): StyleGAN2's upsample_2d / downsample_2d with an
// even-length separable kernel, the two linear, parameter-free operators behind layers.FilteredUpSampling2D and
// layers.FilteredDownSampling2D.  Per axis, with 2T taps t and n low-resolution entries,
//   UP_t(x)[o]   = sum_i t[o - 2i + T - 1] x[i],  o in [0, 2n)        DOWN_t(g)[m] = sum_o t[T + 2m - o] g[o],  m in [0, n)
// with absent terms (a tap index outside [0, 2T), a sample outside the map) for the zero padding; <UP_t x, g> = <x, DOWN_flip(t) g>,
// so the pair serves forward, backward and the gradient penalty's linearised forward of both layers.  One launch does both axes:
// a thread filters the rows of its neighbourhood along W in registers and accumulates them along H; no intermediate map.  Like the
// nearest pair (resample.hip), the upsample optionally applies bg_mul_grad_f32's factor to what it writes.
// Streaming with cache reuse: one thread owns one low-resolution pixel's channel quad (float4 route, C % 4 == 0) or one
// low-resolution element (scalar route), in a grid-stride loop; the threads of a workgroup cover neighbouring pixels of a row, so
// the overlap of their neighbourhoods is served by L1 / L2; size_t indices throughout.
// The taps travel by value in the kernel arguments: a step program replays them with no device table.
#include "common.h"
#include <algorithm>

namespace {

constexpr int kT = 256;

struct FirTaps {
  float t[8];
};

// bg_mul_grad_f32's factor (misc.hip mul_grad_kernel), operation for operation
__device__ inline float grad_factor(float r, bool has_keep, unsigned k, float alpha, float gscale) {
  float f = r > 0.f ? 1.f : alpha;
  if (has_keep) f = k ? f * gscale : 0.f;
  return f;
}

// Consecutive workgroups are placed round-robin over the chip's 8 XCDs, each with an L2 of its own, and a workgroup's vertical
// neighbours (the rows above and below) belong to workgroups a few indices away: left alone they would sit in other L2s and every
// shared row would be fetched from the fabric once per XCD that reads it (measured: 2x / 3x the input map).  So the block
// index is permuted to give each XCD a contiguous run of the work; a bijection where the grid is a multiple of 8 (xcd_grid), the
// identity elsewhere.  Placement is a matter of speed only.
constexpr unsigned kXcds = 8;
__device__ inline size_t xcd_chunked_block() {
  const unsigned nb = gridDim.x, b = blockIdx.x;
  return nb % kXcds ? b : (size_t)(b % kXcds) * (nb / kXcds) + b / kXcds;
}

// bg::grid_cap rounded up to a multiple of 8 where there are at least 8 workgroups (the cap, 2048, is one): surplus workgroups find no unit
unsigned xcd_grid(size_t units) {
  const unsigned g = bg::grid_cap(units, kT);
  return g < kXcds ? g : (g + kXcds - 1) / kXcds * kXcds;
}

// The two routes share every kernel: V is the unit a thread moves (float4 | float), K its slice of the keep mask (uint32_t | uint8_t).
__device__ inline float zero(float) { return 0.f; }
__device__ inline float4 zero(float4) { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ inline void madd(float& a, float t, float v) { a = a + t * v; }
__device__ inline void madd(float4& a, float t, float4 v) {
  a.x = a.x + t * v.x;
  a.y = a.y + t * v.y;
  a.z = a.z + t * v.z;
  a.w = a.w + t * v.w;
}
__device__ inline float scaled(float s, float v) { return s * v; }
__device__ inline float4 scaled(float s, float4 v) { return make_float4(s * v.x, s * v.y, s * v.z, s * v.w); }
__device__ inline float with_factor(float v, float r, bool has_keep, uint8_t k, float alpha, float gscale) {
  return v * grad_factor(r, has_keep, k, alpha, gscale);
}
__device__ inline float4 with_factor(float4 v, float4 r, bool has_keep, uint32_t k, float alpha, float gscale) {
  float4 w;
  w.x = v.x * grad_factor(r.x, has_keep, k & 0xffu, alpha, gscale);
  w.y = v.y * grad_factor(r.y, has_keep, (k >> 8) & 0xffu, alpha, gscale);
  w.z = v.z * grad_factor(r.z, has_keep, (k >> 16) & 0xffu, alpha, gscale);
  w.w = v.w * grad_factor(r.w, has_keep, k >> 24, alpha, gscale);
  return w;
}

// x[B, H, W, CU] -> y[B, 2H, 2W, CU] (CU = channel units per pixel).  Output 2p + d takes x[p - e] with tap 2e + d + T - 1 where
// that is a tap: e in [-T/2, T/2] covers both phases d.  Row p - e is filtered along W into its two phases, then joins the two
// output rows it has a tap for.
template <int T, bool FUSED, class V, class K>
__global__ __launch_bounds__(kT) void fir_upsample2x_kernel(const V* __restrict__ x, V* __restrict__ y, size_t units, size_t H, size_t W,
                                                            size_t CU, FirTaps f, float scale, const V* __restrict__ ref,
                                                            const K* __restrict__ keep, float alpha, float gscale) {
  constexpr int R = T / 2;
  const size_t row = 2 * W * CU;
  for (size_t u = xcd_chunked_block() * kT + threadIdx.x; u < units; u += (size_t)gridDim.x * kT) {
    const size_t c = u % CU, p = u / CU;
    const size_t j = p % W, t = p / W;
    const size_t i = t % H, b = t / H;
    V acc[2][2] = {{zero(V()), zero(V())}, {zero(V()), zero(V())}};
#pragma unroll
    for (int ev = -R; ev <= R; ++ev) {
      if ((ev > 0 && i < (size_t)ev) || (ev < 0 && i + (size_t)(-ev) >= H)) continue;      // the row lies outside the map
      const size_t base = (b * H + (i - ev)) * W;
      V hs[2] = {zero(V()), zero(V())};
#pragma unroll
      for (int eh = -R; eh <= R; ++eh) {
        if ((eh > 0 && j < (size_t)eh) || (eh < 0 && j + (size_t)(-eh) >= W)) continue;
        const V v = x[(base + (j - eh)) * CU + c];
#pragma unroll
        for (int d = 0; d < 2; ++d) {
          const int tap = 2 * eh + d + T - 1;
          if (tap >= 0 && tap < 2 * T) madd(hs[d], f.t[tap], v);
        }
      }
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        const int tap = 2 * ev + d + T - 1;
        if (tap >= 0 && tap < 2 * T) {
          madd(acc[d][0], f.t[tap], hs[0]);
          madd(acc[d][1], f.t[tap], hs[1]);
        }
      }
    }
    const size_t o = ((b * 2 * H + 2 * i) * 2 * W + 2 * j) * CU + c;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const size_t at = o + (q >> 1) * row + (q & 1) * CU;
      const V v = scaled(scale, acc[q >> 1][q & 1]);
      if constexpr (FUSED)
        y[at] = with_factor(v, ref[at], keep != nullptr, keep ? keep[at] : K(0), alpha, gscale);
      else
        y[at] = v;
    }
  }
}

// x[B, 2H, 2W, CU] -> y[B, H, W, CU].  Output m takes x[2m - T + 1 + a] with tap 2T - 1 - a, a in [0, 2T): each of the 2T rows
// is filtered along W, then accumulated along H.
template <int T, class V>
__global__ __launch_bounds__(kT) void fir_downsample2x_kernel(const V* __restrict__ x, V* __restrict__ y, size_t units, size_t H,
                                                              size_t W, size_t CU, FirTaps f, float scale) {
  for (size_t u = xcd_chunked_block() * kT + threadIdx.x; u < units; u += (size_t)gridDim.x * kT) {
    const size_t c = u % CU, p = u / CU;
    const size_t j = p % W, t = p / W;
    const size_t i = t % H, b = t / H;
    V acc = zero(V());
#pragma unroll
    for (int av = 0; av < 2 * T; ++av) {
      const size_t ov = 2 * i + av;           // the row's index + (T - 1)
      if (ov < (size_t)(T - 1) || ov - (T - 1) >= 2 * H) continue;
      const size_t base = (b * 2 * H + (ov - (T - 1))) * 2 * W;
      V hs = zero(V());
#pragma unroll
      for (int ah = 0; ah < 2 * T; ++ah) {
        const size_t oh = 2 * j + ah;
        if (oh < (size_t)(T - 1) || oh - (T - 1) >= 2 * W) continue;
        madd(hs, f.t[2 * T - 1 - ah], x[(base + (oh - (T - 1))) * CU + c]);
      }
      madd(acc, f.t[2 * T - 1 - av], hs);
    }
    y[u] = scaled(scale, acc);
  }
}

template <int T, class V, class K>
void launch_up(dim3 grid, hipStream_t s, const V* x, V* y, size_t units, size_t H, size_t W, size_t CU, const FirTaps& f, float scale,
               const V* ref, const K* keep, float alpha, float gscale) {
  if (ref)
    bg::launch(fir_upsample2x_kernel<T, true, V, K>, grid, dim3(kT), 0, s, x, y, units, H, W, CU, f, scale, ref, keep, alpha, gscale);
  else
    bg::launch(fir_upsample2x_kernel<T, false, V, K>, grid, dim3(kT), 0, s, x, y, units, H, W, CU, f, scale, ref, keep, alpha, gscale);
}

template <class V, class K>
void dispatch_up(int T, dim3 grid, hipStream_t s, const float* x, float* y, size_t units, size_t H, size_t W, size_t CU, const FirTaps& f,
                 float scale, const float* ref, const uint8_t* keep, float alpha, float gscale) {
  const V* xv = reinterpret_cast<const V*>(x);
  const V* rv = reinterpret_cast<const V*>(ref);
  const K* kv = reinterpret_cast<const K*>(keep);
  V* yv = reinterpret_cast<V*>(y);
  switch (T) {
    case 1: launch_up<1, V, K>(grid, s, xv, yv, units, H, W, CU, f, scale, rv, kv, alpha, gscale); break;
    case 2: launch_up<2, V, K>(grid, s, xv, yv, units, H, W, CU, f, scale, rv, kv, alpha, gscale); break;
    case 3: launch_up<3, V, K>(grid, s, xv, yv, units, H, W, CU, f, scale, rv, kv, alpha, gscale); break;
    default: launch_up<4, V, K>(grid, s, xv, yv, units, H, W, CU, f, scale, rv, kv, alpha, gscale); break;
  }
}

template <class V>
void dispatch_down(int T, dim3 grid, hipStream_t s, const float* x, float* y, size_t units, size_t H, size_t W, size_t CU, const FirTaps& f,
                   float scale) {
  const V* xv = reinterpret_cast<const V*>(x);
  V* yv = reinterpret_cast<V*>(y);
  switch (T) {
    case 1: bg::launch(fir_downsample2x_kernel<1, V>, grid, dim3(kT), 0, s, xv, yv, units, H, W, CU, f, scale); break;
    case 2: bg::launch(fir_downsample2x_kernel<2, V>, grid, dim3(kT), 0, s, xv, yv, units, H, W, CU, f, scale); break;
    case 3: bg::launch(fir_downsample2x_kernel<3, V>, grid, dim3(kT), 0, s, xv, yv, units, H, W, CU, f, scale); break;
    default: bg::launch(fir_downsample2x_kernel<4, V>, grid, dim3(kT), 0, s, xv, yv, units, H, W, CU, f, scale); break;
  }
}

bool tap_count_ok(int n_taps) { return n_taps == 2 || n_taps == 4 || n_taps == 6 || n_taps == 8; }

FirTaps taps_by_value(const float* taps, int n_taps) {
  FirTaps f = {};
  std::copy(taps, taps + n_taps, f.t);
  return f;
}

}  // namespace

extern "C" {

int bg_fir_upsample2x_nhwc_f32(const float* x, float* y, int B, int H, int W, int C, const float* taps, int n_taps, float scale,
                               const float* ref, const uint8_t* keep, float alpha, float grad_scale, void* stream) {
  BG_REQUIRE(x && y && taps, BG_ERR_NULL, "bg_fir_upsample2x_nhwc_f32: null pointer");
  BG_REQUIRE(ref || !keep, BG_ERR_NULL, "bg_fir_upsample2x_nhwc_f32: keep needs ref");
  BG_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, BG_ERR_BAD_SHAPE, "bg_fir_upsample2x_nhwc_f32: B=%d H=%d W=%d C=%d", B, H, W, C);
  BG_REQUIRE(tap_count_ok(n_taps), BG_ERR_BAD_SHAPE, "bg_fir_upsample2x_nhwc_f32: n_taps=%d (2, 4, 6 or 8)", n_taps);
  const bool v4 = C % 4 == 0;
  BG_REQUIRE(!v4 || (bg::aligned16(x) && bg::aligned16(y) && bg::aligned16(ref) && bg::aligned16(keep)), BG_ERR_BAD_ALIGNMENT,
             "bg_fir_upsample2x_nhwc_f32: pointers must be 16-byte aligned when C %% 4 == 0");
  const size_t n = (size_t)B * H * W * C, units = v4 ? n / 4 : n, CU = v4 ? C / 4 : C;
  const FirTaps f = taps_by_value(taps, n_taps);
  bg::Launch L(stream, ref ? "fir_upsample2x_mul_grad" : "fir_upsample2x", 0, (20.0 + (ref ? 16.0 : 0.0) + (keep ? 4.0 : 0.0)) * n);
  const dim3 grid(xcd_grid(units));
  if (v4)
    dispatch_up<float4, uint32_t>(n_taps / 2, grid, L.s, x, y, units, (size_t)H, (size_t)W, CU, f, scale, ref, keep, alpha, grad_scale);
  else
    dispatch_up<float, uint8_t>(n_taps / 2, grid, L.s, x, y, units, (size_t)H, (size_t)W, CU, f, scale, ref, keep, alpha, grad_scale);
  return L.done("fir_upsample2x_kernel");
}

int bg_fir_downsample2x_nhwc_f32(const float* x, float* y, int B, int H, int W, int C, const float* taps, int n_taps, float scale,
                                 void* stream) {
  BG_REQUIRE(x && y && taps, BG_ERR_NULL, "bg_fir_downsample2x_nhwc_f32: null pointer");
  BG_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, BG_ERR_BAD_SHAPE, "bg_fir_downsample2x_nhwc_f32: B=%d H=%d W=%d C=%d", B, H, W, C);
  BG_REQUIRE(tap_count_ok(n_taps), BG_ERR_BAD_SHAPE, "bg_fir_downsample2x_nhwc_f32: n_taps=%d (2, 4, 6 or 8)", n_taps);
  const bool v4 = C % 4 == 0;
  BG_REQUIRE(!v4 || (bg::aligned16(x) && bg::aligned16(y)), BG_ERR_BAD_ALIGNMENT,
             "bg_fir_downsample2x_nhwc_f32: pointers must be 16-byte aligned when C %% 4 == 0");
  const size_t n = (size_t)B * H * W * C, units = v4 ? n / 4 : n, CU = v4 ? C / 4 : C;
  const FirTaps f = taps_by_value(taps, n_taps);
  bg::Launch L(stream, "fir_downsample2x", 0, 20.0 * n);
  const dim3 grid(xcd_grid(units));
  if (v4)
    dispatch_down<float4>(n_taps / 2, grid, L.s, x, y, units, (size_t)H, (size_t)W, CU, f, scale);
  else
    dispatch_down<float>(n_taps / 2, grid, L.s, x, y, units, (size_t)H, (size_t)W, CU, f, scale);
  return L.done("fir_downsample2x_kernel");
}

}  // extern "C"
