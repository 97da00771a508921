// Input pipeline of a device-resident uint8 dataset: ONE launch turns a list of sample indices into the step's float32 batch --
// gather -> (x - 127.5) / 127.5 -> tf.image.resize(bilinear, half-pixel centres) -> optional left-right mirror
// (demo_celeba.py:22-35, demo_mnist.py:24-31 behind tfds ... shuffle ... batch).  Bandwidth-bound, no LDS: it reads at most
// B*Hs*Ws*C bytes and writes 4*B*Hd*Wd*C.  The interpolation of a value is, expression for expression, that of
// u8_normalize_resize_kernel (misc.hip) and the normalisation gives the same float for every byte (u8_norm), so the two agree bit
// for bit on the same image.
#include "common.h"
#include <algorithm>

namespace {

constexpr int kT = 256;
typedef float f32x4 __attribute__((ext_vector_type(4)));      // a native vector: its store stays ONE 16-byte instruction

inline unsigned grid_for(size_t n) { return bg::grid_cap(n, kT); }

// [TF] resize_bilinear, half_pixel_centers: in = (out + 0.5) * scale - 0.5; lower = max(floor(in), 0),
// upper = min(ceil(in), size - 1), lerp = in - floor(in)
struct Tap { int i0, i1; float l; };
__device__ __forceinline__ Tap tap_of(int o, float scale, int n_in) {
  const float f = ((float)o + 0.5f) * scale - 0.5f, f0 = floorf(f);
  Tap t;
  t.i0 = max((int)f0, 0);
  t.i1 = min((int)ceilf(f), n_in - 1);
  t.l = f - f0;
  return t;
}

// (v - 127.5) / 127.5 without the division sequence: x = v - 127.5 is exact, q = x * (1 / 127.5) is within an ulp of the quotient,
// and one fused residual step q + (x - q * 127.5) * (1 / 127.5) rounds to it -- for EVERY one of the 256 inputs the float the IEEE
// division of u8_normalize_resize_kernel gives (exhaustive: tests/test_input_dataset_gpu.py), at 4 VALU operations instead of the
// dozen of v_div_scale / v_rcp / v_div_fmas / v_div_fixup; four of these per output float made the kernel VALU-bound otherwise
__device__ __forceinline__ float u8_norm(uint8_t v) {
  constexpr float r = 1.0f / 127.5f;
  const float x = (float)v - 127.5f, q = x * r;
  return fmaf(fmaf(-q, 127.5f, x), r, q);
}

// the C channels of one output pixel: the four source pixels' addresses and both lerp weights are formed once for all channels
template <int CT>
__device__ __forceinline__ void resize_pixel(const uint8_t* __restrict__ img, int Ws, int Cr, const Tap& ty, const Tap& tx, float* o) {
  const int C = CT ? CT : Cr;
  const uint8_t* r0 = img + (size_t)ty.i0 * Ws * C;
  const uint8_t* r1 = img + (size_t)ty.i1 * Ws * C;
  const uint8_t *p00 = r0 + (size_t)tx.i0 * C, *p01 = r0 + (size_t)tx.i1 * C, *p10 = r1 + (size_t)tx.i0 * C, *p11 = r1 + (size_t)tx.i1 * C;
  auto channel = [&](int c) {
    const float v00 = u8_norm(p00[c]), v01 = u8_norm(p01[c]), v10 = u8_norm(p10[c]), v11 = u8_norm(p11[c]);
    const float top = v00 + (v01 - v00) * tx.l;
    const float bot = v10 + (v11 - v10) * tx.l;
    o[c] = top + (bot - top) * ty.l;
  };
  if constexpr (CT > 0) {
#pragma unroll
    for (int c = 0; c < CT; ++c) channel(c);
  } else {
    for (int c = 0; c < Cr; ++c) channel(c);
  }
}

// Position of a thread in the batch's flat pixel sequence q = (b * Hd + y) * Wd + x: one division chain per THREAD; a thread's
// further pixels are reached by stepping.  The sample's base pointer (64-bit byte offset: N*Hs*Ws*C exceeds 2^31 for CelebA) and
// mirror flag are taken when the sample changes.  The mirror acts on the OUTPUT index: pixel x of a mirrored sample is computed
// as pixel Wd-1-x of the unmirrored one, with the same expressions, hence the same bits.
struct Cursor {
  const uint8_t* img;
  int b, y, x, fl;
  Tap ty;
};

struct Geom {
  const uint8_t* src;
  const int32_t* idx;
  const uint8_t* flip;
  size_t img_bytes;
  int P, Hs, Ws, Hd, Wd;
  float sy, sx;
};

__device__ __forceinline__ void take_sample(const Geom& g, Cursor& c) {
  c.img = g.src + (size_t)g.idx[c.b] * g.img_bytes;
  c.fl = g.flip ? (int)g.flip[c.b] : 0;
}

__device__ __forceinline__ Cursor cursor_at(const Geom& g, size_t q) {
  Cursor c;
  c.b = (int)(q / (size_t)g.P);
  const int p = (int)(q - (size_t)c.b * g.P);
  c.y = p / g.Wd;
  c.x = p - c.y * g.Wd;
  take_sample(g, c);
  c.ty = tap_of(c.y, g.sy, g.Hs);
  return c;
}

// to the next pixel of the sequence; `more` = that pixel exists (a step past the batch's last pixel must not read idx[B])
__device__ __forceinline__ void advance(const Geom& g, Cursor& c, bool more) {
  if (++c.x < g.Wd) return;
  c.x = 0;
  if (++c.y == g.Hd) {
    c.y = 0;
    ++c.b;
    if (more) take_sample(g, c);
  }
  c.ty = tap_of(c.y, g.sy, g.Hs);
}

__device__ __forceinline__ Tap tap_x(const Geom& g, const Cursor& c) { return tap_of(c.fl ? g.Wd - 1 - c.x : c.x, g.sx, g.Ws); }

// C known at compile time: FOUR consecutive output pixels per thread = 4*C floats = C 16-byte stores at a 16*C-byte multiple of
// the (16-byte aligned) destination, whatever C is; the n_pix % 4 pixels left over are written by scalar stores.
template <int C>
__global__ __launch_bounds__(kT) void u8_gather_resize_vec_kernel(const Geom g, float* __restrict__ dst, size_t n_pix) {
  const size_t n_grp = n_pix >> 2;
  const size_t tid = (size_t)blockIdx.x * kT + threadIdx.x;
  for (size_t grp = tid; grp < n_grp; grp += (size_t)gridDim.x * kT) {
    Cursor c = cursor_at(g, grp * 4);
    float o[4 * C];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      resize_pixel<C>(c.img, g.Ws, C, c.ty, tap_x(g, c), o + k * C);
      if (k < 3) advance(g, c, true);       // the group is whole: its next pixel exists
    }
    f32x4* d4 = reinterpret_cast<f32x4*>(dst + grp * (size_t)(4 * C));
#pragma unroll
    for (int j = 0; j < C; ++j) {
      f32x4 v;
      v.x = o[4 * j]; v.y = o[4 * j + 1]; v.z = o[4 * j + 2]; v.w = o[4 * j + 3];
      d4[j] = v;
    }
  }
  const size_t q = n_grp * 4 + tid;         // scalar tail: at most 3 pixels
  if (q < n_pix) {
    const Cursor c = cursor_at(g, q);
    float o[C];
    resize_pixel<C>(c.img, g.Ws, C, c.ty, tap_x(g, c), o);
#pragma unroll
    for (int j = 0; j < C; ++j) dst[q * C + j] = o[j];
  }
}

// any other channel count: one pixel per thread, scalar stores
__global__ __launch_bounds__(kT) void u8_gather_resize_any_kernel(const Geom g, float* __restrict__ dst, size_t n_pix, int C) {
  for (size_t q = (size_t)blockIdx.x * kT + threadIdx.x; q < n_pix; q += (size_t)gridDim.x * kT) {
    const Cursor c = cursor_at(g, q);
    resize_pixel<0>(c.img, g.Ws, C, c.ty, tap_x(g, c), dst + q * C);
  }
}

}  // namespace

extern "C" {

int bg_u8_gather_normalize_resize_f32(const uint8_t* src, int N, const int32_t* idx_d, const uint8_t* flip_d, float* dst, int B, int Hs,
                                      int Ws, int C, int Hd, int Wd, void* stream) {
  BG_REQUIRE(src && idx_d && dst, BG_ERR_NULL, "bg_u8_gather_normalize_resize_f32: null pointer");
  BG_REQUIRE(N > 0 && B > 0 && Hs > 0 && Ws > 0 && C > 0 && Hd > 0 && Wd > 0, BG_ERR_BAD_SHAPE,
             "bg_u8_gather_normalize_resize_f32: N=%d B=%d %dx%dx%d -> %dx%d", N, B, Hs, Ws, C, Hd, Wd);
  BG_REQUIRE((double)Hd * Wd < 2147483648.0 && (double)Hs * Ws * C < 2147483648.0, BG_ERR_BAD_SHAPE,
             "bg_u8_gather_normalize_resize_f32: an image of %dx%dx%d -> %dx%d exceeds 2^31 elements", Hs, Ws, C, Hd, Wd);
  BG_REQUIRE(bg::aligned16(dst), BG_ERR_BAD_ALIGNMENT, "bg_u8_gather_normalize_resize_f32: dst must be 16-byte aligned");
  const size_t n_pix = (size_t)B * Hd * Wd;
  Geom g;
  g.src = src; g.idx = idx_d; g.flip = flip_d;
  g.img_bytes = (size_t)Hs * Ws * C;
  g.P = Hd * Wd; g.Hs = Hs; g.Ws = Ws; g.Hd = Hd; g.Wd = Wd;
  g.sy = (float)Hs / (float)Hd; g.sx = (float)Ws / (float)Wd;
  bg::Launch L(stream, "u8_gather_normalize_resize", 0, (double)B * Hs * Ws * C + 4.0 * (double)n_pix * C);
  const dim3 grid(grid_for(bg::cdiv(n_pix, 4))), block(kT);
  switch (C) {
    case 1: bg::launch(u8_gather_resize_vec_kernel<1>, grid, block, 0, L.s, g, dst, n_pix); break;
    case 3: bg::launch(u8_gather_resize_vec_kernel<3>, grid, block, 0, L.s, g, dst, n_pix); break;
    case 4: bg::launch(u8_gather_resize_vec_kernel<4>, grid, block, 0, L.s, g, dst, n_pix); break;
    default: bg::launch(u8_gather_resize_any_kernel, dim3(grid_for(n_pix)), block, 0, L.s, g, dst, n_pix, C); break;
  }
  return L.done("u8_gather_resize_kernel");
}

}  // extern "C"
