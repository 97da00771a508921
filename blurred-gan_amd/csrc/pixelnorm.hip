// Pixel normalisation over the channel axis of NHWC fp32 maps and of latent vectors (include/bgan.h "pixel normalisation"): the
// kernels behind layers.PixelNormalization in the generator -- forward (LeakyReLU + PixelNorm) and backward (through both).  Data is
// [R, C]: R rows of C contiguous channels; the one statistic is a mean over ONE row, so rows are independent and the kernels are
// pure streaming.  No parameters, no column sums, no workspace, no LDS, no atomics: two runs give the same bits.
//
// Per row, with the mean over the row's C channels:  a = LeakyReLU(x),  r = 1 / sqrt(mean(a^2) + eps)  (saved by the forward where
// a backward follows),  y = a * r;  the Jacobian of a -> y is r * (I - y y^T / C), and r > 0 gives sign(y) = sign(x): the backward
// reads LeakyReLU's branch from the stored output and never sees x.
//
// Routes (bg_pixelnorm_route reports the ones a C takes) follow csrc/layernorm.hip's.  A row is read in units of one float4
// (C % 4 == 0 and every matrix of the call 16-byte aligned) or one float (anything else, a misaligned view included: no call is
// refused for its alignment): U = C / 4 or C units.  L = the power of two >= U, at most 64, lanes share a row, so a wave holds
// 64 / L rows; with U > 64 each lane keeps 2 or 4 units (U <= 128, U <= 256).  Up to there a row is read ONCE and stays in
// registers between its sum and its use.  Beyond (U > 256: C > 1024, or C > 256 by single floats) the row is cut into chunks of 64
// units, one per lane, along gridDim.y: a workgroup sweeps the whole row from memory for the sum (the re-read hits L2) and keeps
// only its own chunk in registers.  A workgroup is 4 waves = 4 * 64 / L rows per visit, in a grid-stride loop over at most 1024
// workgroups.  A row's sum is each lane's units in index order, then a fixed butterfly over the lanes that share it.
#include "common.h"
#include <algorithm>

namespace {

constexpr int kT = 256, kWaves = kT / 64, kMaxBlocks = 1024, kChunkUnits = 64;

struct Route { int vec, lg, nv, chunks; };

inline Route route_for(int C, bool aligned = true) {
  Route t;
  t.vec = C % 4 == 0 && aligned ? 4 : 1;
  const int U = C / t.vec;
  t.lg = 0;
  while ((1 << t.lg) < U && t.lg < 6) ++t.lg;
  const int per = (U + 63) / 64;
  t.nv = per <= 1 ? 1 : per <= 2 ? 2 : 4;
  t.chunks = per <= 4 ? 1 : (U + kChunkUnits - 1) / kChunkUnits;
  if (t.chunks > 1) t.nv = 1;
  return t;
}

struct Geo { int R, C, U, lg; };

// the units one lane holds of one row: unit base + j * L + sub for j < NV (zeros where unit_ok says there is none)
template <int VEC, int NV>
struct Tile {
  float v[NV][VEC];
};

template <int VEC>
__device__ __forceinline__ void load_unit(const float* p, size_t unit, float (&d)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 t = reinterpret_cast<const float4*>(p)[unit];
    d[0] = t.x; d[1] = t.y; d[2] = t.z; d[3] = t.w;
  } else {
    d[0] = p[unit];
  }
}

template <int VEC>
__device__ __forceinline__ void store_unit(float* p, size_t unit, const float (&d)[VEC]) {
  if constexpr (VEC == 4) reinterpret_cast<float4*>(p)[unit] = make_float4(d[0], d[1], d[2], d[3]);
  else p[unit] = d[0];
}

// where one lane stands in one visit of its workgroup
struct Pos {
  int L, sub, U;
  size_t row, unit0;      // unit0: index of the row's first unit in the matrix
  bool row_ok;
};

__device__ __forceinline__ bool unit_ok(const Pos& q, int base, int j) { return q.row_ok && base + j * q.L + q.sub < q.U; }

// no __restrict__ on the sources: the output may alias one of them on the register routes
template <int VEC, int NV>
__device__ __forceinline__ Tile<VEC, NV> load_tile(const float* p, const Pos& q, int base) {
  Tile<VEC, NV> t;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) t.v[j][e] = 0.f;
    if (unit_ok(q, base, j)) load_unit<VEC>(p, q.unit0 + base + j * q.L + q.sub, t.v[j]);
  }
  return t;
}

// sum over the lanes that share a row (L a power of two, groups aligned to L: the butterfly never leaves the group)
__device__ __forceinline__ float group_sum(float v, int L) {
  for (int o = L >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float lrelu(float x, float alpha) { return x > 0.f ? x : alpha * x; }

#define PN_POS_SETUP()                                                                                   \
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, rpw = 64 >> g.lg;                          \
  const int base = LOOP ? (int)blockIdx.y * 64 * NV : 0;                                                 \
  const size_t groups = ((size_t)g.R + (size_t)rpw * kWaves - 1) / ((size_t)rpw * kWaves);               \
  const float Cf = (float)g.C;                                                                           \
  Pos q;                                                                                                \
  q.L = LOOP ? 64 : 1 << g.lg; /* the chunked route spreads a row over the whole wave */                 \
  q.sub = lane & (q.L - 1);                                                                              \
  q.U = g.U

#define PN_ROW_SETUP()                                                      \
  q.row = (rg * kWaves + wave) * (size_t)rpw + (size_t)(lane >> g.lg);      \
  q.row_ok = q.row < (size_t)g.R;                                           \
  q.unit0 = q.row * (size_t)g.U

// y = a * r with a = LeakyReLU(x), r = 1 / sqrt(mean(a^2) + eps); saves r where rs != NULL.  (A unit that does not exist is zeros
// and adds nothing to the sum of squares.)
template <int VEC, int NV, bool LOOP>
__global__ __launch_bounds__(kT) void pn_fwd_kernel(const float* x, float* y, Geo g, float eps, float alpha, float* __restrict__ rs) {
  PN_POS_SETUP();
  for (size_t rg = blockIdx.x; rg < groups; rg += gridDim.x) {
    PN_ROW_SETUP();
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
  PN_POS_SETUP();
  for (size_t rg = blockIdx.x; rg < groups; rg += gridDim.x) {
    PN_ROW_SETUP();
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

inline Geo geo_for(int R, int C, const Route& t) { return Geo{R, C, C / t.vec, t.lg}; }

inline dim3 grid_for(int R, const Route& t) {
  const size_t rows_wg = (size_t)kWaves * (64 >> t.lg);
  const size_t groups = ((size_t)R + rows_wg - 1) / rows_wg;
  return dim3((unsigned)std::min<size_t>(groups, kMaxBlocks), (unsigned)t.chunks);
}

#define PN_LAUNCH(KERN, t, grid, s, ...)                                                                  \
  do {                                                                                                    \
    if (t.chunks > 1) {                                                                                   \
      if (t.vec == 4) bg::launch(KERN<4, 1, true>, grid, dim3(kT), 0, s, __VA_ARGS__);                    \
      else bg::launch(KERN<1, 1, true>, grid, dim3(kT), 0, s, __VA_ARGS__);                               \
    } else if (t.vec == 4) {                                                                              \
      if (t.nv == 1) bg::launch(KERN<4, 1, false>, grid, dim3(kT), 0, s, __VA_ARGS__);                    \
      else if (t.nv == 2) bg::launch(KERN<4, 2, false>, grid, dim3(kT), 0, s, __VA_ARGS__);               \
      else bg::launch(KERN<4, 4, false>, grid, dim3(kT), 0, s, __VA_ARGS__);                              \
    } else {                                                                                              \
      if (t.nv == 1) bg::launch(KERN<1, 1, false>, grid, dim3(kT), 0, s, __VA_ARGS__);                    \
      else if (t.nv == 2) bg::launch(KERN<1, 2, false>, grid, dim3(kT), 0, s, __VA_ARGS__);               \
      else bg::launch(KERN<1, 4, false>, grid, dim3(kT), 0, s, __VA_ARGS__);                              \
    }                                                                                                     \
  } while (0)

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
  PN_LAUNCH(pn_fwd_kernel, t, grid, L.s, x, y, geo_for(R, C, t), eps, lrelu_alpha, r);
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
  PN_LAUNCH(pn_bwd_kernel, t, grid, L.s, g, y, r, dz, geo_for(R, C, t), lrelu_alpha);
  return L.done("pn_bwd_kernel");
}

}  // extern "C"
