// How a row of an [R, C] fp32 matrix (R rows of C contiguous channels) is laid over a wave: the routes, the register tile and the
// launch geometry of the kernels that take one statistic per row (layernorm.hip, pixelnorm.hip).  A new row-statistic kernel
// starts from this header; what it computes on a tile stays in its own file.
//
// Routes (route_for).  A row is read in units of one float4 (C % 4 == 0, and where the caller says so only when every matrix of
// the call is 16-byte aligned) or one float (anything else): U = C / 4 or C units.  L = the power of two >= U, at most 64, lanes
// share a row, so a wave holds 64 / L rows; with U > 64 each lane keeps nv = 2 or 4 units (U <= 128, U <= 256).  Up to there a row
// is read ONCE and stays in registers between its statistics and its use.  Beyond (U > 256: C > 1024, or C > 256 by single floats)
// the row is cut into chunks of 64 units, one per lane, along gridDim.y: a workgroup sweeps the whole row from memory for the
// statistics (the re-read hits L2) and keeps only its own chunk in registers.  (One unit per lane there: with more, the sweeps'
// address and mask bookkeeping no longer fits the scalar registers.)  A workgroup is 4 waves = 4 * 64 / L rows per visit, in a
// grid-stride loop over at most 1024 workgroups.  A row's sum is each lane's units in index order, then a fixed butterfly over the
// lanes that share it (group_sum).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>

namespace bg {
namespace rowwise {

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

inline Geo geo_for(int R, int C, const Route& t) { return Geo{R, C, C / t.vec, t.lg}; }

inline dim3 grid_for(int R, const Route& t) {
  const size_t rows_wg = (size_t)kWaves * (64 >> t.lg);
  const size_t groups = ((size_t)R + rows_wg - 1) / rows_wg;
  return dim3((unsigned)std::min<size_t>(groups, kMaxBlocks), (unsigned)t.chunks);
}

// A route's template arguments as a type, and f(Lanes<VEC, NV, LOOP>()) for the route t: the one place that turns a Route into a
// kernel instance.  f is a generic lambda that launches KERN<..., Rt::VEC, Rt::NV, Rt::LOOP> with Rt = decltype of its argument.
template <int V, int N, bool CHUNKED>
struct Lanes {
  static constexpr int VEC = V, NV = N;
  static constexpr bool LOOP = CHUNKED;
};

template <class F>
inline void for_route(const Route& t, F f) {
  if (t.chunks > 1) {
    if (t.vec == 4) f(Lanes<4, 1, true>());
    else f(Lanes<1, 1, true>());
  } else if (t.vec == 4) {
    if (t.nv == 1) f(Lanes<4, 1, false>());
    else if (t.nv == 2) f(Lanes<4, 2, false>());
    else f(Lanes<4, 4, false>());
  } else {
    if (t.nv == 1) f(Lanes<1, 1, false>());
    else if (t.nv == 2) f(Lanes<1, 2, false>());
    else f(Lanes<1, 4, false>());
  }
}

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

// keep bytes of one unit, one per element (nonzero = kept)
template <int VEC>
__device__ __forceinline__ void load_keep(const uint8_t* __restrict__ k, size_t unit, unsigned (&d)[VEC]) {
  if constexpr (VEC == 4) {
    const uint32_t w = reinterpret_cast<const uint32_t*>(k)[unit];
    d[0] = w & 0xffu; d[1] = (w >> 8) & 0xffu; d[2] = (w >> 16) & 0xffu; d[3] = w >> 24;
  } else {
    d[0] = k[unit];
  }
}

// where one lane stands in one visit of its workgroup
struct Pos {
  int L, sub, U;
  size_t row, unit0;      // unit0: index of the row's first unit in the matrix
  bool row_ok;
};

// whether unit j of the tile at ``base`` exists: inside the row, in a row of the matrix.  Recomputed wherever it is needed (a
// compare) rather than kept: a kept flag per unit is a lane mask in a scalar register pair
__device__ __forceinline__ bool unit_ok(const Pos& q, int base, int j) { return q.row_ok && base + j * q.L + q.sub < q.U; }

// no __restrict__ on the source: a kernel's output may alias it on the register routes
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

}  // namespace rowwise
}  // namespace bg

// Lane and row set-up of a kernel<..., NV, LOOP> with Geo g: ROWWISE_POS_SETUP() once, ROWWISE_ROW_SETUP() first thing in every visit
// of ``for (size_t rg = blockIdx.x; rg < groups; rg += gridDim.x)``.  They leave lane, wave, rpw (rows per wave), base (first unit of
// the workgroup's tile: its chunk on the chunked route), groups, Cf and the Pos q.  Macros, not functions: written as functions, the
// same statements left the compiler in another instruction order in most of layernorm.hip's kernels.
// (means are taken by true division by Cf: a row of equal values then has mean == the value, exactly)
#define ROWWISE_POS_SETUP()                                                                              \
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, rpw = 64 >> g.lg;                          \
  const int base = LOOP ? (int)blockIdx.y * 64 * NV : 0;                                                 \
  const size_t groups = ((size_t)g.R + (size_t)rpw * kWaves - 1) / ((size_t)rpw * kWaves);               \
  const float Cf = (float)g.C;                                                                           \
  Pos q;                                                                                                 \
  q.L = LOOP ? 64 : 1 << g.lg; /* the chunked route always spreads a row over the whole wave: a constant stride */ \
  q.sub = lane & (q.L - 1);                                                                              \
  q.U = g.U

#define ROWWISE_ROW_SETUP()                                                 \
  q.row = (rg * kWaves + wave) * (size_t)rpw + (size_t)(lane >> g.lg);      \
  q.row_ok = q.row < (size_t)g.R;                                           \
  q.unit0 = q.row * (size_t)g.U
