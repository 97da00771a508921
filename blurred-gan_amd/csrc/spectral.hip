// Spectral normalisation (include/bgan.h "spectral normalisation"): W-bar = W / sigma with sigma from a running power iteration.
//
// Every entry point is batched over all wrapped layers of one model: a device table of bg_spectral_desc-shaped rows (16 ints per
// layer: float offsets into the theta / state / effective-weight / workspace bases, K, N, taps and the layer's first work unit in
// each of the three unit numberings) tells a workgroup which matrix it works on, so the number of launches does not depend on the
// number of layers.  How a matrix is cut into units depends on (K, N, taps) alone (sn_route), so a batched launch computes bit
// for bit what per-layer launches compute.  fp32 throughout, no atomics, no hand-off between workgroups inside a launch: partial
// sums go to the workspace and a dependent launch adds them in a fixed order.
//
//   power   pass kernel:   t = W u one row strip per workgroup, s_partial = sum_r t_r W[r, :] from the rows still in registers,
//                          ||t||^2 partial (sigma-only: v . t partial), raw t into v
//           finish kernel: one workgroup per layer: v = t / ||t||, s = W^T v, u = s / ||s||, sigma = s . u
//   scale   W-bar = W / sigma into the effective buffer, and (conv layers) its [taps][N][R] transposed copy from the same tile
//   grad    dot kernel:    <g, W-bar> as per-workgroup partials
//           apply kernel:  g <- (g - <g, W-bar> v u^T) / sigma in place, every workgroup adding the partials itself
#include "common.h"

namespace {

struct SnDesc { int w_off, u_off, v_off, sigma_off, eff_off, tr_off, K, N, taps, pass_first, ew_first, tile_first, ws_off, pad0, pad1, pad2; };
static_assert(sizeof(SnDesc) == BG_SPECTRAL_DESC_INTS * sizeof(int), "descriptor row");

constexpr int kEwElems = 16384;       // elements of one dot / apply unit: 256 threads x 16 float4
constexpr int kWideStrip = 4;         // rows of a wide-route unit: one per wave
constexpr float kNormEps = 1e-12f;    // normalize(x) = x / max(||x||, 1e-12)

// How a [K, N] matrix is laid over waves and cut into units.  Packed route (chunks >= 1): a row's N / vec vectors lie over `lanes`
// lanes (a power of two), 64 / lanes rows share a wave, each lane holds `chunks` vectors of its row.  Wide route (chunks == 0): a
// wave strides over its row, and the strip's second sweep, for s, re-reads the four rows from cache.
struct SnRoute { int vec, lanes, chunks, strip, pass_units, ew_units, tiles; };

__host__ __device__ inline SnRoute sn_route(int K, int N, int taps) {
  SnRoute r;
  r.vec = (N % 4 == 0) ? 4 : 1;
  const int cols = N / r.vec;
  if (cols <= 64) {
    r.lanes = 1;
    while (r.lanes < cols) r.lanes <<= 1;
    r.chunks = 1;
  } else if (r.vec == 4 && cols <= 128) {
    r.lanes = 64;
    r.chunks = 2;
  } else {
    r.lanes = 64;
    r.chunks = 0;
  }
  r.strip = r.chunks ? 4 * (64 / r.lanes) * 16 : kWideStrip;
  r.pass_units = (K + r.strip - 1) / r.strip;
  r.ew_units = (int)(((long long)K * N + kEwElems - 1) / kEwElems);
  const int R = K / (taps > 0 ? taps : 1);
  r.tiles = taps * ((R + 63) / 64) * ((N + 63) / 64);
  return r;
}

__host__ __device__ inline int pad4(int n) { return (n + 3) & ~3; }
// workspace of one layer, in floats: [pass_units][N] partial s | [pass_units] partial ||t||^2 | [ew_units] partial <g, W-bar>
__host__ __device__ inline int sn_ws_tt(const SnRoute& r, int N) { return pad4(r.pass_units * N); }
__host__ __device__ inline int sn_ws_dot(const SnRoute& r, int N) { return sn_ws_tt(r, N) + pad4(r.pass_units); }
__host__ __device__ inline long long sn_ws_floats(const SnRoute& r, int N) { return (long long)sn_ws_dot(r, N) + pad4(r.ew_units); }

__device__ inline int find_layer(const SnDesc* __restrict__ desc, int n, int first_field, int unit) {
  int e = 0;          // workgroup-uniform scan of a short table
  while (e + 1 < n && reinterpret_cast<const int*>(desc + e + 1)[first_field] <= unit) ++e;
  return e;
}

__device__ inline float wave_sum(float x) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) x += __shfl_xor(x, o, 64);
  return x;
}

// Sum over the workgroup's 256 threads in a fixed order; every thread gets it.  red: 4 floats of LDS.
// Not reduce.h's block_sum, and not to be replaced by it: the butterfly runs in ascending offsets, the waves add as
// ((r0 + r1) + r2) + r3, and the second barrier FOLLOWS the read because the callers write red again at once.
__device__ inline float block_sum(float x, float* red) {
  x = wave_sum(x);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  const float s = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return s;
}

// The same over the finish kernel's 1024 threads.  red: 16 floats of LDS.
__device__ inline float block_sum16(float x, float* red) {
  x = wave_sum(x);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int w = 1; w < 16; ++w) s += red[w];
  __syncthreads();
  return s;
}

template <int VEC>
__device__ inline void load_vec(const float* p, float* x) {
  if constexpr (VEC == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
  } else {
    x[0] = *p;
  }
}

// ---- power iteration, packed route
template <int VEC, int CH>
__device__ inline void pass_packed(const float* __restrict__ W, const float* u, const float* v_in, float* v_out, float* __restrict__ s_part,
                                   float* __restrict__ tt_part, int K, int N, int L, int strip, int unit, bool sigma_only, float* lds_s,
                                   float* red) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sub = lane & (L - 1), G = 64 / L, grp = lane / L;
  const int cols = N / VEC;
  float uu[CH * VEC], s[CH * VEC];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int vidx = sub + c * 64;
#pragma unroll
    for (int j = 0; j < VEC; ++j) { uu[c * VEC + j] = 0.f; s[c * VEC + j] = 0.f; }
    if (vidx < cols) load_vec<VEC>(u + vidx * VEC, uu + c * VEC);
  }
  const int r0 = unit * strip, r1 = min(K, r0 + strip);
  float acc = 0.f;
  for (int rb = r0; rb < r1; rb += 4 * G) {
    const int r = rb + wave * G + grp;
    const bool live = r < r1;
    float w[CH * VEC];
    float t = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int vidx = sub + c * 64;
#pragma unroll
      for (int j = 0; j < VEC; ++j) w[c * VEC + j] = 0.f;
      if (live && vidx < cols) load_vec<VEC>(W + (size_t)r * N + vidx * VEC, w + c * VEC);
#pragma unroll
      for (int j = 0; j < VEC; ++j) t += w[c * VEC + j] * uu[c * VEC + j];
    }
    for (int o = 1; o < L; o <<= 1) t += __shfl_xor(t, o, 64);       // the L lanes of a row
    if (live) {
      if (!sigma_only) {
#pragma unroll
        for (int j = 0; j < CH * VEC; ++j) s[j] += t * w[j];
      }
      if (sub == 0) {
        if (sigma_only) acc += v_in[r] * t;
        else { v_out[r] = t; acc += t * t; }
      }
    }
  }
  const float a = block_sum(acc, red);
  if (tid == 0) tt_part[unit] = a;
  if (sigma_only) return;
  for (int o = L; o < 64; o <<= 1) {           // the rows that share a wave
#pragma unroll
    for (int j = 0; j < CH * VEC; ++j) s[j] += __shfl_xor(s[j], o, 64);
  }
  if (grp == 0) {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int vidx = sub + c * 64;
      if (vidx < cols) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) lds_s[wave * N + vidx * VEC + j] = s[c * VEC + j];
      }
    }
  }
  __syncthreads();
  for (int c = tid; c < N; c += 256)
    s_part[(size_t)unit * N + c] = ((lds_s[c] + lds_s[N + c]) + lds_s[2 * N + c]) + lds_s[3 * N + c];
}

// ---- power iteration, wide route: wave w owns row r0 + w of the strip
template <int VEC>
__device__ inline void pass_wide(const float* __restrict__ W, const float* u, const float* v_in, float* v_out, float* __restrict__ s_part,
                                 float* __restrict__ tt_part, int K, int N, int unit, bool sigma_only, float* lds_t) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cols = N / VEC;
  const int r0 = unit * kWideStrip, r1 = min(K, r0 + kWideStrip);
  const int r = r0 + wave;
  float t = 0.f;
  if (r < r1) {
    for (int vidx = lane; vidx < cols; vidx += 64) {
      float w[VEC], x[VEC];
      load_vec<VEC>(W + (size_t)r * N + vidx * VEC, w);
      load_vec<VEC>(u + vidx * VEC, x);
#pragma unroll
      for (int j = 0; j < VEC; ++j) t += w[j] * x[j];
    }
  }
  t = wave_sum(t);
  if (lane == 0) {
    lds_t[wave] = t;
    if (r < r1 && !sigma_only) v_out[r] = t;
  }
  __syncthreads();
  if (tid == 0) {
    float acc = 0.f;
    for (int w = 0; w < kWideStrip; ++w)
      if (r0 + w < r1) acc += sigma_only ? v_in[r0 + w] * lds_t[w] : lds_t[w] * lds_t[w];
    tt_part[unit] = acc;
  }
  if (sigma_only) return;
  for (int vidx = tid; vidx < cols; vidx += 256) {
    float s[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) s[j] = 0.f;
#pragma unroll
    for (int w = 0; w < kWideStrip; ++w) {
      if (r0 + w < r1) {
        float x[VEC];
        load_vec<VEC>(W + (size_t)(r0 + w) * N + vidx * VEC, x);
#pragma unroll
        for (int j = 0; j < VEC; ++j) s[j] += lds_t[w] * x[j];
      }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) s_part[(size_t)unit * N + vidx * VEC + j] = s[j];
  }
}

__global__ __launch_bounds__(256) void sn_pass_kernel(const float* __restrict__ theta, float* state, float* __restrict__ ws,
                                                      const SnDesc* __restrict__ desc, int n, int sigma_only) {
  __shared__ float lds_s[4 * 512];      // packed route: the four waves' partial s (N <= 512)
  __shared__ float red[4];
  const int e = find_layer(desc, n, 9, blockIdx.x);
  const SnDesc d = desc[e];
  const SnRoute rt = sn_route(d.K, d.N, d.taps);
  const int unit = blockIdx.x - d.pass_first;
  const float* W = theta + d.w_off;
  const float* u = state + d.u_off;
  float* v = state + d.v_off;
  float* s_part = ws + d.ws_off;
  float* tt_part = ws + d.ws_off + sn_ws_tt(rt, d.N);
  const bool so = sigma_only != 0;
  if (rt.chunks == 0) {
    if (rt.vec == 4) pass_wide<4>(W, u, v, v, s_part, tt_part, d.K, d.N, unit, so, red);
    else pass_wide<1>(W, u, v, v, s_part, tt_part, d.K, d.N, unit, so, red);
  } else if (rt.chunks == 2) {
    pass_packed<4, 2>(W, u, v, v, s_part, tt_part, d.K, d.N, rt.lanes, rt.strip, unit, so, lds_s, red);
  } else if (rt.vec == 4) {
    pass_packed<4, 1>(W, u, v, v, s_part, tt_part, d.K, d.N, rt.lanes, rt.strip, unit, so, lds_s, red);
  } else {
    pass_packed<1, 1>(W, u, v, v, s_part, tt_part, d.K, d.N, rt.lanes, rt.strip, unit, so, lds_s, red);
  }
}

// One workgroup of 1024 threads per layer, behind the pass kernel.  A column's partials are added eight at a time into eight
// accumulators (eight loads in flight: the loop is latency, not bytes) that are then added in a fixed order.
constexpr int kFinishThreads = 1024;

__global__ __launch_bounds__(kFinishThreads) void sn_finish_kernel(const float* __restrict__ ws, float* state, const SnDesc* __restrict__ desc,
                                                                   int sigma_only) {
  __shared__ float red[16];
  const SnDesc d = desc[blockIdx.x];
  const SnRoute rt = sn_route(d.K, d.N, d.taps);
  const int tid = threadIdx.x, N = d.N, P = rt.pass_units;
  const float* s_part = ws + d.ws_off;
  const float* tt_part = ws + d.ws_off + sn_ws_tt(rt, N);
  float* u = state + d.u_off;
  float* v = state + d.v_off;
  float a = 0.f;
  for (int i = tid; i < P; i += kFinishThreads) a += tt_part[i];
  const float T = block_sum16(a, red);
  if (sigma_only) {                       // sigma = v^T W u with the stored u and v
    if (tid == 0) state[d.sigma_off] = T;
    return;
  }
  const float nt = fmaxf(sqrtf(T), kNormEps);
  float ss = 0.f;
  for (int c = tid; c < N; c += kFinishThreads) {    // s = W^T v, kept in u until its norm is known
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int p = 0; p < P; p += 8) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (p + j < P) acc[j] += s_part[(size_t)(p + j) * N + c];
    }
    float s = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    s = s / nt;
    u[c] = s;
    ss += s * s;
  }
  const float ns = fmaxf(sqrtf(block_sum16(ss, red)), kNormEps);
  float sg = 0.f;
  for (int c = tid; c < N; c += kFinishThreads) {    // each thread re-reads what it wrote itself
    const float s = u[c];
    const float un = s / ns;
    u[c] = un;
    sg += s * un;
  }
  const float sigma = block_sum16(sg, red);
  if (tid == 0) state[d.sigma_off] = sigma;
  for (int r = tid; r < d.K; r += kFinishThreads) v[r] = v[r] / nt;
}

// W-bar = W / sigma, 64 x 64 tiles numbered [tap][r-tile][c-tile]; conv layers get the [taps][N][R] copy from the same tile.
__global__ __launch_bounds__(256) void sn_scale_kernel(const float* __restrict__ theta, const float* __restrict__ state, float* __restrict__ eff,
                                                       const SnDesc* __restrict__ desc, int n) {
  __shared__ float tile[64][65];
  const int e = find_layer(desc, n, 11, blockIdx.x);
  const SnDesc d = desc[e];
  const int R = d.K / d.taps, Cc = d.N;
  const int tr = (R + 63) / 64, tc = (Cc + 63) / 64;
  int local = blockIdx.x - d.tile_first;
  const int t = local / (tr * tc);
  local -= t * tr * tc;
  const int r0 = (local / tc) * 64, c0 = (local % tc) * 64;
  const float sigma = state[d.sigma_off];
  const float* s = theta + d.w_off + (size_t)t * R * Cc;
  float* o = eff + d.eff_off + (size_t)t * R * Cc;
  float* ot = d.tr_off >= 0 ? eff + d.tr_off + (size_t)t * R * Cc : nullptr;
  const int tid = threadIdx.x;
  if (((R | Cc) & 3) == 0) {
    const int q = tid & 15, rr = tid >> 4;                    // 16 float4 across 64 columns, 16 rows per pass
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = r0 + rr + 16 * i, c = c0 + 4 * q;
      if (r < R && c < Cc) {
        float4 x = *reinterpret_cast<const float4*>(s + (size_t)r * Cc + c);
        x.x = x.x / sigma; x.y = x.y / sigma; x.z = x.z / sigma; x.w = x.w / sigma;
        *reinterpret_cast<float4*>(o + (size_t)r * Cc + c) = x;
        tile[rr + 16 * i][4 * q] = x.x; tile[rr + 16 * i][4 * q + 1] = x.y; tile[rr + 16 * i][4 * q + 2] = x.z; tile[rr + 16 * i][4 * q + 3] = x.w;
      }
    }
    if (!ot) return;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = c0 + rr + 16 * i, r = r0 + 4 * q;
      if (c < Cc && r < R)
        *reinterpret_cast<float4*>(ot + (size_t)c * R + r) =
            make_float4(tile[4 * q][rr + 16 * i], tile[4 * q + 1][rr + 16 * i], tile[4 * q + 2][rr + 16 * i], tile[4 * q + 3][rr + 16 * i]);
    }
  } else {
    const int tx = tid & 63, ty = tid >> 6;
    for (int i = ty; i < 64; i += 4)
      if (r0 + i < R && c0 + tx < Cc) {
        const float x = s[(size_t)(r0 + i) * Cc + c0 + tx] / sigma;
        o[(size_t)(r0 + i) * Cc + c0 + tx] = x;
        tile[i][tx] = x;
      }
    if (!ot) return;
    __syncthreads();
    for (int i = ty; i < 64; i += 4)
      if (c0 + i < Cc && r0 + tx < R) ot[(size_t)(c0 + i) * R + r0 + tx] = tile[tx][i];
  }
}

// <g, W-bar> of one 16384-element unit.  The bases and the unit's first element are multiples of four floats, so float4 whatever N.
__global__ __launch_bounds__(256) void sn_dot_kernel(const float* __restrict__ grad, const float* __restrict__ eff, float* __restrict__ ws,
                                                     const SnDesc* __restrict__ desc, int n) {
  __shared__ float red[4];
  const int e = find_layer(desc, n, 10, blockIdx.x);
  const SnDesc d = desc[e];
  const SnRoute rt = sn_route(d.K, d.N, d.taps);
  const int unit = blockIdx.x - d.ew_first;
  const int total = d.K * d.N;
  const float* g = grad + d.w_off;
  const float* w = eff + d.eff_off;
  float acc = 0.f;
#pragma unroll 4
  for (int it = 0; it < kEwElems / 1024; ++it) {
    const int i = unit * kEwElems + (it * 256 + (int)threadIdx.x) * 4;
    if (i + 3 < total) {
      const float4 a = *reinterpret_cast<const float4*>(g + i), b = *reinterpret_cast<const float4*>(w + i);
      acc += ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w;
    } else {
      for (int j = i; j < total; ++j) acc += g[j] * w[j];
    }
  }
  const float a = block_sum(acc, red);
  if (threadIdx.x == 0) ws[d.ws_off + sn_ws_dot(rt, d.N) + unit] = a;
}

__global__ __launch_bounds__(256) void sn_apply_kernel(float* __restrict__ grad, const float* __restrict__ state, const float* __restrict__ ws,
                                                       const SnDesc* __restrict__ desc, int n) {
  __shared__ float red[4];
  const int e = find_layer(desc, n, 10, blockIdx.x);
  const SnDesc d = desc[e];
  const SnRoute rt = sn_route(d.K, d.N, d.taps);
  const int unit = blockIdx.x - d.ew_first;
  const int total = d.K * d.N, N = d.N;
  const float* part = ws + d.ws_off + sn_ws_dot(rt, N);
  float a = 0.f;
  for (int i = threadIdx.x; i < rt.ew_units; i += 256) a += part[i];
  const float dot = block_sum(a, red);
  const float sigma = state[d.sigma_off];
  const float* u = state + d.u_off;
  const float* v = state + d.v_off;
  float* g = grad + d.w_off;
#pragma unroll 4
  for (int it = 0; it < kEwElems / 1024; ++it) {
    const int i = unit * kEwElems + (it * 256 + (int)threadIdx.x) * 4;
    if (i + 3 < total) {
      float4 x = *reinterpret_cast<const float4*>(g + i);
      const int r = i / N, c = i - r * N;
      int rr[4], cc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int cj = c + j, rj = r;
        while (cj >= N) { cj -= N; ++rj; }
        rr[j] = rj; cc[j] = cj;
      }
      x.x = (x.x - (dot * v[rr[0]]) * u[cc[0]]) / sigma;
      x.y = (x.y - (dot * v[rr[1]]) * u[cc[1]]) / sigma;
      x.z = (x.z - (dot * v[rr[2]]) * u[cc[2]]) / sigma;
      x.w = (x.w - (dot * v[rr[3]]) * u[cc[3]]) / sigma;
      *reinterpret_cast<float4*>(g + i) = x;
    } else {
      for (int j = i; j < total; ++j) {
        const int r = j / N, c = j - r * N;
        g[j] = (g[j] - (dot * v[r]) * u[c]) / sigma;
      }
    }
  }
}

// ---- host side
struct Plan { int pass_units, ew_units, tiles; long long ws_floats; };

// Checks the host copy of the table; fills the launch sizes.  Nothing touches the device before this has passed.
int check_table(const char* who, const int* desc_h, int n, Plan* plan) {
  BG_REQUIRE(desc_h, BG_ERR_NULL, "%s: null descriptor table", who);
  BG_REQUIRE(n > 0, BG_ERR_BAD_SHAPE, "%s: n=%d layers", who, n);
  const SnDesc* d = reinterpret_cast<const SnDesc*>(desc_h);
  Plan p = {0, 0, 0, 0};
  for (int e = 0; e < n; ++e) {
    BG_REQUIRE(d[e].K > 0 && d[e].N > 0, BG_ERR_BAD_SHAPE, "%s: layer %d: K=%d N=%d", who, e, d[e].K, d[e].N);
    BG_REQUIRE(d[e].taps > 0 && d[e].K % d[e].taps == 0, BG_ERR_BAD_SHAPE, "%s: layer %d: taps=%d does not divide K=%d", who, e, d[e].taps, d[e].K);
    BG_REQUIRE((long long)d[e].K * d[e].N < (1ll << 30), BG_ERR_BAD_SHAPE, "%s: layer %d: K*N too large", who, e);
    BG_REQUIRE(d[e].w_off >= 0 && d[e].u_off >= 0 && d[e].v_off >= 0 && d[e].sigma_off >= 0 && d[e].eff_off >= 0 && d[e].ws_off >= 0 && d[e].tr_off >= -1,
               BG_ERR_BAD_SHAPE, "%s: layer %d: negative offset", who, e);
    BG_REQUIRE(((d[e].w_off | d[e].u_off | d[e].v_off | d[e].eff_off | d[e].ws_off) & 3) == 0 && (d[e].tr_off < 0 || (d[e].tr_off & 3) == 0),
               BG_ERR_BAD_ALIGNMENT, "%s: layer %d: offsets must be multiples of 4 floats", who, e);
    BG_REQUIRE(d[e].pass_first == p.pass_units && d[e].ew_first == p.ew_units && d[e].tile_first == p.tiles, BG_ERR_BAD_SHAPE,
               "%s: layer %d: first units (%d, %d, %d) do not continue the table (%d, %d, %d)", who, e, d[e].pass_first, d[e].ew_first,
               d[e].tile_first, p.pass_units, p.ew_units, p.tiles);
    const SnRoute rt = sn_route(d[e].K, d[e].N, d[e].taps);
    p.pass_units += rt.pass_units;
    p.ew_units += rt.ew_units;
    p.tiles += rt.tiles;
    const long long end = d[e].ws_off + sn_ws_floats(rt, d[e].N);
    if (end > p.ws_floats) p.ws_floats = end;
  }
  *plan = p;
  return BG_OK;
}

}  // namespace

extern "C" {

int bg_spectral_route(int K, int N, int taps, int* vec, int* lanes, int* chunks, int* strip_rows, int* pass_units, int* ew_units, int* tiles,
                      int* ws_floats) {
  BG_REQUIRE(K > 0 && N > 0 && taps > 0 && K % taps == 0 && (long long)K * N < (1ll << 30), BG_ERR_BAD_SHAPE, "bg_spectral_route: K=%d N=%d taps=%d", K, N, taps);
  const SnRoute r = sn_route(K, N, taps);
  if (vec) *vec = r.vec;
  if (lanes) *lanes = r.lanes;
  if (chunks) *chunks = r.chunks;
  if (strip_rows) *strip_rows = r.strip;
  if (pass_units) *pass_units = r.pass_units;
  if (ew_units) *ew_units = r.ew_units;
  if (tiles) *tiles = r.tiles;
  if (ws_floats) *ws_floats = (int)sn_ws_floats(r, N);
  return BG_OK;
}

size_t bg_spectral_workspace_bytes(const int* desc_h, int n) {
  Plan p;
  if (check_table("bg_spectral_workspace_bytes", desc_h, n, &p)) return 0;
  return (size_t)p.ws_floats * sizeof(float);
}

int bg_spectral_power_f32(const float* theta, float* state, const int* desc_d, const int* desc_h, int n, int sigma_only, float* ws,
                          size_t ws_bytes, void* stream) {
  BG_REQUIRE(theta && state && desc_d && ws, BG_ERR_NULL, "bg_spectral_power_f32: null pointer");
  Plan p;
  if (int rc = check_table("bg_spectral_power_f32", desc_h, n, &p)) return rc;
  BG_REQUIRE(bg::aligned16(theta) && bg::aligned16(state) && bg::aligned16(ws) && bg::aligned16(desc_d), BG_ERR_BAD_ALIGNMENT,
             "bg_spectral_power_f32: bases must be 16-byte aligned");
  BG_REQUIRE(ws_bytes >= (size_t)p.ws_floats * sizeof(float), BG_ERR_WORKSPACE, "bg_spectral_power_f32: workspace %zu < %zu bytes", ws_bytes,
             (size_t)p.ws_floats * sizeof(float));
  const SnDesc* dd = reinterpret_cast<const SnDesc*>(desc_d);
  {
    double bytes = 0;
    const SnDesc* h = reinterpret_cast<const SnDesc*>(desc_h);
    for (int e = 0; e < n; ++e) bytes += 4.0 * h[e].K * h[e].N;
    bg::Launch L(stream, sigma_only ? "spectral_sigma" : "spectral_power", 0, bytes);
    bg::launch(sn_pass_kernel, dim3((unsigned)p.pass_units), dim3(256), 0, L.s, theta, state, ws, dd, n, sigma_only);
    if (int rc = L.done("sn_pass_kernel")) return rc;
  }
  bg::Launch L(stream, "spectral_finish", 0, 0);
  bg::launch(sn_finish_kernel, dim3((unsigned)n), dim3(kFinishThreads), 0, L.s, (const float*)ws, state, dd, sigma_only);
  return L.done("sn_finish_kernel");
}

int bg_spectral_scale_f32(const float* theta, const float* state, float* eff, const int* desc_d, const int* desc_h, int n, void* stream) {
  BG_REQUIRE(theta && state && eff && desc_d, BG_ERR_NULL, "bg_spectral_scale_f32: null pointer");
  Plan p;
  if (int rc = check_table("bg_spectral_scale_f32", desc_h, n, &p)) return rc;
  BG_REQUIRE(bg::aligned16(theta) && bg::aligned16(state) && bg::aligned16(eff) && bg::aligned16(desc_d), BG_ERR_BAD_ALIGNMENT,
             "bg_spectral_scale_f32: bases must be 16-byte aligned");
  double bytes = 0;
  const SnDesc* h = reinterpret_cast<const SnDesc*>(desc_h);
  for (int e = 0; e < n; ++e) bytes += (h[e].tr_off >= 0 ? 12.0 : 8.0) * h[e].K * h[e].N;
  bg::Launch L(stream, "spectral_scale", 0, bytes);
  bg::launch(sn_scale_kernel, dim3((unsigned)p.tiles), dim3(256), 0, L.s, theta, state, eff, reinterpret_cast<const SnDesc*>(desc_d), n);
  return L.done("sn_scale_kernel");
}

int bg_spectral_grad_f32(float* grad, const float* eff, const float* state, const int* desc_d, const int* desc_h, int n, float* ws,
                         size_t ws_bytes, void* stream) {
  BG_REQUIRE(grad && eff && state && desc_d && ws, BG_ERR_NULL, "bg_spectral_grad_f32: null pointer");
  Plan p;
  if (int rc = check_table("bg_spectral_grad_f32", desc_h, n, &p)) return rc;
  BG_REQUIRE(bg::aligned16(grad) && bg::aligned16(eff) && bg::aligned16(state) && bg::aligned16(ws) && bg::aligned16(desc_d), BG_ERR_BAD_ALIGNMENT,
             "bg_spectral_grad_f32: bases must be 16-byte aligned");
  BG_REQUIRE(ws_bytes >= (size_t)p.ws_floats * sizeof(float), BG_ERR_WORKSPACE, "bg_spectral_grad_f32: workspace %zu < %zu bytes", ws_bytes,
             (size_t)p.ws_floats * sizeof(float));
  const SnDesc* dd = reinterpret_cast<const SnDesc*>(desc_d);
  double elems = 0;
  const SnDesc* h = reinterpret_cast<const SnDesc*>(desc_h);
  for (int e = 0; e < n; ++e) elems += (double)h[e].K * h[e].N;
  {
    bg::Launch L(stream, "spectral_dot", 0, 8.0 * elems);
    bg::launch(sn_dot_kernel, dim3((unsigned)p.ew_units), dim3(256), 0, L.s, (const float*)grad, eff, ws, dd, n);
    if (int rc = L.done("sn_dot_kernel")) return rc;
  }
  bg::Launch L(stream, "spectral_apply", 0, 8.0 * elems);
  bg::launch(sn_apply_kernel, dim3((unsigned)p.ew_units), dim3(256), 0, L.s, grad, state, (const float*)ws, dd, n);
  return L.done("sn_apply_kernel");
}

}  // extern "C"
