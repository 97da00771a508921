// Layer normalisation over the channel axis of NHWC fp32 maps (include/bgan.h "layer normalisation"): the kernels behind
// layers.LayerNormalization in the critic -- forward (+ LeakyReLU + Dropout), backward, the gradient penalty's tangent and its
// second-order source.  Data is [R, C]: R = B*H*W rows of C contiguous channels; every statistic is a mean over ONE row, so rows
// are independent and the kernels are pure streaming.
//
// Per row, with all means over the row's C channels: mu, r = 1/sqrt(var + eps) (biased variance; saved by the forward),
// xh = (z - mu) * r, and the Jacobian of z -> xh is the symmetric operator  M y = r * (yc - xh * mean(yc * xh)),  yc = y - mean(y).
//
// Routes (bg_ln_route reports the one a C takes): csrc/rowwise.h's, float4 units for every C % 4 == 0 (the entry points refuse a
// misaligned pointer there).  Up to 256 units a row is read ONCE and stays in registers between its statistics and its use, so an
// output may alias the input it replaces; on the chunked route beyond, the row is swept again and it may not.
//
// Column sums (dgamma, dbeta) are deterministic: each lane adds its own channels over the rows it visits, in visit order; the
// lanes of a wave that share a channel are folded by a fixed shuffle tree, the four waves through LDS in wave order, and one
// partial row per workgroup goes to the workspace; ln_finish_kernel adds the partial rows in a fixed order (64 strided lanes and
// a shuffle tree per channel).  No atomics: two runs give the same bits.  LDS holds that cross-wave scratch and nothing else.
#include "common.h"
#include "reduce.h"
#include "rowwise.h"

namespace {

using namespace bg::rowwise;

// body(tile, its base) over what feeds a row's statistics: the lane's own registers, or on the chunked route every chunk of the row
// from memory
template <bool LOOP, int NV, class T, class Load, class Body>
__device__ __forceinline__ void sweep(int U, const T& own, int base, Load load, Body body) {
  if constexpr (!LOOP) {
    body(own, base);
  } else {
    for (int b = 0; b < U; b += 64 * NV) body(load(b), b);
  }
}

// the forward's pre-activation, operation for operation: every kernel that needs LeakyReLU's branch re-derives it from z with this
// expression on the same inputs, so the branch is the forward's bit for bit (alpha >= 0) and the activation itself is never re-read
__device__ __forceinline__ float ln_pre(float z, float mu, float r, float g, float b) { return g * ((z - mu) * r) + b; }

// per-lane column accumulators -> one partial row of this workgroup: partial[(blockIdx.x * NQ + q) * C + c]
template <int VEC, int NV, int NQ>
__device__ __forceinline__ void write_partials(float (&acc)[NQ][NV][VEC], const Geo& g, int base, float* __restrict__ partial) {
  __shared__ float red[kWaves][NQ * NV * VEC][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, L = 1 << g.lg;
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        float v = acc[q][j][e];
        for (int o = 32; o >= L; o >>= 1) v += __shfl_xor(v, o, 64);      // the rows of this wave
        red[wave][(q * NV + j) * VEC + e][lane] = v;
      }
  __syncthreads();
  if (wave == 0 && lane < L) {
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const int u = base + j * L + lane;
        if (u < g.U) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            const int k = (q * NV + j) * VEC + e;
            float s = red[0][k][lane];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) s += red[w][k][lane];
            partial[((size_t)blockIdx.x * NQ + q) * g.C + (size_t)u * VEC + e] = s;
          }
        }
      }
  }
}

// a = Dropout(LeakyReLU(gamma * xh + beta)); saves mu, r
template <int MODE, int VEC, int NV, bool LOOP>
__global__ __launch_bounds__(kT) void ln_fwd_kernel(const float* __restrict__ z, float* __restrict__ a, Geo g,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                    float alpha, const uint8_t* __restrict__ keep, float kscale, size_t keep_rows,
                                                    float* __restrict__ mu, float* __restrict__ rs) {
  ROWWISE_POS_SETUP();
  for (size_t rg = blockIdx.x; rg < groups; rg += gridDim.x) {
    ROWWISE_ROW_SETUP();
    auto load = [&](int b) { return load_tile<VEC, NV>(z, q, b); };
    const Tile<VEC, NV> t = load(base);
    float s = 0.f;
    sweep<LOOP, NV>(g.U, t, base, load, [&](const Tile<VEC, NV>& x, int b) {
#pragma unroll
      for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e) s += x.v[j][e];
    });
    const float mean = group_sum(s, q.L) / Cf;
    float v = 0.f;
    sweep<LOOP, NV>(g.U, t, base, load, [&](const Tile<VEC, NV>& x, int b) {
#pragma unroll
      for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const float d = x.v[j][e] - mean;
          if (unit_ok(q, b, j)) v = fmaf(d, d, v);
        }
    });
    const float r = 1.f / sqrtf(group_sum(v, q.L) / Cf + eps);
    if (q.row_ok && q.sub == 0 && base == 0) {
      mu[q.row] = mean;
      rs[q.row] = r;
    }
    const bool masked = keep != nullptr && q.row < keep_rows;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      if (!unit_ok(q, base, j)) continue;
      const int u = base + j * q.L + q.sub;
      float gm[VEC], bt[VEC], o[VEC];
      unsigned kb[VEC];
      load_unit<VEC>(gamma, (size_t)u, gm);
      load_unit<VEC>(beta, (size_t)u, bt);
      if (masked) load_keep<VEC>(keep, q.unit0 + u, kb);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const float n = ln_pre(t.v[j][e], mean, r, gm[e], bt[e]);
        float y = n > 0.f ? n : alpha * n;
        if (masked) y = kb[e] ? y * kscale : 0.f;
        o[e] = y;
      }
      store_unit<VEC>(a, q.unit0 + u, o);
    }
  }
}

struct ApplyArgs {
  const float* src;        // MODE 0: the gradient at a; MODE 1: the tangent zdot
  const float* z;
  float* out;              // MODE 0: dz; MODE 1: vout
  const float *gamma, *beta, *mu, *rs;
  float alpha;
  const uint8_t* keep;     // MODE 0 only
  float kscale;
  size_t keep_rows;
  const float* addend;     // MODE 0: added to dz (may be NULL)
  float* u_out;            // MODE 0: u of rows [u_row0, u_row0 + u_rows) (may be NULL)
  size_t u_row0, u_rows;
  float* partial;          // MODE 0: column-sum partials of rows [0, dw_rows) (may be NULL)
  size_t dw_rows;
};

// MODE 0, backward:  u = g * LeakyReLU' * Dropout',  dz = M(gamma * u) [+ addend],  partials of sum u * xh and sum u
// MODE 1, tangent:   vout = LeakyReLU' * gamma * M(zdot)
template <int MODE, int VEC, int NV, bool LOOP>
__global__ __launch_bounds__(kT) void ln_apply_kernel(ApplyArgs A, Geo g) {
  ROWWISE_POS_SETUP();
  struct Pair { Tile<VEC, NV> z, u, y; };
  float acc[2][NV][VEC];
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[k][j][e] = 0.f;
  for (size_t rg = blockIdx.x; rg < groups; rg += gridDim.x) {
    ROWWISE_ROW_SETUP();
    const float mean = q.row_ok ? A.mu[q.row] : 0.f, r = q.row_ok ? A.rs[q.row] : 0.f;
    const bool masked = MODE == 0 && A.keep != nullptr && q.row < A.keep_rows;
    // y: the vector M is applied to.  The factor f = LeakyReLU' [* Dropout'] of an element is formed wherever it is needed
    auto factor = [&](float zv, float gm, float bt, unsigned kb) {
      float f = ln_pre(zv, mean, r, gm, bt) > 0.f ? 1.f : A.alpha;
      if (masked) f = kb ? f * A.kscale : 0.f;
      return f;
    };
    auto load = [&](int b) {
      Pair p;
      p.z = load_tile<VEC, NV>(A.z, q, b);
      p.y = load_tile<VEC, NV>(A.src, q, b);
      p.u = p.y;
      if constexpr (MODE == 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          if (!unit_ok(q, b, j)) continue;
          const int u = b + j * q.L + q.sub;
          float gm[VEC], bt[VEC];
          unsigned kb[VEC];
          load_unit<VEC>(A.gamma, (size_t)u, gm);
          load_unit<VEC>(A.beta, (size_t)u, bt);
#pragma unroll
          for (int e = 0; e < VEC; ++e) kb[e] = 0u;
          if (masked) load_keep<VEC>(A.keep, q.unit0 + u, kb);
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            p.u.v[j][e] = p.y.v[j][e] * factor(p.z.v[j][e], gm[e], bt[e], kb[e]);
            p.y.v[j][e] = gm[e] * p.u.v[j][e];
          }
        }
      }
      return p;
    };
    const Pair t = load(base);
    float s = 0.f;
    sweep<LOOP, NV>(g.U, t, base, load, [&](const Pair& x, int b) {
#pragma unroll
      for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e) s += x.y.v[j][e];
    });
    const float ybar = group_sum(s, q.L) / Cf;
    float c = 0.f;
    sweep<LOOP, NV>(g.U, t, base, load, [&](const Pair& x, int b) {
#pragma unroll
      for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e)
          if (unit_ok(q, b, j)) c = fmaf(x.y.v[j][e] - ybar, (x.z.v[j][e] - mean) * r, c);
    });
    const float m2 = group_sum(c, q.L) / Cf;
    const bool keep_u = MODE == 0 && A.u_out != nullptr && q.row >= A.u_row0 && q.row < A.u_row0 + A.u_rows;
    const bool sums = MODE == 0 && A.partial != nullptr && q.row < A.dw_rows;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      if (!unit_ok(q, base, j)) continue;
      const int u = base + j * q.L + q.sub;
      float o[VEC], ad[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) ad[e] = 0.f;
      if (MODE == 0 && A.addend != nullptr) load_unit<VEC>(A.addend, q.unit0 + u, ad);
      float gm[VEC], bt[VEC];
      if constexpr (MODE == 1) {
        load_unit<VEC>(A.gamma, (size_t)u, gm);
        load_unit<VEC>(A.beta, (size_t)u, bt);
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const float xh = (t.z.v[j][e] - mean) * r;
        const float my = r * ((t.y.v[j][e] - ybar) - xh * m2);
        if constexpr (MODE == 0) {
          o[e] = A.addend != nullptr ? my + ad[e] : my;
          if (sums) {
            acc[0][j][e] = fmaf(t.u.v[j][e], xh, acc[0][j][e]);
            acc[1][j][e] += t.u.v[j][e];
          }
        } else {
          o[e] = (factor(t.z.v[j][e], gm[e], bt[e], 0u) * gm[e]) * my;
        }
      }
      store_unit<VEC>(A.out, q.unit0 + u, o);
      if (keep_u) store_unit<VEC>(A.u_out, (q.row - A.u_row0) * (size_t)g.U + u, t.u.v[j]);
    }
  }
  if constexpr (MODE == 0) {
    if (A.partial != nullptr) write_partials<VEC, NV, 2>(acc, g, base, A.partial);
  }
}

// s = -r^2 * (p * Bq + q * A + xh * (D - 3 * A * Bq)) and the partials of sum u * M(zdot); the formulas stand at bg_ln_gp_source_f32
template <int MODE, int VEC, int NV, bool LOOP>
__global__ __launch_bounds__(kT) void ln_source_kernel(const float* __restrict__ u, const float* __restrict__ zdot,
                                                       const float* __restrict__ z, float* __restrict__ s_out, Geo g,
                                                       const float* __restrict__ gamma, const float* __restrict__ mu,
                                                       const float* __restrict__ rs, float* __restrict__ partial) {
  ROWWISE_POS_SETUP();
  struct Trio { Tile<VEC, NV> z, u, p, q; };      // p = gamma * u, q = zdot (both before centring)
  float acc[1][NV][VEC];
#pragma unroll
  for (int j = 0; j < NV; ++j)
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[0][j][e] = 0.f;
  for (size_t rg = blockIdx.x; rg < groups; rg += gridDim.x) {
    ROWWISE_ROW_SETUP();
    const float mean = q.row_ok ? mu[q.row] : 0.f, r = q.row_ok ? rs[q.row] : 0.f;
    auto load = [&](int b) {
      Trio t;
      t.z = load_tile<VEC, NV>(z, q, b);
      t.u = load_tile<VEC, NV>(u, q, b);
      t.q = load_tile<VEC, NV>(zdot, q, b);
      t.p = t.u;
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        if (!unit_ok(q, b, j)) continue;
        float gm[VEC];
        load_unit<VEC>(gamma, (size_t)(b + j * q.L + q.sub), gm);
#pragma unroll
        for (int e = 0; e < VEC; ++e) t.p.v[j][e] = gm[e] * t.u.v[j][e];
      }
      return t;
    };
    const Trio t = load(base);
    float sp = 0.f, sq = 0.f;
    sweep<LOOP, NV>(g.U, t, base, load, [&](const Trio& x, int b) {
#pragma unroll
      for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          sp += x.p.v[j][e];
          sq += x.q.v[j][e];
        }
    });
    const float pbar = group_sum(sp, q.L) / Cf, qbar = group_sum(sq, q.L) / Cf;
    float sa = 0.f, sb = 0.f, sd = 0.f;
    sweep<LOOP, NV>(g.U, t, base, load, [&](const Trio& x, int b) {
#pragma unroll
      for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e)
          if (unit_ok(q, b, j)) {
            const float xh = (x.z.v[j][e] - mean) * r, pc = x.p.v[j][e] - pbar, qc = x.q.v[j][e] - qbar;
            sa = fmaf(pc, xh, sa);
            sb = fmaf(qc, xh, sb);
            sd = fmaf(pc, qc, sd);
          }
    });
    const float Am = group_sum(sa, q.L) / Cf, Bq = group_sum(sb, q.L) / Cf, Dm = group_sum(sd, q.L) / Cf;
    const float tail = Dm - 3.f * Am * Bq, nr2 = -(r * r);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      if (!unit_ok(q, base, j)) continue;
      const int un = base + j * q.L + q.sub;
      float o[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const float xh = (t.z.v[j][e] - mean) * r, pc = t.p.v[j][e] - pbar, qc = t.q.v[j][e] - qbar;
        o[e] = nr2 * (pc * Bq + qc * Am + xh * tail);
        acc[0][j][e] = fmaf(t.u.v[j][e], r * (qc - xh * Bq), acc[0][j][e]);
      }
      store_unit<VEC>(s_out, q.unit0 + un, o);
    }
  }
  write_partials<VEC, NV, 1>(acc, g, base, partial);
}

// out_q[c] = beta * out_q[c] + scale * sum over the partial rows, in a fixed order: one wave per (q, c), lane l adds rows l, l + 64, ...
__global__ __launch_bounds__(kT) void ln_finish_kernel(const float* __restrict__ partial, int nblk, int C, int NQ, float* out0,
                                                       float* out1, float beta, float scale) {
  const int idx = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (idx >= NQ * C) return;
  const int qn = idx / C, c = idx % C;
  float s = bg::lane_sum_partials(partial, nblk, NQ, qn, C, c);
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane == 0) {
    float* out = qn == 0 ? out0 : out1;
    out[c] = (beta != 0.f ? beta * out[c] : 0.f) + scale * s;
  }
}

inline bool al(const void* p) { return bg::aligned16(p); }      // NULL counts as aligned

int finish(void* stream, const float* partial, int nblk, int C, int NQ, float* out0, float* out1, float beta, float scale) {
  bg::Launch L(stream, "ln_finish", 0, 4.0 * nblk * NQ * C);
  bg::launch(ln_finish_kernel, dim3(bg::cdiv((size_t)NQ * C, kWaves)), dim3(kT), 0, L.s, partial, nblk, C, NQ, out0, out1, beta, scale);
  return L.done("ln_finish_kernel");
}

}  // namespace

extern "C" {

int bg_ln_route(int C, int* vec, int* lanes, int* regs, int* chunks) {
  BG_REQUIRE(C > 0, BG_ERR_BAD_SHAPE, "bg_ln_route: C=%d", C);
  const Route t = route_for(C);
  if (vec) *vec = t.vec;
  if (lanes) *lanes = 1 << t.lg;
  if (regs) *regs = t.nv;
  if (chunks) *chunks = t.chunks;
  return BG_OK;
}

size_t bg_ln_workspace_bytes(int R, int C) {
  if (R <= 0 || C <= 0) return 0;
  return (size_t)grid_for(R, route_for(C)).x * 2 * C * sizeof(float);
}

int bg_ln_fwd_f32(const float* z, float* a, int R, int C, const float* gamma, const float* beta, float eps, float lrelu_alpha,
                  const uint8_t* keep, float keep_scale, size_t keep_elems, float* mu, float* r, void* stream) {
  BG_REQUIRE(z && a && gamma && beta && mu && r, BG_ERR_NULL, "bg_ln_fwd_f32: null pointer");
  BG_REQUIRE(R > 0 && C > 0 && eps > 0.f, BG_ERR_BAD_SHAPE, "bg_ln_fwd_f32: R=%d C=%d eps=%g", R, C, (double)eps);
  BG_REQUIRE(keep_elems % (size_t)C == 0 && keep_elems <= (size_t)R * C, BG_ERR_BAD_SHAPE,
             "bg_ln_fwd_f32: keep_elems=%zu is not a whole number of the %d rows of %d", keep_elems, R, C);
  BG_REQUIRE(a != z, BG_ERR_UNSUPPORTED, "bg_ln_fwd_f32: a must not alias z (the backward reads z)");
  const Route t = route_for(C);
  BG_REQUIRE(t.vec == 1 || (al(z) && al(a) && al(gamma) && al(beta) && al(keep)), BG_ERR_BAD_ALIGNMENT,
             "bg_ln_fwd_f32: pointers must be 16-byte aligned when C %% 4 == 0");
  const size_t keep_rows = keep_elems ? keep_elems / (size_t)C : (size_t)R;
  bg::Launch L(stream, "ln_fwd", 0, (8.0 + (keep ? 1.0 : 0.0)) * R * C + 8.0 * R);
  const dim3 grid = grid_for(R, t);
  for_route(t, [&](auto lanes) {
    using Rt = decltype(lanes);
    bg::launch(ln_fwd_kernel<0, Rt::VEC, Rt::NV, Rt::LOOP>, grid, dim3(kT), 0, L.s, z, a, geo_for(R, C, t), gamma, beta, eps, lrelu_alpha, keep,
               keep_scale, keep_rows, mu, r);
  });
  return L.done("ln_fwd_kernel");
}

int bg_ln_bwd_f32(const float* g, const float* z, float* dz, int R, int C, const float* gamma, const float* beta, const float* mu,
                  const float* r, float lrelu_alpha, const uint8_t* keep, float keep_scale, size_t keep_elems, const float* addend,
                  float* u_out, int u_row0, int u_rows, float* dgamma, float* dbeta, int dw_rows, float acc_beta, float acc_scale,
                  void* ws_d, size_t ws_bytes, void* stream) {
  BG_REQUIRE(g && z && dz && gamma && beta && mu && r, BG_ERR_NULL, "bg_ln_bwd_f32: null pointer");
  BG_REQUIRE((dgamma == nullptr) == (dbeta == nullptr), BG_ERR_NULL, "bg_ln_bwd_f32: dgamma and dbeta come together");
  BG_REQUIRE(R > 0 && C > 0, BG_ERR_BAD_SHAPE, "bg_ln_bwd_f32: R=%d C=%d", R, C);
  BG_REQUIRE(lrelu_alpha >= 0.f, BG_ERR_UNSUPPORTED, "bg_ln_bwd_f32: LeakyReLU's branch is re-derived from z, which needs alpha >= 0");
  BG_REQUIRE(keep_elems % (size_t)C == 0 && keep_elems <= (size_t)R * C, BG_ERR_BAD_SHAPE,
             "bg_ln_bwd_f32: keep_elems=%zu is not a whole number of the %d rows of %d", keep_elems, R, C);
  BG_REQUIRE(!u_out || (u_row0 >= 0 && u_rows > 0 && (size_t)u_row0 + u_rows <= (size_t)R), BG_ERR_BAD_SHAPE,
             "bg_ln_bwd_f32: u rows [%d, %d + %d) of %d", u_row0, u_row0, u_rows, R);
  BG_REQUIRE(dw_rows <= R, BG_ERR_BAD_SHAPE, "bg_ln_bwd_f32: dw_rows=%d of %d", dw_rows, R);
  const Route t = route_for(C);
  BG_REQUIRE(t.vec == 1 || (al(g) && al(z) && al(dz) && al(gamma) && al(beta) && al(keep) && al(addend) && al(u_out)),
             BG_ERR_BAD_ALIGNMENT, "bg_ln_bwd_f32: pointers must be 16-byte aligned when C %% 4 == 0");
  BG_REQUIRE(t.chunks == 1 || (dz != g && dz != addend), BG_ERR_UNSUPPORTED,
             "bg_ln_bwd_f32: dz may alias g or addend on the register routes only (C=%d is swept in %d chunks)", C, t.chunks);
  BG_REQUIRE(!dgamma || (ws_d && ws_bytes >= bg_ln_workspace_bytes(R, C)), BG_ERR_WORKSPACE, "bg_ln_bwd_f32: workspace too small");
  const dim3 grid = grid_for(R, t);
  ApplyArgs A;
  A.src = g; A.z = z; A.out = dz; A.gamma = gamma; A.beta = beta; A.mu = mu; A.rs = r; A.alpha = lrelu_alpha;
  A.keep = keep; A.kscale = keep_scale; A.keep_rows = keep_elems ? keep_elems / (size_t)C : (size_t)R;
  A.addend = addend; A.u_out = u_out; A.u_row0 = u_out ? (size_t)u_row0 : 0; A.u_rows = u_out ? (size_t)u_rows : 0;
  A.partial = dgamma ? static_cast<float*>(ws_d) : nullptr;
  A.dw_rows = dw_rows > 0 ? (size_t)dw_rows : (size_t)R;
  {
    bg::Launch L(stream, "ln_bwd", 0, (12.0 + (keep ? 1.0 : 0.0) + (addend ? 4.0 : 0.0)) * R * C + (u_out ? 4.0 * u_rows * C : 0.0) + 8.0 * R);
    for_route(t, [&](auto lanes) {
      using Rt = decltype(lanes);
      bg::launch(ln_apply_kernel<0, Rt::VEC, Rt::NV, Rt::LOOP>, grid, dim3(kT), 0, L.s, A, geo_for(R, C, t));
    });
    const int rc = L.done("ln_apply_kernel");
    if (rc || !dgamma) return rc;
  }
  return finish(stream, A.partial, (int)grid.x, C, 2, dgamma, dbeta, acc_beta, acc_scale);
}

int bg_ln_tangent_f32(const float* zdot, const float* z, float* vout, int R, int C, const float* gamma, const float* beta,
                      const float* mu, const float* r, float lrelu_alpha, void* stream) {
  BG_REQUIRE(zdot && z && vout && gamma && beta && mu && r, BG_ERR_NULL, "bg_ln_tangent_f32: null pointer");
  BG_REQUIRE(R > 0 && C > 0, BG_ERR_BAD_SHAPE, "bg_ln_tangent_f32: R=%d C=%d", R, C);
  BG_REQUIRE(lrelu_alpha >= 0.f, BG_ERR_UNSUPPORTED, "bg_ln_tangent_f32: LeakyReLU's branch is re-derived from z, which needs alpha >= 0");
  const Route t = route_for(C);
  BG_REQUIRE(t.vec == 1 || (al(zdot) && al(z) && al(vout) && al(gamma) && al(beta)), BG_ERR_BAD_ALIGNMENT,
             "bg_ln_tangent_f32: pointers must be 16-byte aligned when C %% 4 == 0");
  BG_REQUIRE(t.chunks == 1 || vout != zdot, BG_ERR_UNSUPPORTED,
             "bg_ln_tangent_f32: vout may alias zdot on the register routes only (C=%d is swept in %d chunks)", C, t.chunks);
  ApplyArgs A;
  A.src = zdot; A.z = z; A.out = vout; A.gamma = gamma; A.beta = beta; A.mu = mu; A.rs = r; A.alpha = lrelu_alpha;
  A.keep = nullptr; A.kscale = 1.f; A.keep_rows = 0; A.addend = nullptr; A.u_out = nullptr; A.u_row0 = A.u_rows = 0;
  A.partial = nullptr; A.dw_rows = 0;
  bg::Launch L(stream, "ln_tangent", 0, 12.0 * R * C + 8.0 * R);
  const dim3 grid = grid_for(R, t);
  for_route(t, [&](auto lanes) {
    using Rt = decltype(lanes);
    bg::launch(ln_apply_kernel<1, Rt::VEC, Rt::NV, Rt::LOOP>, grid, dim3(kT), 0, L.s, A, geo_for(R, C, t));
  });
  return L.done("ln_apply_kernel");
}

int bg_ln_gp_source_f32(const float* u, const float* zdot, const float* z, float* s, int R, int C, const float* gamma, const float* mu,
                        const float* r, float* dgamma, float acc_beta, float acc_scale, void* ws_d, size_t ws_bytes, void* stream) {
  BG_REQUIRE(u && zdot && z && s && gamma && mu && r && dgamma, BG_ERR_NULL, "bg_ln_gp_source_f32: null pointer");
  BG_REQUIRE(R > 0 && C > 0, BG_ERR_BAD_SHAPE, "bg_ln_gp_source_f32: R=%d C=%d", R, C);
  const Route t = route_for(C);
  BG_REQUIRE(t.vec == 1 || (al(u) && al(zdot) && al(z) && al(s) && al(gamma)), BG_ERR_BAD_ALIGNMENT,
             "bg_ln_gp_source_f32: pointers must be 16-byte aligned when C %% 4 == 0");
  BG_REQUIRE(s != u && s != zdot && s != z, BG_ERR_UNSUPPORTED, "bg_ln_gp_source_f32: s must not alias an input");
  BG_REQUIRE(ws_d && ws_bytes >= bg_ln_workspace_bytes(R, C), BG_ERR_WORKSPACE, "bg_ln_gp_source_f32: workspace too small");
  const dim3 grid = grid_for(R, t);
  float* partial = static_cast<float*>(ws_d);
  {
    bg::Launch L(stream, "ln_gp_source", 0, 16.0 * R * C + 8.0 * R);
    for_route(t, [&](auto lanes) {
      using Rt = decltype(lanes);
      bg::launch(ln_source_kernel<0, Rt::VEC, Rt::NV, Rt::LOOP>, grid, dim3(kT), 0, L.s, u, zdot, z, s, geo_for(R, C, t), gamma, mu, r, partial);
    });
    const int rc = L.done("ln_source_kernel");
    if (rc) return rc;
  }
  return finish(stream, partial, (int)grid.x, C, 1, dgamma, dgamma, acc_beta, acc_scale);
}

}  // extern "C"
