// Style-modulated convolutions with weight demodulation (StyleGAN2, Karras et al. 2020) in their un-fused form (include/bgan.h
// "style modulation"): the activations are scaled, not the weights, so the MFMA convolution kernels run unchanged and everything
// new is streaming work on NHWC fp32 maps.  One modulated stage, B samples of P pixels, I channels in and O out:
//
//   xs = x * s[n, :]            bg_mod_scale_f32            d = 1 / sqrt((s * s) . Q + eps)    bg_mod_demod_f32
//   Q  = sum_taps W^2           bg_mod_wsq_f32              y = d[n, :] * z + bias (-> LeakyReLU) bg_mod_scale_f32
//   dd = sum_p dy * z           bg_mod_dot_f32              dq = -1/2 d^3 dd, ds += 2 s (dq . Q^T)  bg_mod_demod_bwd_f32
//   ds = sum_p x * dxs          bg_mod_dot_f32              dW += scale * 2 W dQ                 bg_mod_wsq_grad_f32
//
// All fp32, no atomics, every sum in a fixed order: two runs give the same bits.  Products and sums are rounded separately (the
// build's -ffp-contract=off), 1 / sqrt is a correctly rounded square root and a correctly rounded division.
//
// bg_mod_scale_f32 is a rowwise.h kernel: data [R, C] with R = B * P rows, the row's sample n = r / P picks the row of v.  Float4
// units only where C % 4 == 0 AND every matrix of the call is 16-byte aligned; anything else goes by single floats.  Every element
// is read once and written once by the same lane: out may alias in.
//
// bg_mod_dot_f32 reduces over the pixels of a sample, not over a row: a workgroup holds `lanes` units of the channel axis (a power
// of two, at most 256) times 256 / lanes pixels per visit, walks its slab of pixels in index order, folds the pixel lanes through
// LDS in lane order and leaves one value per channel.  With one slab per sample that value is the result; with more (large P and
// few channels: one workgroup per sample would leave the card idle) the slabs' values go to scratch and a second launch adds them
// in slab order.
#include "common.h"
#include "reduce.h"
#include "rowwise.h"

namespace {

using namespace bg::rowwise;

__device__ __forceinline__ float lrelu(float x, float alpha) { return x > 0.f ? x : alpha * x; }

// out[r, c] = LeakyReLU_alpha(in[r, c] * v[r / P, c] (+ bias[c]))
template <int VEC, int NV, bool LOOP>
__global__ __launch_bounds__(kT) void mod_scale_kernel(const float* in, const float* v, const float* __restrict__ bias, float* out, Geo g,
                                                       int P, float alpha) {
  ROWWISE_POS_SETUP();
  (void)Cf;
  for (size_t rg = blockIdx.x; rg < groups; rg += gridDim.x) {
    ROWWISE_ROW_SETUP();
    const size_t v0 = q.row_ok ? (q.row / (size_t)P) * (size_t)g.U : 0;
    const Tile<VEC, NV> x = load_tile<VEC, NV>(in, q, base);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      if (!unit_ok(q, base, j)) continue;
      const int u = base + j * q.L + q.sub;
      float m[VEC], o[VEC];
      load_unit<VEC>(v, v0 + u, m);
#pragma unroll
      for (int e = 0; e < VEC; ++e) o[e] = x.v[j][e] * m[e];
      if (bias) {
        float b[VEC];
        load_unit<VEC>(bias, (size_t)u, b);
#pragma unroll
        for (int e = 0; e < VEC; ++e) o[e] = o[e] + b[e];
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) o[e] = lrelu(o[e], alpha);
      store_unit<VEC>(out, q.unit0 + u, o);
    }
  }
}

// ---- pixel sums ---------------------------------------------------------------------------------------------------------------
struct DotPlan { int vec, U, lanes, rows, chunks, slabs, slab_rows; };

inline int pow2_at_least(int n, int cap) {
  int p = 1;
  while (p < n && p < cap) p <<= 1;
  return p;
}

// Depends on the shape and on whether float4 units may be used, on nothing else: the same call sums in the same order every time.
inline DotPlan dot_plan(int B, int P, int C, bool aligned) {
  DotPlan d;
  d.vec = C % 4 == 0 && aligned ? 4 : 1;
  d.U = C / d.vec;
  d.lanes = pow2_at_least(d.U, kT);
  d.rows = kT / d.lanes;
  d.chunks = (d.U + d.lanes - 1) / d.lanes;
  // a slab is at least 16 visits of the workgroup; no more slabs than bring the launch to about a thousand workgroups
  const int by_rows = (P + d.rows * 16 - 1) / (d.rows * 16);
  const int by_grid = std::max(1, kMaxBlocks / std::max(1, B * d.chunks));
  d.slabs = std::max(1, std::min(by_rows, by_grid));
  d.slab_rows = (P + d.slabs - 1) / d.slabs;
  d.slabs = (P + d.slab_rows - 1) / d.slab_rows;      // no empty slab
  return d;
}

// grid (chunks, slabs, B).  dst: out (slabs == 1: beta / scale applied) or the scratch [B][slabs][C] (plain sums)
template <int VEC>
__global__ __launch_bounds__(kT) void mod_dot_kernel(const float* __restrict__ a, const float* __restrict__ b, float* dst, int P, int U,
                                                     int lg_lanes, int slab_rows, int direct, float beta, float scale) {
  __shared__ float red[kT * VEC];
  const int lanes = 1 << lg_lanes, rows = kT >> lg_lanes;
  const int ul = threadIdx.x & (lanes - 1), rl = threadIdx.x >> lg_lanes;
  const int u = (int)blockIdx.x * lanes + ul;
  const int n = blockIdx.z, slab = blockIdx.y;
  const int p0 = slab * slab_rows, p1 = min(P, p0 + slab_rows);
  float acc[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
  if (u < U) {
    const size_t s0 = (size_t)n * P * U;
    for (int p = p0 + rl; p < p1; p += rows) {
      float x[VEC], y[VEC];
      load_unit<VEC>(a, s0 + (size_t)p * U + u, x);
      load_unit<VEC>(b, s0 + (size_t)p * U + u, y);
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[e] += x[e] * y[e];
    }
  }
#pragma unroll
  for (int e = 0; e < VEC; ++e) red[threadIdx.x * VEC + e] = acc[e];
  __syncthreads();
  if (rl == 0 && u < U) {
    for (int r = 1; r < rows; ++r)
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[e] += red[(r * lanes + ul) * VEC + e];
    const size_t o = direct ? (size_t)n * U + u : ((size_t)n * gridDim.y + slab) * U + u;
    if (direct) {
      float old[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) old[e] = 0.f;
      if (beta != 0.f) load_unit<VEC>(dst, o, old);
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        acc[e] = scale * acc[e];
        if (beta != 0.f) acc[e] += beta * old[e];
      }
    }
    store_unit<VEC>(dst, o, acc);
  }
}

// out[n, c] = beta * out + scale * (the slabs' values of (n, c), added in slab order)
__global__ __launch_bounds__(kT) void mod_dot_finish_kernel(const float* __restrict__ part, float* out, int BC, int C, int slabs, float beta,
                                                            float scale) {
  for (int i = blockIdx.x * kT + threadIdx.x; i < BC; i += gridDim.x * kT) {
    const int n = i / C, c = i - n * C;
    const float* p = part + (size_t)n * slabs * C + c;
    float s = p[0];
    for (int k = 1; k < slabs; ++k) s += p[(size_t)k * C];
    float v = scale * s;
    if (beta != 0.f) v += beta * out[i];
    out[i] = v;
  }
}

// ---- weights: Q and its gradient ------------------------------------------------------------------------------------------------
// W is [taps][Rr][Cc] as stored: (Rr, Cc) = (I, O) for a Conv2D kernel, (O, I) for a Conv2DTranspose's (tr).  A thread owns one
// (r, c) of the stored layout, so the reads of a wave are contiguous; Q is [I][O] either way.
__global__ __launch_bounds__(kT) void mod_wsq_kernel(const float* __restrict__ w, float* __restrict__ q, int taps, int Rr, int Cc, int tr) {
  const int n = Rr * Cc;
  for (int e = blockIdx.x * kT + threadIdx.x; e < n; e += gridDim.x * kT) {
    float s = 0.f;
    for (int t = 0; t < taps; ++t) {
      const float x = w[(size_t)t * n + e];
      s += x * x;
    }
    const int r = e / Cc, c = e - r * Cc;
    q[tr ? (size_t)c * Rr + r : (size_t)e] = s;
  }
}

__global__ __launch_bounds__(kT) void mod_wsq_grad_kernel(const float* __restrict__ w, const float* __restrict__ dq, float* dw, int taps, int Rr,
                                                          int Cc, int tr, float scale) {
  const int n = Rr * Cc;
  for (int e = blockIdx.x * kT + threadIdx.x; e < n; e += gridDim.x * kT) {
    const int r = e / Cc, c = e - r * Cc;
    const float g = dq[tr ? (size_t)c * Rr + r : (size_t)e];
    for (int t = 0; t < taps; ++t) {
      const size_t i = (size_t)t * n + e;
      const float v = scale * ((2.f * w[i]) * g);
      dw[i] = dw[i] + v;
    }
  }
}

// ---- demodulation ---------------------------------------------------------------------------------------------------------------
// d[n, o] = 1 / sqrt(sum_i (s[n, i] * s[n, i]) * Q[i, o] + eps), i in index order.  A thread owns one (n, o): a wave reads Q rows
// contiguously and s[n, i] as a broadcast
__global__ __launch_bounds__(kT) void mod_demod_kernel(const float* __restrict__ s, const float* __restrict__ Q, float* __restrict__ d, int B, int I,
                                                       int O, float eps) {
  const size_t tot = (size_t)B * O;
  for (size_t e = (size_t)blockIdx.x * kT + threadIdx.x; e < tot; e += (size_t)gridDim.x * kT) {
    const int n = (int)(e / O), o = (int)(e - (size_t)n * O);
    const float* sn = s + (size_t)n * I;
    const float* qo = Q + o;
    float q = 0.f;
    int i = 0;
    for (; i + 8 <= I; i += 8) {        // eight loads in flight, added in index order: the sum keeps its bits, a lane waits once per eight
      float sv[8], qv[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) { sv[k] = sn[i + k]; qv[k] = qo[(size_t)(i + k) * O]; }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float t = sv[k] * sv[k];
        q += t * qv[k];
      }
    }
    for (; i < I; ++i) {
      const float t = sn[i] * sn[i];
      q += t * qo[(size_t)i * O];
    }
    d[e] = 1.0f / sqrtf(q + eps);
  }
}

// dq[n, o] = -1/2 * d^3 * dd
__global__ __launch_bounds__(kT) void mod_dq_kernel(const float* __restrict__ d, const float* __restrict__ dd, float* __restrict__ dq, size_t n) {
  for (size_t e = (size_t)blockIdx.x * kT + threadIdx.x; e < n; e += (size_t)gridDim.x * kT) {
    const float x = d[e];
    dq[e] = -0.5f * (((x * x) * x) * dd[e]);
  }
}

// ds[n, i] += 2 * s[n, i] * sum_o dq[n, o] * Q[i, o]: one wave per (n, i); a lane adds o = lane, lane + 64, ... in that order, the
// lanes fold in a fixed butterfly
__global__ __launch_bounds__(kT) void mod_demod_bwd_kernel(const float* __restrict__ dq, const float* __restrict__ s, const float* __restrict__ Q,
                                                           float* ds, int B, int I, int O) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t tot = (size_t)B * I;
  for (size_t e = (size_t)blockIdx.x * kWaves + wave; e < tot; e += (size_t)gridDim.x * kWaves) {
    const int n = (int)(e / I), i = (int)(e - (size_t)n * I);
    const float* g = dq + (size_t)n * O;
    const float* qi = Q + (size_t)i * O;
    float acc = 0.f;
    for (int o = lane; o < O; o += 64) acc += g[o] * qi[o];
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) ds[e] = ds[e] + (2.f * s[e]) * acc;
  }
}

inline bool al(const void* p) { return bg::aligned16(p); }
inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
inline int lg2(int p) {
  int l = 0;
  while ((1 << l) < p) ++l;
  return l;
}

}  // namespace

extern "C" {

int bg_mod_scale_f32(const float* in, const float* v, const float* bias, float* out, int B, int P, int C, float lrelu_alpha, void* stream) {
  BG_REQUIRE(in && v && out, BG_ERR_NULL, "bg_mod_scale_f32: null pointer");
  BG_REQUIRE(B > 0 && P > 0 && C > 0 && (size_t)B * P <= 0x7fffffffu, BG_ERR_BAD_SHAPE, "bg_mod_scale_f32: B=%d P=%d C=%d", B, P, C);
  BG_REQUIRE(al4(in) && al4(v) && al4(bias) && al4(out), BG_ERR_BAD_ALIGNMENT, "bg_mod_scale_f32: pointers must be 4-byte aligned");
  const int R = B * P;
  const Route t = route_for(C, al(in) && al(v) && al(out) && (!bias || al(bias)));
  bg::Launch L(stream, "mod_scale", 0, 8.0 * R * C + 4.0 * B * C);
  const dim3 grid = grid_for(R, t);
  for_route(t, [&](auto lanes) {
    using Rt = decltype(lanes);
    bg::launch(mod_scale_kernel<Rt::VEC, Rt::NV, Rt::LOOP>, grid, dim3(kT), 0, L.s, in, v, bias, out, geo_for(R, C, t), P, lrelu_alpha);
  });
  return L.done("mod_scale_kernel");
}

int bg_mod_dot_plan(int B, int P, int C, int* out) {
  BG_REQUIRE(out, BG_ERR_NULL, "bg_mod_dot_plan: null pointer");
  BG_REQUIRE(B > 0 && P > 0 && C > 0, BG_ERR_BAD_SHAPE, "bg_mod_dot_plan: B=%d P=%d C=%d", B, P, C);
  for (int k = 0; k < 2; ++k) {
    const DotPlan d = dot_plan(B, P, C, k == 0);
    out[4 * k + 0] = d.vec;
    out[4 * k + 1] = d.lanes;
    out[4 * k + 2] = d.chunks;
    out[4 * k + 3] = d.slabs;
  }
  return BG_OK;
}

size_t bg_mod_dot_workspace_bytes(int B, int P, int C) {
  if (B <= 0 || P <= 0 || C <= 0) return 0;
  const int s = std::max(dot_plan(B, P, C, true).slabs, dot_plan(B, P, C, false).slabs);
  return s > 1 ? sizeof(float) * (size_t)B * s * C : 0;
}

int bg_mod_dot_f32(const float* a, const float* b, float* out, int B, int P, int C, void* ws, size_t ws_bytes, float beta, float scale,
                   void* stream) {
  BG_REQUIRE(a && b && out, BG_ERR_NULL, "bg_mod_dot_f32: null pointer");
  BG_REQUIRE(B > 0 && B <= 65535 && P > 0 && C > 0 && (size_t)B * C <= 0x7fffffffu, BG_ERR_BAD_SHAPE, "bg_mod_dot_f32: B=%d P=%d C=%d", B, P, C);
  BG_REQUIRE(al4(a) && al4(b) && al4(out) && al4(ws), BG_ERR_BAD_ALIGNMENT, "bg_mod_dot_f32: pointers must be 4-byte aligned");
  // float4 units where every matrix of the call, the scratch included, is 16-byte aligned
  const DotPlan d = dot_plan(B, P, C, al(a) && al(b) && al(out) && (!ws || al(ws)));
  const int direct = d.slabs == 1;
  if (!direct)
    BG_REQUIRE(ws && ws_bytes >= sizeof(float) * (size_t)B * d.slabs * C, BG_ERR_WORKSPACE, "bg_mod_dot_f32: workspace of %zu bytes, need %zu",
               ws_bytes, sizeof(float) * (size_t)B * d.slabs * C);
  float* dst = direct ? out : static_cast<float*>(ws);
  const dim3 grid(d.chunks, d.slabs, B);
  {
    bg::Launch L(stream, "mod_dot", 0, 8.0 * B * P * C);
    if (d.vec == 4)
      bg::launch(mod_dot_kernel<4>, grid, dim3(kT), 0, L.s, a, b, dst, P, d.U, lg2(d.lanes), d.slab_rows, direct, beta, scale);
    else
      bg::launch(mod_dot_kernel<1>, grid, dim3(kT), 0, L.s, a, b, dst, P, d.U, lg2(d.lanes), d.slab_rows, direct, beta, scale);
    const int rc = L.done("mod_dot_kernel");
    if (rc != BG_OK || direct) return rc;
  }
  bg::Launch L(stream, "mod_dot_finish", 0, 4.0 * B * C * (d.slabs + 1));
  bg::launch(mod_dot_finish_kernel, dim3(bg::grid_cap((size_t)B * C, kT)), dim3(kT), 0, L.s, (const float*)dst, out, B * C, C, d.slabs, beta,
             scale);
  return L.done("mod_dot_finish_kernel");
}

int bg_mod_wsq_f32(const float* w, float* q, int taps, int I, int O, int transposed, void* stream) {
  BG_REQUIRE(w && q, BG_ERR_NULL, "bg_mod_wsq_f32: null pointer");
  BG_REQUIRE(taps > 0 && I > 0 && O > 0 && (size_t)I * O <= 0x7fffffffu, BG_ERR_BAD_SHAPE, "bg_mod_wsq_f32: taps=%d I=%d O=%d", taps, I, O);
  BG_REQUIRE(al4(w) && al4(q), BG_ERR_BAD_ALIGNMENT, "bg_mod_wsq_f32: pointers must be 4-byte aligned");
  const int Rr = transposed ? O : I, Cc = transposed ? I : O;
  bg::Launch L(stream, "mod_wsq", 0, 4.0 * I * O * (taps + 1));
  bg::launch(mod_wsq_kernel, dim3(bg::grid_cap((size_t)I * O, kT)), dim3(kT), 0, L.s, w, q, taps, Rr, Cc, transposed ? 1 : 0);
  return L.done("mod_wsq_kernel");
}

int bg_mod_wsq_grad_f32(const float* w, const float* dq, float* dw, int taps, int I, int O, int transposed, float scale, void* stream) {
  BG_REQUIRE(w && dq && dw, BG_ERR_NULL, "bg_mod_wsq_grad_f32: null pointer");
  BG_REQUIRE(taps > 0 && I > 0 && O > 0 && (size_t)I * O <= 0x7fffffffu, BG_ERR_BAD_SHAPE, "bg_mod_wsq_grad_f32: taps=%d I=%d O=%d", taps, I, O);
  BG_REQUIRE(al4(w) && al4(dq) && al4(dw), BG_ERR_BAD_ALIGNMENT, "bg_mod_wsq_grad_f32: pointers must be 4-byte aligned");
  const int Rr = transposed ? O : I, Cc = transposed ? I : O;
  bg::Launch L(stream, "mod_wsq_grad", 0, 4.0 * I * O * (3.0 * taps + 1));
  bg::launch(mod_wsq_grad_kernel, dim3(bg::grid_cap((size_t)I * O, kT)), dim3(kT), 0, L.s, w, dq, dw, taps, Rr, Cc, transposed ? 1 : 0, scale);
  return L.done("mod_wsq_grad_kernel");
}

int bg_mod_demod_f32(const float* s, const float* Q, float* d, int B, int I, int O, float eps, void* stream) {
  BG_REQUIRE(s && Q && d, BG_ERR_NULL, "bg_mod_demod_f32: null pointer");
  BG_REQUIRE(B > 0 && I > 0 && O > 0, BG_ERR_BAD_SHAPE, "bg_mod_demod_f32: B=%d I=%d O=%d", B, I, O);
  BG_REQUIRE(eps > 0.f, BG_ERR_BAD_SHAPE, "bg_mod_demod_f32: eps=%g must be positive", (double)eps);
  BG_REQUIRE(al4(s) && al4(Q) && al4(d), BG_ERR_BAD_ALIGNMENT, "bg_mod_demod_f32: pointers must be 4-byte aligned");
  bg::Launch L(stream, "mod_demod", 2.0 * B * I * O, 4.0 * ((double)B * I + (double)I * O + (double)B * O));
  bg::launch(mod_demod_kernel, dim3(bg::grid_cap((size_t)B * O, kT)), dim3(kT), 0, L.s, s, Q, d, B, I, O, eps);
  return L.done("mod_demod_kernel");
}

int bg_mod_demod_bwd_f32(const float* d, const float* dd, const float* s, const float* Q, float* dq, float* ds, int B, int I, int O,
                         void* stream) {
  BG_REQUIRE(d && dd && s && Q && dq && ds, BG_ERR_NULL, "bg_mod_demod_bwd_f32: null pointer");
  BG_REQUIRE(B > 0 && I > 0 && O > 0, BG_ERR_BAD_SHAPE, "bg_mod_demod_bwd_f32: B=%d I=%d O=%d", B, I, O);
  BG_REQUIRE(al4(d) && al4(dd) && al4(s) && al4(Q) && al4(dq) && al4(ds), BG_ERR_BAD_ALIGNMENT,
             "bg_mod_demod_bwd_f32: pointers must be 4-byte aligned");
  {
    bg::Launch L(stream, "mod_dq", 0, 12.0 * B * O);
    bg::launch(mod_dq_kernel, dim3(bg::grid_cap((size_t)B * O, kT)), dim3(kT), 0, L.s, d, dd, dq, (size_t)B * O);
    const int rc = L.done("mod_dq_kernel");
    if (rc != BG_OK) return rc;
  }
  bg::Launch L(stream, "mod_demod_bwd", 2.0 * B * I * O, 4.0 * ((double)B * O + (double)I * O + 3.0 * B * I));
  bg::launch(mod_demod_bwd_kernel, dim3(bg::grid_cap((size_t)B * I, kWaves)), dim3(kT), 0, L.s, (const float*)dq, s, Q, ds, B, I, O);
  return L.done("mod_demod_bwd_kernel");
}

}  // extern "C"
