// The StyleGAN mapping network z -> w (include/bgan.h "mapping network"; layers.MappingNetwork): a skinny fp32 Dense with its
// equalised-learning-rate coefficient, bias multiplier and LeakyReLU in the epilogue, the LeakyReLU' + bias-gradient pass of its
// backward, and the truncation trick.  Everything else of the layer runs on bg_gemm_f32 / bg_colsum_f32 / bg_ema_f32.
//
//   dense_lrelu   y = LeakyReLU_alpha(c * (x . W) + bias_mul * bias), x [M, K], W [K, N] row-major.  M is the batch (256), N, K <= 512:
//                 gemm_tiled_kernel's 64x64 tiles would make 32 workgroups of a 256-CU part and 16 serial K-steps each.  Here a
//                 workgroup owns a 32x32 tile of y (kTM x kTN: (256, 512) -> 128 workgroups, (256, 100) -> 32) and its four waves
//                 SPLIT the K-step: a step stages 64 k (kTK) of both operands in LDS, wave w multiplies k in [16 w, 16 w + 16) with
//                 eight v_mfma_f32_32x32x2_f32 (exact fp32, bg_gemm_f32's instruction) into its own 32x32 accumulator; the next
//                 step's global loads are in flight under the products.  After the last step the four accumulators are added
//                 through LDS in wave order (a fixed order: two runs give the same bits) and the epilogue runs in registers: the
//                 pre-activation is never written.  K = 512 is 8 round trips of 8 products per wave, K = 100 two: the kernel is
//                 bound by launch and load latency, not by flops.  Loads are single floats, coalesced along
//                 the contiguous index and predicated on the edges: any M, N, K >= 1 and any 4-byte aligned pointer takes the
//                 same route.
//   lrelu_bias_bwd  gp = g * (y > 0 ? 1 : alpha) (bg_mul_grad_f32's convention; gp may alias g) and, in the same pass,
//                 dbias[n] = beta * old + scale * sum_m gp[m, n].  rowwise.h's layout: a lane keeps the same columns in every visit,
//                 so it adds its rows' values in visit order; lanes of a wave that hold the same columns fold by a butterfly in
//                 descending offsets, the waves in wave order through LDS, and a workgroup leaves ONE partial row; a second launch
//                 adds the partial rows in reduce.h's lane_sum_partials order.  No atomics.
//   truncate      out = w_avg + psi * (w - w_avg), w_avg read from device memory; psi == 1 copies w (the identity, bit for bit).
#include "common.h"
#include "reduce.h"
#include "rowwise.h"

namespace {

using namespace bg::rowwise;

constexpr int kTM = 32, kTN = 32, kTK = 64;      // the tile of y a workgroup owns and the k it stages per step (bg_dense_lrelu_plan)
constexpr int kLd = kTM + 1;                     // LDS row stride of a staged operand ([k][m] / [k][n]): odd, so the k-fastest stores of x spread over the banks

typedef float map_floatx16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(kT) void dense_lrelu_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                         const float* __restrict__ bias, float* __restrict__ y, int M, int N, int K,
                                                         float c, float bias_mul, float alpha) {
  constexpr int NL = kTM * kTK / kT;                          // 8 elements per thread per operand tile
  constexpr int kStage = 2 * kTK * kLd, kRed = kWaves * 16 * 64;
  __shared__ float lds[kStage > kRed ? kStage : kRed];
  float(*As)[kLd] = reinterpret_cast<float(*)[kLd]>(lds);
  float(*Bs)[kLd] = reinterpret_cast<float(*)[kLd]>(lds + kTK * kLd);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 31, kk = lane >> 5;
  const int m0 = blockIdx.y * kTM, n0 = blockIdx.x * kTN;
  map_floatx16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.f;
  float ra[NL], rb[NL];
  auto gload = [&](int k0) {                                  // x tile -> As[k][m] (k fastest in memory); W tile -> Bs[k][n] (n fastest)
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int e = threadIdx.x + i * kT;
      const int mm = e / kTK, ka = e - mm * kTK;
      const int m = m0 + mm, k = k0 + ka;
      ra[i] = (m < M && k < K) ? x[(size_t)m * K + k] : 0.f;
      const int kb = e / kTN, nn = e - kb * kTN;
      const int n = n0 + nn, k2 = k0 + kb;
      rb[i] = (n < N && k2 < K) ? W[(size_t)k2 * N + n] : 0.f;
    }
  };
  auto lstore = [&]() {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int e = threadIdx.x + i * kT;
      const int mm = e / kTK, ka = e - mm * kTK;
      As[ka][mm] = ra[i];
      const int kb = e / kTN, nn = e - kb * kTN;
      Bs[kb][nn] = rb[i];
    }
  };
  gload(0);
  for (int k0 = 0; k0 < K; k0 += kTK) {
    lstore();
    __syncthreads();
    if (k0 + kTK < K) gload(k0 + kTK);                        // in flight under this step's products
    const float* ap = &As[wave * (kTK / kWaves) + kk][li];    // + 2p rows: x[m = li][k = 16 wave + 2p + kk]
    const float* bp = &Bs[wave * (kTK / kWaves) + kk][li];
#pragma unroll
    for (int p = 0; p < kTK / kWaves / 2; ++p) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * p * kLd], bp[2 * p * kLd], acc, 0, 0, 0);
    __syncthreads();
  }
  // the waves' shares of k, added in wave order: red[wave][q][lane]
  float* red = lds;
#pragma unroll
  for (int q = 0; q < 16; ++q) red[(wave * 16 + q) * 64 + lane] = acc[q];
  __syncthreads();
  // element (q, lane) of the tile = y[row (q & 3) + 8 (q >> 2) + 4 kk][col li]; a thread finishes four of the 1024
#pragma unroll
  for (int i = 0; i < 16 / kWaves; ++i) {
    const int q = wave + i * kWaves;
    float s = red[q * 64 + lane];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) s += red[(w * 16 + q) * 64 + lane];
    const int m = m0 + (q & 3) + 8 * (q >> 2) + 4 * kk, n = n0 + li;
    if (m >= M || n >= N) continue;
    float v = c * s;
    if (bias) v += bias_mul * bias[n];
    y[(size_t)m * N + n] = v > 0.f ? v : alpha * v;
  }
}

// part[blockIdx.x * C + col] = the workgroup's column sums of gp over the rows it visits
template <int VEC, int NV, bool LOOP>
__global__ __launch_bounds__(kT) void lrelu_bias_bwd_kernel(const float* gr, const float* __restrict__ y, float* gp,
                                                            float* __restrict__ part, Geo g, float alpha) {
  __shared__ float red[kWaves][NV * VEC][64];
  ROWWISE_POS_SETUP();
  (void)Cf;
  float acc[NV][VEC];
#pragma unroll
  for (int j = 0; j < NV; ++j)
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[j][e] = 0.f;
  for (size_t rg = blockIdx.x; rg < groups; rg += gridDim.x) {
    ROWWISE_ROW_SETUP();
    const Tile<VEC, NV> tg = load_tile<VEC, NV>(gr, q, base);
    const Tile<VEC, NV> ty = load_tile<VEC, NV>(y, q, base);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      if (!unit_ok(q, base, j)) continue;
      float o[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        o[e] = tg.v[j][e] * (ty.v[j][e] > 0.f ? 1.f : alpha);
        acc[j][e] += o[e];
      }
      store_unit<VEC>(gp, q.unit0 + base + j * q.L + q.sub, o);
    }
  }
  // lanes sub, sub + L, ... of a wave hold the same columns: butterfly over them, then the waves in wave order
#pragma unroll
  for (int j = 0; j < NV; ++j)
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      float v = acc[j][e];
      for (int o = 32; o >= q.L; o >>= 1) v += __shfl_xor(v, o, 64);
      if (lane < q.L) red[wave][j * VEC + e][lane] = v;
    }
  __syncthreads();
  if (wave == 0 && lane < q.L) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int unit = base + j * q.L + q.sub;
      if (unit >= q.U) continue;
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        float s = red[0][j * VEC + e][lane];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) s += red[w][j * VEC + e][lane];
        part[(size_t)blockIdx.x * g.C + (size_t)unit * VEC + e] = s;
      }
    }
  }
}

// one wave per column: dbias[n] = beta * old + scale * sum of the partial rows (beta == 0: old is not read)
__global__ __launch_bounds__(kT) void lrelu_bias_finish_kernel(const float* __restrict__ part, int nblk, int N, float* dbias, float beta,
                                                               float scale) {
  const int n = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (n >= N) return;
  float s = bg::lane_sum_partials(part, nblk, 1, 0, N, n);
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((threadIdx.x & 63) == 0) {
    float v = scale * s;
    if (beta != 0.f) v += beta * dbias[n];
    dbias[n] = v;
  }
}

__global__ __launch_bounds__(kT) void truncate_kernel(const float* w, const float* __restrict__ w_avg, float* out, float psi, size_t n, int U) {
  for (size_t e = (size_t)blockIdx.x * kT + threadIdx.x; e < n; e += (size_t)gridDim.x * kT) {
    const float a = w_avg[e % (size_t)U], v = w[e];
    out[e] = psi == 1.f ? v : a + psi * (v - a);
  }
}

inline bool al(const void* p) { return bg::aligned16(p); }
inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace

extern "C" {

int bg_dense_lrelu_plan(int M, int N, int K, int* out) {
  BG_REQUIRE(out, BG_ERR_NULL, "bg_dense_lrelu_plan: null pointer");
  BG_REQUIRE(M > 0 && N > 0 && K > 0, BG_ERR_BAD_SHAPE, "bg_dense_lrelu_plan: M=%d N=%d K=%d", M, N, K);
  out[0] = kTM;
  out[1] = kTN;
  out[2] = kTK;
  out[3] = (int)(bg::cdiv(M, kTM) * bg::cdiv(N, kTN));
  return BG_OK;
}

int bg_dense_lrelu_f32(const float* x, const float* W, const float* bias, float* y, int M, int N, int K, float c, float bias_mul,
                       float alpha, void* stream) {
  BG_REQUIRE(x && W && y, BG_ERR_NULL, "bg_dense_lrelu_f32: null pointer");
  BG_REQUIRE(M > 0 && N > 0 && K > 0, BG_ERR_BAD_SHAPE, "bg_dense_lrelu_f32: M=%d N=%d K=%d", M, N, K);
  BG_REQUIRE(al4(x) && al4(W) && al4(bias) && al4(y), BG_ERR_BAD_ALIGNMENT, "bg_dense_lrelu_f32: pointers must be 4-byte aligned");
  BG_REQUIRE(bg::cdiv(M, kTM) <= 65535u, BG_ERR_BAD_SHAPE, "bg_dense_lrelu_f32: M=%d (more than 65535 row tiles)", M);
  BG_REQUIRE(y != x && y != W, BG_ERR_UNSUPPORTED, "bg_dense_lrelu_f32: y must not alias an operand");
  bg::Launch L(stream, "dense_lrelu", 2.0 * M * (double)N * K, 4.0 * ((double)M * K + (double)K * N + (double)M * N));
  bg::launch(dense_lrelu_kernel, dim3(bg::cdiv(N, kTN), bg::cdiv(M, kTM)), dim3(kT), 0, L.s, x, W, bias, y, M, N, K, c, bias_mul, alpha);
  return L.done("dense_lrelu_kernel");
}

size_t bg_lrelu_bias_bwd_workspace_bytes(int M, int N) {
  if (M <= 0 || N <= 0) return 0;
  return sizeof(float) * (size_t)N * std::max(grid_for(M, route_for(N, true)).x, grid_for(M, route_for(N, false)).x);
}

int bg_lrelu_bias_bwd_f32(const float* g, const float* y, float* gp, float* dbias, int M, int N, float alpha, float beta, float scale,
                          void* ws, size_t ws_bytes, void* stream) {
  BG_REQUIRE(g && y && gp && dbias, BG_ERR_NULL, "bg_lrelu_bias_bwd_f32: null pointer");
  BG_REQUIRE(M > 0 && N > 0, BG_ERR_BAD_SHAPE, "bg_lrelu_bias_bwd_f32: M=%d N=%d", M, N);
  BG_REQUIRE(al4(g) && al4(y) && al4(gp) && al4(dbias) && al4(ws), BG_ERR_BAD_ALIGNMENT, "bg_lrelu_bias_bwd_f32: pointers must be 4-byte aligned");
  BG_REQUIRE(gp != y, BG_ERR_UNSUPPORTED, "bg_lrelu_bias_bwd_f32: gp must not alias y");
  BG_REQUIRE(ws && ws_bytes >= bg_lrelu_bias_bwd_workspace_bytes(M, N), BG_ERR_WORKSPACE, "bg_lrelu_bias_bwd_f32: workspace too small");
  const Route t = route_for(N, al(g) && al(y) && al(gp));
  const dim3 grid = grid_for(M, t);
  float* part = static_cast<float*>(ws);
  {
    bg::Launch L(stream, "lrelu_bias_bwd", 0, 12.0 * M * N);
    for_route(t, [&](auto lanes) {
      using Rt = decltype(lanes);
      bg::launch(lrelu_bias_bwd_kernel<Rt::VEC, Rt::NV, Rt::LOOP>, grid, dim3(kT), 0, L.s, g, y, gp, part, geo_for(M, N, t), alpha);
    });
    const int rc = L.done("lrelu_bias_bwd_kernel");
    if (rc != BG_OK) return rc;
  }
  bg::Launch L(stream, "lrelu_bias_finish", 0, 4.0 * grid.x * N);
  bg::launch(lrelu_bias_finish_kernel, dim3(bg::cdiv(N, kWaves)), dim3(kT), 0, L.s, (const float*)part, (int)grid.x, N, dbias, beta, scale);
  return L.done("lrelu_bias_finish_kernel");
}

int bg_truncate_f32(const float* w, const float* w_avg, float* out, float psi, int B, int U, void* stream) {
  BG_REQUIRE(w && w_avg && out, BG_ERR_NULL, "bg_truncate_f32: null pointer");
  BG_REQUIRE(B > 0 && U > 0, BG_ERR_BAD_SHAPE, "bg_truncate_f32: B=%d U=%d", B, U);
  BG_REQUIRE(al4(w) && al4(w_avg) && al4(out), BG_ERR_BAD_ALIGNMENT, "bg_truncate_f32: pointers must be 4-byte aligned");
  const size_t n = (size_t)B * U;
  bg::Launch L(stream, "truncate", 0, 8.0 * n);
  bg::launch(truncate_kernel, dim3(bg::grid_cap(n, kT)), dim3(kT), 0, L.s, w, w_avg, out, psi, n, U);
  return L.done("truncate_kernel");
}

}  // extern "C"
