// Minibatch standard deviation (include/bgan.h "minibatch standard deviation"; Karras et al. 2018, StyleGAN2's layer with one new
// feature) in front of the critic's head.  x is [N, P, C] fp32 (P pixels), a sample E = P * C contiguous floats; a GROUP is G
// consecutive samples, G * E contiguous floats of x and Ly = G * P * (C + 1) contiguous floats of the output.  Per group and column
// j in [0, E):  mu = mean_n x,  s = sqrt(mean_n (x - mu)^2 + eps),  f = mean_j s;  y = x with f appended as channel C of every pixel.
//
// Three calls, each the same two phases on one group:
//   (f is formed as s_0 + mean_j (s_j - s_0) with column 0's s: exact where every column has the same s, see first_column_s)
//   columns   a lane takes four consecutive columns (16 bytes where the address of the group's mu row allows, scalar head and
//             tail), walks the G members of each, and adds what the group's scalar is summed over to a partial of its own, in loop
//             order.  Where every operand's group base is 16-byte aligned and E % 4 == 0 (every call of the engine) that is
//             established once per group and all operands move as unconditional float4s; else each access tests its own address.  The forward leaves mu and 1 / s per group and column; the penalty call writes the source term here.
//   reduce    a fixed shuffle tree per wave, the waves added in wave order: the same bits on every run, no atomics.
//   emit      the group's output range is swept flat, four consecutive OUTPUT floats per lane as one float4 (scalar head and tail
//             from the range's own address: its row stride C + 1 is odd for every stock critic, so no pixel is aligned, the flat
//             range is); the pass-through floats are gathered one at a time, the scalar lands in every (C + 1)-th slot.
// Routes (plan_for, reported by bg_mbstd_plan): a group of at most kResident floats waits in LDS between the two phases and is read
// from memory once, one workgroup per group, one launch.  A larger one takes two launches: the columns cut over gridDim.y workgroups,
// each leaving its partial in the workspace, then the emit cut over gridDim.y workgroups, each adding the partials in index order
// (the same bits in every workgroup) and reading the pass-through floats again, out of L2.
// The backward needs no such wait: its scalar q is a sum over the G * P floats of channel C of the incoming gradient, which every
// workgroup of the group adds up for itself in the same order; one launch on either route, nothing in LDS but the waves' partials.
#include "common.h"
#include "reduce.h"
#include <algorithm>
#include <cmath>

namespace {

constexpr int kT = 256, kMaxWaves = kT / 64, kMaxBlocks = 1024;
constexpr int kResident = 15360 - 4;       // floats of a group the resident route takes (60 KiB of LDS less the alignment pad)
constexpr int kCutFloats = 8192;           // two-launch route: at least this many floats of the group per workgroup
constexpr int kMaxCuts = 64;

enum { CALL_FWD = 0, CALL_BWD = 1, CALL_GP = 2 };
enum { MODE_RESIDENT = 0, MODE_COLUMNS = 1, MODE_EMIT = 2 };

struct Geo {
  int N, G, P, C, E;        // E = P * C
  int GE, Ly;               // floats of a group of x, of y
  int Kc;                   // cuts of the column phase: the partials per group the emit phase adds up
  float k;                  // 1 / (G * E)
  float eps;
};

// W floats from p.  W == 4: one 16-byte access where p is 16-byte aligned -- KNOWN: the caller has established that it is (the
// call's fast path: every operand's group base aligned and E % 4 == 0), and the access is unconditional; else tested per access.
template <int W, bool KNOWN = false>
__device__ __forceinline__ void ld(const float* p, float (&v)[4]) {
  if (W == 4 && (KNOWN || (reinterpret_cast<uintptr_t>(p) & 15u) == 0)) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int q = 0; q < W; ++q) v[q] = p[q];
  }
}

template <int W, bool KNOWN = false>
__device__ __forceinline__ void st(float* p, const float (&v)[4]) {
  if (W == 4 && (KNOWN || (reinterpret_cast<uintptr_t>(p) & 15u) == 0)) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int q = 0; q < W; ++q) p[q] = v[q];
  }
}

using bg::block_sum;      // reduce.h: the workgroup's sum; red may still be read from the previous group, hence its first barrier
using bg::sweep;          // reduce.h: scalar head, float4 runs dealt to the K workgroups of the group, scalar tail

// whether every one of the pointers is 16-byte aligned
template <class... P>
__device__ __forceinline__ bool all_aligned(P... p) {
  return (((reinterpret_cast<uintptr_t>(p)) | ...) & 15u) == 0;
}

// the group's output range: out[o] = img[o - o / (C + 1)] in channels [0, C), ``val`` in channel C
template <class At>
__device__ __forceinline__ void emit(float* out, At at, float val, const Geo& g, int k, int K) {
  const int C1 = g.C + 1;
  auto e1 = [&](int o) {
    const int pix = o / C1;
    out[o] = (o - pix * C1 == g.C) ? val : at(o - pix);
  };
  auto e4 = [&](int o) {
    int pix = o / C1, c = o - pix * C1;
    float r[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (c == g.C) {
        r[q] = val;
        c = 0;
        ++pix;
      } else {
        r[q] = at(o + q - pix);
        ++c;
      }
    }
    *reinterpret_cast<float4*>(out + o) = make_float4(r[0], r[1], r[2], r[3]);
  };
  sweep(reinterpret_cast<uintptr_t>(out), g.Ly, k, K, e4, e1);
}

// the group's image into LDS, shifted by ``pad`` floats so that the float4s read from memory land 16-byte aligned there too
__device__ __forceinline__ void stage_in(const float* src, float* img, int n) {
  auto c1 = [&](int o) { img[o] = src[o]; };
  auto c4 = [&](int o) { *reinterpret_cast<float4*>(img + o) = *reinterpret_cast<const float4*>(src + o); };
  sweep(reinterpret_cast<uintptr_t>(src), n, 0, 1, c4, c1);
}

// add the K partials of group ``grp`` in index order
__device__ __forceinline__ float sum_partials(const float* ws, int grp, int K) {
  float s = ws[(size_t)grp * K];
  for (int j = 1; j < K; ++j) s += ws[(size_t)grp * K + j];
  return s;
}

// s of column 0 of a group (``img``: its G * E floats), by the operations the column sweep applies to every column.  The group's
// scalar is taken as s_0 + mean(s - s_0): columns that all have the same s (a group without variance: s = sqrt(eps) everywhere) give
// exactly that s, whatever the order of the sum, and the sum itself carries the spread of s, not its size.
__device__ __forceinline__ float first_column_s(const float* img, int G, int E, float eps) {
  const float Gf = (float)G, x0 = img[0];
  float m = 0.f, v = 0.f;
  for (int n = 1; n < G; ++n) m += img[(size_t)n * E] - x0;
  m = x0 + m / Gf;
  for (int n = 0; n < G; ++n) {
    const float d = img[(size_t)n * E] - m;
    v += d * d;
  }
  return sqrtf(v / Gf + eps);
}

// Forward.  MODE_RESIDENT: both phases, the group's x in LDS; MODE_COLUMNS: statistics and the cut's partial into ws[group, cut];
// MODE_EMIT: f from the partials, the output from memory.
template <int MODE>
__global__ __launch_bounds__(kT) void mbstd_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, float* __restrict__ mu,
                                                        float* __restrict__ rs, float* __restrict__ f, float* __restrict__ ws, Geo g) {
  extern __shared__ float4 lds4[];
  float* red = reinterpret_cast<float*>(lds4);
  float* stage = red + kMaxWaves;
  const int k = MODE == MODE_RESIDENT ? 0 : (int)blockIdx.y, K = MODE == MODE_RESIDENT ? 1 : (int)gridDim.y;
  const int ngroups = g.N / g.G, G = g.G, E = g.E;
  const float Gf = (float)G;
  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const float* xg = x + (size_t)grp * g.GE;
    float* yg = y + (size_t)grp * g.Ly;
    const float* img = xg;
    if (MODE == MODE_RESIDENT) {
      __syncthreads();                                   // the previous group's emit has finished with the image
      float* dst = stage + (int)((reinterpret_cast<uintptr_t>(xg) & 15u) >> 2);
      stage_in(xg, dst, g.GE);
      img = dst;
      __syncthreads();
    }
    float fg = 0.f;
    const float s0 = first_column_s(img, G, E, g.eps);
    if (MODE != MODE_EMIT) {
      float* mg = mu + (size_t)grp * E;
      float* rg = rs + (size_t)grp * E;
      float part = 0.f;
      auto cols = [&](int o, auto width, auto known) {
        constexpr int W = decltype(width)::value;
        constexpr bool A = decltype(known)::value;
        float x0[4], t[4], m[4], v[4], r[4];
        ld<W, A>(img + o, x0);
        // mean as x_0 + mean(x_n - x_0): members that are all equal give mu = x_0 and x - mu = 0 exactly
#pragma unroll
        for (int q = 0; q < W; ++q) m[q] = 0.f;
        for (int n = 1; n < G; ++n) {
          ld<W, A>(img + (size_t)n * E + o, t);
#pragma unroll
          for (int q = 0; q < W; ++q) m[q] += t[q] - x0[q];
        }
#pragma unroll
        for (int q = 0; q < W; ++q) { m[q] = x0[q] + m[q] / Gf; v[q] = 0.f; }
        for (int n = 0; n < G; ++n) {
          ld<W, A>(img + (size_t)n * E + o, t);
#pragma unroll
          for (int q = 0; q < W; ++q) { const float d = t[q] - m[q]; v[q] += d * d; }
        }
#pragma unroll
        for (int q = 0; q < W; ++q) {
          const float s = sqrtf(v[q] / Gf + g.eps);
          r[q] = 1.f / s;
          part += s - s0;
        }
        st<W, A>(mg + o, m);
        st<W, A>(rg + o, r);
      };
      auto c1 = [&](int o) { cols(o, std::integral_constant<int, 1>(), std::false_type()); };
      // the fast path: every float4 of every operand is aligned, established once per group
      if ((E & 3) == 0 && all_aligned(img, mg, rg))
        sweep(reinterpret_cast<uintptr_t>(mg), E, k, K, [&](int o) { cols(o, std::integral_constant<int, 4>(), std::true_type()); }, c1);
      else
        sweep(reinterpret_cast<uintptr_t>(mg), E, k, K, [&](int o) { cols(o, std::integral_constant<int, 4>(), std::false_type()); }, c1);
      const float total = block_sum(part, red);
      if (MODE == MODE_COLUMNS) {
        if (threadIdx.x == 0) ws[(size_t)grp * K + k] = total;
      } else {
        fg = s0 + total / (float)E;
      }
    } else {
      fg = s0 + sum_partials(ws, grp, g.Kc) / (float)E;
    }
    if (MODE != MODE_COLUMNS) {
      if (k == 0 && threadIdx.x == 0) f[grp] = fg;
      emit(yg, [&](int o) { return img[o]; }, fg, g, k, K);
    }
  }
}

// Backward: dx = u[..., :C] + q * k * (x - mu) / s,  q = sum of u[..., C] over the group (every workgroup of the group adds it up
// in the same order); q[group] is kept for the penalty.
__global__ __launch_bounds__(kT) void mbstd_bwd_kernel(const float* __restrict__ u, const float* __restrict__ x, const float* __restrict__ mu,
                                                        const float* __restrict__ rs, float* __restrict__ dx, float* __restrict__ qout, Geo g) {
  __shared__ float red[kMaxWaves];
  const int k = (int)blockIdx.y, K = (int)gridDim.y;
  const int ngroups = g.N / g.G, E = g.E, C = g.C, C1 = g.C + 1;
  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const float* ug = u + (size_t)grp * g.Ly;
    const float* xg = x + (size_t)grp * g.GE;
    const float* mg = mu + (size_t)grp * E;
    const float* rg = rs + (size_t)grp * E;
    float* dg = dx + (size_t)grp * g.GE;
    float part = 0.f;
    for (int j = threadIdx.x, n = g.G * g.P; j < n; j += blockDim.x) part += ug[(size_t)j * C1 + C];
    const float q = block_sum(part, red);
    if (k == 0 && threadIdx.x == 0) qout[grp] = q;
    const float qk = q * g.k;
    auto b1 = [&](int o) {
      const int col = o % E;
      dg[o] = ug[o + o / C] + qk * ((xg[o] - mg[col]) * rg[col]);
    };
    auto b4 = [&](int o, auto known) {
      constexpr bool A = decltype(known)::value;
      float xv[4], m[4], r[4], out[4];
      ld<4, A>(xg + o, xv);
      const int col = o % E;
      if (A || col + 3 < E) {           // the fast path: E % 4 == 0 and aligned bases, no float4 straddles two samples
        ld<4, A>(mg + col, m);
        ld<4, A>(rg + col, r);
      } else {
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          const int c2 = (col + q4) % E;
          m[q4] = mg[c2];
          r[q4] = rg[c2];
        }
      }
      int pix = o / C, c = o - pix * C;
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        out[q4] = ug[o + q4 + pix] + qk * ((xv[q4] - m[q4]) * r[q4]);
        if (++c == C) { c = 0; ++pix; }
      }
      *reinterpret_cast<float4*>(dg + o) = make_float4(out[0], out[1], out[2], out[3]);
    };
    if ((E & 3) == 0 && all_aligned(dg, xg, mg, rg))
      sweep(reinterpret_cast<uintptr_t>(dg), g.GE, k, K, [&](int o) { b4(o, std::true_type()); }, b1);
    else
      sweep(reinterpret_cast<uintptr_t>(dg), g.GE, k, K, [&](int o) { b4(o, std::false_type()); }, b1);
  }
}

// The penalty's tangent and source.  Columns: src and the partial of fdot = k * sum (x - mu) / s * d;  emit: vout = d with fdot in
// channel C.  Modes as the forward's; the resident one keeps d in LDS.
//   src = q * k / s^3 * ( (d - dbar) * eps + [ (d - dbar) * var - (x - mu) * m ] ),   var + eps = s^2,  m = mean_n (x - mu) * d.
// The bracket is (1 / G) sum_j xc_j * (dc_n * xc_j - xc_n * dc_j) over the members' centred values: at G = 2 they are one another's
// negatives bit for bit when formed as half the members' difference, every term vanishes, and the bracket is taken as the 0 it is.
template <int MODE>
__global__ __launch_bounds__(kT) void mbstd_gp_kernel(const float* __restrict__ d, const float* __restrict__ x, const float* __restrict__ mu,
                                                       const float* __restrict__ rs, const float* __restrict__ qin, float* __restrict__ vout,
                                                       float* __restrict__ src, float* __restrict__ fdot, float* __restrict__ ws, Geo g) {
  extern __shared__ float4 lds4[];
  float* red = reinterpret_cast<float*>(lds4);
  float* stage = red + kMaxWaves;
  const int k = MODE == MODE_RESIDENT ? 0 : (int)blockIdx.y, K = MODE == MODE_RESIDENT ? 1 : (int)gridDim.y;
  const int ngroups = g.N / g.G, G = g.G, E = g.E;
  const float Gf = (float)G;
  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const float* dgp = d + (size_t)grp * g.GE;
    const float* xg = x + (size_t)grp * g.GE;
    float* vg = vout + (size_t)grp * g.Ly;
    const float* img = dgp;
    if (MODE == MODE_RESIDENT) {
      __syncthreads();
      float* dst = stage + (int)((reinterpret_cast<uintptr_t>(dgp) & 15u) >> 2);
      stage_in(dgp, dst, g.GE);
      img = dst;
      __syncthreads();
    }
    float fd = 0.f;
    if (MODE != MODE_EMIT) {
      const float* mg = mu + (size_t)grp * E;
      const float* rg = rs + (size_t)grp * E;
      float* sg = src + (size_t)grp * g.GE;
      const float qk = qin[grp] * g.k;
      float part = 0.f;
      auto cols = [&](int o, auto width, auto known) {
        constexpr int W = decltype(width)::value;
        constexpr bool A = decltype(known)::value;
        float m[4], r[4], xv[4], dv[4], x1[4], d1[4], out[4];
        ld<W, A>(mg + o, m);
        ld<W, A>(rg + o, r);
        if (G == 2) {
          ld<W, A>(xg + o, xv);
          ld<W, A>(img + o, dv);
          ld<W, A>(xg + (size_t)E + o, x1);
          ld<W, A>(img + (size_t)E + o, d1);
#pragma unroll
          for (int q = 0; q < W; ++q) {
            part += ((xv[q] - m[q]) * r[q]) * dv[q];
            part += ((x1[q] - m[q]) * r[q]) * d1[q];
            const float dc = (dv[q] - d1[q]) * 0.5f;
            out[q] = qk * (((r[q] * r[q]) * r[q]) * (dc * g.eps));
          }
          st<W, A>(sg + o, out);
#pragma unroll
          for (int q = 0; q < W; ++q) out[q] = -out[q];
          st<W, A>(sg + (size_t)E + o, out);
          return;
        }
        float dbar[4], mm[4], var[4];
        ld<W, A>(img + o, d1);
#pragma unroll
        for (int q = 0; q < W; ++q) { dbar[q] = 0.f; mm[q] = 0.f; var[q] = 0.f; }
        for (int n = 1; n < G; ++n) {
          ld<W, A>(img + (size_t)n * E + o, dv);
#pragma unroll
          for (int q = 0; q < W; ++q) dbar[q] += dv[q] - d1[q];
        }
#pragma unroll
        for (int q = 0; q < W; ++q) dbar[q] = d1[q] + dbar[q] / Gf;
        for (int n = 0; n < G; ++n) {
          ld<W, A>(xg + (size_t)n * E + o, xv);
          ld<W, A>(img + (size_t)n * E + o, dv);
#pragma unroll
          for (int q = 0; q < W; ++q) {
            const float xc = xv[q] - m[q];
            part += (xc * r[q]) * dv[q];
            mm[q] += xc * (dv[q] - dbar[q]);
            var[q] += xc * xc;
          }
        }
#pragma unroll
        for (int q = 0; q < W; ++q) { mm[q] = mm[q] / Gf; var[q] = var[q] / Gf; }
        for (int n = 0; n < G; ++n) {
          ld<W, A>(xg + (size_t)n * E + o, xv);
          ld<W, A>(img + (size_t)n * E + o, dv);
#pragma unroll
          for (int q = 0; q < W; ++q) {
            const float xc = xv[q] - m[q], dc = dv[q] - dbar[q];
            out[q] = qk * (((r[q] * r[q]) * r[q]) * (dc * g.eps + (dc * var[q] - xc * mm[q])));
          }
          st<W, A>(sg + (size_t)n * E + o, out);
        }
      };
      auto c1 = [&](int o) { cols(o, std::integral_constant<int, 1>(), std::false_type()); };
      if ((E & 3) == 0 && all_aligned(img, xg, mg, rg, sg))
        sweep(reinterpret_cast<uintptr_t>(mg), E, k, K, [&](int o) { cols(o, std::integral_constant<int, 4>(), std::true_type()); }, c1);
      else
        sweep(reinterpret_cast<uintptr_t>(mg), E, k, K, [&](int o) { cols(o, std::integral_constant<int, 4>(), std::false_type()); }, c1);
      const float total = block_sum(part, red);
      if (MODE == MODE_COLUMNS) {
        if (threadIdx.x == 0) ws[(size_t)grp * K + k] = total;
      } else {
        fd = total * g.k;
      }
    } else {
      fd = sum_partials(ws, grp, g.Kc) * g.k;
    }
    if (MODE != MODE_COLUMNS) {
      if (k == 0 && threadIdx.x == 0) fdot[grp] = fd;
      emit(vg, [&](int o) { return img[o]; }, fd, g, k, K);
    }
  }
}

// What a call launches for N samples in groups of G with E = P * C floats each: the one place that decides (bg_mbstd_plan reports it).
struct LaunchPlan {
  bool resident;
  unsigned threads, gx, gy_cols, gy_emit;      // gy_cols: workgroups a group's columns (the backward: its dx range) are cut over
  size_t lds;
  int launches;
};

inline LaunchPlan plan_for(int call, int N, int G, size_t E, int C) {
  LaunchPlan p;
  const size_t GE = (size_t)G * E, Ly = GE / C * (C + 1);
  p.threads = kT;
  p.gx = (unsigned)std::min(N / G, kMaxBlocks);
  p.resident = GE <= (size_t)kResident;
  const size_t red_bytes = kMaxWaves * sizeof(float);
  p.lds = red_bytes;
  p.gy_cols = p.gy_emit = 1;
  p.launches = 1;
  if (p.resident) {
    // the image's room: the group, the alignment pad in front of it, rounded up to whole float4s (the backward keeps no image)
    if (call != CALL_BWD) p.lds = red_bytes + (GE + 3 + 3) / 4 * 16;
  } else {
    auto cuts = [](size_t floats) { return (unsigned)std::min<size_t>(std::max<size_t>((floats + kCutFloats - 1) / kCutFloats, 1), kMaxCuts); };
    p.gy_cols = cuts(call == CALL_BWD ? GE : E * (size_t)G);
    // the column phase deals float4s of the E columns: no more cuts than there are float4s
    if (call != CALL_BWD) p.gy_cols = (unsigned)std::min<size_t>(p.gy_cols, std::max<size_t>(E / 4, 1));
    p.gy_emit = cuts(Ly);
    if (call != CALL_BWD) p.launches = 2;
  }
  return p;
}

inline bool host_pointer(const void* p) {
  hipPointerAttribute_t a;
  const hipError_t e = hipPointerGetAttributes(&a, p);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return e == hipErrorInvalidValue;       // a pointer the runtime has never seen (no device: other errors, no verdict)
  }
  return a.type == hipMemoryTypeHost || a.type == hipMemoryTypeUnregistered;
}

int check(const char* what, int N, int G, int P, int C, Geo* g, float eps) {
  BG_REQUIRE(N > 0 && P > 0 && C > 0, BG_ERR_BAD_SHAPE, "%s: N=%d P=%d C=%d", what, N, P, C);
  BG_REQUIRE(G >= 2, BG_ERR_BAD_SHAPE, "%s: group size G=%d (at least 2)", what, G);
  BG_REQUIRE(N % G == 0, BG_ERR_BAD_SHAPE, "%s: N=%d rows are no multiple of the group size G=%d", what, N, G);
  BG_REQUIRE((size_t)G * P * (C + 1) <= (size_t)1 << 30, BG_ERR_BAD_SHAPE, "%s: a group of G=%d P=%d C=%d exceeds 2^30 floats", what, G, P, C);
  g->N = N; g->G = G; g->P = P; g->C = C; g->E = P * C;
  g->GE = G * g->E; g->Ly = G * P * (C + 1);
  g->k = (float)(1.0 / ((double)G * (double)g->E));
  g->Kc = 1;
  g->eps = eps;
  return BG_OK;
}

int pointers(const char* what, std::initializer_list<const void*> ps) {
  for (const void* p : ps) BG_REQUIRE(p, BG_ERR_NULL, "%s: null pointer", what);
  for (const void* p : ps)
    BG_REQUIRE((reinterpret_cast<uintptr_t>(p) & 3u) == 0, BG_ERR_BAD_ALIGNMENT, "%s: pointers must be 4-byte aligned", what);
  for (const void* p : ps) BG_REQUIRE(!host_pointer(p), BG_ERR_UNSUPPORTED, "%s: %p is not device memory", what, p);
  return BG_OK;
}

size_t ws_bytes_for(int N, int G, size_t E, int C) {
  const LaunchPlan p = plan_for(CALL_FWD, N, G, E, C);
  return p.resident ? 0 : (size_t)(N / G) * p.gy_cols * sizeof(float);
}

}  // namespace

extern "C" {

int bg_mbstd_plan(int N, int G, int P, int C, int call, int offset_floats, int* out) {
  Geo g;
  BG_REQUIRE(out, BG_ERR_NULL, "bg_mbstd_plan: null pointer");
  if (int e = check("bg_mbstd_plan", N, G, P, C, &g, 0.f)) return e;
  BG_REQUIRE(call >= CALL_FWD && call <= CALL_GP, BG_ERR_UNSUPPORTED, "bg_mbstd_plan: call=%d (0 forward, 1 backward, 2 penalty)", call);
  BG_REQUIRE(offset_floats >= 0 && offset_floats < 4, BG_ERR_UNSUPPORTED, "bg_mbstd_plan: offset_floats=%d outside [0, 4)", offset_floats);
  const LaunchPlan p = plan_for(call, N, G, (size_t)g.E, C);
  // the sweep the plan describes: the columns of group 0 (forward, penalty: E floats from mu's address) or its dx range (backward)
  const int n = call == CALL_BWD ? g.GE : g.E, K = (int)p.gy_cols, T = (int)p.threads;
  const int h = std::min((4 - offset_floats) & 3, n), nv = (n - h) >> 2, per = (nv + K - 1) / K;
  const int last = std::max(nv - (K - 1) * per, 0);        // float4s of the last cut (the ragged one)
  out[0] = p.resident ? 1 : 0;
  out[1] = T;
  out[2] = (int)p.gx;
  out[3] = K;
  out[4] = (int)p.gy_emit;
  out[5] = (int)p.lds;
  out[6] = p.launches;
  out[7] = nv;
  out[8] = last / T;
  out[9] = (per + T - 1) / T;
  out[10] = h;
  out[11] = n - h - 4 * nv;
  return BG_OK;
}

size_t bg_mbstd_workspace_bytes(int N, int G, int P, int C) {
  if (N <= 0 || G < 2 || P <= 0 || C <= 0 || N % G) return 0;
  return ws_bytes_for(N, G, (size_t)P * C, C);
}

int bg_mbstd_fwd_f32(const float* x, float* y, float* mu, float* rs, float* f, int N, int G, int P, int C, float eps, void* ws_d,
                     size_t ws_bytes, void* stream) {
  Geo g;
  if (int e = check("bg_mbstd_fwd_f32", N, G, P, C, &g, eps)) return e;
  BG_REQUIRE(eps > 0.f, BG_ERR_UNSUPPORTED, "bg_mbstd_fwd_f32: eps=%g (must be positive)", (double)eps);
  if (int e = pointers("bg_mbstd_fwd_f32", {x, y, mu, rs, f})) return e;
  const LaunchPlan p = plan_for(CALL_FWD, N, G, (size_t)g.E, C);
  const size_t need = ws_bytes_for(N, G, (size_t)g.E, C);
  BG_REQUIRE(need == 0 || (ws_d && ws_bytes >= need), BG_ERR_WORKSPACE, "bg_mbstd_fwd_f32: workspace of %zu bytes, %zu needed", ws_bytes, need);
  float* ws = static_cast<float*>(ws_d);
  g.Kc = (int)p.gy_cols;
  const double bytes = 4.0 * ((double)N * g.E * 2 + (double)N * P + 2.0 * (N / G) * g.E);
  if (p.resident) {
    bg::Launch L(stream, "mbstd_fwd", 0, bytes);
    bg::launch(mbstd_fwd_kernel<MODE_RESIDENT>, dim3(p.gx), dim3(p.threads), p.lds, L.s, x, y, mu, rs, f, ws, g);
    return L.done("mbstd_fwd_kernel");
  }
  {
    bg::Launch L(stream, "mbstd_fwd_columns", 0, bytes / 2);
    bg::launch(mbstd_fwd_kernel<MODE_COLUMNS>, dim3(p.gx, p.gy_cols), dim3(p.threads), p.lds, L.s, x, y, mu, rs, f, ws, g);
    if (int e = L.done("mbstd_fwd_kernel")) return e;
  }
  bg::Launch L(stream, "mbstd_fwd_emit", 0, bytes / 2);
  bg::launch(mbstd_fwd_kernel<MODE_EMIT>, dim3(p.gx, p.gy_emit), dim3(p.threads), p.lds, L.s, x, y, mu, rs, f, ws, g);
  return L.done("mbstd_fwd_kernel");
}

int bg_mbstd_bwd_f32(const float* u, const float* x, const float* mu, const float* rs, float* dx, float* q, int N, int G, int P, int C,
                     void* stream) {
  Geo g;
  if (int e = check("bg_mbstd_bwd_f32", N, G, P, C, &g, 0.f)) return e;
  if (int e = pointers("bg_mbstd_bwd_f32", {u, x, mu, rs, dx, q})) return e;
  const LaunchPlan p = plan_for(CALL_BWD, N, G, (size_t)g.E, C);
  bg::Launch L(stream, "mbstd_bwd", 0, 4.0 * ((double)N * g.E * 3 + (double)N * P + 2.0 * (N / G) * g.E));
  bg::launch(mbstd_bwd_kernel, dim3(p.gx, p.gy_cols), dim3(p.threads), 0, L.s, u, x, mu, rs, dx, q, g);
  return L.done("mbstd_bwd_kernel");
}

int bg_mbstd_gp_f32(const float* d, const float* x, const float* mu, const float* rs, const float* q, float* vout, float* src,
                    float* fdot, int N, int G, int P, int C, float eps, void* ws_d, size_t ws_bytes, void* stream) {
  Geo g;
  if (int e = check("bg_mbstd_gp_f32", N, G, P, C, &g, eps)) return e;
  BG_REQUIRE(eps > 0.f, BG_ERR_UNSUPPORTED, "bg_mbstd_gp_f32: eps=%g (must be positive)", (double)eps);
  if (int e = pointers("bg_mbstd_gp_f32", {d, x, mu, rs, q, vout, src, fdot})) return e;
  const LaunchPlan p = plan_for(CALL_GP, N, G, (size_t)g.E, C);
  const size_t need = ws_bytes_for(N, G, (size_t)g.E, C);
  BG_REQUIRE(need == 0 || (ws_d && ws_bytes >= need), BG_ERR_WORKSPACE, "bg_mbstd_gp_f32: workspace of %zu bytes, %zu needed", ws_bytes, need);
  float* ws = static_cast<float*>(ws_d);
  g.Kc = (int)p.gy_cols;
  const double bytes = 4.0 * ((double)N * g.E * 4 + (double)N * P + 2.0 * (N / G) * g.E);
  if (p.resident) {
    bg::Launch L(stream, "mbstd_gp", 0, bytes);
    bg::launch(mbstd_gp_kernel<MODE_RESIDENT>, dim3(p.gx), dim3(p.threads), p.lds, L.s, d, x, mu, rs, q, vout, src, fdot, ws, g);
    return L.done("mbstd_gp_kernel");
  }
  {
    bg::Launch L(stream, "mbstd_gp_columns", 0, bytes * 0.6);
    bg::launch(mbstd_gp_kernel<MODE_COLUMNS>, dim3(p.gx, p.gy_cols), dim3(p.threads), p.lds, L.s, d, x, mu, rs, q, vout, src, fdot, ws, g);
    if (int e = L.done("mbstd_gp_kernel")) return e;
  }
  bg::Launch L(stream, "mbstd_gp_emit", 0, bytes * 0.4);
  bg::launch(mbstd_gp_kernel<MODE_EMIT>, dim3(p.gx, p.gy_emit), dim3(p.threads), p.lds, L.s, d, x, mu, rs, q, vout, src, fdot, ws, g);
  return L.done("mbstd_gp_kernel");
}

}  // extern "C"
