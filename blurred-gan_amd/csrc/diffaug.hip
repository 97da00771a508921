// Differentiable augmentation in front of the critic (include/bgan.h "differentiable augmentation"; Zhao et al. 2020): per sample a
// colour jitter, a translation and a cutout, T(x) = L x + k, and the adjoint L^T the critic's input gradient goes through.  Data is
// [n, H, W, C] fp32, a sample E = H * W * C contiguous floats; every statistic is a mean over ONE sample, so samples are independent.
//
// Both directions are the same three steps on one sample, one launch for all samples:
//   sweep 1   read the sample once, 16 bytes per lane where the sample's address allows (scalar head and tail), adding up what the
//             sample mean is taken over -- the forward: every element; the adjoint: the elements of g that L^T does not drop.  Only
//             with ``color`` in the policy: without it there is no mean, sweep 1 and the LDS image are skipped on either route,
//             and sweep 2 copies values bit for bit straight from memory.
//   reduce    per-thread partials in loop order, a fixed shuffle tree per wave, the four waves added in wave order: the same bits
//             on every run, no atomics.
//   sweep 2   every lane forms four consecutive OUTPUT elements and stores them as one float4 (scalar head and tail again); the
//             source pixel of each -- shifted by the translation, so never aligned -- is read one float at a time.
// Routes (bg_diffaug_route): a sample of at most kResident floats is kept in LDS between the sweeps (read from memory ONCE, one
// workgroup per sample, its LDS sized to the sample; 1024 threads from 8192 floats on, so that the two workgroups a compute unit
// then holds fill its wave slots, 256 below); a larger one is swept twice from memory, the second time out of L2, and its output is cut along
// gridDim.y so that a small batch of large images still fills the chip (every workgroup of a sample repeats sweep 1 in the same
// order: the same mean, bit for bit).
#include "common.h"
#include "reduce.h"
#include <algorithm>
#include <cmath>

namespace {

constexpr int kTBig = 1024, kTSmall = 256, kMaxWaves = kTBig / 64, kMaxBlocks = 1024;
constexpr int kBigFloats = 8192;           // samples from this size on get workgroups of kTBig threads, smaller ones kTSmall
constexpr int kResident = 15360 - 4;       // floats of a sample the resident route takes (60 KiB of LDS less the alignment pad)
constexpr int kBatch = 3;
constexpr int kChunkFloats = 8192;         // two-sweep route: at least this much output per workgroup

enum { OP_COLOR = 1, OP_TRANSLATION = 2, OP_CUTOUT = 4 };

struct Geo {
  int n, H, W, C, E;
  int ops, linear;
  int Sy, Sx, cy, cx;       // shift ranges and cutout size (host: round half up of extent * ratio)
};

// one sample's draw, decoded (bgan.h): float32 arithmetic, one multiply per value
struct Draw {
  float b, s, c;
  int ty, tx, y0, x0, y1, x1;      // the cutout box is rows [y0, y1) x columns [x0, x1); it may reach outside the map
};

__host__ __device__ inline int pick(float u, int n) {        // min(floor(u * n), n - 1)
  const int k = (int)floorf(u * (float)n);
  return k < n - 1 ? k : n - 1;
}

__host__ __device__ inline Draw decode(const float* u, const Geo& g) {
  Draw d;
  d.b = 0.f; d.s = 1.f; d.c = 1.f;
  d.ty = d.tx = 0;
  d.y0 = d.y1 = d.x0 = d.x1 = 0;
  if (g.ops & OP_COLOR) {
    d.b = g.linear ? 0.f : u[0] - 0.5f;
    d.s = 2.f * u[1];
    d.c = u[2] + 0.5f;
  }
  if (g.ops & OP_TRANSLATION) {
    d.ty = pick(u[3], 2 * g.Sy + 1) - g.Sy;
    d.tx = pick(u[4], 2 * g.Sx + 1) - g.Sx;
  }
  if (g.ops & OP_CUTOUT) {
    d.y0 = pick(u[5], g.H + 1 - (g.cy & 1)) - g.cy / 2;
    d.x0 = pick(u[6], g.W + 1 - (g.cx & 1)) - g.cx / 2;
    d.y1 = d.y0 + g.cy;
    d.x1 = d.x0 + g.cx;
  }
  return d;
}

inline int round_half_up(int extent, float ratio) { return (int)floorf((float)extent * ratio + 0.5f); }

using bg::block_sum;      // reduce.h: the workgroup's sum; red may still be read from the previous sample, hence its first barrier
using bg::sweep;          // reduce.h: scalar head, float4 runs dealt to the K workgroups of the sample, scalar tail

// sweep() over a whole sample for reading: the float4s are LOADED kBatch at a time per lane (ld) before any is consumed (use), so a
// lane waits for memory once per batch (three: a 64 x 64 x 3 sample in one batch of a 1024-thread workgroup, in 64 registers); they are consumed in the loop's own order, which keeps a lane's partial sum's bits
template <class Ld, class Use, class F1>
__device__ __forceinline__ void sweep_read(uintptr_t addr, int E, Ld ld, Use use, F1 f1) {
  const int tid = threadIdx.x, T = blockDim.x;
  int head = (int)(((16u - (unsigned)(addr & 15u)) & 15u) >> 2);
  head = head < E ? head : E;
  const int nvec = (E - head) >> 2, tail0 = head + 4 * nvec;
  if (tid < head) f1(tid);
  for (int v = tid; v < nvec; v += kBatch * T) {
    float4 r[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; ++u)
      if (v + u * T < nvec) r[u] = ld(head + 4 * (v + u * T));
#pragma unroll
    for (int u = 0; u < kBatch; ++u)
      if (v + u * T < nvec) use(head + 4 * (v + u * T), r[u]);
  }
  if (tid < E - tail0) f1(tail0 + tid);
}

// ADJ = false:  y = T(x) (linear: L x).   ADJ = true:  dx = L^T g.
// RESIDENT: the sample waits in LDS between the sweeps; else it is read from memory twice and blockIdx.y cuts the output.
template <bool ADJ, bool RESIDENT>
__global__ __launch_bounds__(kTBig, 8) void diffaug_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                        const float* __restrict__ params, Geo g) {
  // dynamic LDS (lds_bytes): the waves' partial sums, then -- resident route -- the sample's image, 16-byte aligned
  extern __shared__ float4 lds4[];
  float* red = reinterpret_cast<float*>(lds4);
  float* stage = red + kMaxWaves;
  const bool color = (g.ops & OP_COLOR) != 0;
  const int W = g.W, H = g.H, C = g.C, E = g.E;
  const float Ef = (float)E, Cf = (float)C;
  const int k = RESIDENT ? 0 : (int)blockIdx.y, K = RESIDENT ? 1 : (int)gridDim.y;
  for (int smp = blockIdx.x; smp < g.n; smp += gridDim.x) {
    const float* src = in + (size_t)smp * E;
    float* dst = out + (size_t)smp * E;
    const Draw d = decode(params + (size_t)smp * 8, g);
    // source pixel of output pixel (i, j): the forward gathers from (i + ty, j + tx), the adjoint from (i - ty, j - tx); the
    // cutout acts on the coordinates of y: the forward's output pixel, the adjoint's source pixel
    const int dy = ADJ ? -d.ty : d.ty, dxs = ADJ ? -d.tx : d.tx;
    auto cut = [&](int i, int j) { return i >= d.y0 && i < d.y1 && j >= d.x0 && j < d.x1; };
    const uintptr_t saddr = reinterpret_cast<uintptr_t>(src);
    // LDS image of the sample, shifted so that the float4s of sweep 1 land 16-byte aligned there too
    const int pad = RESIDENT ? (int)((saddr & 15u) >> 2) : 0;
    float mean = 0.f;
    if (RESIDENT || color) {
      if (RESIDENT) __syncthreads();                     // the previous sample's sweep 2 has finished with the image
      float part = 0.f;
      // what element o adds to the mean: the forward all of x, the adjoint g where L^T keeps it (not cut, and its target
      // (i + ty, j + tx) inside the map)
      auto live = [&](int i, int j) {
        return !ADJ || (!cut(i, j) && (unsigned)(i + d.ty) < (unsigned)H && (unsigned)(j + d.tx) < (unsigned)W);
      };
      auto f1 = [&](int o) {
        const float v = src[o];
        if (RESIDENT) stage[pad + o] = v;
        const int pix = o / C, i = pix / W;
        if (color && live(i, pix - i * W)) part += v;
      };
      auto ld = [&](int o) { return *reinterpret_cast<const float4*>(src + o); };
      auto f4 = [&](int o, const float4& v) {
        if (RESIDENT) *reinterpret_cast<float4*>(stage + pad + o) = v;
        if (color) {
          if (!ADJ) {
            part += (v.x + v.y) + (v.z + v.w);
          } else {
            const int pix = o / C;
            int ch = o - pix * C, i = pix / W, j = pix - i * W;
            bool ok = live(i, j);
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              if (ok) part += e[q];
              if (++ch == C) {
                ch = 0;
                if (++j == W) { j = 0; ++i; }
                ok = live(i, j);
              }
            }
          }
        }
      };
      sweep_read(saddr, E, ld, f4, f1);
      if (color) mean = block_sum(part, red) / Ef;
      else if (RESIDENT) __syncthreads();
    }
    // what L^T leaves where it gathers nothing (h = 0):  e = (1 - c) * mean,  s * e + (1 - s) * e
    const float e0 = (1.f - d.c) * mean, fill = color && ADJ ? d.s * e0 + (1.f - d.s) * e0 : 0.f;
    auto at = [&](int o) { return RESIDENT ? stage[pad + o] : src[o]; };
    // what the output elements of pixel (i, j) share: whether they gather anything, where from, and the source pixel's channel mean
    struct Px { bool live; int base; float m; };
    auto pixel = [&](int i, int j) {
      Px p;
      const int si = i + dy, sj = j + dxs;
      p.live = (unsigned)si < (unsigned)H && (unsigned)sj < (unsigned)W && !(ADJ ? cut(si, sj) : cut(i, j));
      p.base = (si * W + sj) * C;
      p.m = 0.f;
      if (color && p.live) {
        for (int q = 0; q < C; ++q) p.m += at(p.base + q);
        p.m /= Cf;
      }
      return p;
    };
    auto value = [&](const Px& p, int ch) {
      if (!p.live) return fill;
      const float v = at(p.base + ch);
      if (!color) return v;
      if (!ADJ) return d.c * (d.s * (v - p.m) + p.m - mean) + mean + d.b;
      const float e = d.c * v + (1.f - d.c) * mean, me = d.c * p.m + (1.f - d.c) * mean;
      return d.s * e + (1.f - d.s) * me;
    };
    auto g1 = [&](int o) {
      const int pix = o / C, i = pix / W;
      dst[o] = value(pixel(i, pix - i * W), o - pix * C);
    };
    auto g4 = [&](int o) {
      const int pix = o / C;
      int ch = o - pix * C, i = pix / W, j = pix - i * W;
      Px p = pixel(i, j);
      float r[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        r[q] = value(p, ch);
        if (++ch == C && q < 3) {
          ch = 0;
          if (++j == W) { j = 0; ++i; }
          p = pixel(i, j);
        }
      }
      *reinterpret_cast<float4*>(dst + o) = make_float4(r[0], r[1], r[2], r[3]);
    };
    sweep(reinterpret_cast<uintptr_t>(dst), E, k, K, g4, g1);
  }
}

inline bool resident(size_t E) { return E <= (size_t)kResident; }

// What run() launches for n samples of E floats: the one place that decides (bg_diffaug_plan reports it).
struct LaunchPlan { bool resident; unsigned threads, gx, gy; size_t lds; };

inline LaunchPlan plan_for(int n, size_t E, int ops_mask) {
  const bool color = (ops_mask & OP_COLOR) != 0;
  LaunchPlan p;
  p.gx = (unsigned)std::min(n, kMaxBlocks);
  p.gy = 1;
  p.threads = color && E >= (size_t)kBigFloats ? kTBig : kTSmall;
  const size_t red_bytes = kMaxWaves * sizeof(float);
  // (without colour there is no mean to wait for: every sample size is one gathering sweep straight from memory)
  p.resident = resident(E) && color;
  if (p.resident) {
    // the image's room: the sample, the alignment pad in front of it, rounded up to whole float4s
    p.lds = red_bytes + (E + 3 + 3) / 4 * 16;
  } else {
    // a small batch of large images is cut along the sample until the chip has two workgroups per compute unit: with colour every
    // workgroup of a sample repeats sweep 1, so no further.  Without colour a cut costs nothing: 256-thread workgroups, eight per
    // compute unit, at least a quarter of a chunk each
    const unsigned want = color ? 512u : 2048u;
    unsigned gy = (unsigned)std::min<size_t>(std::max<size_t>(E / (color ? kChunkFloats : kChunkFloats / 4), 1), 64);
    p.gy = std::min(gy, std::max(1u, want / p.gx));
    p.lds = red_bytes;
  }
  return p;
}

int run(bool adj, const float* in, float* out, const float* params, int n, int H, int W, int C, int ops_mask, float translation_ratio,
        float cutout_ratio, int linear, void* stream, const char* what) {
  BG_REQUIRE(in && out && params, BG_ERR_NULL, "%s: null pointer", what);
  BG_REQUIRE(n > 0 && H > 0 && W > 0 && C > 0 && (size_t)H * W * C <= (size_t)1 << 30, BG_ERR_BAD_SHAPE, "%s: n=%d H=%d W=%d C=%d", what,
             n, H, W, C);
  BG_REQUIRE(ops_mask >= 0 && ops_mask <= 7, BG_ERR_UNSUPPORTED, "%s: ops_mask=%d (bits: 1 color, 2 translation, 4 cutout)", what, ops_mask);
  BG_REQUIRE(translation_ratio >= 0.f && translation_ratio <= 1.f && cutout_ratio >= 0.f && cutout_ratio <= 1.f, BG_ERR_UNSUPPORTED,
             "%s: translation_ratio=%g cutout_ratio=%g outside [0, 1]", what, (double)translation_ratio, (double)cutout_ratio);
  const size_t E = (size_t)H * W * C, bytes = (size_t)n * E * sizeof(float);
  const char *a = reinterpret_cast<const char*>(in), *b = reinterpret_cast<const char*>(out);
  BG_REQUIRE(a + bytes <= b || b + bytes <= a, BG_ERR_UNSUPPORTED, "%s: the output must not overlap the input (a gather: every output "
             "element reads other positions of the input)", what);
  BG_REQUIRE(((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(params)) & 3u) == 0,
             BG_ERR_BAD_ALIGNMENT, "%s: pointers must be 4-byte aligned", what);
  Geo g;
  g.n = n; g.H = H; g.W = W; g.C = C; g.E = (int)E;
  g.ops = ops_mask; g.linear = linear ? 1 : 0;
  g.Sy = round_half_up(H, translation_ratio); g.Sx = round_half_up(W, translation_ratio);
  g.cy = round_half_up(H, cutout_ratio); g.cx = round_half_up(W, cutout_ratio);
  const LaunchPlan p = plan_for(n, E, ops_mask);
  bg::Launch L(stream, adj ? "diffaug_adjoint" : "diffaug", 0, 8.0 * n * E + 32.0 * n);
  const dim3 grid(p.gx, p.gy), block(p.threads);
  if (p.resident) {
    if (adj) bg::launch(diffaug_kernel<true, true>, grid, block, p.lds, L.s, in, out, params, g);
    else bg::launch(diffaug_kernel<false, true>, grid, block, p.lds, L.s, in, out, params, g);
  } else {
    if (adj) bg::launch(diffaug_kernel<true, false>, grid, block, p.lds, L.s, in, out, params, g);
    else bg::launch(diffaug_kernel<false, false>, grid, block, p.lds, L.s, in, out, params, g);
  }
  return L.done("diffaug_kernel");
}

}  // namespace

extern "C" {

int bg_diffaug_route(int H, int W, int C, int* is_resident, int* resident_floats) {
  BG_REQUIRE(H > 0 && W > 0 && C > 0, BG_ERR_BAD_SHAPE, "bg_diffaug_route: H=%d W=%d C=%d", H, W, C);
  if (is_resident) *is_resident = resident((size_t)H * W * C) ? 1 : 0;
  if (resident_floats) *resident_floats = kResident;
  return BG_OK;
}

int bg_diffaug_plan(int n, int H, int W, int C, int ops_mask, int* is_resident, int* threads, int* grid_x, int* grid_y, int* lds_bytes) {
  BG_REQUIRE(n > 0 && H > 0 && W > 0 && C > 0 && (size_t)H * W * C <= (size_t)1 << 30, BG_ERR_BAD_SHAPE, "bg_diffaug_plan: n=%d H=%d W=%d C=%d", n, H,
             W, C);
  BG_REQUIRE(ops_mask >= 0 && ops_mask <= 7, BG_ERR_UNSUPPORTED, "bg_diffaug_plan: ops_mask=%d (bits: 1 color, 2 translation, 4 cutout)", ops_mask);
  const LaunchPlan p = plan_for(n, (size_t)H * W * C, ops_mask);
  if (is_resident) *is_resident = p.resident ? 1 : 0;
  if (threads) *threads = (int)p.threads;
  if (grid_x) *grid_x = (int)p.gx;
  if (grid_y) *grid_y = (int)p.gy;
  if (lds_bytes) *lds_bytes = (int)p.lds;
  return BG_OK;
}

int bg_diffaug_decode(const float* u, int H, int W, int ops_mask, float translation_ratio, float cutout_ratio, float* bsc, int* geo) {
  BG_REQUIRE(u && bsc && geo, BG_ERR_NULL, "bg_diffaug_decode: null pointer");
  BG_REQUIRE(H > 0 && W > 0, BG_ERR_BAD_SHAPE, "bg_diffaug_decode: H=%d W=%d", H, W);
  Geo g;
  g.n = 1; g.H = H; g.W = W; g.C = 1; g.E = H * W;
  g.ops = ops_mask; g.linear = 0;
  g.Sy = round_half_up(H, translation_ratio); g.Sx = round_half_up(W, translation_ratio);
  g.cy = round_half_up(H, cutout_ratio); g.cx = round_half_up(W, cutout_ratio);
  const Draw d = decode(u, g);
  bsc[0] = d.b; bsc[1] = d.s; bsc[2] = d.c;
  geo[0] = d.ty; geo[1] = d.tx; geo[2] = d.y0; geo[3] = d.x0; geo[4] = g.cy; geo[5] = g.cx; geo[6] = g.Sy; geo[7] = g.Sx;
  return BG_OK;
}

int bg_diffaug_f32(const float* x, float* y, const float* params, int n, int H, int W, int C, int ops_mask, float translation_ratio,
                   float cutout_ratio, int linear, void* stream) {
  return run(false, x, y, params, n, H, W, C, ops_mask, translation_ratio, cutout_ratio, linear, stream, "bg_diffaug_f32");
}

int bg_diffaug_adjoint_f32(const float* dy, float* dx, const float* params, int n, int H, int W, int C, int ops_mask,
                           float translation_ratio, float cutout_ratio, void* stream) {
  return run(true, dy, dx, params, n, H, W, C, ops_mask, translation_ratio, cutout_ratio, 1, stream, "bg_diffaug_adjoint_f32");
}

}  // extern "C"
