// The DiffAugment kernel template and its launcher, shared by diffaug.hip (the ungated entry points: GATED = false, the kernels
// that file has always held) and ada.hip (the gated entry points of adaptive augmentation: GATED = true).  Everything is in an
// unnamed namespace: each of the two files gets its own instantiations, and neither holds the other's kernels.
#pragma once
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

// what a kernel receives: Geo as it is for the ungated calls (the same kernel arguments as before the gate existed), Geo and the
// device address of p for the gated ones
template <bool GATED> struct KGeo : Geo {};
template <> struct KGeo<true> : Geo { const float* gate_p; };

// one sample's draw, decoded (bgan.h): float32 arithmetic, one multiply per value
struct Draw {
  float b, s, c;
  int ty, tx, y0, x0, y1, x1;      // the cutout box is rows [y0, y1) x columns [x0, x1); it may reach outside the map
};

__host__ __device__ inline int pick(float u, int n) {        // min(floor(u * n), n - 1)
  const int k = (int)floorf(u * (float)n);
  return k < n - 1 ? k : n - 1;
}

__host__ __device__ inline Draw decode(const float* u, const Geo& g, int ops) {
  Draw d;
  d.b = 0.f; d.s = 1.f; d.c = 1.f;
  d.ty = d.tx = 0;
  d.y0 = d.y1 = d.x0 = d.x1 = 0;
  if (ops & OP_COLOR) {
    d.b = g.linear ? 0.f : u[0] - 0.5f;
    d.s = 2.f * u[1];
    d.c = u[2] + 0.5f;
  }
  if (ops & OP_TRANSLATION) {
    d.ty = pick(u[3], 2 * g.Sy + 1) - g.Sy;
    d.tx = pick(u[4], 2 * g.Sx + 1) - g.Sx;
  }
  if (ops & OP_CUTOUT) {
    d.y0 = pick(u[5], g.H + 1 - (g.cy & 1)) - g.cy / 2;
    d.x0 = pick(u[6], g.W + 1 - (g.cx & 1)) - g.cx / 2;
    d.y1 = d.y0 + g.cy;
    d.x1 = d.x0 + g.cx;
  }
  return d;
}

// the gated calls (bgan.h): a row is 12 uniforms, u8 / u9 / u10 the gates of colour / translation / cutout; an operation of the
// policy fires iff its gate is below p, compared in float32 (u < 1 always holds: p = 1 is the ungated call)
constexpr int kRow = 8, kRowGated = 12;

__host__ __device__ inline int fired_ops(const float* u, float p, int ops) {
  return ops & ((u[8] < p ? OP_COLOR : 0) | (u[9] < p ? OP_TRANSLATION : 0) | (u[10] < p ? OP_CUTOUT : 0));
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
// GATED: rows of kRowGated uniforms, and the sample's operations are those of the policy whose gate is below *g.gate_p, read from
// device memory at launch time (a replayed step program sees the controller's current p).  The mask is uniform over the workgroup,
// so a sample without colour skips sweep 1 and the LDS image and gathers straight from memory, as a policy without colour does.
// Without GATED there is no gate_p to read, and every branch on the mask is the kernel-uniform one of before.
template <bool ADJ, bool RESIDENT, bool GATED>
__global__ __launch_bounds__(kTBig, 8) void diffaug_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                        const float* __restrict__ params, KGeo<GATED> g) {
  // dynamic LDS (lds_bytes): the waves' partial sums, then -- resident route -- the sample's image, 16-byte aligned
  extern __shared__ float4 lds4[];
  float* red = reinterpret_cast<float*>(lds4);
  float* stage = red + kMaxWaves;
  float pgate = 0.f;
  if constexpr (GATED) pgate = *g.gate_p;
  const bool policy_color = (g.ops & OP_COLOR) != 0;
  const int W = g.W, H = g.H, C = g.C, E = g.E;
  const float Ef = (float)E, Cf = (float)C;
  const int k = RESIDENT ? 0 : (int)blockIdx.y, K = RESIDENT ? 1 : (int)gridDim.y;
  for (int smp = blockIdx.x; smp < g.n; smp += gridDim.x) {
    const float* src = in + (size_t)smp * E;
    float* dst = out + (size_t)smp * E;
    const float* u = params + (size_t)smp * (GATED ? kRowGated : kRow);
    const int ops = GATED ? fired_ops(u, pgate, g.ops) : g.ops;
    const bool color = GATED ? (ops & OP_COLOR) != 0 : policy_color;
    const bool staged = RESIDENT && (!GATED || color);      // whether this sample's image goes through LDS
    const Draw d = decode(u, g, ops);
    // source pixel of output pixel (i, j): the forward gathers from (i + ty, j + tx), the adjoint from (i - ty, j - tx); the
    // cutout acts on the coordinates of y: the forward's output pixel, the adjoint's source pixel
    const int dy = ADJ ? -d.ty : d.ty, dxs = ADJ ? -d.tx : d.tx;
    auto cut = [&](int i, int j) { return i >= d.y0 && i < d.y1 && j >= d.x0 && j < d.x1; };
    const uintptr_t saddr = reinterpret_cast<uintptr_t>(src);
    // LDS image of the sample, shifted so that the float4s of sweep 1 land 16-byte aligned there too
    const int pad = staged ? (int)((saddr & 15u) >> 2) : 0;
    float mean = 0.f;
    if (staged || color) {
      if (staged) __syncthreads();                     // the previous sample's sweep 2 has finished with the image
      float part = 0.f;
      // what element o adds to the mean: the forward all of x, the adjoint g where L^T keeps it (not cut, and its target
      // (i + ty, j + tx) inside the map)
      auto live = [&](int i, int j) {
        return !ADJ || (!cut(i, j) && (unsigned)(i + d.ty) < (unsigned)H && (unsigned)(j + d.tx) < (unsigned)W);
      };
      auto f1 = [&](int o) {
        const float v = src[o];
        if (staged) stage[pad + o] = v;
        const int pix = o / C, i = pix / W;
        if (color && live(i, pix - i * W)) part += v;
      };
      auto ld = [&](int o) { return *reinterpret_cast<const float4*>(src + o); };
      auto f4 = [&](int o, const float4& v) {
        if (staged) *reinterpret_cast<float4*>(stage + pad + o) = v;
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
      else if (staged) __syncthreads();
    }
    // what L^T leaves where it gathers nothing (h = 0):  e = (1 - c) * mean,  s * e + (1 - s) * e
    const float e0 = (1.f - d.c) * mean, fill = color && ADJ ? d.s * e0 + (1.f - d.s) * e0 : 0.f;
    auto at = [&](int o) { return staged ? stage[pad + o] : src[o]; };
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

// gate_p: NULL for the ungated calls; the gated ones have refused a null p before they come here
template <bool GATED>
int run(bool adj, const float* in, float* out, const float* params, const float* gate_p, int n, int H, int W, int C, int ops_mask,
        float translation_ratio, float cutout_ratio, int linear, void* stream, const char* what) {
  BG_REQUIRE(in && out && params && (!GATED || gate_p), BG_ERR_NULL, "%s: null pointer", what);
  BG_REQUIRE(n > 0 && H > 0 && W > 0 && C > 0 && (size_t)H * W * C <= (size_t)1 << 30, BG_ERR_BAD_SHAPE, "%s: n=%d H=%d W=%d C=%d", what,
             n, H, W, C);
  BG_REQUIRE(ops_mask >= 0 && ops_mask <= 7, BG_ERR_UNSUPPORTED, "%s: ops_mask=%d (bits: 1 color, 2 translation, 4 cutout)", what, ops_mask);
  BG_REQUIRE(translation_ratio >= 0.f && translation_ratio <= 1.f && cutout_ratio >= 0.f && cutout_ratio <= 1.f, BG_ERR_UNSUPPORTED,
             "%s: translation_ratio=%g cutout_ratio=%g outside [0, 1]", what, (double)translation_ratio, (double)cutout_ratio);
  const size_t E = (size_t)H * W * C, bytes = (size_t)n * E * sizeof(float);
  const char *a = reinterpret_cast<const char*>(in), *b = reinterpret_cast<const char*>(out);
  BG_REQUIRE(a + bytes <= b || b + bytes <= a, BG_ERR_UNSUPPORTED, "%s: the output must not overlap the input (a gather: every output "
             "element reads other positions of the input)", what);
  BG_REQUIRE(((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(params) |
               reinterpret_cast<uintptr_t>(gate_p)) & 3u) == 0,
             BG_ERR_BAD_ALIGNMENT, "%s: pointers must be 4-byte aligned", what);
  KGeo<GATED> g;
  if constexpr (GATED) g.gate_p = gate_p;
  g.n = n; g.H = H; g.W = W; g.C = C; g.E = (int)E;
  g.ops = ops_mask; g.linear = linear ? 1 : 0;
  g.Sy = round_half_up(H, translation_ratio); g.Sx = round_half_up(W, translation_ratio);
  g.cy = round_half_up(H, cutout_ratio); g.cx = round_half_up(W, cutout_ratio);
  const LaunchPlan p = plan_for(n, E, ops_mask);
  bg::Launch L(stream, GATED ? (adj ? "diffaug_gated_adjoint" : "diffaug_gated") : (adj ? "diffaug_adjoint" : "diffaug"), 0,
               8.0 * n * E + (GATED ? 48.0 : 32.0) * n);
  const dim3 grid(p.gx, p.gy), block(p.threads);
  if (p.resident) {
    if (adj) bg::launch(diffaug_kernel<true, true, GATED>, grid, block, p.lds, L.s, in, out, params, g);
    else bg::launch(diffaug_kernel<false, true, GATED>, grid, block, p.lds, L.s, in, out, params, g);
  } else {
    if (adj) bg::launch(diffaug_kernel<true, false, GATED>, grid, block, p.lds, L.s, in, out, params, g);
    else bg::launch(diffaug_kernel<false, false, GATED>, grid, block, p.lds, L.s, in, out, params, g);
  }
  return L.done("diffaug_kernel");
}

}  // namespace
