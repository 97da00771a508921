// Sliced Wasserstein distance on the device (include/bgan.h "SWD metric"; reference sliced_wasserstein.py:13-51,72-88): the
// evaluation the reference's SWDMetricCallback runs inside the training loop.  Everything works on float32 planar NCHW buffers,
// the metric's layout, and everything is bandwidth-bound:
//   ingest       model.images (NHWC or NCHW, 1 or 3 channels) -> [B,3,H,W] * scale + shift                       one launch
//   pyr_down     5-tap binomial, reflect-101, keep every second pixel: the host pyr_down BIT FOR BIT              one launch
//   pyr_up       zero-stuff, the same filter, gain 4, optionally minuend - result: one Laplacian level            one launch
//   gather       nhood x nhood x 3 patches around int32 centres the host drew: 8 bytes uploaded per descriptor    one launch
//   standardize  per-channel mean / population std in float64 (two-stage partials, fixed order), applied in place  four launches
//   sort_rows    data-oblivious bitonic network per row: chunks and merge tails in LDS, one launch per global distance
//   abs_diff     mean |a - b| per segment, fp32 difference, float64 sum in a fixed order                          two launches
// The projection between standardize and sort is bg_gemm_f32.  The bodies move 16 bytes per lane where the geometry keeps the
// addresses aligned (V = 4) and fall back to one element per lane otherwise (V = 1); -ffp-contract=off keeps every a * b + c two
// roundings, which the bit-exact pyramid relies on.  No float atomics anywhere: every sum has one order.
#include "common.h"
#include <algorithm>
#include <cmath>

namespace {

constexpr int kT = 256;
typedef float f32x4 __attribute__((ext_vector_type(4)));

inline unsigned grid_for(size_t n) { return (unsigned)std::max<size_t>(1, std::min<size_t>(bg::cdiv(n, (size_t)kT), 256 * 8)); }
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// ------------------------------------------------------------------------------------------------ ingest
// LAYOUT 0: one channel (NHWC == NCHW), replicated three times; 1: NCHW with 3 channels; 2: NHWC with 3 channels.
// One thread takes V consecutive pixels of an image: V * C source floats, three V-wide stores.
template <int LAYOUT, int V>
__global__ __launch_bounds__(kT) void swd_ingest_kernel(const float* __restrict__ src, float* __restrict__ dst, unsigned n_grp,
                                                        unsigned grp_per_img, float scale, float shift) {
  const unsigned HW = grp_per_img * V;
  for (unsigned g = blockIdx.x * kT + threadIdx.x; g < n_grp; g += gridDim.x * kT) {
    const unsigned b = g / grp_per_img, p = (g - b * grp_per_img) * V;
    float v[3][V];
    if constexpr (LAYOUT == 2) {
      const float* s = src + ((size_t)b * HW + p) * 3;
      float in[3 * V];
      if constexpr (V == 4) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const f32x4 t = reinterpret_cast<const f32x4*>(s)[q];
          in[4 * q] = t.x; in[4 * q + 1] = t.y; in[4 * q + 2] = t.z; in[4 * q + 3] = t.w;
        }
      } else {
#pragma unroll
        for (int q = 0; q < 3; ++q) in[q] = s[q];
      }
#pragma unroll
      for (int k = 0; k < V; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][k] = in[3 * k + c];
    } else {
#pragma unroll
      for (int c = 0; c < (LAYOUT == 0 ? 1 : 3); ++c) {
        const float* s = src + ((size_t)b * (LAYOUT == 0 ? 1 : 3) + c) * HW + p;
        if constexpr (V == 4) {
          const f32x4 t = *reinterpret_cast<const f32x4*>(s);
          v[c][0] = t.x; v[c][1] = t.y; v[c][2] = t.z; v[c][3] = t.w;
        } else {
          v[c][0] = s[0];
        }
      }
      if constexpr (LAYOUT == 0) {
#pragma unroll
        for (int k = 0; k < V; ++k) v[1][k] = v[2][k] = v[0][k];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float* d = dst + ((size_t)b * 3 + c) * HW + p;
      float o[V];
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float m = v[c][k] * scale;       // two roundings, as numpy's x * scale + shift
        o[k] = m + shift;
      }
      if constexpr (V == 4) {
        f32x4 t;
        t.x = o[0]; t.y = o[1]; t.z = o[2]; t.w = o[3];
        *reinterpret_cast<f32x4*>(d) = t;
      } else {
        d[0] = o[0];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ pyramid
// reflect-101 for an index at most two outside [0, n), n >= 3 (or n >= 2 and at most one outside)
__device__ __forceinline__ int refl(int i, int n) {
  i = i < 0 ? -i : i;
  return i >= n ? 2 * n - 2 - i : i;
}

#define BG_BINOMIAL5 {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f}      /* [1 4 6 4 1] / 16, exact in fp32 */

// One thread: V adjacent outputs of one output row.  They need columns 2*ox-2 .. 2*ox+2V of the H-filtered image at row 2*oy:
// the H pass is accumulated tap by tap (j = 0..4, from 0.0f) per column, then the W pass the same way per output -- the host's
// order of operations, hence its bits.  Away from the left / right border a V = 4 thread reads its 11 columns as four 16-byte
// loads (columns 2*ox-4 .. 2*ox+11); at the border it reads them one by one through the reflection.
template <int V>
__global__ __launch_bounds__(kT) void pyr_down_kernel(const float* __restrict__ x, float* __restrict__ y, unsigned n_grp, int H, int W,
                                                      int Ho, int grp_per_row, int vec_in) {
  constexpr int NC = 2 * V + 3;
  const float wt[5] = BG_BINOMIAL5;
  for (unsigned g = blockIdx.x * kT + threadIdx.x; g < n_grp; g += gridDim.x * kT) {
    const unsigned r = g / (unsigned)grp_per_row, plane = r / (unsigned)Ho;
    const int ox = (int)(g - r * grp_per_row) * V, oy = (int)(r - plane * Ho);
    const float* img = x + (size_t)plane * H * W;
    float t[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) t[i] = 0.0f;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const float* row = img + (size_t)refl(2 * oy + j - 2, H) * W;
      float v[NC];
      if (V == 4 && vec_in && ox >= 2 && 2 * ox + 11 < W) {
        const f32x4* q4 = reinterpret_cast<const f32x4*>(row + 2 * ox - 4);
        float in[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 u = q4[q];
          in[4 * q] = u.x; in[4 * q + 1] = u.y; in[4 * q + 2] = u.z; in[4 * q + 3] = u.w;
        }
#pragma unroll
        for (int i = 0; i < NC; ++i) v[i] = in[(i + 2) & 15];
      } else {
#pragma unroll
        for (int i = 0; i < NC; ++i) v[i] = row[refl(2 * ox - 2 + i, W)];
      }
#pragma unroll
      for (int i = 0; i < NC; ++i) {
        const float p = wt[j] * v[i];
        t[i] = t[i] + p;
      }
    }
    float o[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      float acc = 0.0f;
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const float p = wt[j] * t[2 * k + j];
        acc = acc + p;
      }
      o[k] = acc;
    }
    float* d = y + (size_t)r * ((size_t)grp_per_row * V) + ox;
    if constexpr (V == 4) {
      f32x4 u;
      u.x = o[0]; u.y = o[1]; u.z = o[2]; u.w = o[3];
      *reinterpret_cast<f32x4*>(d) = u;
    } else {
      d[0] = o[0];
    }
  }
}

// pyr_up on the zero-stuffed 2h x 2w grid, without the grid: reflect-101 keeps an index's parity, so the taps of output row Y
// that land on real rows are j = 0, 2, 4 (low rows m-1, m, m+1) for Y = 2m and j = 1, 3 (m, m+1) for Y = 2m+1, and the same
// along X; the others multiply a stuffed zero and add an exact +0.0f to an accumulator that is never -0.0f (it starts as
// 0.0f + p), so skipping them changes no bit.  Reflection in low-image terms: row -1 -> 1, row h -> h-1.
struct UpRows { int r0, r1, r2; };      // Y even: three rows (w0, w2, w4); Y odd: r0, r1 (w1, w3)

__device__ __forceinline__ float up_col(const float* __restrict__ img, int w, int q, int odd, const UpRows& R) {
  const float wt[5] = BG_BINOMIAL5;
  float acc = 0.0f;
  if (odd) {
    const float p1 = wt[1] * img[(size_t)R.r0 * w + q];
    acc = acc + p1;
    const float p3 = wt[3] * img[(size_t)R.r1 * w + q];
    acc = acc + p3;
  } else {
    const float p0 = wt[0] * img[(size_t)R.r0 * w + q];
    acc = acc + p0;
    const float p2 = wt[2] * img[(size_t)R.r1 * w + q];
    acc = acc + p2;
    const float p4 = wt[4] * img[(size_t)R.r2 * w + q];
    acc = acc + p4;
  }
  return acc;
}

__device__ __forceinline__ float up_even(float tl, float tc, float tr) {      // X = 2q: columns q-1, q, q+1
  const float wt[5] = BG_BINOMIAL5;
  float acc = 0.0f;
  const float p0 = wt[0] * tl;
  acc = acc + p0;
  const float p2 = wt[2] * tc;
  acc = acc + p2;
  const float p4 = wt[4] * tr;
  acc = acc + p4;
  return acc * 4.0f;
}

__device__ __forceinline__ float up_odd(float tc, float tr) {                 // X = 2q+1: columns q, q+1
  const float wt[5] = BG_BINOMIAL5;
  float acc = 0.0f;
  const float p1 = wt[1] * tc;
  acc = acc + p1;
  const float p3 = wt[3] * tr;
  acc = acc + p3;
  return acc * 4.0f;
}

// V = 4: outputs X = 4*gx .. 4*gx+3 of row Y from low columns q0-1 .. q0+2 (q0 = 2*gx; w is even on this path); V = 1: one output
template <int V>
__global__ __launch_bounds__(kT) void pyr_up_kernel(const float* __restrict__ low, const float* minuend, float* out, unsigned n_grp,
                                                    int h, int w, int grp_per_row) {
  for (unsigned g = blockIdx.x * kT + threadIdx.x; g < n_grp; g += gridDim.x * kT) {
    const unsigned r = g / (unsigned)grp_per_row, plane = r / (unsigned)(2 * h);
    const int gx = (int)(g - r * grp_per_row), Y = (int)(r - plane * 2 * h), m = Y >> 1, odd = Y & 1;
    const float* img = low + (size_t)plane * h * w;
    const int up = m + 1 < h ? m + 1 : h - 1;
    UpRows R;
    if (odd) { R.r0 = m; R.r1 = up; R.r2 = up; }
    else { R.r0 = m ? m - 1 : 1; R.r1 = m; R.r2 = up; }
    const size_t o = (size_t)r * ((size_t)grp_per_row * V) + (size_t)gx * V;
    if constexpr (V == 4) {
      const int q0 = 2 * gx;
      const float tl = up_col(img, w, q0 ? q0 - 1 : 1, odd, R), t0 = up_col(img, w, q0, odd, R), t1 = up_col(img, w, q0 + 1, odd, R),
                  tr = up_col(img, w, q0 + 2 < w ? q0 + 2 : w - 1, odd, R);
      f32x4 u;
      u.x = up_even(tl, t0, t1); u.y = up_odd(t0, t1); u.z = up_even(t0, t1, tr); u.w = up_odd(t1, tr);
      if (minuend) {
        const f32x4 mv = *reinterpret_cast<const f32x4*>(minuend + o);
        u.x = mv.x - u.x; u.y = mv.y - u.y; u.z = mv.z - u.z; u.w = mv.w - u.w;
      }
      *reinterpret_cast<f32x4*>(out + o) = u;
    } else {
      const int q = gx >> 1, qr = q + 1 < w ? q + 1 : w - 1;
      float val;
      if (gx & 1) val = up_odd(up_col(img, w, q, odd, R), up_col(img, w, qr, odd, R));
      else val = up_even(up_col(img, w, q ? q - 1 : 1, odd, R), up_col(img, w, q, odd, R), up_col(img, w, qr, odd, R));
      if (minuend) val = minuend[o] - val;
      out[o] = val;
    }
  }
}

// ------------------------------------------------------------------------------------------------ descriptor gather
// desc[t, c, a, b] = level[t / per_image, c, cy[t] + b - half, cx[t] + a - half]: a walks x, b walks y (sliced_wasserstein.py:13-23).
// One thread writes V consecutive floats of desc; the (t, c, a, b) of the first comes from one division chain, the others by stepping.
template <int V>
__global__ __launch_bounds__(kT) void swd_gather_kernel(const float* __restrict__ level, const int* __restrict__ cx,
                                                        const int* __restrict__ cy, float* __restrict__ desc, unsigned n_grp, int H, int W,
                                                        int nhood, int per_image) {
  const unsigned nn = (unsigned)(nhood * nhood), D = 3 * nn;
  const int half = nhood / 2;
  for (unsigned g = blockIdx.x * kT + threadIdx.x; g < n_grp; g += gridDim.x * kT) {
    const unsigned o = g * V;
    unsigned t = o / D, rem = o - t * D, c = rem / nn;
    rem -= c * nn;
    int a = (int)(rem / (unsigned)nhood), b = (int)(rem - (unsigned)a * nhood);
    int x0 = cx[t] - half, y0 = cy[t] - half;
    const float* plane = level + ((size_t)(t / (unsigned)per_image) * 3 + c) * H * W;
    float v[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      v[k] = plane[(size_t)(y0 + b) * W + (x0 + a)];
      if (k + 1 < V) {
        if (++b == nhood) {
          b = 0;
          if (++a == nhood) {
            a = 0;
            if (++c == 3) {
              c = 0;
              ++t;
              x0 = cx[t] - half;
              y0 = cy[t] - half;
            }
            plane = level + ((size_t)(t / (unsigned)per_image) * 3 + c) * H * W;
          }
        }
      }
    }
    if constexpr (V == 4) {
      f32x4 u;
      u.x = v[0]; u.y = v[1]; u.z = v[2]; u.w = v[3];
      reinterpret_cast<f32x4*>(desc)[g] = u;
    } else {
      desc[g] = v[0];
    }
  }
}

// ------------------------------------------------------------------------------------------------ float64 reductions
// sum over the block in a fixed tree order; every thread gets the result
__device__ __forceinline__ double block_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = kT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// sum of nb (<= kT) partials, the same order in every block that asks
__device__ __forceinline__ double partial_sum(const double* part, int nb, double* red) {
  return block_sum((int)threadIdx.x < nb ? part[threadIdx.x] : 0.0, red);
}

// ------------------------------------------------------------------------------------------------ standardize
// desc is [rows, 3, nn] flat; the channel of flat element e is (e / nn) % 3.  A thread finds its position by one division and keeps
// it while it strides: (r, c) = offset inside the channel's nn-run and channel.
struct ChanPos { unsigned r, c; };

__device__ __forceinline__ ChanPos chan_at(unsigned e, unsigned nn) {
  const unsigned q = e / nn;
  ChanPos p;
  p.r = e - q * nn;
  p.c = q % 3u;
  return p;
}

__device__ __forceinline__ void chan_step(ChanPos& p, unsigned dr, unsigned dc, unsigned nn) {
  p.r += dr;
  if (p.r >= nn) { p.r -= nn; p.c += 1; }
  p.c += dc;                       // <= 2 + 1 + 2
  if (p.c >= 3) p.c -= 3;
}

// channel of the k-th element after position p
__device__ __forceinline__ unsigned chan_of(const ChanPos& p, unsigned k, unsigned nn) {
  unsigned r = p.r + k, c = p.c;
  while (r >= nn) { r -= nn; c = c == 2 ? 0 : c + 1; }
  return c;
}

template <int V>
__device__ __forceinline__ void load_v(const float* p, float* v) {
  if constexpr (V == 4) {
    const f32x4 u = *reinterpret_cast<const f32x4*>(p);
    v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
  } else {
    v[0] = p[0];
  }
}

// PASS 0: per-block sums -> part[c * nb + block]; PASS 1: per-block sums of (x - mean_c)^2 -> part[(3 + c) * nb + block], with mean_c
// reduced from pass 0's partials by every block in the same order
template <int V, int PASS>
__global__ __launch_bounds__(kT) void swd_stats_kernel(const float* __restrict__ desc, unsigned total, unsigned nn, double count,
                                                       double* __restrict__ part) {
  __shared__ double red[kT];
  const int nb = (int)gridDim.x;
  double mean[3] = {0.0, 0.0, 0.0};
  if constexpr (PASS == 1) {
#pragma unroll
    for (int c = 0; c < 3; ++c) mean[c] = partial_sum(part + c * nb, nb, red) / count;
  }
  const unsigned stride = gridDim.x * kT * V, first = (blockIdx.x * kT + threadIdx.x) * V;
  const unsigned dr = stride % nn, dc = (stride / nn) % 3u;
  double s[3] = {0.0, 0.0, 0.0};
  if (first < total) {
    ChanPos p = chan_at(first, nn);
    for (unsigned e = first; e < total; e += stride) {
      float v[V];
      load_v<V>(desc + e, v);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const unsigned c = chan_of(p, k, nn);
        double d = (double)v[k];
        if constexpr (PASS == 1) {
          d = d - (c == 0 ? mean[0] : c == 1 ? mean[1] : mean[2]);
          d = d * d;
        }
        s[0] += c == 0 ? d : 0.0;
        s[1] += c == 1 ? d : 0.0;
        s[2] += c == 2 ? d : 0.0;
      }
      chan_step(p, dr, dc, nn);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double b = block_sum(s[c], red);
    if (threadIdx.x == 0) part[(PASS * 3 + c) * nb + blockIdx.x] = b;
  }
}

// one block: the partials of both passes -> fin[2c] = mean_c, fin[2c + 1] = population standard deviation of channel c (and stats_out)
__global__ __launch_bounds__(kT) void swd_stats_final_kernel(const double* __restrict__ part, int nb, double count, double* __restrict__ fin,
                                                             double* stats_out) {
  __shared__ double red[kT];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double mean = partial_sum(part + c * nb, nb, red) / count;
    const double sd = sqrt(partial_sum(part + (3 + c) * nb, nb, red) / count);
    if (threadIdx.x == 0) {
      fin[2 * c] = mean;
      fin[2 * c + 1] = sd;
      if (stats_out) {
        stats_out[2 * c] = mean;
        stats_out[2 * c + 1] = sd;
      }
    }
  }
}

// desc = (desc - mean32) / std32 in place; fin: the six doubles of swd_stats_final_kernel
template <int V>
__global__ __launch_bounds__(kT) void swd_standardize_apply_kernel(float* __restrict__ desc, unsigned total, unsigned nn,
                                                                   const double* __restrict__ fin) {
  float m32[3], s32[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    m32[c] = (float)fin[2 * c];
    s32[c] = (float)fin[2 * c + 1];
  }
  const unsigned stride = gridDim.x * kT * V, first = (blockIdx.x * kT + threadIdx.x) * V;
  const unsigned dr = stride % nn, dc = (stride / nn) % 3u;
  if (first >= total) return;
  ChanPos p = chan_at(first, nn);
  for (unsigned e = first; e < total; e += stride) {
    float v[V];
    load_v<V>(desc + e, v);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const unsigned c = chan_of(p, k, nn);
      const float d = v[k] - (c == 0 ? m32[0] : c == 1 ? m32[1] : m32[2]);
      v[k] = d / (c == 0 ? s32[0] : c == 1 ? s32[1] : s32[2]);
    }
    if constexpr (V == 4) {
      f32x4 u;
      u.x = v[0]; u.y = v[1]; u.z = v[2]; u.w = v[3];
      *reinterpret_cast<f32x4*>(desc + e) = u;
    } else {
      desc[e] = v[0];
    }
    chan_step(p, dr, dc, nn);
  }
}

inline int stats_blocks(size_t total) { return (int)std::max<size_t>(1, std::min<size_t>(bg::cdiv(total, (size_t)kT * 16), kT)); }

// ------------------------------------------------------------------------------------------------ row sort
// Bitonic sorting network in the form whose compare-exchanges ALL put the smaller value at the lower index: the merge of two sorted
// runs of k/2 starts with the "mirror" stage (i against i ^ (k-1)) and continues with the half-cleaners (i against i ^ j,
// j = k/4 .. 1).  The network is laid over N = the next power of two >= n; an index >= n stands for +inf, and because no exchange
// ever moves a larger value down, a pair whose upper index is >= n never swaps and is simply skipped -- no padded copy.  Which
// addresses are touched depends on (n, stage) only, never on the data, so NaNs cannot make it run away: a comparison with a NaN is
// false and the pair stays as it is.
constexpr int kSortT = 512;
constexpr unsigned kSortChunk = 4096;        // floats of a row a block holds in LDS (16 KiB)

__device__ __forceinline__ void cmpx(float& a, float& b) {
  const float x = a, y = b;
  const bool sw = x > y;
  a = sw ? y : x;
  b = sw ? x : y;
}

// pair t of a stage with distance j (a power of two): the lower index
__device__ __forceinline__ unsigned pair_lo(unsigned t, unsigned j) { return ((t & ~(j - 1)) << 1) | (t & (j - 1)); }

// TAIL = false: sorts every `span`-long chunk (span = min(N, kSortChunk)) of every row: stages k = 2 .. span.
// TAIL = true : the half-cleaners j = span/2 .. 1 of a merge whose wider stages ran in global memory.
template <bool VEC, bool TAIL>
__global__ __launch_bounds__(kSortT) void sort_chunk_kernel(float* __restrict__ x, size_t n_chunks, unsigned chunks_per_row, unsigned n,
                                                            unsigned span) {
  __shared__ __attribute__((aligned(16))) float s[kSortChunk];
  const float inf = __builtin_inff();
  for (size_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
    const size_t row = ch / chunks_per_row;
    const unsigned e0 = (unsigned)(ch - row * chunks_per_row) * span;
    float* base = x + row * (size_t)n;
    if constexpr (VEC) {
      for (unsigned q = threadIdx.x; q < span / 4; q += kSortT) {
        const unsigned e = e0 + 4 * q;        // n % 4 == 0: the quad is whole or absent
        f32x4 u;
        u.x = u.y = u.z = u.w = inf;
        if (e < n) u = *reinterpret_cast<const f32x4*>(base + e);
        reinterpret_cast<f32x4*>(s)[q] = u;
      }
    } else {
      for (unsigned i = threadIdx.x; i < span; i += kSortT) s[i] = e0 + i < n ? base[e0 + i] : inf;
    }
    __syncthreads();
    if constexpr (!TAIL) {
      for (unsigned k = 2; k <= span; k <<= 1) {
        for (unsigned t = threadIdx.x; t < span / 2; t += kSortT) {
          const unsigned i = pair_lo(t, k >> 1);
          cmpx(s[i], s[i ^ (k - 1)]);
        }
        __syncthreads();
        for (unsigned j = k >> 2; j >= 1; j >>= 1) {
          for (unsigned t = threadIdx.x; t < span / 2; t += kSortT) {
            const unsigned i = pair_lo(t, j);
            cmpx(s[i], s[i + j]);
          }
          __syncthreads();
        }
      }
    } else {
      for (unsigned j = span >> 1; j >= 1; j >>= 1) {
        for (unsigned t = threadIdx.x; t < span / 2; t += kSortT) {
          const unsigned i = pair_lo(t, j);
          cmpx(s[i], s[i + j]);
        }
        __syncthreads();
      }
    }
    if constexpr (VEC) {
      for (unsigned q = threadIdx.x; q < span / 4; q += kSortT) {
        const unsigned e = e0 + 4 * q;
        if (e < n) *reinterpret_cast<f32x4*>(base + e) = reinterpret_cast<const f32x4*>(s)[q];
      }
    } else {
      for (unsigned i = threadIdx.x; i < span; i += kSortT)
        if (e0 + i < n) base[e0 + i] = s[i];
    }
    __syncthreads();
  }
}

// One global stage of distance j >= kSortChunk over every row: mirror = k - 1 for the first stage of the merge of width k, 0 for a
// half-cleaner.  A thread takes V adjacent pairs: lower indices i .. i+V-1 and the partners i ^ j (ascending) or i ^ (k-1)
// (descending: the quad that ENDS at the partner of i, compared in reverse).
template <int V>
__global__ __launch_bounds__(kT) void sort_global_kernel(float* __restrict__ x, size_t n_work, unsigned work_per_row, unsigned n,
                                                         unsigned j, unsigned mirror) {
  for (size_t w = (size_t)blockIdx.x * kT + threadIdx.x; w < n_work; w += (size_t)gridDim.x * kT) {
    const size_t row = w / work_per_row;
    const unsigned t = (unsigned)(w - row * work_per_row) * V, i = pair_lo(t, j), l = mirror ? i ^ mirror : i + j;
    if (l >= n) continue;                    // the partner (and with n % V == 0 its whole group) stands for +inf
    float* base = x + row * (size_t)n;
    if constexpr (V == 4) {
      f32x4* pa = reinterpret_cast<f32x4*>(base + i);
      f32x4* pb = reinterpret_cast<f32x4*>(base + (mirror ? l - 3 : l));
      const f32x4 va = *pa, vb = *pb;
      float a[4] = {va.x, va.y, va.z, va.w}, b[4];
      if (mirror) { b[0] = vb.w; b[1] = vb.z; b[2] = vb.y; b[3] = vb.x; }
      else { b[0] = vb.x; b[1] = vb.y; b[2] = vb.z; b[3] = vb.w; }
#pragma unroll
      for (int q = 0; q < 4; ++q) cmpx(a[q], b[q]);
      f32x4 oa, ob;
      oa.x = a[0]; oa.y = a[1]; oa.z = a[2]; oa.w = a[3];
      if (mirror) { ob.x = b[3]; ob.y = b[2]; ob.z = b[1]; ob.w = b[0]; }
      else { ob.x = b[0]; ob.y = b[1]; ob.z = b[2]; ob.w = b[3]; }
      *pa = oa;
      *pb = ob;
    } else {
      float a = base[i], b = base[l];
      cmpx(a, b);
      base[i] = a;
      base[l] = b;
    }
  }
}

// ------------------------------------------------------------------------------------------------ mean |a - b| per segment
// grid (nb, nseg): block (p, s) sums its share of segment s in float64 -> part[s * nb + p]
template <int V>
__global__ __launch_bounds__(kT) void abs_diff_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, size_t seg,
                                                              double* __restrict__ part) {
  __shared__ double red[kT];
  const size_t base = (size_t)blockIdx.y * seg, stride = (size_t)gridDim.x * kT * V;
  double acc = 0.0;
  for (size_t e = ((size_t)blockIdx.x * kT + threadIdx.x) * V; e < seg; e += stride) {
    float va[V], vb[V];
    load_v<V>(a + base + e, va);
    load_v<V>(b + base + e, vb);
#pragma unroll
    for (int k = 0; k < V; ++k) acc += (double)fabsf(va[k] - vb[k]);
  }
  const double tot = block_sum(acc, red);
  if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = tot;
}

__global__ __launch_bounds__(kT) void abs_diff_final_kernel(const double* __restrict__ part, int nb, double seg, double* __restrict__ out) {
  __shared__ double red[kT];
  const double tot = partial_sum(part + (size_t)blockIdx.x * nb, nb, red);
  if (threadIdx.x == 0) out[blockIdx.x] = tot / seg;
}

inline int abs_diff_blocks(size_t seg) { return (int)std::max<size_t>(1, std::min<size_t>(bg::cdiv(seg, (size_t)kT * 16), kT)); }

constexpr double kMaxElems = 2147483648.0;      // the kernels above index groups in 32 bits

}  // namespace

extern "C" {

int bg_swd_ingest_f32(const float* src, float* dst, int B, int H, int W, int C, int src_nhwc, float scale, float shift, void* stream) {
  BG_REQUIRE(src && dst, BG_ERR_NULL, "bg_swd_ingest_f32: null pointer");
  BG_REQUIRE(B > 0 && H > 0 && W > 0 && (C == 1 || C == 3), BG_ERR_BAD_SHAPE, "bg_swd_ingest_f32: B=%d %dx%d C=%d (C must be 1 or 3)", B, H,
             W, C);
  BG_REQUIRE((double)B * 3.0 * H * W < kMaxElems, BG_ERR_BAD_SHAPE, "bg_swd_ingest_f32: %dx3x%dx%d exceeds 2^31 elements", B, H, W);
  BG_REQUIRE(aligned4(src) && aligned4(dst), BG_ERR_BAD_ALIGNMENT, "bg_swd_ingest_f32: pointers must be 4-byte aligned");
  const unsigned HW = (unsigned)H * W;
  const bool vec = HW % 4 == 0 && bg::aligned16(src) && bg::aligned16(dst);
  const unsigned gpi = vec ? HW / 4 : HW, n_grp = gpi * (unsigned)B;
  const int layout = C == 1 ? 0 : (src_nhwc ? 2 : 1);
  bg::Launch L(stream, "swd_ingest", 0, 4.0 * B * (double)HW * (C + 3));
  const dim3 grid(grid_for(n_grp)), block(kT);
#define BG_INGEST(LAY)                                                                                            \
  do {                                                                                                            \
    if (vec) bg::launch(swd_ingest_kernel<LAY, 4>, grid, block, 0, L.s, src, dst, n_grp, gpi, scale, shift);      \
    else bg::launch(swd_ingest_kernel<LAY, 1>, grid, block, 0, L.s, src, dst, n_grp, gpi, scale, shift);          \
  } while (0)
  if (layout == 0) BG_INGEST(0);
  else if (layout == 1) BG_INGEST(1);
  else BG_INGEST(2);
#undef BG_INGEST
  return L.done("swd_ingest_kernel");
}

int bg_pyr_down_f32(const float* x, float* y, int planes, int H, int W, void* stream) {
  BG_REQUIRE(x && y, BG_ERR_NULL, "bg_pyr_down_f32: null pointer");
  BG_REQUIRE(planes > 0 && H >= 3 && W >= 3, BG_ERR_BAD_SHAPE, "bg_pyr_down_f32: planes=%d %dx%d (H, W >= 3)", planes, H, W);
  BG_REQUIRE((double)planes * H * W < kMaxElems, BG_ERR_BAD_SHAPE, "bg_pyr_down_f32: %dx%dx%d exceeds 2^31 elements", planes, H, W);
  BG_REQUIRE(aligned4(x) && aligned4(y), BG_ERR_BAD_ALIGNMENT, "bg_pyr_down_f32: pointers must be 4-byte aligned");
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const bool vec = Wo % 4 == 0 && bg::aligned16(y);
  const int vec_in = W % 4 == 0 && bg::aligned16(x);
  const int gpr = vec ? Wo / 4 : Wo;
  const unsigned n_grp = (unsigned)planes * Ho * gpr;
  bg::Launch L(stream, "pyr_down", 0, 4.0 * planes * ((double)H * W + (double)Ho * Wo));
  const dim3 grid(grid_for(n_grp)), block(kT);
  if (vec) bg::launch(pyr_down_kernel<4>, grid, block, 0, L.s, x, y, n_grp, H, W, Ho, gpr, vec_in);
  else bg::launch(pyr_down_kernel<1>, grid, block, 0, L.s, x, y, n_grp, H, W, Ho, gpr, 0);
  return L.done("pyr_down_kernel");
}

int bg_pyr_up_f32(const float* low, const float* minuend, float* out, int planes, int h, int w, void* stream) {
  BG_REQUIRE(low && out, BG_ERR_NULL, "bg_pyr_up_f32: null pointer");
  BG_REQUIRE(planes > 0 && h >= 2 && w >= 2, BG_ERR_BAD_SHAPE, "bg_pyr_up_f32: planes=%d %dx%d (h, w >= 2)", planes, h, w);
  BG_REQUIRE((double)planes * 4.0 * h * w < kMaxElems, BG_ERR_BAD_SHAPE, "bg_pyr_up_f32: %dx%dx%d exceeds 2^31 elements", planes, 2 * h,
             2 * w);
  BG_REQUIRE(aligned4(low) && aligned4(out) && aligned4(minuend), BG_ERR_BAD_ALIGNMENT, "bg_pyr_up_f32: pointers must be 4-byte aligned");
  const bool vec = w % 2 == 0 && bg::aligned16(out) && bg::aligned16(minuend);
  const int gpr = vec ? 2 * w / 4 : 2 * w;
  const unsigned n_grp = (unsigned)planes * 2 * h * gpr;
  bg::Launch L(stream, "pyr_up", 0, 4.0 * planes * (double)h * w * (minuend ? 9 : 5));
  const dim3 grid(grid_for(n_grp)), block(kT);
  if (vec) bg::launch(pyr_up_kernel<4>, grid, block, 0, L.s, low, minuend, out, n_grp, h, w, gpr);
  else bg::launch(pyr_up_kernel<1>, grid, block, 0, L.s, low, minuend, out, n_grp, h, w, gpr);
  return L.done("pyr_up_kernel");
}

int bg_swd_gather_f32(const float* level, const int32_t* cx_d, const int32_t* cy_d, float* desc, int B, int H, int W, int nhood,
                      int per_image, void* stream) {
  BG_REQUIRE(level && cx_d && cy_d && desc, BG_ERR_NULL, "bg_swd_gather_f32: null pointer");
  BG_REQUIRE(B > 0 && H > 0 && W > 0 && per_image > 0, BG_ERR_BAD_SHAPE, "bg_swd_gather_f32: B=%d %dx%d per_image=%d", B, H, W, per_image);
  BG_REQUIRE(nhood > 0 && nhood % 2 == 1 && nhood <= std::min(H, W), BG_ERR_BAD_SHAPE,
             "bg_swd_gather_f32: nhood=%d must be odd and <= min(H, W) = %d", nhood, std::min(H, W));
  const double total_d = (double)B * per_image * 3.0 * nhood * nhood;
  BG_REQUIRE(total_d < kMaxElems && (double)B * 3.0 * H * W < kMaxElems, BG_ERR_BAD_SHAPE, "bg_swd_gather_f32: exceeds 2^31 elements");
  BG_REQUIRE(aligned4(level) && aligned4(cx_d) && aligned4(cy_d) && aligned4(desc), BG_ERR_BAD_ALIGNMENT,
             "bg_swd_gather_f32: pointers must be 4-byte aligned");
  const unsigned total = (unsigned)total_d;
  const bool vec = total % 4 == 0 && bg::aligned16(desc);
  const unsigned n_grp = vec ? total / 4 : total;
  bg::Launch L(stream, "swd_gather", 0, 8.0 * total + 8.0 * B * per_image);
  const dim3 grid(grid_for(n_grp)), block(kT);
  if (vec) bg::launch(swd_gather_kernel<4>, grid, block, 0, L.s, level, cx_d, cy_d, desc, n_grp, H, W, nhood, per_image);
  else bg::launch(swd_gather_kernel<1>, grid, block, 0, L.s, level, cx_d, cy_d, desc, n_grp, H, W, nhood, per_image);
  return L.done("swd_gather_kernel");
}

size_t bg_swd_standardize_workspace_bytes(int rows, int nhood) {
  if (rows <= 0 || nhood <= 0) return 0;
  return ((size_t)6 * stats_blocks((size_t)rows * 3 * nhood * nhood) + 6) * sizeof(double);      // partials of both passes + mean, std
}

int bg_swd_standardize_f32(float* desc, int rows, int nhood, double* stats_out, void* ws, size_t ws_bytes, void* stream) {
  BG_REQUIRE(desc, BG_ERR_NULL, "bg_swd_standardize_f32: null pointer");
  BG_REQUIRE(rows > 0 && nhood > 0 && nhood % 2 == 1, BG_ERR_BAD_SHAPE, "bg_swd_standardize_f32: rows=%d nhood=%d (odd)", rows, nhood);
  const double total_d = (double)rows * 3.0 * nhood * nhood;
  BG_REQUIRE(total_d < kMaxElems, BG_ERR_BAD_SHAPE, "bg_swd_standardize_f32: rows=%d nhood=%d exceeds 2^31 elements", rows, nhood);
  BG_REQUIRE(ws && ws_bytes >= bg_swd_standardize_workspace_bytes(rows, nhood), BG_ERR_WORKSPACE,
             "bg_swd_standardize_f32: workspace too small");
  BG_REQUIRE(aligned4(desc) && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0 && (reinterpret_cast<uintptr_t>(stats_out) & 7u) == 0,
             BG_ERR_BAD_ALIGNMENT, "bg_swd_standardize_f32: desc must be 4-byte, ws and stats_out 8-byte aligned");
  const unsigned total = (unsigned)total_d, nn = (unsigned)(nhood * nhood);
  const bool vec = total % 4 == 0 && bg::aligned16(desc);
  const int nb = stats_blocks(total);
  const double count = (double)rows * nn;
  double* part = static_cast<double*>(ws);
  const dim3 block(kT);
  {
    bg::Launch L(stream, "swd_stats_sum", 0, 4.0 * total);
    if (vec) bg::launch(swd_stats_kernel<4, 0>, dim3(nb), block, 0, L.s, desc, total, nn, count, part);
    else bg::launch(swd_stats_kernel<1, 0>, dim3(nb), block, 0, L.s, desc, total, nn, count, part);
    const int rc = L.done("swd_stats_kernel");
    if (rc) return rc;
  }
  {
    bg::Launch L(stream, "swd_stats_dev", 0, 4.0 * total);
    if (vec) bg::launch(swd_stats_kernel<4, 1>, dim3(nb), block, 0, L.s, desc, total, nn, count, part);
    else bg::launch(swd_stats_kernel<1, 1>, dim3(nb), block, 0, L.s, desc, total, nn, count, part);
    const int rc = L.done("swd_stats_kernel");
    if (rc) return rc;
  }
  double* fin = part + 6 * nb;
  {
    bg::Launch L(stream, "swd_stats_final", 0, 48.0 * nb);
    bg::launch(swd_stats_final_kernel, dim3(1), block, 0, L.s, (const double*)part, nb, count, fin, stats_out);
    const int rc = L.done("swd_stats_final_kernel");
    if (rc) return rc;
  }
  bg::Launch L(stream, "swd_standardize", 0, 8.0 * total);
  const dim3 grid(grid_for(vec ? total / 4 : total));
  if (vec) bg::launch(swd_standardize_apply_kernel<4>, grid, block, 0, L.s, desc, total, nn, (const double*)fin);
  else bg::launch(swd_standardize_apply_kernel<1>, grid, block, 0, L.s, desc, total, nn, (const double*)fin);
  return L.done("swd_standardize_apply_kernel");
}

int bg_sort_rows_f32(float* x, int rows, int n, void* stream) {
  BG_REQUIRE(x, BG_ERR_NULL, "bg_sort_rows_f32: null pointer");
  BG_REQUIRE(rows > 0 && n >= 1 && n <= (1 << 24) && (double)rows * n < kMaxElems, BG_ERR_BAD_SHAPE,
             "bg_sort_rows_f32: rows=%d n=%d (1 <= n <= 2^24, rows * n < 2^31)", rows, n);
  BG_REQUIRE(aligned4(x), BG_ERR_BAD_ALIGNMENT, "bg_sort_rows_f32: x must be 4-byte aligned");
  if (n == 1) return BG_OK;
  unsigned N = 2;
  while (N < (unsigned)n) N <<= 1;
  const bool vec = n % 4 == 0 && bg::aligned16(x);
  const unsigned span = std::min(N, kSortChunk), cpr = bg::cdiv((size_t)n, span);
  const size_t n_chunks = (size_t)rows * cpr;
  const dim3 cgrid((unsigned)std::min<size_t>(n_chunks, 256 * 16)), cblock(kSortT);
  const double bytes = 8.0 * rows * (double)n;
  {
    bg::Launch L(stream, "sort_rows_chunk", 0, bytes);
    if (vec) bg::launch(sort_chunk_kernel<true, false>, cgrid, cblock, 0, L.s, x, n_chunks, cpr, (unsigned)n, span);
    else bg::launch(sort_chunk_kernel<false, false>, cgrid, cblock, 0, L.s, x, n_chunks, cpr, (unsigned)n, span);
    const int rc = L.done("sort_chunk_kernel");
    if (rc) return rc;
  }
  const unsigned wpr = vec ? N / 8 : N / 2;            // groups of pairs per row in a global stage
  const size_t n_work = (size_t)rows * wpr;
  const dim3 ggrid(grid_for(n_work)), gblock(kT);
  for (unsigned k = 2 * kSortChunk; k <= N && k != 0; k <<= 1) {
    for (unsigned j = k >> 1; j >= kSortChunk; j >>= 1) {
      const unsigned mirror = j == (k >> 1) ? k - 1 : 0;
      bg::Launch L(stream, "sort_rows_global", 0, bytes);
      if (vec) bg::launch(sort_global_kernel<4>, ggrid, gblock, 0, L.s, x, n_work, wpr, (unsigned)n, j, mirror);
      else bg::launch(sort_global_kernel<1>, ggrid, gblock, 0, L.s, x, n_work, wpr, (unsigned)n, j, mirror);
      const int rc = L.done("sort_global_kernel");
      if (rc) return rc;
    }
    bg::Launch L(stream, "sort_rows_tail", 0, bytes);
    if (vec) bg::launch(sort_chunk_kernel<true, true>, cgrid, cblock, 0, L.s, x, n_chunks, cpr, (unsigned)n, span);
    else bg::launch(sort_chunk_kernel<false, true>, cgrid, cblock, 0, L.s, x, n_chunks, cpr, (unsigned)n, span);
    const int rc = L.done("sort_chunk_kernel");
    if (rc) return rc;
  }
  return BG_OK;
}

size_t bg_abs_diff_mean_workspace_bytes(size_t seg, int nseg) {
  if (seg == 0 || nseg <= 0) return 0;
  return (size_t)nseg * abs_diff_blocks(seg) * sizeof(double);
}

int bg_abs_diff_mean_f32(const float* a, const float* b, size_t seg, int nseg, double* out, void* ws, size_t ws_bytes, void* stream) {
  BG_REQUIRE(a && b && out, BG_ERR_NULL, "bg_abs_diff_mean_f32: null pointer");
  BG_REQUIRE(seg > 0 && nseg > 0 && nseg <= 65535, BG_ERR_BAD_SHAPE, "bg_abs_diff_mean_f32: seg=%zu nseg=%d (1 <= nseg <= 65535)", seg, nseg);
  BG_REQUIRE(ws && ws_bytes >= bg_abs_diff_mean_workspace_bytes(seg, nseg), BG_ERR_WORKSPACE, "bg_abs_diff_mean_f32: workspace too small");
  BG_REQUIRE(aligned4(a) && aligned4(b) && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0 && (reinterpret_cast<uintptr_t>(out) & 7u) == 0,
             BG_ERR_BAD_ALIGNMENT, "bg_abs_diff_mean_f32: a, b must be 4-byte, ws and out 8-byte aligned");
  const bool vec = seg % 4 == 0 && bg::aligned16(a) && bg::aligned16(b);
  const int nb = abs_diff_blocks(seg);
  double* part = static_cast<double*>(ws);
  {
    bg::Launch L(stream, "abs_diff_partial", 0, 8.0 * (double)seg * nseg);
    if (vec) bg::launch(abs_diff_partial_kernel<4>, dim3(nb, nseg), dim3(kT), 0, L.s, a, b, seg, part);
    else bg::launch(abs_diff_partial_kernel<1>, dim3(nb, nseg), dim3(kT), 0, L.s, a, b, seg, part);
    const int rc = L.done("abs_diff_partial_kernel");
    if (rc) return rc;
  }
  bg::Launch L(stream, "abs_diff_mean", 0, 8.0 * nb * nseg);
  bg::launch(abs_diff_final_kernel, dim3(nseg), dim3(kT), 0, L.s, (const double*)part, nb, (double)seg, out);
  return L.done("abs_diff_final_kernel");
}

}  // extern "C"
