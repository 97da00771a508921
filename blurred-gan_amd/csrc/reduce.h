// The reductions that more than one file uses, each with a summation order that is part of what the tests hold to exact bits.
//
// Deliberately NOT here -- three other workgroup sums that look like block_sum below but add in another order or synchronise
// differently; none can stand in for another without changing bits or racing on the LDS scratch:
//   misc.hip block_sum (loss kernels)     folds a wave with __shfl_down (only lane 0 holds the wave's sum) and adds red[0..3] as one
//                                         expression, for exactly four waves
//   spectral.hip block_sum / block_sum16  butterfly in ASCENDING offsets, ((r0 + r1) + r2) + r3, and the second barrier comes AFTER
//                                         the read (its callers write red again at once); block_sum16 is the 16-wave variant
//   swd.hip                               a float64 tree through LDS
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace bg {

// One lane's share of the sum over nblk partial rows of partial[(b * NQ + q) * C + c]: rows lane, lane + 64, ... in that order.
// The loads are issued eight at a time and added in the loop's own order: the sum keeps its bits, and a lane waits for memory once
// per eight partial rows instead of once per row (the launches that finish a column sum are pure latency).  The caller folds the 64
// lanes, for (off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64), and ends in its own way.
__device__ __forceinline__ float lane_sum_partials(const float* partial, int nblk, int NQ, int q, int C, int c) {
  float s = 0.f;
  int b = threadIdx.x & 63;
  const size_t step = (size_t)64 * NQ * C;
  const float* p = partial + ((size_t)b * NQ + q) * C + c;
  for (; b + 7 * 64 < nblk; b += 8 * 64, p += 8 * step) {
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = p[i * step];
#pragma unroll
    for (int i = 0; i < 8; ++i) s += v[i];
  }
  if (b < nblk) {                               // the last, partial batch (all of it when nblk < 512): predicated, still one wait
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = b + i * 64 < nblk ? p[i * step] : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (b + i * 64 < nblk) s += v[i];
  }
  return s;
}

// sum over the workgroup in a fixed order; every thread gets it.  red: one float of LDS per wave.  Xor butterfly in descending
// offsets, the waves added in wave order; the first barrier is there because red may still be read from the caller's previous sum
__device__ __forceinline__ float block_sum(float v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = red[0];
  for (int w = 1, nw = blockDim.x >> 6; w < nw; ++w) s += red[w];
  return s;
}

// f1(o) for the scalar head and tail, f4(o) for every float4 of the flat range [0, n) that starts at byte address ``addr`` (4-byte
// aligned): o of an f4 call is 16-byte aligned in memory.  The float4s are dealt to K workgroups in contiguous runs (k-th of K);
// the head goes with the first run, the tail with the last.
template <class F4, class F1>
__device__ __forceinline__ void sweep(uintptr_t addr, int n, int k, int K, F4 f4, F1 f1) {
  const int tid = threadIdx.x, T = blockDim.x;
  int head = (int)(((16u - (unsigned)(addr & 15u)) & 15u) >> 2);
  head = head < n ? head : n;
  const int nvec = (n - head) >> 2, tail0 = head + 4 * nvec;
  const int per = (nvec + K - 1) / K, vlo = k * per, vhi = vlo + per < nvec ? vlo + per : nvec;
  if (k == 0 && tid < head) f1(tid);
  for (int v = vlo + tid; v < vhi; v += T) f4(head + 4 * v);
  if (k == K - 1 && tid < n - tail0) f1(tail0 + tid);
}

}  // namespace bg
