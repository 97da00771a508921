// Adaptive augmentation (include/bgan.h "adaptive augmentation"; Karras et al. 2020).  Two things live here.
// The gated entry points of the DiffAugment kernel: diffaug_kernel.h's template with GATED = true (diffaug.hip keeps the ungated
// instantiations and nothing else, so its code object holds the four kernels it always held).
// And the controller: the overfitting heuristic r_t = E[sign(D(reals))] steers the probability p the gated launches read.  Two
// launches per critic step, both one workgroup, both far below a microsecond of work: what matters is that they are launches -- a
// step program records them, and p never leaves the device.
//   stats    sum of sign(score) and the number of scores: +-1 and 0 only, so the fp32 sum is exact in any order (n < 2^24)
//   update   the accumulators, the step counter and, every ``interval`` calls, p itself: plain C++ stores from lane 0
// Between the two, data parallelism sum-all-reduces the 4-float stats, so every rank holds the same p bit for bit.
#include "common.h"
#include "reduce.h"
#include "diffaug_kernel.h"

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void ada_stats_kernel(const float* __restrict__ scores, int n, float* __restrict__ stats) {
  __shared__ float red[kThreads / 64];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += kThreads) {
    const float v = scores[i];
    s += v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f);        // sign(0) = 0; NaN compares false both ways: 0
  }
  s = bg::block_sum(s, red);
  if (threadIdx.x == 0) {
    stats[0] = s;
    stats[1] = (float)n;
    stats[2] = 0.f;
    stats[3] = 0.f;
  }
}

// state = {p, acc_sign, acc_count, k, r_last, 0, 0, 0}
__global__ void ada_update_kernel(const float* __restrict__ stats, float* __restrict__ state, float* __restrict__ metrics_out, float target,
                                  int interval, float inv_speed_images) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float p = state[0], r_last = state[4];
  float acc_sign = state[1] + stats[0], acc_count = state[2] + stats[1], k = state[3] + 1.f;
  if (k >= (float)interval) {
    const float r = acc_sign / acc_count;
    const float dir = r > target ? 1.f : (r < target ? -1.f : 0.f);        // sgn(0) = 0; a NaN r (no scores) moves nothing
    p = __fadd_rn(p, __fmul_rn(dir * acc_count, inv_speed_images));      // two roundings, never an fma: the rule as written
    p = p < 0.f ? 0.f : (p > 1.f ? 1.f : p);
    r_last = r;
    acc_sign = 0.f; acc_count = 0.f; k = 0.f;
  }
  state[0] = p; state[1] = acc_sign; state[2] = acc_count; state[3] = k; state[4] = r_last;
  if (metrics_out) {
    metrics_out[0] = p;
    metrics_out[1] = r_last;
  }
}

}  // namespace

extern "C" {

int bg_diffaug_decode_gated(const float* u, float p, int H, int W, int ops_mask, float translation_ratio, float cutout_ratio, float* bsc,
                            int* geo, int* fired_mask) {
  BG_REQUIRE(u && bsc && geo && fired_mask, BG_ERR_NULL, "bg_diffaug_decode_gated: null pointer");
  BG_REQUIRE(H > 0 && W > 0, BG_ERR_BAD_SHAPE, "bg_diffaug_decode_gated: H=%d W=%d", H, W);
  BG_REQUIRE(ops_mask >= 0 && ops_mask <= 7, BG_ERR_UNSUPPORTED, "bg_diffaug_decode_gated: ops_mask=%d (bits: 1 color, 2 translation, 4 cutout)",
             ops_mask);
  Geo g;
  g.n = 1; g.H = H; g.W = W; g.C = 1; g.E = H * W;
  g.ops = ops_mask; g.linear = 0;
  g.Sy = round_half_up(H, translation_ratio); g.Sx = round_half_up(W, translation_ratio);
  g.cy = round_half_up(H, cutout_ratio); g.cx = round_half_up(W, cutout_ratio);
  const int ops = fired_ops(u, p, ops_mask);
  const Draw d = decode(u, g, ops);
  bsc[0] = d.b; bsc[1] = d.s; bsc[2] = d.c;
  // an operation that did not fire has an empty box: its size is reported as 0
  geo[0] = d.ty; geo[1] = d.tx; geo[2] = d.y0; geo[3] = d.x0; geo[4] = d.y1 - d.y0; geo[5] = d.x1 - d.x0; geo[6] = g.Sy; geo[7] = g.Sx;
  *fired_mask = ops;
  return BG_OK;
}

int bg_diffaug_gated_f32(const float* x, float* y, const float* params, const float* p, int n, int H, int W, int C, int ops_mask,
                         float translation_ratio, float cutout_ratio, int linear, void* stream) {
  return run<true>(false, x, y, params, p, n, H, W, C, ops_mask, translation_ratio, cutout_ratio, linear, stream, "bg_diffaug_gated_f32");
}

int bg_diffaug_gated_adjoint_f32(const float* dy, float* dx, const float* params, const float* p, int n, int H, int W, int C, int ops_mask,
                                 float translation_ratio, float cutout_ratio, void* stream) {
  return run<true>(true, dy, dx, params, p, n, H, W, C, ops_mask, translation_ratio, cutout_ratio, 1, stream,
                   "bg_diffaug_gated_adjoint_f32");
}

int bg_ada_stats_f32(const float* scores, int n, float* stats, void* stream) {
  BG_REQUIRE(scores && stats, BG_ERR_NULL, "bg_ada_stats_f32: null pointer");
  BG_REQUIRE(n > 0 && n < (1 << 24), BG_ERR_BAD_SHAPE, "bg_ada_stats_f32: n=%d (1 .. 2^24 - 1: the count is exact in fp32)", n);
  BG_REQUIRE(((reinterpret_cast<uintptr_t>(scores) | reinterpret_cast<uintptr_t>(stats)) & 3u) == 0, BG_ERR_BAD_ALIGNMENT,
             "bg_ada_stats_f32: pointers must be 4-byte aligned");
  bg::Launch L(stream, "ada_stats", 0, 4.0 * n + 16.0);
  bg::launch(ada_stats_kernel, dim3(1), dim3(kThreads), 0, L.s, scores, n, stats);
  return L.done("ada_stats_kernel");
}

int bg_ada_update_f32(const float* stats, float* state, float* metrics_out, float target, int interval, float inv_speed_images,
                      void* stream) {
  BG_REQUIRE(stats && state, BG_ERR_NULL, "bg_ada_update_f32: null pointer");
  BG_REQUIRE(interval >= 1, BG_ERR_BAD_SHAPE, "bg_ada_update_f32: interval=%d", interval);
  BG_REQUIRE(target > -1.f && target < 1.f && inv_speed_images > 0.f, BG_ERR_UNSUPPORTED,
             "bg_ada_update_f32: target=%g outside (-1, 1) or inv_speed_images=%g not above 0", (double)target, (double)inv_speed_images);
  BG_REQUIRE(((reinterpret_cast<uintptr_t>(stats) | reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(metrics_out)) & 3u) == 0,
             BG_ERR_BAD_ALIGNMENT, "bg_ada_update_f32: pointers must be 4-byte aligned");
  bg::Launch L(stream, "ada_update", 0, 64.0);
  bg::launch(ada_update_kernel, dim3(1), dim3(64), 0, L.s, stats, state, metrics_out, target, interval, inv_speed_images);
  return L.done("ada_update_kernel");
}

}  // extern "C"
