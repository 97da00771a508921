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
#include "diffaug_kernel.h"

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
  const Draw d = decode(u, g, g.ops);
  bsc[0] = d.b; bsc[1] = d.s; bsc[2] = d.c;
  geo[0] = d.ty; geo[1] = d.tx; geo[2] = d.y0; geo[3] = d.x0; geo[4] = g.cy; geo[5] = g.cx; geo[6] = g.Sy; geo[7] = g.Sx;
  return BG_OK;
}

int bg_diffaug_f32(const float* x, float* y, const float* params, int n, int H, int W, int C, int ops_mask, float translation_ratio,
                   float cutout_ratio, int linear, void* stream) {
  return run<false>(false, x, y, params, nullptr, n, H, W, C, ops_mask, translation_ratio, cutout_ratio, linear, stream, "bg_diffaug_f32");
}

int bg_diffaug_adjoint_f32(const float* dy, float* dx, const float* params, int n, int H, int W, int C, int ops_mask,
                           float translation_ratio, float cutout_ratio, void* stream) {
  return run<false>(true, dy, dx, params, nullptr, n, H, W, C, ops_mask, translation_ratio, cutout_ratio, 1, stream, "bg_diffaug_adjoint_f32");
}

}  // extern "C"
