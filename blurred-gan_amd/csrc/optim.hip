// Optimiser updates besides the default Adam (bg_adam_f32, misc.hip): tf.keras.optimizers SGD, RMSprop and Adam(amsgrad=True),
// as TF 2.5's keras/optimizer_v2 and the training_ops functors it calls define them (include/bgan.h "optimisers").  The host
// computes the step's learning rate (schedule, inverse-time decay, Adam's bias correction); the kernels apply the elementwise
// rule over a model's flat trainable buffer.  One kernel per static variant (momentum / Nesterov / centered are template
// parameters); the body moves float4 quads in a grid-stride loop, and the n % 4 last elements go through a scalar tail.
// bg_ema_f32 (the averaged generator's update, tf.train.ExponentialMovingAverage) sweeps two buffers the same way in one launch.
#include "common.h"
#include <algorithm>
#include <cmath>

namespace {

constexpr int kT = 256;

// The sweep every variant shares.  f(theta, s1, s2, s3, g) updates one element in place; slot streams the variant does not use
// (U* = false) are neither loaded nor stored, so their pointers may be null.
template <bool U1, bool U2, bool U3, class F>
__device__ inline void sweep(float* __restrict__ th, float* __restrict__ s1, float* __restrict__ s2, float* __restrict__ s3,
                             const float* __restrict__ g, size_t n, F f) {
  const size_t n4 = n >> 2, stride = (size_t)gridDim.x * kT;
  float4* t4 = reinterpret_cast<float4*>(th);
  float4* a4 = reinterpret_cast<float4*>(s1);
  float4* b4 = reinterpret_cast<float4*>(s2);
  float4* c4 = reinterpret_cast<float4*>(s3);
  const float4* g4 = reinterpret_cast<const float4*>(g);
  for (size_t q = (size_t)blockIdx.x * kT + threadIdx.x; q < n4; q += stride) {
    float4 t = t4[q], a = {0.f, 0.f, 0.f, 0.f}, b = a, c = a;
    const float4 gg = g4[q];
    if constexpr (U1) a = a4[q];
    if constexpr (U2) b = b4[q];
    if constexpr (U3) c = c4[q];
    f(t.x, a.x, b.x, c.x, gg.x);
    f(t.y, a.y, b.y, c.y, gg.y);
    f(t.z, a.z, b.z, c.z, gg.z);
    f(t.w, a.w, b.w, c.w, gg.w);
    t4[q] = t;
    if constexpr (U1) a4[q] = a;
    if constexpr (U2) b4[q] = b;
    if constexpr (U3) c4[q] = c;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const size_t e = (n4 << 2) + threadIdx.x;
    float t = th[e], a = U1 ? s1[e] : 0.f, b = U2 ? s2[e] : 0.f, c = U3 ? s3[e] : 0.f;
    f(t, a, b, c, g[e]);
    th[e] = t;
    if constexpr (U1) s1[e] = a;
    if constexpr (U2) s2[e] = b;
    if constexpr (U3) s3[e] = c;
  }
}

// SGD: ResourceApplyGradientDescent (momentum 0) / ResourceApplyKerasMomentum: a = mu*a - lr*g; theta += a (Nesterov:
// theta += mu*a - lr*g)
template <bool MOM, bool NEST>
__global__ __launch_bounds__(kT) void sgd_kernel(float* theta, float* a, const float* g, size_t n, float lr, float mu) {
  sweep<MOM, false, false>(theta, a, nullptr, nullptr, g, n, [=](float& t, float& ai, float&, float&, float gi) {
    if constexpr (MOM) {
      ai = mu * ai - lr * gi;
      t = NEST ? t + (mu * ai - lr * gi) : t + ai;
    } else {
      t = t - lr * gi;
    }
  });
}

// RMSprop: r = rho*r + (1-rho)*g^2; centered: mg = rho*mg + (1-rho)*g, d = r - mg^2 (else d = r).
// momentum 0 (Keras' Python path): theta -= lr*g / (sqrt(d) + eps);  momentum > 0 (ResourceApplyRMSProp /
// ResourceApplyCenteredRMSProp, epsilon INSIDE the root): p = mu*p + lr*g / sqrt(d + eps); theta -= p
template <bool MOM, bool CEN>
__global__ __launch_bounds__(kT) void rmsprop_kernel(float* theta, float* r, float* p, float* mg, const float* g, size_t n, float lr,
                                                     float rho, float mu, float eps) {
  sweep<true, MOM, CEN>(theta, r, p, mg, g, n, [=](float& t, float& ri, float& pi, float& mgi, float gi) {
    ri = rho * ri + (1.f - rho) * gi * gi;
    float d = ri;
    if constexpr (CEN) {
      mgi = rho * mgi + (1.f - rho) * gi;
      d = ri - mgi * mgi;
    }
    if constexpr (MOM) {
      pi = mu * pi + lr * gi / sqrtf(d + eps);
      t = t - pi;
    } else {
      t = t - lr * gi / (sqrtf(d) + eps);
    }
  });
}

// Adam with amsgrad (ResourceApplyAdamWithAmsgrad): bg_adam_f32's m / v, vhat = max(vhat, v), theta -= lr_t*m / (sqrt(vhat) + eps)
__global__ __launch_bounds__(kT) void adam_amsgrad_kernel(float* theta, float* m, float* v, float* vh, const float* g, size_t n,
                                                          float lr_t, float b1, float b2, float eps) {
  sweep<true, true, true>(theta, m, v, vh, g, n, [=](float& t, float& mi, float& vi, float& vhi, float gi) {
    mi = b1 * mi + (1.f - b1) * gi;
    vi = b2 * vi + (1.f - b2) * gi * gi;
    vhi = fmaxf(vhi, vi);
    t = t - lr_t * mi / (sqrtf(vhi) + eps);
  });
}

// Weight averaging (TF assign_moving_average): avg -= w * (avg - theta), w = 1 - decay.  The same sweep shape over one buffer.
__device__ inline void ema_sweep(float* __restrict__ avg, const float* __restrict__ th, size_t n, float w) {
  const size_t n4 = n >> 2, stride = (size_t)gridDim.x * kT;
  float4* a4 = reinterpret_cast<float4*>(avg);
  const float4* t4 = reinterpret_cast<const float4*>(th);
  for (size_t q = (size_t)blockIdx.x * kT + threadIdx.x; q < n4; q += stride) {
    float4 a = a4[q];
    const float4 t = t4[q];
    a.x = a.x - w * (a.x - t.x);
    a.y = a.y - w * (a.y - t.y);
    a.z = a.z - w * (a.z - t.z);
    a.w = a.w - w * (a.w - t.w);
    a4[q] = a;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const size_t e = (n4 << 2) + threadIdx.x;
    const float a = avg[e];
    avg[e] = a - w * (a - th[e]);
  }
}

// Both segments of a network in one launch: the trainable buffer, then the (small) non-trainable state buffer; n2 == 0 touches
// neither avg2 nor theta2.
__global__ __launch_bounds__(kT) void ema_kernel(float* avg, const float* theta, size_t n, float* avg2, const float* theta2, size_t n2,
                                                 float w) {
  ema_sweep(avg, theta, n, w);
  ema_sweep(avg2, theta2, n2, w);
}

bool al(const void* p) { return p == nullptr || bg::aligned16(p); }

}  // namespace

extern "C" {

int bg_sgd_f32(float* theta, float* a, const float* g, size_t n, float lr, float momentum, int nesterov, void* stream) {
  BG_REQUIRE(theta && g, BG_ERR_NULL, "bg_sgd_f32: null pointer");
  BG_REQUIRE(n > 0, BG_ERR_BAD_SHAPE, "bg_sgd_f32: empty tensor");
  BG_REQUIRE(momentum >= 0.f && momentum <= 1.f, BG_ERR_BAD_SHAPE, "bg_sgd_f32: momentum=%g outside [0, 1]", momentum);
  const bool mom = momentum > 0.f;
  BG_REQUIRE(!mom || a, BG_ERR_NULL, "bg_sgd_f32: momentum > 0 needs the momentum slot");
  BG_REQUIRE(al(theta) && al(g) && (!mom || al(a)), BG_ERR_BAD_ALIGNMENT, "bg_sgd_f32: pointers must be 16-byte aligned");
  bg::Launch L(stream, !mom ? "sgd" : nesterov ? "sgd_nesterov" : "sgd_momentum", 0, (mom ? 20.0 : 12.0) * n);
  const int slot = bg::take_bind(BG_BIND_OPT_LR);          // step program: lr re-read from a slot before every replay
  auto k = !mom ? sgd_kernel<false, false> : nesterov ? sgd_kernel<true, true> : sgd_kernel<true, false>;
  bg::launch(k, dim3(bg::grid_cap(n, kT, 4)), dim3(kT), 0, L.s, theta, mom ? a : nullptr, g, n, lr, momentum);
  bg::bind_last(4, bg::BIND_F32_FROM_F64, slot);
  return L.done("sgd_kernel");
}

int bg_rmsprop_f32(float* theta, float* r, float* p, float* mg, const float* g, size_t n, float lr, float rho, float momentum, float eps,
                   int centered, void* stream) {
  BG_REQUIRE(theta && r && g, BG_ERR_NULL, "bg_rmsprop_f32: null pointer");
  BG_REQUIRE(n > 0, BG_ERR_BAD_SHAPE, "bg_rmsprop_f32: empty tensor");
  BG_REQUIRE(momentum >= 0.f, BG_ERR_BAD_SHAPE, "bg_rmsprop_f32: momentum=%g", momentum);
  const bool mom = momentum > 0.f, cen = centered != 0;
  BG_REQUIRE(!mom || p, BG_ERR_NULL, "bg_rmsprop_f32: momentum > 0 needs the momentum slot");
  BG_REQUIRE(!cen || mg, BG_ERR_NULL, "bg_rmsprop_f32: centered needs the mean-gradient slot");
  BG_REQUIRE(al(theta) && al(r) && al(g) && (!mom || al(p)) && (!cen || al(mg)), BG_ERR_BAD_ALIGNMENT,
             "bg_rmsprop_f32: pointers must be 16-byte aligned");
  static const char* names[4] = {"rmsprop", "rmsprop_momentum", "rmsprop_centered", "rmsprop_centered_momentum"};
  bg::Launch L(stream, names[(cen ? 2 : 0) + (mom ? 1 : 0)], 0, (20.0 + (mom ? 8.0 : 0.0) + (cen ? 8.0 : 0.0)) * n);
  const int slot = bg::take_bind(BG_BIND_OPT_LR);
  auto k = mom ? (cen ? rmsprop_kernel<true, true> : rmsprop_kernel<true, false>)
               : (cen ? rmsprop_kernel<false, true> : rmsprop_kernel<false, false>);
  bg::launch(k, dim3(bg::grid_cap(n, kT, 4)), dim3(kT), 0, L.s, theta, r, mom ? p : nullptr, cen ? mg : nullptr, g, n, lr, rho, momentum, eps);
  bg::bind_last(6, bg::BIND_F32_FROM_F64, slot);
  return L.done("rmsprop_kernel");
}

int bg_adam_amsgrad_f32(float* theta, float* m, float* v, float* vhat, const float* g, size_t n, float lr_t, float b1, float b2,
                        float eps, void* stream) {
  BG_REQUIRE(theta && m && v && vhat && g, BG_ERR_NULL, "bg_adam_amsgrad_f32: null pointer");
  BG_REQUIRE(n > 0, BG_ERR_BAD_SHAPE, "bg_adam_amsgrad_f32: empty tensor");
  BG_REQUIRE(al(theta) && al(m) && al(v) && al(vhat) && al(g), BG_ERR_BAD_ALIGNMENT, "bg_adam_amsgrad_f32: pointers must be 16-byte aligned");
  bg::Launch L(stream, "adam_amsgrad", 0, 36.0 * n);
  const int slot = bg::take_bind(BG_BIND_OPT_LR);
  bg::launch(adam_amsgrad_kernel, dim3(bg::grid_cap(n, kT, 4)), dim3(kT), 0, L.s, theta, m, v, vhat, g, n, lr_t, b1, b2, eps);
  bg::bind_last(6, bg::BIND_F32_FROM_F64, slot);
  return L.done("adam_amsgrad_kernel");
}

int bg_ema_f32(float* avg, const float* theta, size_t n, float* avg2, const float* theta2, size_t n2, float w, void* stream) {
  BG_REQUIRE(avg && theta && (n2 == 0 || (avg2 && theta2)), BG_ERR_NULL, "bg_ema_f32: null pointer");
  BG_REQUIRE(n > 0, BG_ERR_BAD_SHAPE, "bg_ema_f32: empty tensor");
  BG_REQUIRE(w >= 0.f && w <= 1.f, BG_ERR_BAD_SHAPE, "bg_ema_f32: w=%g outside [0, 1]", w);
  BG_REQUIRE(al(avg) && al(theta) && (n2 == 0 || (al(avg2) && al(theta2))), BG_ERR_BAD_ALIGNMENT,
             "bg_ema_f32: pointers must be 16-byte aligned");
  bg::Launch L(stream, "ema", 0, 12.0 * (double)(n + n2));
  const int slot = bg::take_bind(BG_BIND_EMA_W);           // step program: w re-read from a slot before every replay
  bg::launch(ema_kernel, dim3(bg::grid_cap(n, kT, 4)), dim3(kT), 0, L.s, avg, theta, n, n2 ? avg2 : nullptr, n2 ? theta2 : nullptr, n2, w);
  bg::bind_last(6, bg::BIND_F32_FROM_F64, slot);
  return L.done("ema_kernel");
}

}  // extern "C"
