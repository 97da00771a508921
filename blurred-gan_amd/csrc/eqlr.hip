// Equalised learning rate (include/bgan.h "equalised learning rate"): the engine computes with W_eff = c * W, c = gain / sqrt(fan_in)
// a per-layer constant, and the optimizer sees dL/dW = c * dL/dW_eff.
//
// Both entry points are batched over all wrapped layers of one model through a device table of bg_eqlr_desc-shaped rows (12 ints
// per layer: float offsets into theta / the flat gradient buffer and into the effective-weight base, K, N, taps, the layer's first
// work unit in each of the two unit numberings and the bits of c), so the number of launches does not depend on the number of
// layers.  How a matrix is cut into units depends on (K, N, taps) alone, every element is written by exactly one thread and gets
// exactly one fp32 multiply: a batched launch computes bit for bit what per-layer launches compute.  No atomics.
//
//   scale   eff = c * W, 64 x 64 tiles numbered [tap][r-tile][c-tile]; conv layers get the [taps][N][R] transposed copy from the same
//           LDS tile.  The tile walk is spectral.hip's sn_scale_kernel; the multiplier comes from the table instead of 1 / sigma from
//           device state, which is why the body is a separate one: sn_scale_kernel divides, and its code object stays as it is.
//   grad    g *= c in place over [w_off, w_off + K * N) of the flat gradient buffer, units of kUnitElems floats numbered across
//           layers: float4 body, scalar tail for the last K * N % 4 floats; the padding behind a segment is not touched.
#include "common.h"

namespace {

struct EqDesc { int w_off, eff_off, tr_off, K, N, taps, tile_first, unit_first; float c; int pad0, pad1, pad2; };
static_assert(sizeof(EqDesc) == BG_EQLR_DESC_INTS * sizeof(int), "descriptor row");

constexpr int kUnitElems = 16384;     // elements of one gradient unit: 256 threads x 16 float4

struct EqPlan { int tiles, vec, grad_units; };

__host__ __device__ inline EqPlan eq_plan(int K, int N, int taps) {
  EqPlan p;
  const int R = K / (taps > 0 ? taps : 1);
  p.tiles = taps * ((R + 63) / 64) * ((N + 63) / 64);
  p.vec = (((R | N) & 3) == 0) ? 4 : 1;
  p.grad_units = (int)(((long long)K * N + kUnitElems - 1) / kUnitElems);
  return p;
}

__device__ inline int find_layer(const EqDesc* __restrict__ desc, int n, int first_field, int unit) {
  int e = 0;          // workgroup-uniform scan of a short table
  while (e + 1 < n && reinterpret_cast<const int*>(desc + e + 1)[first_field] <= unit) ++e;
  return e;
}

__global__ __launch_bounds__(256) void eqlr_scale_kernel(const float* __restrict__ theta, float* __restrict__ eff, const EqDesc* __restrict__ desc,
                                                         int n) {
  __shared__ float tile[64][65];
  const int e = find_layer(desc, n, 6, blockIdx.x);
  const EqDesc d = desc[e];
  const int R = d.K / d.taps, Cc = d.N;
  const int tr = (R + 63) / 64, tc = (Cc + 63) / 64;
  int local = blockIdx.x - d.tile_first;
  const int t = local / (tr * tc);
  local -= t * tr * tc;
  const int r0 = (local / tc) * 64, c0 = (local % tc) * 64;
  const float c = d.c;
  const float* s = theta + d.w_off + (size_t)t * R * Cc;
  float* o = eff + d.eff_off + (size_t)t * R * Cc;
  float* ot = d.tr_off >= 0 ? eff + d.tr_off + (size_t)t * R * Cc : nullptr;
  const int tid = threadIdx.x;
  if (((R | Cc) & 3) == 0) {
    const int q = tid & 15, rr = tid >> 4;                    // 16 float4 across 64 columns, 16 rows per pass
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = r0 + rr + 16 * i, col = c0 + 4 * q;
      if (r < R && col < Cc) {
        float4 x = *reinterpret_cast<const float4*>(s + (size_t)r * Cc + col);
        x.x = c * x.x; x.y = c * x.y; x.z = c * x.z; x.w = c * x.w;
        *reinterpret_cast<float4*>(o + (size_t)r * Cc + col) = x;
        tile[rr + 16 * i][4 * q] = x.x; tile[rr + 16 * i][4 * q + 1] = x.y; tile[rr + 16 * i][4 * q + 2] = x.z; tile[rr + 16 * i][4 * q + 3] = x.w;
      }
    }
    if (!ot) return;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int col = c0 + rr + 16 * i, r = r0 + 4 * q;
      if (col < Cc && r < R)
        *reinterpret_cast<float4*>(ot + (size_t)col * R + r) =
            make_float4(tile[4 * q][rr + 16 * i], tile[4 * q + 1][rr + 16 * i], tile[4 * q + 2][rr + 16 * i], tile[4 * q + 3][rr + 16 * i]);
    }
  } else {
    const int tx = tid & 63, ty = tid >> 6;
    for (int i = ty; i < 64; i += 4)
      if (r0 + i < R && c0 + tx < Cc) {
        const float x = c * s[(size_t)(r0 + i) * Cc + c0 + tx];
        o[(size_t)(r0 + i) * Cc + c0 + tx] = x;
        tile[i][tx] = x;
      }
    if (!ot) return;
    __syncthreads();
    for (int i = ty; i < 64; i += 4)
      if (c0 + i < Cc && r0 + tx < R) ot[(size_t)(c0 + i) * R + r0 + tx] = tile[tx][i];
  }
}

// g *= c over one kUnitElems unit of a layer's segment.  w_off and the unit's first element are multiples of four floats.
__global__ __launch_bounds__(256) void eqlr_grad_kernel(float* __restrict__ grad, const EqDesc* __restrict__ desc, int n) {
  const int e = find_layer(desc, n, 7, blockIdx.x);
  const EqDesc d = desc[e];
  const int unit = blockIdx.x - d.unit_first;
  const int total = d.K * d.N;
  const float c = d.c;
  float* g = grad + d.w_off;
#pragma unroll 4
  for (int it = 0; it < kUnitElems / 1024; ++it) {
    const int i = unit * kUnitElems + (it * 256 + (int)threadIdx.x) * 4;
    if (i + 3 < total) {
      float4 x = *reinterpret_cast<const float4*>(g + i);
      x.x = c * x.x; x.y = c * x.y; x.z = c * x.z; x.w = c * x.w;
      *reinterpret_cast<float4*>(g + i) = x;
    } else {
      for (int j = i; j < total; ++j) g[j] = c * g[j];
    }
  }
}

// ---- host side
struct Sizes { int tiles, grad_units; double elems, tr_elems; };

inline bool overlap(long long a0, long long a1, long long b0, long long b1) { return a0 < b1 && b0 < a1; }

// Checks the host copy of the table against the sizes of the buffers it points into; fills the launch sizes.  Nothing touches the
// device before this has passed.  eff_floats < 0: the call takes no effective-weight base (the gradient call), eff_off / tr_off are
// still checked for sign, alignment and overlap.
int check_table(const char* who, const int* desc_h, int n, long long theta_floats, long long eff_floats, Sizes* sizes) {
  BG_REQUIRE(desc_h, BG_ERR_NULL, "%s: null descriptor table", who);
  BG_REQUIRE(n > 0, BG_ERR_BAD_SHAPE, "%s: n=%d layers", who, n);
  BG_REQUIRE(theta_floats > 0, BG_ERR_BAD_SHAPE, "%s: theta_floats=%lld", who, theta_floats);
  const EqDesc* d = reinterpret_cast<const EqDesc*>(desc_h);
  Sizes s = {0, 0, 0.0, 0.0};
  for (int e = 0; e < n; ++e) {
    BG_REQUIRE(d[e].K > 0 && d[e].N > 0, BG_ERR_BAD_SHAPE, "%s: layer %d: K=%d N=%d", who, e, d[e].K, d[e].N);
    BG_REQUIRE(d[e].taps > 0 && d[e].K % d[e].taps == 0, BG_ERR_BAD_SHAPE, "%s: layer %d: taps=%d does not divide K=%d", who, e, d[e].taps, d[e].K);
    BG_REQUIRE((long long)d[e].K * d[e].N < (1ll << 30), BG_ERR_BAD_SHAPE, "%s: layer %d: K*N too large", who, e);
    BG_REQUIRE(d[e].c > 0.f && d[e].c <= 3.0e38f, BG_ERR_BAD_SHAPE, "%s: layer %d: coefficient %g must be positive and finite", who, e, (double)d[e].c);
    BG_REQUIRE(d[e].w_off >= 0 && d[e].eff_off >= 0 && d[e].tr_off >= -1, BG_ERR_BAD_SHAPE, "%s: layer %d: negative offset", who, e);
    BG_REQUIRE(((d[e].w_off | d[e].eff_off) & 3) == 0 && (d[e].tr_off < 0 || (d[e].tr_off & 3) == 0), BG_ERR_BAD_ALIGNMENT,
               "%s: layer %d: offsets must be multiples of 4 floats", who, e);
    BG_REQUIRE(d[e].tile_first == s.tiles && d[e].unit_first == s.grad_units, BG_ERR_BAD_SHAPE,
               "%s: layer %d: first units (%d, %d) do not continue the table (%d, %d)", who, e, d[e].tile_first, d[e].unit_first, s.tiles, s.grad_units);
    const long long kn = (long long)d[e].K * d[e].N;
    BG_REQUIRE(d[e].w_off + kn <= theta_floats, BG_ERR_BAD_SHAPE, "%s: layer %d: kernel [%d, %lld) ends behind the %lld floats of the buffer", who, e,
               d[e].w_off, d[e].w_off + kn, theta_floats);
    if (eff_floats >= 0)
      BG_REQUIRE(d[e].eff_off + kn <= eff_floats && (d[e].tr_off < 0 || d[e].tr_off + kn <= eff_floats), BG_ERR_BAD_SHAPE,
                 "%s: layer %d: effective weights (eff_off %d, tr_off %d, %lld floats each) end behind the %lld floats of the buffer", who, e,
                 d[e].eff_off, d[e].tr_off, kn, eff_floats);
    BG_REQUIRE(d[e].tr_off < 0 || !overlap(d[e].eff_off, d[e].eff_off + kn, d[e].tr_off, d[e].tr_off + kn), BG_ERR_BAD_SHAPE,
               "%s: layer %d: the transposed copy overlaps the effective kernel", who, e);
    for (int f = 0; f < e; ++f) {         // a short table: pairwise
      const long long fn = (long long)d[f].K * d[f].N;
      BG_REQUIRE(!overlap(d[e].w_off, d[e].w_off + kn, d[f].w_off, d[f].w_off + fn), BG_ERR_BAD_SHAPE, "%s: layers %d and %d: kernels overlap", who, f, e);
      const long long es[2] = {d[e].eff_off, d[e].tr_off}, fs[2] = {d[f].eff_off, d[f].tr_off};
      for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b)
          BG_REQUIRE(es[a] < 0 || fs[b] < 0 || !overlap(es[a], es[a] + kn, fs[b], fs[b] + fn), BG_ERR_BAD_SHAPE,
                     "%s: layers %d and %d: effective-weight segments overlap", who, f, e);
    }
    const EqPlan p = eq_plan(d[e].K, d[e].N, d[e].taps);
    s.tiles += p.tiles;
    s.grad_units += p.grad_units;
    s.elems += (double)kn;
    if (d[e].tr_off >= 0) s.tr_elems += (double)kn;
  }
  if (sizes) *sizes = s;
  return BG_OK;
}

}  // namespace

extern "C" {

int bg_eqlr_plan(int K, int N, int taps, int* tiles, int* vec, int* grad_units, int* unit_elems) {
  BG_REQUIRE(K > 0 && N > 0 && taps > 0 && K % taps == 0 && (long long)K * N < (1ll << 30), BG_ERR_BAD_SHAPE, "bg_eqlr_plan: K=%d N=%d taps=%d", K, N, taps);
  const EqPlan p = eq_plan(K, N, taps);
  if (tiles) *tiles = p.tiles;
  if (vec) *vec = p.vec;
  if (grad_units) *grad_units = p.grad_units;
  if (unit_elems) *unit_elems = kUnitElems;
  return BG_OK;
}

int bg_eqlr_check_table(const int* desc_h, int n, size_t theta_floats, size_t eff_floats) {
  return check_table("bg_eqlr_check_table", desc_h, n, (long long)theta_floats, (long long)eff_floats, nullptr);
}

int bg_eqlr_scale_f32(const float* theta, size_t theta_floats, float* eff, size_t eff_floats, const int* desc_d, const int* desc_h, int n,
                      void* stream) {
  BG_REQUIRE(theta && eff && desc_d, BG_ERR_NULL, "bg_eqlr_scale_f32: null pointer");
  Sizes z;
  if (int rc = check_table("bg_eqlr_scale_f32", desc_h, n, (long long)theta_floats, (long long)eff_floats, &z)) return rc;
  BG_REQUIRE(bg::aligned16(theta) && bg::aligned16(eff) && bg::aligned16(desc_d), BG_ERR_BAD_ALIGNMENT, "bg_eqlr_scale_f32: bases must be 16-byte aligned");
  bg::Launch L(stream, "eqlr_scale", 0, 8.0 * z.elems + 4.0 * z.tr_elems);
  bg::launch(eqlr_scale_kernel, dim3((unsigned)z.tiles), dim3(256), 0, L.s, theta, eff, reinterpret_cast<const EqDesc*>(desc_d), n);
  return L.done("eqlr_scale_kernel");
}

int bg_eqlr_grad_f32(float* grad, size_t grad_floats, const int* desc_d, const int* desc_h, int n, void* stream) {
  BG_REQUIRE(grad && desc_d, BG_ERR_NULL, "bg_eqlr_grad_f32: null pointer");
  Sizes z;
  if (int rc = check_table("bg_eqlr_grad_f32", desc_h, n, (long long)grad_floats, -1, &z)) return rc;
  BG_REQUIRE(bg::aligned16(grad) && bg::aligned16(desc_d), BG_ERR_BAD_ALIGNMENT, "bg_eqlr_grad_f32: bases must be 16-byte aligned");
  bg::Launch L(stream, "eqlr_grad", 0, 8.0 * z.elems);
  bg::launch(eqlr_grad_kernel, dim3((unsigned)z.grad_units), dim3(256), 0, L.s, grad, reinterpret_cast<const EqDesc*>(desc_d), n);
  return L.done("eqlr_grad_kernel");
}

}  // extern "C"
