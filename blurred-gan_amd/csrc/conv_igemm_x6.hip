// Opt-in split-bf16 conv math (include/bgan.h BG_CONV_MATH_BF16X6): the gather-GEMM of conv_igemm.hip with its fp32 products
// rebuilt from bf16 pieces on the bf16 matrix pipe, for the conv forward and data gradient.
//
// Every fp32 operand x is split EXACTLY into three bf16 pieces while the tile is staged into LDS (once per element, not per wave
// and fragment):  hi = top 16 bits of x,  r = x - hi (exact),  mid = top 16 bits of r,  lo = bf16_rne(r - mid).  A product
// a * b is rebuilt from the six cross terms that reach fp32 precision -- hi.hi, hi.mid, mid.hi, hi.lo, lo.hi, mid.mid -- each a
// v_mfma_f32_32x32x16_bf16 accumulating in fp32, the small terms issued before the large ones.  The three terms left out
// (mid.lo, lo.mid, lo.lo) are below 2^-24 of |a b|.  An Inf / NaN element keeps its value in hi and gets mid = lo = 0, so the
// result carries the same Inf / NaN as the fp32 kernel (not a NaN made by inf - inf); a zero mid / lo piece of a finite element
// is lifted to +-2^-126 with the element's sign (no_zero_bf16x2) so that it never meets an Inf of the other operand as Inf x 0.
//
//   conv_igemm_x6_kernel   BM = 128 pixel rows x BN = 128 / 64 / 32 output channels, 4 waves, K steps of 32 channels (two
//                          32x32x16 k-slices), one LDS stage of the three pieces (6 B per element: 60 / 45 / 38 KB, two to
//                          three workgroups per CU) refilled from a register prefetch one step ahead.  Pixel-major rows, no
//                          split-K, no phase merging: each workgroup runs one phase's whole K loop in a fixed order, so results
//                          are bit-reproducible from run to run.  Epilogue: every bg_epilogue mode, and the BatchNorm statistics
//                          partials (stats, mode NONE without bias) as one row per workgroup.
//   Loader: the ideas of the fp32 kernel -- buffer descriptors whose range check returns zeros for poisoned offsets (bit 31:
//   the row's source pixel is SAME padding at this tap, bit t of a per-row mask taken once), the channel chunk and the weight tap
//   offset in the instruction's scalar offset, and a descriptor of zero records for the prefetch past the last step.
//
// Which geometries take it is a static table (kX6Table below), from MI355X measurements (profiles/r06_a_conv_math_bf16x6.md):
// a geometry runs x6 only where it measured faster than the fp32 kernel; every other call runs the fp32 path unchanged.
#include "conv_common.h"
#include <algorithm>
#include <cstdlib>

namespace {

using bg::GatherParams;
using bg::GatherPhase;
using bg::RowAnchor;

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kBK = 32;          // fp32 channels per K step: two 32x32x16 k-slices
constexpr int kLDK = kBK + 8;    // bf16 per LDS row (80 B): the 16 rows of a ds_read_b128 lane group land on 16 distinct bank slots
constexpr int kNT = 256;

// Two bf16 pieces of a packed word with a zero (or subnormal) magnitude get the smallest normal magnitude 2^-126, and every
// piece gets the sign of its ELEMENT (`signs`: the packed hi pieces).  A finite element's pieces then never multiply an Inf of
// the other operand as exactly 0 (Inf x 0 = NaN, where the fp32 product is +-Inf), nor with the wrong sign (x - hi = +0 for a
// negative x): truncation gives every nonzero piece the sign of its element, so Inf times the pieces adds up to the same signed
// Inf.  The cost is 2^-126 x |other operand| per piece, far below an fp32 ulp of any product that is not itself of that order.
__device__ __forceinline__ unsigned no_zero_bf16x2(unsigned w, unsigned signs) {
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  const u16x2 mag = __builtin_bit_cast(u16x2, w & 0x7fff7fffu);
  const u16x2 lift = __builtin_elementwise_max(mag, (u16x2){0x0080, 0x0080});       // v_pk_max_u16
  return (__builtin_bit_cast(unsigned, lift) & 0x7fff7fffu) | (signs & 0x80008000u);
}

// Four fp32 values -> their hi / mid / lo bf16 pieces, four of each packed in a uint2 (element 0 in the low half).
__device__ __forceinline__ void split4(const float4 v, uint2& hi, uint2& mid, uint2& lo) {
  const float x[4] = {v.x, v.y, v.z, v.w};
  unsigned hb[4], rb[4];
  float l[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    // a NaN whose payload sits in the low half would truncate to Inf: it becomes the canonical quiet NaN
    hb[e] = __builtin_isnan(x[e]) ? 0x7fc00000u : __float_as_uint(x[e]);
    const float h = __uint_as_float(hb[e] & 0xffff0000u);
    float r = x[e] - h;                                          // exact; NaN exactly when x is Inf or NaN
    r = r == r ? r : 0.f;                                        // Inf / NaN: mid = lo = 0 (not a NaN made by inf - inf)
    rb[e] = __float_as_uint(r);
    l[e] = r - __uint_as_float(rb[e] & 0xffff0000u);             // exact; at most 8 significant bits
  }
  // v_perm_b32: the top halves of two words side by side (truncation: hi and mid are bit masks, not roundings)
  hi.x = __builtin_amdgcn_perm(hb[1], hb[0], 0x07060302u);
  hi.y = __builtin_amdgcn_perm(hb[3], hb[2], 0x07060302u);
  mid.x = no_zero_bf16x2(__builtin_amdgcn_perm(rb[1], rb[0], 0x07060302u), hi.x);
  mid.y = no_zero_bf16x2(__builtin_amdgcn_perm(rb[3], rb[2], 0x07060302u), hi.y);
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  const bf16x2 l01 = {(__bf16)l[0], (__bf16)l[1]}, l23 = {(__bf16)l[2], (__bf16)l[3]};   // v_cvt_pk_bf16_f32 (round to nearest even)
  lo.x = no_zero_bf16x2(__builtin_bit_cast(unsigned, l01), hi.x);
  lo.y = no_zero_bf16x2(__builtin_bit_cast(unsigned, l23), hi.y);
}

template <int BM, int BN, int WAVES_M, int WAVES_N>
__global__ __launch_bounds__(kNT, 2) void conv_igemm_x6_kernel(const GatherParams p) {
  static_assert(WAVES_M * WAVES_N * 64 == kNT, "4 waves per workgroup");
  constexpr int WTM = BM / WAVES_M, WTN = BN / WAVES_N;
  constexpr int MI = WTM / 32, NI = WTN / 32;
  static_assert(MI >= 1 && NI >= 1 && WTM % 32 == 0 && WTN % 32 == 0, "wave tile");
  constexpr int TPR = kBK / 4;                // loader threads per row (one float4 each)
  constexpr int RPP = kNT / TPR;              // rows per loader pass
  constexpr int AP = BM / RPP, BP = BN / RPP;
  static_assert(BM % RPP == 0 && BN % RPP == 0, "loader passes tile the rows exactly");
  constexpr int PA = BM * kLDK, PB = BN * kLDK;   // one piece plane of A / B, in bf16
  // [hi A][mid A][lo A][hi B][mid B][lo B]
  __shared__ __attribute__((aligned(16))) __bf16 smem[3 * (PA + PB)];
  __shared__ int rowdst[BM];
  __shared__ __attribute__((aligned(16))) float s_epi[2][BN];

  const int phase = blockIdx.z;
  const GatherPhase& g = p.ph[phase];
  const int Mph = p.B * g.Ha * g.Wa;
  const int L = p.xcd_swizzle ? bg::xcd_remap(blockIdx.x, gridDim.x) : (int)blockIdx.x;
  const int n_tile = L / p.mtiles, m_tile = L - n_tile * p.mtiles;      // n-major: an XCD keeps its share of the weight panels
  const int m0 = m_tile * BM, n0 = n_tile * BN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  float* stats_row = p.stats ? p.stats + ((size_t)phase * p.mtiles + m_tile) * 2 * p.N : nullptr;
  if (m0 >= Mph) {                                               // phases with a smaller anchor grid: empty tile, zero partials
    if (stats_row && tid < BN && n0 + tid < p.N) { stats_row[n0 + tid] = 0.f; stats_row[p.N + n0 + tid] = 0.f; }
    return;
  }

  // ---- loader bookkeeping
  constexpr unsigned kOob = 0x80000000u;                          // >= num_records: tensors are < 2 GiB (host-checked)
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.A), 0, (int)p.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.Wt), 0, (int)p.w_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsNull = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.A), 0, 0, 0x00020000);
  const int lrow = tid / TPR, lq = tid % TPR;
  const int ntaps = g.ntaps;
  unsigned a_off[AP], a_bad[AP], b_off[BP];
#pragma unroll
  for (int i = 0; i < AP; ++i) {
    RowAnchor ra;
    int dst;
    bg::decode_row(p, g, m0 + lrow + i * RPP, Mph, ra, dst);
    a_off[i] = (unsigned)(((ra.b * p.Hs + ra.ay) * p.Ws + ra.ax) * p.Ck + lq * 4) * 4u;     // garbage for invalid rows: never used
    unsigned bad = 0u;                                           // bit t: tap t falls on SAME padding for this row (or no row)
    for (int t = 0; t < ntaps; ++t) {
      const int tp = g.tap[t];
      bad |= ((unsigned)(ra.ay + bg::tap_dy(tp)) < (unsigned)p.Hs && (unsigned)(ra.ax + bg::tap_dx(tp)) < (unsigned)p.Ws) ? 0u : (1u << t);
    }
    a_bad[i] = bad;
  }
#pragma unroll
  for (int i = 0; i < BP; ++i) {
    const int n = n0 + lrow + i * RPP;
    b_off[i] = n < p.N ? (unsigned)(n * p.Ck + lq * 4) * 4u : kOob;
  }
  if (tid < BM) {
    RowAnchor tmp;
    int dst;
    bg::decode_row(p, g, m0 + tid, Mph, tmp, dst);
    rowdst[tid] = dst;
  }
  if (tid < BN) {
    const int n = n0 + tid;
    s_epi[0][tid] = (p.bias && n < p.N) ? p.bias[n] : 0.f;
    s_epi[1][tid] = (p.epi_mode == BG_EPI_AFFINE_LRELU && n < p.N) ? p.ref[n] : 1.f;
  }

  const int kchunks = p.Ck / kBK;
  const int nsteps = ntaps * kchunks;
  int g_t = 0, g_kc = 0, g_left = nsteps;                         // the NEXT load's tap / channel chunk, steps still to load
  unsigned a_voff[AP];                                            // row offset at the current tap (bit 31: poisoned)
  unsigned g_woff = 0;                                            // weight offset of the current tap (scalar)
  auto new_tap = [&]() {
    const int t = min(g_t, ntaps - 1);
    const int tp = g.tap[t];
    const unsigned tapoff = (unsigned)(((bg::tap_dy(tp) * p.Ws + bg::tap_dx(tp)) * p.Ck) * 4);
    g_woff = (unsigned)((bg::tap_wi(tp) * p.N * p.Ck) * 4);
#pragma unroll
    for (int i = 0; i < AP; ++i) a_voff[i] = (((a_bad[i] >> t) & 1u) << 31) | (a_off[i] + tapoff);
  };
  new_tap();
  float4 rA[AP], rB[BP];
  auto gload = [&]() {
    const bool live = g_left > 0;
    const int c0b = g_kc * kBK * 4;                               // this step's channel chunk, in bytes: the scalar offset
    const __amdgpu_buffer_rsrc_t ra = live ? rsA : rsNull, rb = live ? rsB : rsNull;
#pragma unroll
    for (int i = 0; i < AP; ++i) rA[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(ra, a_voff[i], c0b, 0));
#pragma unroll
    for (int i = 0; i < BP; ++i) rB[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rb, b_off[i], (int)g_woff + c0b, 0));
    --g_left;
    if (++g_kc == kchunks) {
      g_kc = 0;
      ++g_t;
      new_tap();
    }
  };
  // split while staging: three ds_write_b64 per float4, one per piece plane
  auto lstore = [&]() {
#pragma unroll
    for (int i = 0; i < AP; ++i) {
      uint2 h, m, l;
      split4(rA[i], h, m, l);
      __bf16* d = smem + (lrow + i * RPP) * kLDK + lq * 4;
      *reinterpret_cast<uint2*>(d) = h;
      *reinterpret_cast<uint2*>(d + PA) = m;
      *reinterpret_cast<uint2*>(d + 2 * PA) = l;
    }
#pragma unroll
    for (int i = 0; i < BP; ++i) {
      uint2 h, m, l;
      split4(rB[i], h, m, l);
      __bf16* d = smem + 3 * PA + (lrow + i * RPP) * kLDK + lq * 4;
      *reinterpret_cast<uint2*>(d) = h;
      *reinterpret_cast<uint2*>(d + PB) = m;
      *reinterpret_cast<uint2*>(d + 2 * PB) = l;
    }
  };

  floatx16 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // fragments of a 32x32x16 k-slice: lane l holds row (l & 31), k = 8 (l >> 5) .. + 7 -- one ds_read_b128 per piece and block
  const int frow = lane & 31, fk = (lane >> 5) * 8;
  const __bf16* fa0 = smem + (wm * WTM + frow) * kLDK + fk;
  const __bf16* fb0 = smem + 3 * PA + (wn * WTN + frow) * kLDK + fk;

  gload();
  for (int step = 0; step < nsteps; ++step) {
    __syncthreads();                                              // every fragment read of the previous step is done
    lstore();
    __syncthreads();
    gload();                                                      // the next step's tile, in flight under this step's MFMAs
#pragma unroll
    for (int ks = 0; ks < kBK / 16; ++ks) {
      bf16x8 af[3][MI], bw[3][NI];
#pragma unroll
      for (int pc = 0; pc < 3; ++pc) {
#pragma unroll
        for (int i = 0; i < MI; ++i) af[pc][i] = *reinterpret_cast<const bf16x8*>(fa0 + pc * PA + i * 32 * kLDK + ks * 16);
#pragma unroll
        for (int j = 0; j < NI; ++j) bw[pc][j] = *reinterpret_cast<const bf16x8*>(fb0 + pc * PB + j * 32 * kLDK + ks * 16);
      }
      // Accumulators TRANSPOSED as in the fp32 kernel (weights are the row operand): a lane ends with 4 consecutive output
      // channels of one pixel in 4 consecutive registers and the epilogue moves float4.  Small terms first.
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) {
          floatx16 c = acc[i][j];
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bw[2][j], af[0][i], c, 0, 0, 0);   // lo . hi
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bw[0][j], af[2][i], c, 0, 0, 0);   // hi . lo
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bw[1][j], af[1][i], c, 0, 0, 0);   // mid . mid
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bw[1][j], af[0][i], c, 0, 0, 0);   // mid . hi
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bw[0][j], af[1][i], c, 0, 0, 0);   // hi . mid
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bw[0][j], af[0][i], c, 0, 0, 0);   // hi . hi
          acc[i][j] = c;
        }
    }
  }

  // ---- epilogue: acc reg r of lane l holds C[pixel row l & 31][channel (r & 3) + 8 (r >> 2) + 4 (l >> 5)] of the 32x32 block
  const int col = lane & 31, rhalf = (lane >> 5) * 4;
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int dst = rowdst[wm * WTM + i * 32 + col];
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int nl = wn * WTN + j * 32 + 8 * g4 + rhalf;
        const float4 v = make_float4(acc[i][j][4 * g4], acc[i][j][4 * g4 + 1], acc[i][j][4 * g4 + 2], acc[i][j][4 * g4 + 3]);
        if (dst >= 0 && n0 + nl < p.N) {
          const size_t idx = (size_t)dst * p.N + n0 + nl;
          *reinterpret_cast<float4*>(p.C + idx) = bg::apply_epilogue4(p, v, idx, &s_epi[0][nl], &s_epi[1][nl]);
        }
      }
  }
  if (stats_row) {
    // BatchNorm partials of the stored tile (mode NONE, no bias: stored == accumulated).  Rows past M and channels past N hold
    // exact zeros.  Fixed order: the wave's M blocks in registers, then a butterfly over the 32 pixel lanes, then the waves along M.
    float* red = reinterpret_cast<float*>(smem);                  // [WAVES_M][BN][2]
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float s = 0.f, q = 0.f;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
          s += acc[i][j][r];
          q = fmaf(acc[i][j][r], acc[i][j][r], q);
        }
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) {
          s += __shfl_xor(s, o, 64);
          q += __shfl_xor(q, o, 64);
        }
        if (col == 0) {
          const int nl = wn * WTN + j * 32 + (r & 3) + 8 * (r >> 2) + rhalf;
          red[(wm * BN + nl) * 2] = s;
          red[(wm * BN + nl) * 2 + 1] = q;
        }
      }
    __syncthreads();
    if (tid < BN && n0 + tid < p.N) {
      float a = 0.f, b = 0.f;
#pragma unroll
      for (int w = 0; w < WAVES_M; ++w) { a += red[(w * BN + tid) * 2]; b += red[(w * BN + tid) * 2 + 1]; }
      stats_row[n0 + tid] = a;
      stats_row[p.N + n0 + tid] = b;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
// The dispatch table: conv geometries (5 x 5 taps; H, W, Cin, Cout on the conv's input side as in the C ABI; bwd = data
// gradient / Conv2DTranspose forward) that run x6, for any batch.  Every entry measured faster than the fp32 kernel at
// B = 256 (tools/bench_conv.py --math bf16x6, profiles/r06_a_conv_math_bf16x6.md); a layer that measured level or slower stays
// on fp32 and is not listed.
struct X6Entry { int bwd, H, W, Cin, Cout, s; };
constexpr X6Entry kX6Table[] = {
    {0, 32, 32, 64, 128, 2},    // celeba64 / celeba128 G4: data gradient of the transposed conv   0.84 ... 0.89 of the fp32 time
    {0, 64, 64, 32, 64, 2},     // celeba64 / celeba128 G5: data gradient of the transposed conv   0.94 ... 0.998
};
// Measured and left out (x6 / fp32 time): G4's forward 0.96 ... 1.04 (slower with the step's epilogue), G5's forward 1.0 ... 1.14,
// G3 1.2 ... 1.25, D2 1.07 ... 1.19, D3 1.39 ... 1.81, MNIST D2 / G2 1.6 ... 2.1, the 4 x 4-map layers (not run: tap skipping).

bool x6_in_table(int bwd, int H, int W, int Cin, int Cout, int k, int s) {
  if (k != 5) return false;
  for (const X6Entry& e : kX6Table)
    if (e.bwd == bwd && e.H == H && e.W == W && e.Cin == Cin && e.Cout == Cout && e.s == s) return true;
  return false;
}

// what the kernel can run: 32-channel K steps, output channels in whole 32-column tiles, pixel-major tiles (the smallest maps
// -- 4 x 4 maps -- lose most of their taps to SAME padding: the fp32 kernel skips those per position-major tile; x6 does not)
bool x6_geometry_ok(const GatherParams& p) {
  if (p.Ck % kBK != 0 || p.N % 32 != 0) return false;
  int maxpos = 0;
  for (int i = 0; i < p.nphase; ++i) maxpos = std::max(maxpos, p.ph[i].Ha * p.ph[i].Wa);
  if (maxpos <= 16) return false;
  int ntap_w = 0;
  for (int i = 0; i < p.nphase; ++i)
    for (int t = 0; t < p.ph[i].ntaps; ++t) ntap_w = std::max(ntap_w, bg::tap_wi(p.ph[i].tap[t]) + 1);
  return (size_t)p.B * p.Hs * p.Ws * p.Ck * sizeof(float) < (1ull << 31) && (size_t)p.B * p.Hd * p.Wd * (size_t)p.N < (1ull << 31) &&
         (size_t)ntap_w * p.N * p.Ck * sizeof(float) < (1ull << 31);
}

bool make_params(GatherParams& p, int bwd, int B, int H, int W, int Cin, int Cout, int k, int s) {
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || k < 1 || !(k & 1) || k * k > bg::kMaxTaps || (s != 1 && s != 2)) return false;
  memset(&p, 0, sizeof p);
  if (bwd) bg::make_bwd_data_params(p, B, H, W, Cin, Cout, k, s);
  else bg::make_fwd_params(p, B, H, W, Cin, Cout, k, s);
  return true;
}

// BG_CONV_X6_FORCE=1 (tuning aid, tools/bench_conv.py --math bf16x6 --all): x6 for every geometry the kernel can run, table or not
bool x6_takes(const GatherParams& p, int bwd, int H, int W, int Cin, int Cout, int k, int s) {
  static const int force = getenv("BG_CONV_X6_FORCE") ? atoi(getenv("BG_CONV_X6_FORCE")) : 0;
  return x6_geometry_ok(p) && (force || x6_in_table(bwd, H, W, Cin, Cout, k, s));
}

template <int BM, int BN, int WMv, int WNv>
int launch_x6(GatherParams& p, const bg_epilogue* epi, void* stream, const char* name) {
  int Mmax = 0;
  for (int i = 0; i < p.nphase; ++i) Mmax = std::max(Mmax, p.B * p.ph[i].Ha * p.ph[i].Wa);
  p.mtiles = (int)bg::cdiv(Mmax, BM);
  const size_t srows = (size_t)p.nphase * p.mtiles;
  if (p.stats) *epi->stats_rows = (int)srows;
  double flops = 0, exec = 0;
  for (int i = 0; i < p.nphase; ++i) {
    const double kk = (double)p.Ck * p.ph[i].ntaps;
    flops += 2.0 * p.B * p.ph[i].Ha * p.ph[i].Wa * (double)p.N * kk;
    exec += 2.0 * (double)bg::cdiv((size_t)p.B * p.ph[i].Ha * p.ph[i].Wa, BM) * BM * (double)bg::cdiv(p.N, BN) * BN * kk;
  }
  int nw = 0;
  bool used[bg::kMaxTaps] = {false};
  for (int i = 0; i < p.nphase; ++i)
    for (int t = 0; t < p.ph[i].ntaps; ++t) {
      const int wi = bg::tap_wi(p.ph[i].tap[t]);
      if (!used[wi]) { used[wi] = true; ++nw; }
    }
  const double bytes = 4.0 * ((double)p.B * p.Hs * p.Ws * p.Ck + (double)nw * p.N * p.Ck + (double)p.B * p.Hd * p.Wd * p.N);
  // flops and executed flops are fp32-EQUIVALENT (one multiply-add per product): the six bf16 MFMAs per product are the
  // kernel's own business; roofline fractions of this mode are taken against the bf16 roof / 6 beside the fp32 roof
  bg::Launch L(stream, name, flops, bytes);
  if (L.prof) L.exec_flops(exec);
  const dim3 grid(p.mtiles * bg::cdiv(p.N, BN), 1, p.nphase);
  bg::launch((conv_igemm_x6_kernel<BM, BN, WMv, WNv>), grid, dim3(kNT), 0, L.s, p);
  return L.done(name);
}

// *taken = 0: the call is not for x6 (geometry, alignment or statistics capacity) and the caller runs the fp32 path
int try_conv_x6(int bwd, const float* a, const float* w, float* c, int B, int H, int W, int Cin, int Cout, int k, int s,
                const bg_epilogue* epi, void* stream, int* taken) {
  *taken = 0;
  GatherParams p;
  if (!make_params(p, bwd, B, H, W, Cin, Cout, k, s) || !x6_takes(p, bwd, H, W, Cin, Cout, k, s)) return BG_OK;
  p.A = a; p.Wt = w; p.C = c;
  p.epi_mode = BG_EPI_NONE; p.alpha = 0.3f; p.scale = 1.f;
  if (epi) {
    if (epi->mode < BG_EPI_NONE || epi->mode > BG_EPI_AFFINE_LRELU) return BG_OK;      // the fp32 path reports it
    if (epi->mode == BG_EPI_MUL_GRAD && !epi->ref) return BG_OK;
    if (epi->mode == BG_EPI_AFFINE_LRELU && !(epi->ref && epi->bias)) return BG_OK;
    p.epi_mode = epi->mode; p.bias = epi->bias; p.ref = epi->ref; p.keep = epi->keep; p.keep_elems = epi->keep_elems;
    p.alpha = epi->alpha; p.scale = epi->scale;
  }
  const auto al = [](const void* q, size_t n) { return (reinterpret_cast<uintptr_t>(q) & (n - 1)) == 0; };
  if (!(al(p.C, 16) && al(p.bias, 16) && ((p.epi_mode != BG_EPI_MUL_GRAD && p.epi_mode != BG_EPI_AFFINE_LRELU) || al(p.ref, 16)) &&
        al(p.keep, 4) && p.keep_elems % 4 == 0))
    return BG_OK;
  const int BN = p.N % 128 == 0 ? 128 : p.N % 64 == 0 ? 64 : 32;
  int Mmax = 0;
  for (int i = 0; i < p.nphase; ++i) Mmax = std::max(Mmax, p.B * p.ph[i].Ha * p.ph[i].Wa);
  const size_t srows = (size_t)p.nphase * bg::cdiv(Mmax, 128);
  p.stats = nullptr;
  if (epi && epi->stats) {
    if (!(epi->stats_rows && p.epi_mode == BG_EPI_NONE && !p.bias && epi->stats_capacity >= srows * 2 * (size_t)p.N)) return BG_OK;
    p.stats = epi->stats;
  }
  p.a_bytes = (unsigned)((size_t)p.B * p.Hs * p.Ws * p.Ck * sizeof(float));
  int ntap_w = 0;
  for (int i = 0; i < p.nphase; ++i)
    for (int t = 0; t < p.ph[i].ntaps; ++t) ntap_w = std::max(ntap_w, bg::tap_wi(p.ph[i].tap[t]) + 1);
  p.w_bytes = (unsigned)((size_t)ntap_w * p.N * p.Ck * sizeof(float));
  static const int no_swz = getenv("BG_NO_XCD_SWIZZLE") ? 1 : 0;
  p.xcd_swizzle = !no_swz;
  p.ksplit = 1;
  *taken = 1;
  char name[64];
  snprintf(name, sizeof name, "conv_igemm_x6_%s", bwd ? "dgrad" : "fwd");
  if (BN == 128) return launch_x6<128, 128, 2, 2>(p, epi, stream, name);
  if (BN == 64) return launch_x6<128, 64, 2, 2>(p, epi, stream, name);
  return launch_x6<128, 32, 4, 1>(p, epi, stream, name);
}

}  // namespace

extern "C" {

int bg_conv2d_math_taken(int bwd_data, int B, int H, int W, int Cin, int Cout, int ksize, int stride, int math) {
  if (math != BG_CONV_MATH_BF16X6) return 0;
  GatherParams p;
  if (!make_params(p, bwd_data ? 1 : 0, B, H, W, Cin, Cout, ksize, stride)) return 0;
  return x6_geometry_ok(p) && x6_in_table(bwd_data ? 1 : 0, H, W, Cin, Cout, ksize, stride) ? 1 : 0;
}

int bg_conv2d_fwd_math(const float* x, const float* wT_d, float* y, int B, int H, int W, int Cin, int Cout, int ksize, int stride,
                       const bg_epilogue* epi, void* stream, int math) {
  BG_REQUIRE(math == BG_CONV_MATH_FP32 || math == BG_CONV_MATH_BF16X6, BG_ERR_UNSUPPORTED, "bg_conv2d_fwd_math: math %d", math);
  if (math == BG_CONV_MATH_BF16X6 && x && wT_d && y && bg::aligned16(x) && bg::aligned16(wT_d) && bg::aligned16(y)) {
    if (epi && epi->stats_rows) *epi->stats_rows = 0;
    bg::UsefulScope useful(bg::conv_useful_flops(B, H, W, Cin, Cout, ksize, stride));
    int taken = 0;
    const int rc = try_conv_x6(0, x, wT_d, y, B, H, W, Cin, Cout, ksize, stride, epi, stream, &taken);
    if (rc || taken) return rc;
  }
  return bg_conv2d_fwd(x, wT_d, y, B, H, W, Cin, Cout, ksize, stride, epi, stream);
}

int bg_conv2d_bwd_data_math(const float* dy, const float* w_d, float* dx, int B, int H, int W, int Cin, int Cout, int ksize,
                            int stride, const bg_epilogue* epi, void* stream, int math) {
  BG_REQUIRE(math == BG_CONV_MATH_FP32 || math == BG_CONV_MATH_BF16X6, BG_ERR_UNSUPPORTED, "bg_conv2d_bwd_data_math: math %d", math);
  if (math == BG_CONV_MATH_BF16X6 && dy && w_d && dx && bg::aligned16(dy) && bg::aligned16(w_d) && bg::aligned16(dx)) {
    if (epi && epi->stats_rows) *epi->stats_rows = 0;
    bg::UsefulScope useful(bg::conv_useful_flops(B, H, W, Cin, Cout, ksize, stride));
    int taken = 0;
    const int rc = try_conv_x6(1, dy, w_d, dx, B, H, W, Cin, Cout, ksize, stride, epi, stream, &taken);
    if (rc || taken) return rc;
  }
  return bg_conv2d_bwd_data(dy, w_d, dx, B, H, W, Cin, Cout, ksize, stride, epi, stream);
}

}  // extern "C"
