// What does v_mfma_f32_32x32x16_bf16 do with an accumulator that is tiny beside its products?  The split-bf16 conv kernel
// (csrc/conv_igemm_x6.hip) stores zero mid / lo pieces as +-2^-126, so on integer data the accumulator that enters the hi.hi MFMA
// of a k-slice is a residue of a few 2^-126 whenever the sum so far is 0.  One wave runs the kernel's six-MFMA chain on 40 000
// random k-slices of integers in [-3, 3] (accumulator 0 or an integer in [-20, 20]) and prints the chains whose result is not the
// exact integer.  MI355X, 2026-10-19: 329 of 40 000; the twelve it prints each have a NEGATIVE residue entering hi.hi and a result exactly 2^-22
// below the integer (2^-25 of 8, the power of two of the largest product): the residue is aligned to the largest product and
// floored, not dropped.  A positive residue, and a tiny PRODUCT of either sign beside large ones, are dropped (exact result).
// tests/x6_cases.py adder_unit is the bound the exact x6 tests draw from this.
//   hipcc --offload-arch=gfx950 -O2 tools/probes/mfma_tiny_accumulator.hip -o /tmp/mfma_tiny_accumulator && /tmp/mfma_tiny_accumulator
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <vector>
#include <cmath>
#include <random>
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
// P: [test][operand a/b][piece 3][16] bf16 ; out [test][6]
__global__ void probe(const unsigned short* P, const float* C, float* out, int nt) {
  const int lane = threadIdx.x;
  for (int t = 0; t < nt; ++t) {
    bf16x8 a[3], b[3];
    for (int pc = 0; pc < 3; ++pc)
      for (int i = 0; i < 8; ++i) {
        a[pc][i] = __builtin_bit_cast(__bf16, P[((t * 2 + 0) * 3 + pc) * 16 + 8 * (lane >> 5) + i]);
        b[pc][i] = __builtin_bit_cast(__bf16, P[((t * 2 + 1) * 3 + pc) * 16 + 8 * (lane >> 5) + i]);
      }
    floatx16 c;
    for (int r = 0; r < 16; ++r) c[r] = C[t];
    const int ia[6] = {0, 2, 1, 0, 1, 0}, ib[6] = {2, 0, 1, 1, 0, 0};      // (activation piece, weight piece) in issue order
    for (int s = 0; s < 6; ++s) {
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b[ib[s]], a[ia[s]], c, 0, 0, 0);
      if (lane == 0) out[t * 6 + s] = c[0];
    }
  }
}
static unsigned short bf(float x) { unsigned u; memcpy(&u, &x, 4); return (unsigned short)(u >> 16); }
int main(int argc, char** argv) {
  const int nt = 40000;
  const float tiny = ldexpf(1.f, -126);
  std::mt19937 rng(7);
  std::vector<unsigned short> P((size_t)nt * 96);
  std::vector<float> C(nt), out((size_t)nt * 6, -777.f), xa((size_t)nt * 16), xb((size_t)nt * 16);
  for (int t = 0; t < nt; ++t) {
    C[t] = (float)((int)(rng() % 41) - 20);
    if (t % 4 == 0) C[t] = 0.f;
    for (int k = 0; k < 16; ++k)
      for (int o = 0; o < 2; ++o) {
        float x = (float)((int)(rng() % 7) - 3);
        (o ? xb : xa)[(size_t)t * 16 + k] = x;
        const float sg = std::signbit(x) ? -1.f : 1.f;
        P[((t * 2 + o) * 3 + 0) * 16 + k] = bf(x);
        P[((t * 2 + o) * 3 + 1) * 16 + k] = bf(sg * tiny);
        P[((t * 2 + o) * 3 + 2) * 16 + k] = bf(sg * tiny);
      }
  }
  unsigned short* dP; float *dC, *dO;
  if (hipMalloc(&dP, P.size() * 2) || hipMalloc(&dC, nt * 4) || hipMalloc(&dO, out.size() * 4)) return 2;
  (void)hipMemcpy(dP, P.data(), P.size() * 2, hipMemcpyHostToDevice);
  (void)hipMemcpy(dC, C.data(), nt * 4, hipMemcpyHostToDevice);
  hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, dP, dC, dO, nt);
  if (hipDeviceSynchronize() != hipSuccess) { printf("kernel failed\n"); return 3; }
  (void)hipMemcpy(out.data(), dO, out.size() * 4, hipMemcpyDeviceToHost);
  int bad = 0, badzero = 0;
  for (int t = 0; t < nt; ++t) {
    double dot = 0;
    for (int k = 0; k < 16; ++k) dot += (double)xa[(size_t)t * 16 + k] * xb[(size_t)t * 16 + k];
    const double want = C[t] + dot;
    const float got = out[(size_t)t * 6 + 5];
    const bool wrong = want != 0 ? (double)got != want : fabs(got) > 1e-30;
    if (wrong) {
      if (++bad <= 12) {
        printf("test %d: c=%g want %g got %.9g (diff %.3g); after each MFMA:", t, C[t], want, got, got - want);
        for (int s = 0; s < 6; ++s) printf(" %.9g", out[(size_t)t * 6 + s]);
        printf("\n   a:");
        for (int k = 0; k < 16; ++k) printf(" %g", xa[(size_t)t * 16 + k]);
        printf("\n   b:");
        for (int k = 0; k < 16; ++k) printf(" %g", xb[(size_t)t * 16 + k]);
        printf("\n");
      }
      badzero += want == 0;
    }
  }
  printf("%d of %d chains wrong (%d of them with an exact result of 0)\n", bad, nt, badzero);
  return 0;
}
