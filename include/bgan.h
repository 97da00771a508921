/*
 * bgan.h -- C ABI of libbgan_hip.so: the MI355X (gfx950) kernels behind blurred-GAN's
 * WGAN-GP training step.
 *
 * The reference (lebrice/blurred-GAN) has no FFI seam of its own: its hot path is Python that
 * calls TensorFlow ops.  This header is the seam the build introduces: one
 * extern "C" entry point per TF op family the reference's step invokes, each citing the
 * reference call site it replaces.  Conventions:
 *
 *   - every pointer named *_d / typed `const float*` etc. is a raw DEVICE address (HBM); the caller
 *     (Python via torch.Tensor.data_ptr()) owns every buffer including workspaces; the library
 *     keeps no device memory between calls;
 *   - tensors are dense NHWC float32; Conv2D kernels are [kh,kw,Cin,Cout], Conv2DTranspose kernels
 *     [kh,kw,Cout,Cin], Dense kernels [in,out] -- exactly as TF/Keras stores them;
 *   - `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream); launches are
 *     asynchronous, nothing synchronises the device;
 *   - every function returns 0 on success or a negative bg_status; bg_last_error() gives the
 *     thread-local message; nothing aborts or throws across the boundary.
 */
#ifndef BGAN_H
#define BGAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BG_ABI_VERSION 5

typedef enum {
  BG_OK = 0,
  BG_ERR_BAD_SHAPE = -1,      /* non-positive / inconsistent dimensions                       */
  BG_ERR_BAD_ALIGNMENT = -2,  /* pointer not aligned as the kernel requires (16 B)             */
  BG_ERR_UNSUPPORTED = -3,    /* valid request this build has no kernel for                    */
  BG_ERR_HIP = -4,            /* a HIP runtime call failed (message has hipGetErrorString)     */
  BG_ERR_WORKSPACE = -5,      /* workspace missing or too small (see *_workspace_bytes)        */
  BG_ERR_NULL = -6,           /* required pointer is NULL                                      */
  BG_ERR_RCCL = -7            /* RCCL missing or a collective call failed (message has the RCCL string) */
} bg_status;

/* ---- meta ------------------------------------------------------------------------------- */
int bg_version(void);
const char* bg_last_error(void);
const char* bg_status_string(int status);

/* ---- profiling hooks (bench.py roofline: per-kernel HIP-event timing on the launch stream) */
int bg_prof_enable(int on);                       /* record an event pair around every launch */
int bg_prof_reset(void);
int bg_prof_count(void);                          /* synchronises the recorded events          */
int bg_prof_get(int i, char* name, int name_cap, float* ms, double* flops, double* bytes);
/* flops record i ISSUED on the matrix pipe: whole MFMA tiles (row / column padding counted), minus the padding taps the
   position-major tiles skip.  Equals the algorithmic figure of bg_prof_get for kernels that do not report their own. */
int bg_prof_get_exec(int i, double* exec_flops);
/* flops of record i that multiply REAL data: SURVEY 8d's F_l (bg_prof_get) charges all 25 taps at every output position of a
   SAME convolution (demo_celeba.py:62,99); the taps that land on the zero padding -- 51 % of them on a 4x4 map, 28 % on 8x8 --
   are work no implementation has to do.  "useful" counts exactly the (output pixel, tap) pairs inside the image, with no tile
   padding either, so  useful <= executed-or-algorithmic  and a rate priced by it cannot read above the roof.  Equals the
   algorithmic figure for launches that are not convolutions.  bg_conv2d_useful_flops is the closed form (conv input side
   H x W x Cin; one count serves the forward, the data gradient / transposed convolution and the filter gradient). */
int bg_prof_get_useful(int i, double* useful_flops);
double bg_conv2d_useful_flops(int B, int H, int W, int Cin, int Cout, int ksize, int stride);

/* Named ranges on the profiler timeline (rocprofv3 --marker-trace): D-step / G-step / blur / all-reduce of one train_on_batch
   (wgan.py:86-114).  roctx (librocprofiler-sdk-roctx.so) is bound with dlopen on first use; without it, or with
   bg_range_enable(0) (the default), both calls return immediately.  bg_range_enable returns 1 when ranges will be emitted. */
int bg_range_enable(int on);
int bg_range_push(const char* name);
int bg_range_pop(void);

/* ---- Gaussian blur: gaussian_blur.py:15-132 ---------------------------------------------- */
/* gaussian_blur.py:21-31,58-72 (appropriate_kernel_size, appropriate_std, clip, max): host maths, float32. */
int bg_blur_policy(float sigma, int H, int W, float* kernel_size, float* sigma_eff, int* n_taps);
/* gaussian_blur.py:83-88 (gaussian_kernel_1d): writes n_taps float32 weights to HOST memory. */
int bg_gauss_kernel_1d(float sigma_eff, float kernel_size, float* taps_host, int cap, int* n_taps);
/* gaussian_blur.py:91-132 (two tf.nn.depthwise_conv2d, SAME, zero padding): y = blur(x), NHWC.
 * taps_d: n_taps device floats.  tmp_d: scratch of the same size as x (may be NULL when the whole
 * image fits the fused kernel, see bg_blur_workspace_bytes).  The op is self-adjoint, so the same
 * call is its own backward. */
size_t bg_blur_workspace_bytes(int B, int H, int W, int C, int n_taps);
int bg_blur_nhwc_f32(const float* x, float* y, int B, int H, int W, int C,
                     const float* taps_d, int n_taps, float* tmp_d, void* stream);

/* The critic's batch of one discriminator_step in ONE launch (wgan.py:138-139 fakes and reals, wgan.py:239-240 x-hat):
 *   y3[0:B] = blur(f), y3[B:2B] = blur(r), y3[2B:3B] = blur(r + alpha[b] * (f - r))
 * x-hat is formed while its rows are staged (the expression of bg_lerp_f32: bit-identical to bg_lerp_f32 followed by bg_blur_nhwc_f32)
 * and never written to memory.  Only geometries of the row-block kernel (images up to 64 x 64, <= 4 channels, >= 13 taps;
 * bg_blur3_lerp_supported tells) -- anything else returns BG_ERR_UNSUPPORTED and the caller runs the three separate calls. */
int bg_blur3_lerp_supported(int B, int H, int W, int C, int n_taps);
int bg_blur3_lerp_nhwc_f32(const float* f, const float* r, const float* alpha_b, float* y3, int B, int H, int W, int C,
                           const float* taps_d, int n_taps, void* stream);

/* ---- convolution family: layers.Conv2D / Conv2DTranspose (demo_celeba.py:62-119,
 *      demo_mnist.py:60-81) and their tape gradients (wgan.py:140,166,244) -------------------
 * Geometry is TF 'SAME' for a kxk kernel (k odd, k*k <= 25), stride 1 or 2:
 *   Ho = ceil(H/s), pad_total = max((Ho-1)s + k - H, 0), pad_before = pad_total/2.
 * H, W, Cin always describe the conv's INPUT side, Ho/Wo/Cout its OUTPUT side, also for the
 * backward calls.  A Conv2DTranspose with kernel [k,k,Cout_t,Cin_t] is the data-gradient of the
 * conv whose kernel is that same array read as [k,k,Cin=Cout_t,Cout=Cin_t]; call bg_conv2d_bwd_data
 * for its forward, bg_conv2d_fwd for its data-gradient, bg_conv2d_bwd_filter(x := dy_t, dy := x_t)
 * for its filter-gradient.
 *
 * Weight operand layout expected by the MFMA kernels is "NK": [tap][n][k] with the contraction
 * index k contiguous.  For bg_conv2d_bwd_data that IS the TF layout [kh,kw,Cin,Cout]; for
 * bg_conv2d_fwd it is the last-two-dims transpose [kh,kw,Cout,Cin] (bg_transpose_last2 makes it).
 */
typedef enum {
  BG_EPI_NONE = 0,        /* y = acc (+ bias)                                                   */
  BG_EPI_BIAS_LRELU = 1,  /* y = lrelu(acc + bias); then y *= keep ? scale : 0 when keep != NULL */
  BG_EPI_MUL_GRAD = 2,    /* y = acc * (ref > 0 ? 1 : alpha) [* keep ? scale : 0].  `ref` MAY ALIAS the output (the penalty's
                           * linearised forward overwrites the activations whose signs it consumes): every kernel reads
                           * ref[i] in the thread that stores y[i], before that store                      */
  BG_EPI_TANH = 3,        /* y = tanh(acc + bias)                                               */
  BG_EPI_AFFINE_LRELU = 4 /* y = lrelu(acc * ref[c] + bias[c]): inference BatchNormalization folded (bg_bn_fold_f32), ref = per-channel scale */
} bg_epi_mode;

typedef struct {
  int mode;               /* bg_epi_mode                                                        */
  const float* bias;      /* [Cout] or NULL                                                     */
  const float* ref;       /* BG_EPI_MUL_GRAD: activation whose sign selects 1 / alpha, same shape as y */
  const uint8_t* keep;    /* dropout keep mask (1 = kept), same shape as y, or NULL             */
  float alpha;            /* LeakyReLU slope (Keras default 0.3)                                */
  float scale;            /* 1 / keep_prob                                                      */
  void* splitk_ws;        /* optional scratch for split-K partial sums (small-M layers); NULL = never split */
  size_t splitk_ws_bytes; /* >= bg_conv2d_splitk_workspace_bytes(...) for the call to use split-K      */
  size_t keep_elems;      /* the keep mask covers output elements [0, keep_elems) only (a batch whose leading samples ran with
                           * Dropout and whose trailing samples without: fake+real and x-hat of wgan.py:138,240 in one pass);
                           * 0 = every element */
  float* stats;           /* optional (mode BG_EPI_NONE, no bias): the MFMA gather kernel also leaves per-workgroup column sums and
                           * sums of squares of what it stores -- partial[row][2][Cout] -- so that the BatchNormalization that
                           * follows (demo_celeba.py:62-90) needs no statistics pass over the tensor; `*stats_rows` tells how many
                           * rows THIS call wrote (0: this geometry took another kernel, run the normal pass) */
  size_t stats_capacity;  /* floats available behind `stats` */
  int* stats_rows;        /* HOST pointer, out (required when `stats` is set): rows of `stats` this call wrote.  Returned through
                           * the call itself -- ABI 2 kept it in per-thread last-call state (bg_conv2d_stats_rows, removed in 3) */
} bg_epilogue;

/* bytes of split-K scratch the forward (bwd_data = 0) / data-gradient (bwd_data = 1) call can use; 0 = never splits */
size_t bg_conv2d_splitk_workspace_bytes(int bwd_data, int B, int H, int W, int Cin, int Cout, int ksize, int stride);
/* Alignment: x / w / y (dy / w / dx) must be 16-byte aligned (BG_ERR_BAD_ALIGNMENT otherwise).  The epilogue's operands may sit
 * anywhere, but the matrix-core kernels read them four at a time: they are taken when bias / ref / the split-K scratch are
 * 16-byte aligned, the mask 4-byte aligned with keep_elems % 4 == 0, and the output channel count a multiple of 4 -- what a
 * framework allocator hands out; anything else runs on the direct kernel (same results, slower). */
/* y[B,Ho,Wo,Cout] = conv(x[B,H,W,Cin], w) ; wT_d = [k*k][Cout][Cin] */
int bg_conv2d_fwd(const float* x, const float* wT_d, float* y, int B, int H, int W, int Cin, int Cout,
                  int ksize, int stride, const bg_epilogue* epi, void* stream);
/* dx[B,H,W,Cin] = conv^T(dy[B,Ho,Wo,Cout], w) ; w_d = [k*k][Cin][Cout] (TF Conv2D layout) */
int bg_conv2d_bwd_data(const float* dy, const float* w_d, float* dx, int B, int H, int W, int Cin, int Cout,
                       int ksize, int stride, const bg_epilogue* epi, void* stream);
/* Conv math modes of the forward and data gradient (bg_conv2d_fwd_math / bg_conv2d_bwd_data_math).
 *   BG_CONV_MATH_FP32    exactly bg_conv2d_fwd / bg_conv2d_bwd_data: fp32 operands on the fp32 matrix pipe.
 *   BG_CONV_MATH_BF16X6  opt-in split-bf16 math: every fp32 operand element is split exactly into three bf16 pieces
 *                        (hi = top 16 bits, mid = top 16 bits of x - hi, lo = round-to-nearest of the rest) and a product is
 *                        rebuilt from the six cross terms hi.hi, hi.mid, mid.hi, hi.lo, lo.hi, mid.mid on the bf16 matrix pipe,
 *                        accumulated in fp32.  Accuracy contract: the terms left out are below 2^-24 of each product, so the
 *                        error against an exact result is of the order of the fp32 path's (fp32 accumulation order dominates
 *                        both) and within the same bounds; results are NOT bit-identical to BG_CONV_MATH_FP32, but are
 *                        bit-reproducible from run to run (fixed summation order, no atomics).  Inf / NaN inputs give the same
 *                        Inf / NaN outputs as the fp32 path.  Only the geometries of a static table (measured faster) run the
 *                        split kernel -- bg_conv2d_math_taken says which; every other call, and every call whose epilogue or
 *                        statistics buffer the split kernel does not take, runs the fp32 path unchanged. */
typedef enum { BG_CONV_MATH_FP32 = 0, BG_CONV_MATH_BF16X6 = 1 } bg_conv_math;
/* the same calls with a math mode; BG_ERR_UNSUPPORTED for an unknown mode */
int bg_conv2d_fwd_math(const float* x, const float* wT_d, float* y, int B, int H, int W, int Cin, int Cout,
                       int ksize, int stride, const bg_epilogue* epi, void* stream, int math);
int bg_conv2d_bwd_data_math(const float* dy, const float* w_d, float* dx, int B, int H, int W, int Cin, int Cout,
                            int ksize, int stride, const bg_epilogue* epi, void* stream, int math);
/* pure host query: 1 when the call of that geometry in mode `math` runs the split-bf16 kernel (0 for BG_CONV_MATH_FP32) */
int bg_conv2d_math_taken(int bwd_data, int B, int H, int W, int Cin, int Cout, int ksize, int stride, int math);
/* dw[k,k,Cin,Cout] = beta*dw + scale * sum_pixels x (x) dy.  ws_d: bg_conv2d_bwd_filter_workspace_bytes */
size_t bg_conv2d_bwd_filter_workspace_bytes(int B, int H, int W, int Cin, int Cout, int ksize, int stride);
int bg_conv2d_bwd_filter(const float* x, const float* dy, float* dw, int B, int H, int W, int Cin, int Cout,
                         int ksize, int stride, float beta, float scale, void* ws_d, size_t ws_bytes, void* stream);
/* dst[t][c][r] = src[t][r][c] */
int bg_transpose_last2(const float* src, float* dst, int T, int R, int C, void* stream);
/* The same for every conv kernel of a network in one launch (after each optimiser step: layers.ParamStore.refresh_transposed).
 * desc_d: n x 6 int32 on the device {src_off, dst_off, T, R, C, first_tile}: float offsets from the two bases (multiples of 4),
 * 64x64 tiles numbered from first_tile in [t][ceil(R/64)][ceil(C/64)] order, first_tile ascending; total_tiles = their sum. */
int bg_transpose_last2_batched(const float* src_base, float* dst_base, const int* desc_d, int n, int total_tiles, void* stream);

/* ---- Dense (demo_celeba.py:55,124): row-major C[M,N] = op(A)[M,K] * op(B)[K,N] (+ bias[N]) --- */
int bg_gemm_f32(const float* A, const float* Bm, float* C, int M, int N, int K, int transA, int transB,
                const float* bias, float beta, float scale, void* stream);

/* ---- reductions: column sums of a row-major [M,N] matrix (bias grads, BN statistics, JVP tail) */
size_t bg_colsum_workspace_bytes(int M, int N);
/* out[n] = beta*out[n] + scale * sum_m f(x[m,n]) ; square != 0 sums x^2 */
int bg_colsum_f32(const float* x, float* out, int M, int N, int square, float beta, float scale,
                  void* ws_d, size_t ws_bytes, void* stream);

/* ---- BatchNormalization + LeakyReLU (demo_celeba.py:56-90), x viewed as [M, C] --------------- */
/* training forward: batch mean / biased var -> y = lrelu(gamma*(x-mean)*inv + beta); saves mean, inv;
 * moving stats <- moving*momentum + stat*(1-momentum), var scaled by M/(M-1) when unbiased != 0. */
size_t bg_bn_workspace_bytes(int M, int C);
int bg_bn_train_fwd(const float* x, float* y, int M, int C, const float* gamma, const float* beta,
                    float* moving_mean, float* moving_var, float* save_mean, float* save_inv,
                    float eps, float momentum, int unbiased, float lrelu_alpha,
                    void* ws_d, size_t ws_bytes, void* stream);
/* inference forward with moving stats (generator inside the D-step, wgan.py:135). */
int bg_bn_infer_fwd(const float* x, float* y, int M, int C, const float* gamma, const float* beta,
                    const float* moving_mean, const float* moving_var, float eps, float lrelu_alpha, void* stream);
/* backward through lrelu + training BN: dy is the gradient w.r.t. y (post-lrelu), y the saved output.
 * y may be NULL (here and in bg_bn_bwd_stats_f32 / bg_bn_bwd_apply_f32) when beta is given and lrelu_alpha >= 0: the sign of y is
 * then re-derived from x with the forward's own expression gamma * ((x - mean) * inv) + beta -- the same operations on the same
 * inputs, so the result is bit-identical -- and each pass reads one tensor less. */
int bg_bn_train_bwd(const float* dy, const float* y, const float* x, float* dx, int M, int C,
                    const float* gamma, const float* beta, const float* save_mean, const float* save_inv,
                    float* dgamma, float* dbeta, float lrelu_alpha, void* ws_d, size_t ws_bytes, void* stream);

/* inference BatchNormalization as a per-channel affine: scale = gamma / sqrt(moving_var + eps), shift = beta - moving_mean * scale
 * (feeds BG_EPI_AFFINE_LRELU so the generator's inference forward inside the D-step, wgan.py:135, needs no separate BN pass) */
int bg_bn_fold_f32(const float* gamma, const float* beta, const float* moving_mean, const float* moving_var, float eps, int C,
                   float* scale_out, float* shift_out, void* stream);
/* the same for n <= 8 layers in ONE launch (HOST arrays of n device pointers / values; same arithmetic per channel): every
 * BatchNorm of the generator's inference forward is folded before its first conv */
int bg_bn_fold_many_f32(int n, const float* const* gamma, const float* const* beta, const float* const* moving_mean,
                        const float* const* moving_var, const float* eps, const int* C, float* const* scale_out,
                        float* const* shift_out, void* stream);
/* The same BatchNormalization in separable pieces, for data-parallel SyncBN: the per-channel sums are
 * all-reduced by the caller between the pieces.  sums_d = [2*C]: forward {sum x, sum x^2}; backward {sum dz, sum dz*xhat}
 * with dz = dy * lrelu'(y).  M_total = rows summed over all replicas. */
int bg_bn_stats_f32(const float* x, int M, int C, float* sums_d, void* ws_d, size_t ws_bytes, void* stream);
int bg_bn_finalize_f32(const float* sums_d, int M_total, int C, float* save_mean, float* save_inv, float* moving_mean,
                       float* moving_var, float eps, float momentum, int unbiased, void* stream);
int bg_bn_apply_f32(const float* x, float* y, int M, int C, const float* gamma, const float* beta, const float* mean,
                    const float* inv, float lrelu_alpha, void* stream);
/* bg_bn_finalize_f32 + bg_bn_apply_f32 in ONE launch (same arithmetic, bit-identical y / saved / moving statistics): behind a conv
 * that left its statistics in the epilogue (bg_epilogue.stats) the SyncBN forward chain is bg_bn_sums_from_partials -> all-reduce
 * -> this, two launches per layer beside the exchange. */
int bg_bn_finalize_apply_f32(const float* sums_d, int M_total, const float* x, float* y, int M, int C, const float* gamma,
                             const float* beta, float* save_mean, float* save_inv, float* moving_mean, float* moving_var, float eps,
                             float momentum, int unbiased, float lrelu_alpha, void* stream);
/* training-mode BatchNormalization + LeakyReLU from statistics PARTIALS partial[nrows][2][C] (column sums, sums of squares) left
   by the producing conv (bg_epilogue.stats): finalize (+ moving statistics) and apply, no statistics pass over x */
int bg_bn_train_fwd_partials(const float* partial_d, int nrows, const float* x, float* y, int M, int C, const float* gamma,
                             const float* beta, float* moving_mean, float* moving_var, float* save_mean, float* save_inv, float eps,
                             float momentum, int unbiased, float lrelu_alpha, void* stream);
/* sums[0:C] = column sums, sums[C:2C] = sums of squares out of the same partials (SyncBN: what gets all-reduced) */
int bg_bn_sums_from_partials(const float* partial_d, int nrows, int C, float* sums_d, void* stream);
int bg_bn_bwd_stats_f32(const float* dy, const float* y, const float* x, int M, int C, const float* gamma, const float* beta,
                        const float* save_mean, const float* save_inv, float lrelu_alpha, float* sums_d, void* ws_d, size_t ws_bytes,
                        void* stream);
int bg_bn_bwd_apply_f32(const float* dy, const float* y, const float* x, float* dx, int M, int M_total, int C, const float* gamma,
                        const float* beta, const float* save_mean, const float* save_inv, const float* sums_d, float lrelu_alpha,
                        void* stream);
/* dbeta[c] = scale * sums[c], dgamma[c] = scale * sums[C + c]: gamma / beta gradients out of the all-reduced backward sums
   (scale = 1 / replicas, so that the SUM all-reduce of the flat gradient buffer restores the global value) */
int bg_bn_param_grads_f32(const float* sums_d, int C, float scale, float* dgamma, float* dbeta, void* stream);

/* ---- layer normalisation: tf.keras.layers.LayerNormalization(axis=-1) + LeakyReLU (+ Dropout) over NHWC fp32 maps ------------
 * Data is [R, C]: R = B*H*W rows of C contiguous channels.  Per row, with every mean taken over the row's C channels:
 *   mu = mean(z),  r = 1 / sqrt(mean((z - mu)^2) + eps)   (saved by the forward, [R] floats each),   xh = (z - mu) * r,
 *   M y = r * (yc - xh * mean(yc * xh)),  yc = y - mean(y)   (the Jacobian of z -> xh; symmetric).
 * LeakyReLU's branch is never read from the activation: every call re-derives n = gamma * xh + beta from z with the forward's own
 * expression (the same operations on the same inputs: the same bits), which needs lrelu_alpha >= 0 (BG_ERR_UNSUPPORTED otherwise).
 * keep / keep_scale / keep_elems follow bg_epilogue: the uint8 mask covers the first keep_elems elements (0 = all of them; a whole
 * number of rows), a masked element is multiplied by keep ? keep_scale : 0.
 * C % 4 == 0 moves float4s and wants z, a, g, dz, zdot, vout, u, s, addend, u_out, keep, gamma and beta 16-byte aligned
 * (BG_ERR_BAD_ALIGNMENT otherwise); any other C goes one float at a time.  bg_ln_route tells how a C is laid over a wave: floats
 * per unit (4 or 1), lanes that share a row (64 / lanes rows per wave, four waves per workgroup), units a lane keeps in registers,
 * and the chunks a row is swept in when it exceeds what one wave holds (1: the row is read once).  A refused call launches
 * nothing.  Column sums are reduced through per-workgroup partials in the workspace and a fixed-order finish: no floating-point
 * atomics, the same bits on every run.  No call takes a step-program binding. */
int bg_ln_route(int C, int* vec, int* lanes, int* regs, int* chunks);
size_t bg_ln_workspace_bytes(int R, int C);
/* a = Dropout(LeakyReLU(gamma * xh + beta)); writes mu, r.  a must not alias z. */
int bg_ln_fwd_f32(const float* z, float* a, int R, int C, const float* gamma, const float* beta, float eps, float lrelu_alpha,
                  const uint8_t* keep /* may be NULL */, float keep_scale, size_t keep_elems, float* mu, float* r, void* stream);
/* g: the gradient at a.  u = g * LeakyReLU' * Dropout' (the gradient at n),  dz = M(gamma * u) [+ addend].
 * u_out (may be NULL): u of rows [u_row0, u_row0 + u_rows), stored from its own row 0 (the penalty keeps the x-hat rows' u).
 * dgamma / dbeta (both or neither; NULL: the generator step's form, no sums and no workspace):
 *   dgamma = acc_beta * dgamma + acc_scale * sum_rows u * xh,  dbeta = acc_beta * dbeta + acc_scale * sum_rows u
 * over rows [0, dw_rows) (dw_rows <= 0: all of them).  dz may alias g (or addend) where bg_ln_route gives chunks == 1. */
int bg_ln_bwd_f32(const float* g, const float* z, float* dz, int R, int C, const float* gamma, const float* beta, const float* mu,
                  const float* r, float lrelu_alpha, const uint8_t* keep, float keep_scale, size_t keep_elems,
                  const float* addend /* may be NULL */, float* u_out, int u_row0, int u_rows, float* dgamma, float* dbeta, int dw_rows,
                  float acc_beta, float acc_scale, void* ws_d, size_t ws_bytes, void* stream);
/* the penalty's tangent through the stage (no Dropout on the x-hat rows):  vout = LeakyReLU' * gamma * M(zdot).  The same kernel
 * as the backward.  vout may alias zdot where bg_ln_route gives chunks == 1. */
int bg_ln_tangent_f32(const float* zdot, const float* z, float* vout, int R, int C, const float* gamma, const float* beta,
                      const float* mu, const float* r, float lrelu_alpha, void* stream);
/* the penalty's second-order source.  u: the first-order gradient at n on the x-hat rows, zdot: the tangent at z.  The term
 * T = <u, gamma * M(zdot)> of the linearised forward depends on z through xh and r, and on gamma directly:
 *   dT/dgamma = sum_rows u * M(zdot)                          -> dgamma = acc_beta * dgamma + acc_scale * that
 *   dT/dz = s = -r^2 * (p * Bq + q * A + xh * (D - 3 * A * Bq))
 *   with  p = gamma * u - mean(gamma * u),  q = zdot - mean(zdot),  A = mean(p * xh),  Bq = mean(q * xh),  D = mean(p * q).
 * (dT/dzdot = M(gamma * u) is the dz bg_ln_bwd_f32 left behind.)  s must not alias an input. */
int bg_ln_gp_source_f32(const float* u, const float* zdot, const float* z, float* s, int R, int C, const float* gamma, const float* mu,
                        const float* r, float* dgamma, float acc_beta, float acc_scale, void* ws_d, size_t ws_bytes, void* stream);

/* ---- pixel normalisation (Karras et al. 2018; layers.PixelNormalization) + the LeakyReLU in front of it, fp32 -----------------
 * Data is [R, C]: R rows (the pixels of NHWC maps, or latent vectors) of C contiguous channels.  Per row, means over its C channels:
 *   a = x > 0 ? x : lrelu_alpha * x   (lrelu_alpha = 1: the identity),   r = 1 / sqrt(mean(a^2) + eps),   y = a * r.
 * The Jacobian of a -> y is r * (I - y y^T / C), and r > 0 gives sign(y) = sign(x), so the backward runs through the normalisation
 * and the LeakyReLU in one pass from the stored output, r and the incoming gradient g alone (x is never re-read):
 *   dz = (y > 0 ? 1 : lrelu_alpha) * r * (g - y * mean(g * y))          (the comparison is bg_mul_grad_f32's).
 * No parameters, no workspace, no atomics: a row's sum is taken in a fixed order, the same bits on every run.
 * Any R, C >= 1.  Pointers 4-byte aligned (BG_ERR_BAD_ALIGNMENT).  A call moves float4s where C % 4 == 0 and x, y, g, dz are all
 * 16-byte aligned, single floats otherwise; no call is refused for a misaligned view.  bg_pixelnorm_route (host only):
 * out[BG_PIXELNORM_ROUTE_INTS] = {floats per unit (4 or 1), lanes that share a row (64 / lanes rows per wave, four waves per
 * workgroup), units a lane keeps in registers, chunks a row is swept in when it exceeds what one wave holds (1: read once)} of a
 * call whose matrices are all 16-byte aligned, then the same four of a call with a misaligned one.  A refused call launches
 * nothing.  No call takes a step-program binding. */
#define BG_PIXELNORM_ROUTE_INTS 8
int bg_pixelnorm_route(int C, int* out);
/* y = a * r; r ([R] floats, kept for the backward) may be NULL: nothing is kept (latents, passes without a backward).  y may alias
 * x where the call's route has chunks == 1 (BG_ERR_UNSUPPORTED otherwise). */
int bg_pixelnorm_fwd_f32(const float* x, float* y, float* r /* may be NULL */, int R, int C, float eps, float lrelu_alpha, void* stream);
/* dz as above.  dz may alias g where the call's route has chunks == 1; it must not alias y (BG_ERR_UNSUPPORTED). */
int bg_pixelnorm_bwd_f32(const float* g, const float* y, const float* r, float* dz, int R, int C, float lrelu_alpha, void* stream);

/* ---- noise inputs (Karras et al. 2019 / 2020; layers.NoiseInjection) + the LeakyReLU behind them, fp32 ------------------------
 * What a StyleGAN2 synthesis layer does between its convolution and its activation: it draws one N(0, 1) value per pixel of the
 * map, multiplies it by ONE learned scalar, the layer's noise strength (initialised to zero), adds the product to every channel of
 * that pixel, and then applies the bias / LeakyReLU.  Data is [R, C]: R = B * H * W rows (pixels of NHWC maps) of C contiguous
 * channels; noise is [R]; strength is one float in DEVICE memory (a trainable variable; a replayed step program sees its current
 * value).
 *   forward   t_r = strength[0] * noise[r] (rounded to fp32 once),  y[r, c] = a > 0 ? a : lrelu_alpha * a  with a = x[r, c] + t_r
 *             (lrelu_alpha = 1: no activation).  y may alias x.  No LDS.
 *   gradient  dstrength[0] = beta * old + scale * sum_r noise[r] * (sum_c dz[r, c])   (beta = 0: old is not read), dz the
 *             gradient at a.  Deterministic: a row's channel sum, a workgroup's sum and the finish run in a fixed order, no
 *             atomics, two launches, dz read once.  ws: bg_noise_grad_workspace_bytes(R, C) bytes of device scratch.
 * Any R, C >= 1.  Pointers 4-byte aligned (BG_ERR_BAD_ALIGNMENT).  A call moves float4s where C % 4 == 0 and x, y (dz) are 16-byte
 * aligned, single floats otherwise; no call is refused for a misaligned view.  bg_noise_route (host only): the eight ints of
 * bg_pixelnorm_route, for these kernels.  A refused call launches nothing.  No call takes a step-program binding. */
#define BG_NOISE_ROUTE_INTS 8
int bg_noise_route(int C, int* out);
int bg_noise_add_f32(const float* x, const float* noise, const float* strength, float* y, int R, int C, float lrelu_alpha, void* stream);
size_t bg_noise_grad_workspace_bytes(int R, int C);
int bg_noise_grad_f32(const float* dz, const float* noise, float* dstrength, int R, int C, void* ws, float beta, float scale, void* stream);

/* ---- style modulation (StyleGAN2, Karras et al. 2020; layers.StyleModulation), un-fused: the activations are scaled, fp32 --------
 * One modulated stage: B samples of P pixels, I input and O output channels, styles s [B, I].  xs = x * s[n, :] goes through the
 * ordinary convolution; with demodulation its output z is scaled by d[n, :] = 1 / sqrt((s * s) . Q + eps), Q[i, o] = sum over the
 * taps of W^2 (it depends on the weights only).  Every sum runs in a fixed order, no atomics: two runs give the same bits; products
 * and sums are rounded separately.  Pointers 4-byte aligned (BG_ERR_BAD_ALIGNMENT); float4 accesses where C % 4 == 0 and every
 * matrix of the call is 16-byte aligned, single floats otherwise: no call is refused for a misaligned view.  Any size >= 1.  A
 * refused call launches nothing.  No call takes a step-program binding: every operand is device memory.
 *   scale      out[n, p, c] = act(in[n, p, c] * v[n, c] (+ bias[c])), act = LeakyReLU(lrelu_alpha) (1: none); bias may be NULL; out
 *              may alias in.  Serves xs, y = d * z + bias, dz = d * dy and dx = s * dxs.
 *   dot        out[n, c] = beta * out + scale * sum_p a[n, p, c] * b[n, p, c] (beta = 0: out is not read).  Serves dd = sum dy * z
 *              and ds = sum x * dxs.  Large P with few channels is cut into slabs of pixels whose sums a second launch adds in slab
 *              order: ws of bg_mod_dot_workspace_bytes(B, P, C) bytes (0: none needed; ws may then be NULL).  bg_mod_dot_plan (host
 *              only): {vec, lanes, chunks, slabs} with float4 units allowed, then the four with single floats.
 *   wsq        Q [I, O] from a kernel [taps, I, O] (Conv2D) or, transposed != 0, [taps, O, I] (Conv2DTranspose); taps in index order.
 *   demod      d[n, o] = 1 / sqrt(sum_i (s[n, i] * s[n, i]) * Q[i, o] + eps), i in index order; correctly rounded sqrt and division.
 *   demod_bwd  dq[n, o] = -1/2 * d^3 * dd[n, o];  ds[n, i] += 2 * s[n, i] * sum_o dq[n, o] * Q[i, o]   (two launches).
 *   wsq_grad   dw[t, ., .] += scale * 2 * w[t, ., .] * dQ (dQ [I, O], broadcast over the taps, either kernel layout). */
#define BG_MOD_DOT_PLAN_INTS 8
int bg_mod_scale_f32(const float* in, const float* v, const float* bias, float* out, int B, int P, int C, float lrelu_alpha, void* stream);
int bg_mod_dot_plan(int B, int P, int C, int* out);
size_t bg_mod_dot_workspace_bytes(int B, int P, int C);
int bg_mod_dot_f32(const float* a, const float* b, float* out, int B, int P, int C, void* ws, size_t ws_bytes, float beta, float scale,
                   void* stream);
int bg_mod_wsq_f32(const float* w, float* q, int taps, int I, int O, int transposed, void* stream);
int bg_mod_wsq_grad_f32(const float* w, const float* dq, float* dw, int taps, int I, int O, int transposed, float scale, void* stream);
int bg_mod_demod_f32(const float* s, const float* Q, float* d, int B, int I, int O, float eps, void* stream);
int bg_mod_demod_bwd_f32(const float* d, const float* dd, const float* s, const float* Q, float* dq, float* ds, int B, int I, int O,
                         void* stream);

/* ---- mapping network (StyleGAN's G_mapping, Karras et al. 2019; layers.MappingNetwork): z -> w, fp32 ------------------------------
 * A stack of skinny Dense layers with the equalised-learning-rate coefficient, the bias multiplier and the LeakyReLU in the epilogue,
 * the pointwise / bias part of its backward, and the truncation trick.  Everything is deterministic (fixed summation orders, no
 * atomics: two runs give the same bits), products and sums are rounded separately.  Pointers 4-byte aligned
 * (BG_ERR_BAD_ALIGNMENT); any size >= 1; a refused call launches nothing.  c, bias_mul, alpha and psi travel by value in the kernel
 * arguments: a recorded step program replays them with nothing bound.
 *   dense_lrelu     y[m, n] = act(c * sum_k x[m, k] * W[k, n] + bias_mul * bias[n]), act = LeakyReLU(alpha) (alpha = 1: linear); x
 *                   [M, K], W [K, N], y [M, N] row-major; bias may be NULL.  The products run on the exact fp32 matrix instruction
 *                   of bg_gemm_f32; a workgroup owns a BG_DENSE_LRELU tile of y and its four waves share each K-step, their sums
 *                   added in wave order; the pre-activation is never written.  y must not alias x or W (BG_ERR_UNSUPPORTED).
 *                   bg_dense_lrelu_plan (host only): {tile rows, tile columns, k per step, workgroups} of a call.
 *   lrelu_bias_bwd  gp[m, n] = g[m, n] * (y[m, n] > 0 ? 1 : alpha)   (bg_mul_grad_f32's convention: y is the stored OUTPUT, whose sign
 *                   is the pre-activation's for alpha > 0); gp may alias g, not y (BG_ERR_UNSUPPORTED).  In the same pass
 *                   dbias[n] = beta * old + scale * sum_m gp[m, n] (beta = 0: old is not read).  float4 units where N % 4 == 0 and
 *                   g, y, gp are 16-byte aligned, single floats otherwise: no shape or view is refused.  ws:
 *                   bg_lrelu_bias_bwd_workspace_bytes(M, N) bytes of device scratch (BG_ERR_WORKSPACE).  Two launches.
 *   truncate        out[b, u] = w_avg[u] + psi * (w[b, u] - w_avg[u]), w_avg [U] in device memory; psi == 1 copies w bit for bit;
 *                   out may alias w. */
#define BG_DENSE_LRELU_PLAN_INTS 4
int bg_dense_lrelu_plan(int M, int N, int K, int* out);
int bg_dense_lrelu_f32(const float* x, const float* W, const float* bias /* may be NULL */, float* y, int M, int N, int K, float c,
                       float bias_mul, float alpha, void* stream);
size_t bg_lrelu_bias_bwd_workspace_bytes(int M, int N);
int bg_lrelu_bias_bwd_f32(const float* g, const float* y, float* gp, float* dbias, int M, int N, float alpha, float beta, float scale,
                          void* ws, size_t ws_bytes, void* stream);
int bg_truncate_f32(const float* w, const float* w_avg, float* out, float psi, int B, int U, void* stream);

/* ---- differentiable augmentation (DiffAugment, Zhao et al. 2020) of the critic's input, NHWC fp32 -----------------------------
 * Per sample an affine map T(x) = L x + k of its [H, W, C] map: colour, then translation, then cutout.  ops_mask: bit 0 colour,
 * bit 1 translation, bit 2 cutout; an absent operation takes its neutral value and does no arithmetic (without colour values are
 * copied bit for bit).  params: [n, 8] uniforms in [0, 1) per sample, decoded in float32 with one multiply per value:
 *   b = u0 - 0.5,  s = 2 u1,  c = u2 + 0.5;
 *   Sy = floor(H * translation_ratio + 0.5),  ty = min(floor(u3 * (2 Sy + 1)), 2 Sy) - Sy    (tx from W, u4);
 *   cy = floor(H * cutout_ratio + 0.5),  ny = H + 1 - cy % 2,  oy = min(floor(u5 * ny), ny - 1)    (cx, nx, ox from W, u6); u7 unused.
 * Forward, with m(p) the mean over the channels of pixel p and mu the mean over the sample:
 *   v(p, c) = c * (s * (x(p, c) - m(p)) + m(p) - mu) + mu + b,     w(i, j) = v(i + ty, j + tx) inside the map, else 0,
 *   y(i, j) = 0 for oy - cy / 2 <= i < oy - cy / 2 + cy and likewise in j, else w(i, j).           linear != 0: b = 0 (this is L).
 * Adjoint, g the gradient at y:  h(i', j') = g(i' - ty, j' - tx) where that pixel is inside the map and not cut, else 0;
 *   e = c * h + (1 - c) * mean(h),   dx(p, c) = s * e(p, c) + (1 - s) * mean_c e(p, .).
 * Each direction is one launch that contains the sample mean; sums are taken in a fixed order without atomics (the same bits on
 * every run).  bg_diffaug_route: *resident = 1 where a sample (H * W * C <= *resident_floats) waits in LDS between its mean and
 * its use and is read from memory once, 0 where it is swept twice (the second read out of L2).  (Without colour there is no mean:
 * either geometry is then one gathering sweep from memory.)  Any H, W, C >= 1; pointers 4-byte
 * aligned (BG_ERR_BAD_ALIGNMENT), 16 bytes per lane wherever a sample's address allows.  The output must not overlap the input
 * (BG_ERR_UNSUPPORTED); ratios outside [0, 1] and unknown mask bits: BG_ERR_UNSUPPORTED.  A refused call launches nothing.  No
 * call takes a step-program binding: params live in device memory.
 * bg_diffaug_decode: the decode above on the host, for one row u[8]: bsc[3] = {b, s, c}, geo[8] = {ty, tx, oy - cy / 2,
 * ox - cx / 2, cy, cx, Sy, Sx}.
 * bg_diffaug_plan (host only): what bg_diffaug_f32 / bg_diffaug_adjoint_f32 launch for this batch and mask -- the calls take
 * their geometry from the same function.  *resident = 1: the resident kernel (never without colour, whatever bg_diffaug_route says
 * of the sample size); threads per workgroup; the grid (grid_x workgroups stride over the n samples, grid_y cut a sample's output on
 * the two-sweep route, 1 on the resident one); the dynamic LDS in bytes.  Any out pointer may be NULL. */
int bg_diffaug_route(int H, int W, int C, int* resident, int* resident_floats);
int bg_diffaug_plan(int n, int H, int W, int C, int ops_mask, int* resident, int* threads, int* grid_x, int* grid_y, int* lds_bytes);
int bg_diffaug_decode(const float* u, int H, int W, int ops_mask, float translation_ratio, float cutout_ratio, float* bsc, int* geo);
int bg_diffaug_f32(const float* x, float* y, const float* params, int n, int H, int W, int C, int ops_mask, float translation_ratio,
                   float cutout_ratio, int linear, void* stream);
int bg_diffaug_adjoint_f32(const float* dy, float* dx, const float* params, int n, int H, int W, int C, int ops_mask,
                           float translation_ratio, float cutout_ratio, void* stream);

/* ---- adaptive augmentation (ADA, Karras et al. 2020): gated DiffAugment and the controller of its probability ---------------------
 * The gated calls are the two calls above with a per-sample gate on every operation.  params: [n, 12] uniforms; u0..u7 are decoded
 * exactly as above, u8 / u9 / u10 are the gates of colour / translation / cutout, u11 is unused.  p: ONE float in DEVICE memory, read
 * by the kernel when it runs (a replayed step program sees the value the controller left there).  An operation of ops_mask fires for
 * a sample iff its gate < *p, compared in fp32; one that does not fire takes its neutral value and does no arithmetic for that sample
 * (colour off: the sample is gathered bit for bit and its mean is never formed; translation off: shift 0; cutout off: an empty box).
 * *p = 1: the ungated call on params[:, :8], bit for bit (u < 1 always holds).  *p = 0, or a sample none of whose gates fired: a
 * bit-for-bit copy.  The launch geometry is bg_diffaug_plan's for ops_mask, whatever fires.  Refusals and statuses of the ungated
 * calls, plus BG_ERR_NULL for a null p and BG_ERR_BAD_ALIGNMENT for a misaligned one.  The ungated calls run the code they ran
 * before these existed: the gate is a template parameter of the kernel, and their instantiations read neither p nor a gate.
 * bg_diffaug_decode_gated (host): the decode of one row u[12] at probability p.  *fired_mask = ops_mask & fired bits; bsc and geo as
 * bg_diffaug_decode with the neutral values of what did not fire (geo[4], geo[5]: the box's extent, 0 where the cutout did not fire).
 *
 * Controller.  bg_ada_stats_f32: stats[4] = {sum_i sign(scores[i]), n, 0, 0} with sign(0) = sign(NaN) = 0: a sum of +-1 and 0, exact
 * in fp32 in any order (0 < n < 2^24).  bg_ada_update_f32: state[8] = {p, acc_sign, acc_count, k, r_last, 0, 0, 0};
 *   acc_sign += stats[0];  acc_count += stats[1];  k += 1;
 *   when k == interval:  r = acc_sign / acc_count;  p = clamp(p + sgn(r - target) * acc_count * inv_speed_images, 0, 1), sgn(0) = 0,
 *                        the product and the sum rounded separately;  r_last = r;  acc_sign = acc_count = k = 0
 * (StyleGAN2-ADA's adjust = sign(r_t - target) * batch * interval / (ada_kimg * 1000)).  metrics_out, if not NULL, receives {p, r_last}
 * after the update.  target in (-1, 1), inv_speed_images > 0 (BG_ERR_UNSUPPORTED), interval >= 1 (BG_ERR_BAD_SHAPE).  Under data
 * parallelism the caller sum-all-reduces stats between the two calls.  One workgroup each, plain stores from one lane, no atomics.
 * No call takes a step-program binding: everything that changes lives in device memory. */
int bg_diffaug_gated_f32(const float* x, float* y, const float* params /* [n, 12] */, const float* p /* device, 1 float */, int n, int H,
                         int W, int C, int ops_mask, float translation_ratio, float cutout_ratio, int linear, void* stream);
int bg_diffaug_gated_adjoint_f32(const float* dy, float* dx, const float* params /* [n, 12] */, const float* p /* device, 1 float */, int n,
                                 int H, int W, int C, int ops_mask, float translation_ratio, float cutout_ratio, void* stream);
int bg_diffaug_decode_gated(const float* u /* 12 */, float p, int H, int W, int ops_mask, float translation_ratio, float cutout_ratio,
                            float* bsc, int* geo, int* fired_mask);
int bg_ada_stats_f32(const float* scores, int n, float* stats /* [4] */, void* stream);
int bg_ada_update_f32(const float* stats, float* state /* [8] */, float* metrics_out /* 2 floats, may be NULL */, float target, int interval,
                      float inv_speed_images, void* stream);

/* ---- minibatch standard deviation (Karras et al. 2018; StyleGAN2's layer with one new feature; layers.MinibatchStdDev) ---------
 * x: [N, P, C] fp32, P pixels; a group is G CONSECUTIVE samples (N % G == 0, G >= 2: BG_ERR_BAD_SHAPE otherwise).  Per group g and
 * column (p, c), with k = 1 / (G * P * C):
 *   mu = mean_n x,   s = sqrt(mean_n (x - mu)^2 + eps)   (two-pass, centred),   f_g = mean_{p,c} s.
 * bg_mbstd_fwd_f32: y [N, P, C + 1] = x in channels [0, C), f_g in channel C of every pixel of every sample of the group; keeps
 * mu and rs = 1 / s ([N / G, P * C] each) and f ([N / G]) for the other calls.
 * bg_mbstd_bwd_f32: u is the gradient at y; q_g = sum_{n in g, p} u[n, p, C] (kept in q [N / G]: the penalty's source needs it),
 *   dx = u[..., :C] + q_g * k * (x - mu) * rs.
 * bg_mbstd_gp_f32: the gradient penalty's tangent and source in one call, d the tangent at x, q from the first-order backward:
 *   vout [N, P, C + 1] = d in channels [0, C),  fdot_g = k * sum_{n in g, p, c} (x - mu) * rs * d  in channel C  (kept in fdot [N / G]);
 *   src = q_g * k * rs^3 * ((d - dbar) * eps + [(d - dbar) * var - (x - mu) * m]),  dbar = mean_n d,  m = mean_n (x - mu) * d,
 *   which is q_g * k * ((d - dbar) / s - (x - mu) * m / s^3) with the difference taken before the division.  At G = 2 the bracket is
 *   identically zero (the members' centred values are one another's negatives) and is not evaluated.
 * mu is formed as x_0 + mean_n (x_n - x_0) and f_g as s_0 + mean (s - s_0) over the columns: equal members give mu = x_0, equal
 * columns f_g = s_0, exactly and in any order of summation (a group without variance: f_g = sqrt(eps)).
 * A column whose members are all equal has x - mu = 0 exactly and adds exactly 0 to dx and fdot (and to src where d is equal too).
 * Every sum runs in a fixed order: per-thread partials in loop order, a fixed tree, no atomics -- the same bits on every run.
 * A group of at most 15356 floats is read from memory once (one workgroup per group, the group in LDS between its statistics and
 * its output; one launch).  A larger group takes two launches in the forward and the penalty call: its columns cut over several
 * workgroups that leave partial sums in the workspace (bg_mbstd_workspace_bytes; 0 on the resident route), then the output, every
 * workgroup adding the partials in index order.  The backward is one launch on either route and takes no workspace.
 * Pointers 4-byte aligned (BG_ERR_BAD_ALIGNMENT); 16 bytes per lane wherever an address allows, scalar heads and tails elsewhere
 * (the output's row stride C + 1 is odd for every stock critic: its groups are swept as flat ranges).  NULL: BG_ERR_NULL; a pointer
 * the runtime knows as host memory: BG_ERR_UNSUPPORTED.  No output may alias an input.  A refused call launches nothing.  No call
 * takes a step-program binding.
 * bg_mbstd_plan (host only): what call (0 forward, 1 backward, 2 penalty) launches, the calls take their geometry from the same
 * function.  offset_floats in [0, 4): where the swept pointer (mu; the backward: dx) stands after a 16-byte boundary.
 * out[BG_MBSTD_PLAN_INTS] = {resident, threads, grid_x (workgroups stride over the groups), grid_y of the column phase (the
 * backward: of its one sweep), grid_y of the output phase, dynamic LDS bytes, launches, float4s of that sweep per group, fewest and
 * most float4 trips of a lane, scalar head, scalar tail}. */
#define BG_MBSTD_PLAN_INTS 12
int bg_mbstd_plan(int N, int G, int P, int C, int call, int offset_floats, int* out);
size_t bg_mbstd_workspace_bytes(int N, int G, int P, int C);
int bg_mbstd_fwd_f32(const float* x, float* y, float* mu, float* rs, float* f, int N, int G, int P, int C, float eps, void* ws_d,
                     size_t ws_bytes, void* stream);
int bg_mbstd_bwd_f32(const float* u, const float* x, const float* mu, const float* rs, float* dx, float* q, int N, int G, int P, int C,
                     void* stream);
int bg_mbstd_gp_f32(const float* d, const float* x, const float* mu, const float* rs, const float* q, float* vout, float* src,
                    float* fdot, int N, int G, int P, int C, float eps, void* ws_d, size_t ws_bytes, void* stream);

/* ---- spectral normalisation (Miyato et al. 2018; layers.SpectralNormalization) -------------------------------------------
 * A wrapped layer's kernel is the row-major matrix W[K, N] (N = the kernel's last axis, K = the rest); the engine runs on
 * W-bar = W / sigma, sigma from a running power iteration with the unit vectors u[N], v[K] (layer state).
 *
 * Every call is batched over all wrapped layers of one model.  The table has BG_SPECTRAL_DESC_INTS int32 per layer:
 *   {w_off, u_off, v_off, sigma_off, eff_off, tr_off, K, N, taps, pass_first, ew_first, tile_first, ws_off, 0, 0, 0}
 * w_off: floats from `theta` (and from the flat gradient buffer); u_off / v_off / sigma_off: from `state`; eff_off / tr_off: from
 * the effective-weight base (tr_off = -1: no transposed copy); ws_off: from the workspace.  All but sigma_off are multiples of 4.
 * taps divides K (k * k for conv kernels, 1 for Dense).  pass_first / ew_first / tile_first: the layer's first work unit in the
 * power pass, in the dot / apply kernels and in the scale kernel -- running sums of bg_spectral_route's pass_units / ew_units /
 * tiles.  The table is handed over twice: desc_d on the device, which the kernels read, and the same rows in host memory, desc_h,
 * which the call checks before anything touches the device: null pointer BG_ERR_NULL, K / N / taps <= 0 or first units that do not
 * continue the table BG_ERR_BAD_SHAPE, a base or an offset that is not 16-byte aligned BG_ERR_BAD_ALIGNMENT, a workspace smaller
 * than bg_spectral_workspace_bytes BG_ERR_WORKSPACE.  A matrix is cut into units by (K, N, taps) alone, partial sums are added in
 * unit order and nothing is atomic: results are the same bits from run to run and for any batching of the layers. */
#define BG_SPECTRAL_DESC_INTS 16
/* pure host query: how [K, N] is laid over a wave (vec floats per access, `lanes` lanes per row, `chunks` vectors per lane; chunks
 * = 0: rows wider than a wave holds, a wave strides over its row), the rows of a pass unit, the unit counts, the workspace floats */
int bg_spectral_route(int K, int N, int taps, int* vec, int* lanes, int* chunks, int* strip_rows, int* pass_units, int* ew_units,
                      int* tiles, int* ws_floats);
/* pure host query over a host table; 0 for a table the calls would refuse */
size_t bg_spectral_workspace_bytes(const int* desc_h, int n);
/* One power round: t = W u, v = t / max(||t||, 1e-12), s = W^T v, u = s / max(||s||, 1e-12), sigma = s . u (= v^T W u) -- W is
 * read once: a workgroup takes a strip of rows and adds t_r * W[r, :] while row r is in registers; a second launch adds the
 * strips' partials.  sigma_only != 0: sigma = v^T W u with the stored u and v, both left as they are. */
int bg_spectral_power_f32(const float* theta, float* state, const int* desc_d, const int* desc_h, int n, int sigma_only, float* ws_d,
                          size_t ws_bytes, void* stream);
/* eff[eff_off + i] = W[i] / sigma, and where tr_off >= 0 the copy eff[tr_off + (t * N + c) * R + r] of element (t * R + r, c), R =
 * K / taps: the [taps][C][R] array bg_conv2d_fwd reads, out of the same launch (no bg_transpose_last2_batched for such a model) */
int bg_spectral_scale_f32(const float* theta, const float* state, float* eff, const int* desc_d, const int* desc_h, int n, void* stream);
/* g = dL/dW-bar in the flat gradient buffer (at w_off) becomes dL/dW, u and v held constant:
 *   g <- (g - <g, W-bar> * v u^T) / sigma         (two launches: the dot's per-workgroup partials, then the apply) */
int bg_spectral_grad_f32(float* grad, const float* eff, const float* state, const int* desc_d, const int* desc_h, int n, float* ws_d,
                         size_t ws_bytes, void* stream);

/* ---- equalised learning rate (Karras et al. 2018; layers.EqualizedLearningRate) ------------------------------------------
 * A wrapped layer's kernel W[K, N] (as above) is drawn from N(0, 1); the engine runs on W_eff = c * W with the per-layer constant
 * c = gain / sqrt(fan_in), and the optimizer sees dL/dW = c * dL/dW_eff.
 *
 * Both calls are batched over all wrapped layers of one model.  The table has BG_EQLR_DESC_INTS int32 per layer:
 *   {w_off, eff_off, tr_off, K, N, taps, tile_first, unit_first, c, 0, 0, 0}           (c: the bits of the fp32 coefficient)
 * w_off: floats from `theta` (and from the flat gradient buffer); eff_off / tr_off: from the effective-weight base (tr_off = -1: no
 * transposed copy); all multiples of 4.  taps divides K.  tile_first / unit_first: the layer's first work unit in the scale and in
 * the gradient kernel -- running sums of bg_eqlr_plan's tiles / grad_units.  The table is handed over twice: desc_d on the device,
 * which the kernels read, and the same rows in host memory, desc_h, which the call checks before anything touches the device: null
 * pointer BG_ERR_NULL; K / N / taps <= 0, first units that do not continue the table, c not positive and finite, a segment that
 * ends behind its buffer (`*_floats`: the floats behind each base) or overlaps another BG_ERR_BAD_SHAPE; a base or an offset that
 * is not 16-byte aligned BG_ERR_BAD_ALIGNMENT.  Every element is written by one thread and multiplied once: the same bits from run
 * to run and for any batching of the layers. */
#define BG_EQLR_DESC_INTS 12
/* pure host query: the 64 x 64 tiles of the scale kernel, its access width (4: R = K / taps and N both multiples of 4, else 1), the
 * units of the gradient kernel and the floats of one unit */
int bg_eqlr_plan(int K, int N, int taps, int* tiles, int* vec, int* grad_units, int* unit_elems);
/* pure host query: the status the two calls below would give this table (eff_floats: of the effective-weight buffer) */
int bg_eqlr_check_table(const int* desc_h, int n, size_t theta_floats, size_t eff_floats);
/* eff[eff_off + i] = c * W[i] (one fp32 multiply), and where tr_off >= 0 the copy eff[tr_off + (t * N + col) * R + r] of element
 * (t * R + r, col), R = K / taps: the [taps][C][R] array bg_conv2d_fwd reads, out of the same launch */
int bg_eqlr_scale_f32(const float* theta, size_t theta_floats, float* eff, size_t eff_floats, const int* desc_d, const int* desc_h, int n,
                      void* stream);
/* g[w_off + i] *= c in place for i < K * N of every layer; nothing else of the buffer is written */
int bg_eqlr_grad_f32(float* grad, size_t grad_floats, const int* desc_d, const int* desc_h, int n, void* stream);

/* ---- pointwise ------------------------------------------------------------------------------ */
/* wgan.py:239: xhat[b,:] = r[b,:] + alpha[b] * (f[b,:] - r[b,:]) */
int bg_lerp_f32(const float* r, const float* f, const float* alpha_b, float* xhat, int B, int n_per, void* stream);
/* wgan.py:245: norm[b] = ||g[b,:]||_2 */
int bg_row_norm_f32(const float* g, float* norm_b, int B, int n_per, void* stream);
/* second-order seed: out[b,:] = coef * (norm[b]-1)/norm[b] * g[b,:]   (d mean((n-1)^2) / dg) */
int bg_gp_seed_f32(const float* g, const float* norm_b, float coef, float* out, int B, int n_per, void* stream);
/* the same with the subgradient 0 for a sample whose norm is exactly 0 (the reference, like tf.norm's gradient at 0, yields NaN
   there and Adam then spreads it into every weight): build-side switch WGANGP(gp_zero_norm_guard=True), off by default */
int bg_gp_seed_guarded_f32(const float* g, const float* norm_b, float coef, float* out, int B, int n_per, void* stream);
/* out = d * (ref > 0 ? 1 : alpha) [* keep ? scale : 0] */
int bg_mul_grad_f32(const float* d, const float* ref, const uint8_t* keep, float alpha, float scale,
                    float* out, size_t n, void* stream);
/* out = dy * (1 - y^2) */
int bg_tanh_bwd_f32(const float* dy, const float* y, float* out, size_t n, void* stream);
/* out[b, k] = s[b] * w[k] */
int bg_outer_f32(const float* s_b, const float* w_k, float* out, int B, int K, void* stream);
int bg_fill_f32(float* x, float v, size_t n, void* stream);
int bg_scale_f32(float* x, float v, size_t n, void* stream);
/* dst[0:n] = src[0:n] as a KERNEL (a blur-less critic's [fakes; reals; x-hat] batch is assembled with it: a launch that a step
   program records like any other, which a runtime memcpy would not be) */
int bg_copy_f32(float* dst, const float* src, size_t n, void* stream);

/* ---- resampling: tf.keras.layers.UpSampling2D(2, "nearest") / AveragePooling2D(2) over NHWC fp32 maps --------------------
 * Two linear, parameter-free operators, each the transpose of the other: UpSampling2D forward = upsample at scale 1, backward =
 * pool-sum at scale 1; AveragePooling2D forward = pool-sum at scale 0.25, backward = upsample at scale 0.25; the gradient
 * penalty's linearised forward of either layer is its forward.  H, W are the LOW-resolution map's in both calls.  C % 4 == 0
 * moves float4s and wants every pointer 16-byte aligned (BG_ERR_BAD_ALIGNMENT otherwise); any other C goes one float at a time
 * with no alignment demand.  Null x / y: BG_ERR_NULL; a non-positive dimension: BG_ERR_BAD_SHAPE.  A refused call launches
 * nothing.  Indices are formed in 64 bits.  Neither call takes a step-program binding. */
/* y[b, 2i+di, 2j+dj, c] = scale * x[b, i, j, c], di, dj in {0, 1}: x[B,H,W,C] -> y[B,2H,2W,C].  With ref (shape of y; keep, uint8 of
 * the same shape, may come with it) every written element is further multiplied by bg_mul_grad_f32's factor
 * (ref > 0 ? 1 : alpha) [* keep ? grad_scale : 0]: the result equals this call without ref followed by bg_mul_grad_f32 on its
 * output, bit for bit -- a pooling layer's backward written straight as the dz of the conv + LeakyReLU (+ Dropout) stage below
 * it.  ref and keep must not overlap y. */
int bg_upsample2x_nhwc_f32(const float* x, float* y, int B, int H, int W, int C, float scale, const float* ref /* may be NULL */,
                           const uint8_t* keep /* may be NULL */, float alpha, float grad_scale, void* stream);
/* y[b, i, j, c] = scale * ((x[b,2i,2j,c] + x[b,2i,2j+1,c]) + (x[b,2i+1,2j,c] + x[b,2i+1,2j+1,c])): x[B,2H,2W,C] -> y[B,H,W,C], summed
 * in exactly this order. */
int bg_pool2x_sum_nhwc_f32(const float* x, float* y, int B, int H, int W, int C, float scale, void* stream);
/* FIR-filtered 2x resampling (StyleGAN2's upsample_2d / downsample_2d) with a separable kernel of 2T taps, T in 1..4.  Per axis,
 * for n low-resolution entries,
 *   UP_t(x)[o]   = sum_i t[o - 2i + T - 1] * x[i],  o in [0, 2n)
 *   DOWN_t(g)[m] = sum_o t[T + 2m - o] * g[o],      m in [0, n)
 * where a term whose tap index falls outside [0, 2T) or whose sample falls outside the map is absent (zero padding); the 2-D
 * operators are the products over H and W, and a call computes y = scale * op(x) in one launch, no intermediate map.
 * <UP_t x, g> = <x, DOWN_flip(t) g> with flip(t)[j] = t[2T - 1 - j]: FilteredUpSampling2D forward = UP_f at scale 4, backward =
 * DOWN_flip(f) at scale 4; FilteredDownSampling2D forward (and penalty tangent) = DOWN_f at scale 1, backward = UP_flip(f) at
 * scale 1.  taps = (0.5, 0.5) gives the nearest pair above.  H, W are the LOW-resolution map's in both calls.  taps is a HOST
 * pointer to n_taps in {2, 4, 6, 8} floats, copied by value into the kernel's arguments: a step program replays them with no device
 * table.  Routes, alignment and statuses as for the nearest pair; additionally null taps: BG_ERR_NULL, any other n_taps:
 * BG_ERR_BAD_SHAPE.  ref / keep / alpha / grad_scale of the upsample: as bg_upsample2x_nhwc_f32's, bit for bit this call without
 * ref followed by bg_mul_grad_f32.  Neither call takes a step-program binding. */
int bg_fir_upsample2x_nhwc_f32(const float* x, float* y, int B, int H, int W, int C, const float* taps, int n_taps, float scale,
                               const float* ref /* may be NULL */, const uint8_t* keep /* may be NULL */, float alpha, float grad_scale,
                               void* stream);
int bg_fir_downsample2x_nhwc_f32(const float* x, float* y, int B, int H, int W, int C, const float* taps, int n_taps, float scale,
                                 void* stream);

/* ---- losses (wgan.py:128-130,155-157,272-285) ----------------------------------------------- */
/* From scores fs[B], rs[B] and the per-sample norms n[B] of the GP gradient:
 *   metrics_d[0..5] = mean(fs), mean(rs), disc_loss (mean of the [B] vector), gp_term, mean(norm_term), GP
 *   dfs[b] = vec_scale*inv_gbs + e_drift*sign(fs[b]);  drs[b] = -vec_scale*inv_gbs + e_drift*sign(rs[b])
 * vec_scale is B when the reference's [B]-vector loss quirk (Q1) is reproduced, 1 otherwise. */
int bg_wgangp_d_loss(const float* fs, const float* rs, const float* norm_b, int B, float inv_gbs,
                     float gp_coef, float e_drift, float vec_scale, float* dfs, float* drs,
                     float* metrics_d, void* stream);
/* metrics_d[0] = mean(s), metrics_d[1] = -sum(s)*inv_gbs ; ds[b] = -inv_gbs */
int bg_wgan_g_loss(const float* s, int B, float inv_gbs, float* ds, float* metrics_d, void* stream);

/* ---- GAN objectives: the loss as an argument, the penalty's target as an argument -----------------------------------------
 * With s+ = softplus, sums scaled by inv_gbs:
 *   BG_LOSS_WASSERSTEIN    critic sum(fs - rs)                         generator -sum(fs)
 *   BG_LOSS_HINGE          critic sum(relu(1 + fs) + relu(1 - rs))     generator -sum(fs)
 *   BG_LOSS_NONSATURATING  critic sum(s+(fs) + s+(-rs))                generator sum(s+(-fs))
 * Softplus is max(x, 0) + log1p(exp(-|x|)) and the sigmoid takes the branch whose exponential cannot overflow: finite at any
 * score.  The hinge's subgradient at its kink is 0 (fs == -1 and rs == 1 are off).  Refused calls (BG_ERR_NULL: null pointer;
 * BG_ERR_BAD_SHAPE: B <= 0, n_per <= 0; BG_ERR_UNSUPPORTED: unknown loss, target < 0) launch nothing.  None takes a
 * step-program binding. */
typedef enum { BG_LOSS_WASSERSTEIN = 0, BG_LOSS_HINGE = 1, BG_LOSS_NONSATURATING = 2 } bg_gan_loss;
/* bg_wgangp_d_loss for any loss and penalty target t: one workgroup, the same summation order, the same six metric slots with
 * metrics_d[5] = mean((n - t)^2) (0 without norm_b) and the loss of the table in metrics_d[2].  Seeds, w = vec_scale * inv_gbs:
 *   wasserstein    dfs = w + e_drift*sign(fs)                     drs = -w + e_drift*sign(rs)
 *   hinge          dfs = (fs > -1 ? w : 0) + e_drift*sign(fs)     drs = (rs < 1 ? -w : 0) + e_drift*sign(rs)
 *   nonsaturating  dfs = w*sigmoid(fs) + e_drift*sign(fs)         drs = -w*sigmoid(-rs) + e_drift*sign(rs)
 * BG_LOSS_WASSERSTEIN with gp_target 1 is bg_wgangp_d_loss bit for bit. */
int bg_gan_d_loss(const float* fs, const float* rs, const float* norm_b /* may be NULL */, int B, int loss, float inv_gbs, float gp_coef,
                  float gp_target, float e_drift, float vec_scale, float* dfs, float* drs, float* metrics_d, void* stream);
/* nonsaturating: ds = -inv_gbs*sigmoid(-s), metrics_d[1] = sum(s+(-s))*inv_gbs; the other two losses: bg_wgan_g_loss.
 * metrics_d[0] = mean(s). */
int bg_gan_g_loss(const float* s, int B, int loss, float inv_gbs, float* ds, float* metrics_d, void* stream);
/* second-order seed for the target t >= 0: out[b,:] = coef * (norm[b]-t)/norm[b] * g[b,:].  t == 0 runs an instantiation that
 * computes coef * g with no division (a zero-norm sample gives 0, never NaN, whatever guard says); for t > 0, guard != 0 is
 * bg_gp_seed_guarded_f32's subgradient 0 at a zero norm, guard == 0 bg_gp_seed_f32's NaN, and t == 1 equals those calls bit for
 * bit.  float4 where out and g are 16-byte aligned and n_per % 4 == 0, one float at a time otherwise.  out may be g. */
int bg_gp_seed_target_f32(const float* g, const float* norm_b, float coef, float target, int guard, float* out, int B, int n_per,
                          void* stream);

/* ---- input pipeline (demo_celeba.py:22-35, demo_mnist.py:24-31): uint8 NHWC -> float32, (x - 127.5) / 127.5, then
 *      tf.image.resize(bilinear, half-pixel centres) to [Hd, Wd] (normalise BEFORE resize, aspect not preserved).
 *      Hd == Hs && Wd == Ws is the MNIST pipeline (normalise only). */
int bg_u8_normalize_resize_f32(const uint8_t* src, float* dst, int B, int Hs, int Ws, int C, int Hd, int Wd, void* stream);
/* The same pipeline fed from a DEVICE-RESIDENT uint8 dataset src[N, Hs, Ws, C] in ONE launch (the tfds ... map ... shuffle ... batch
 * chain of demo_celeba.py:15-48 with the whole dataset in HBM): dst[b] = resize(normalise(src[idx_d[b]])), b < B, with the arithmetic
 * of bg_u8_normalize_resize_f32, bit for bit.  idx_d[B] (device, int32) may repeat and come in any order; image byte offsets are
 * formed in 64 bits.  flip_d[B] (device, uint8; may be NULL = no mirroring): where flip_d[b] != 0 the sample is mirrored left-right
 * at the OUTPUT index, dst[b, y, x, c] = unmirrored[b, y, Wd-1-x, c], so a mirrored sample is bit-identical to the mirror of the
 * unmirrored one.  dst must be 16-byte aligned (BG_ERR_BAD_ALIGNMENT, nothing launched): C = 1, 3, 4 write 16-byte stores with a
 * scalar tail of (B*Hd*Wd) % 4 pixels.  The library cannot see device memory: EVERY idx_d[b] MUST lie in [0, N) -- the caller
 * guarantees it.  Takes no step-program binding; it is meant to run between steps, outside any recorded program. */
int bg_u8_gather_normalize_resize_f32(const uint8_t* src, int N, const int32_t* idx_d, const uint8_t* flip_d /* may be NULL */,
                                      float* dst, int B, int Hs, int Ws, int C, int Hd, int Wd, void* stream);

/* ---- SWD metric: sliced Wasserstein distance between image sets (sliced_wasserstein.py:13-51,72-88; metrics.py:93-157) ----
 * The evaluation the reference's SWDMetricCallback runs inside the training loop, as kernels over float32 planar NCHW buffers.
 * The random DRAWS (patch centres, directions) stay on the host; the projection between standardize and sort is bg_gemm_f32
 * (P[dirs, rows] = dirs^T * desc^T, transA = transB = 1: each direction's projections are one contiguous row).  Every entry
 * moves 16 bytes per lane where the geometry keeps the addresses 16-byte aligned and one float per lane otherwise; pointers
 * must be 4-byte (doubles: 8-byte) aligned (BG_ERR_BAD_ALIGNMENT).  A refused call launches nothing.  None of the entries takes
 * a step-program binding: they run between steps, outside any recorded program.  Buffers hold fewer than 2^31 elements. */
/* dst[B,3,H,W] = src * scale + shift (two fp32 roundings), src NHWC (src_nhwc != 0) or NCHW with C = 1 or 3 channels
 * (BG_ERR_BAD_SHAPE otherwise); C = 1 is replicated three times (tf.image.grayscale_to_rgb).  model.images ([-1, 1], NHWC) enter
 * the metric through this call with scale = shift = 127.5 and no transpose (demo_mnist.py:180-184). */
int bg_swd_ingest_f32(const float* src, float* dst, int B, int H, int W, int C, int src_nhwc, float scale, float shift, void* stream);
/* sliced_wasserstein.py:65-74 (pyr_down): y[planes, ceil(H/2), ceil(W/2)] = every second pixel of the separable 5-tap binomial
 * [1 4 6 4 1]/16 with reflect-101 borders; H pass over every row, then W pass, each accumulated tap by tap (j = 0..4 from 0.0f,
 * fp32 products and sums): the host pyr_down on float32 input bit for bit.  H, W >= 3. */
int bg_pyr_down_f32(const float* x, float* y, int planes, int H, int W, void* stream);
/* sliced_wasserstein.py:76-81 (pyr_up) and the subtraction of :83-88 (one Laplacian level in one launch):
 * out[planes, 2h, 2w] = pyr_up(low), or minuend - pyr_up(low) when minuend != NULL (out == minuend allowed).  pyr_up = zero-stuff
 * to 2h x 2w, the same filter with reflect-101 on the stuffed grid, gain 4 after the filter; the taps on stuffed zeros add an exact
 * zero and are skipped, so the result is the host pyr_up bit for bit.  h, w >= 2. */
int bg_pyr_up_f32(const float* low, const float* minuend /* may be NULL */, float* out, int planes, int h, int w, void* stream);
/* sliced_wasserstein.py:13-23 (get_descriptors_for_minibatch) from the centres the host drew: level[B,3,H,W]; cx_d, cy_d int32
 * device vectors of B * per_image entries; desc[t, c, a, b] = level[t / per_image, c, cy[t] + b - half, cx[t] + a - half] with
 * half = nhood / 2 -- the reference's transposed patch: a walks x, b walks y.  nhood odd, <= min(H, W).  The library cannot see
 * device memory: EVERY centre MUST lie in [half, size - half) -- the caller checks the draws' range on the host. */
int bg_swd_gather_f32(const float* level, const int32_t* cx_d, const int32_t* cy_d, float* desc, int B, int H, int W, int nhood,
                      int per_image, void* stream);
/* sliced_wasserstein.py:27-34 (finalize_descriptors) over desc[rows, 3, nhood, nhood], in place: per-channel mean and POPULATION
 * standard deviation accumulated in float64 (two-stage partials in a fixed order, no atomics; the deviation is summed around the
 * mean in a second pass), both rounded to fp32, then desc = (desc - mean32) / std32 as two fp32 operations.  A constant channel
 * gives the IEEE result of the division.  stats_out (may be NULL): 3 x {mean, std} doubles on the device. */
size_t bg_swd_standardize_workspace_bytes(int rows, int nhood);
int bg_swd_standardize_f32(float* desc, int rows, int nhood, double* stats_out /* may be NULL */, void* ws, size_t ws_bytes, void* stream);
/* np.sort(x, axis=1) in place over x[rows, n] (sliced_wasserstein.py:47-48, transposed): a data-oblivious bitonic network -- 4096-float chunks
 * and the merge tails in LDS, one launch per compare-exchange distance above the chunk, indices >= n standing for +inf without a
 * padded copy.  Finite input: the values of np.sort (-0.0 and +0.0 compare equal).  NaNs end up anywhere but never fault: the
 * access pattern depends on (rows, n) only.  1 <= n <= 2^24, rows * n < 2^31. */
int bg_sort_rows_f32(float* x, int rows, int n, void* stream);
/* out[s] (double, device) = mean over e < seg of |a[s * seg + e] - b[s * seg + e]| (sliced_wasserstein.py:49-50): the difference in
 * fp32, the sum in float64 in a fixed order.  One segment per direction repeat.  nseg <= 65535. */
size_t bg_abs_diff_mean_workspace_bytes(size_t seg, int nseg);
int bg_abs_diff_mean_f32(const float* a, const float* b, size_t seg, int nseg, double* out, void* ws, size_t ws_bytes, void* stream);

/* ---- optimiser: tf.keras.optimizers.Adam (wgan.py:56-61,141,167) ----------------------------- */
/* lr_t = lr*sqrt(1-b2^t)/(1-b1^t) is computed by the caller (host) per step. */
int bg_adam_f32(float* theta, float* m, float* v, const float* g, size_t n, float lr_t, float b1, float b2,
                float eps, void* stream);

/* ---- optimisers: the Keras objects a user assigns to gan.<net>.optimizer (wgan.py:56-61,141,167; TF 2.5 optimizer_v2) --
 * All three take a 16-byte aligned theta / slot / gradient (BG_ERR_BAD_ALIGNMENT otherwise) and any n (a scalar tail covers
 * n % 4).  lr is the step's rate after the host applied the schedule and the inverse-time decay (Adam: lr_t with the bias
 * correction); under a step program it is bound with BG_BIND_OPT_LR. */
/* tf.keras.optimizers.SGD: ResourceApplyGradientDescent (momentum 0; a may be NULL) / ResourceApplyKerasMomentum
 * (a = momentum*a - lr*g; theta += a, or theta += momentum*a - lr*g with nesterov) */
int bg_sgd_f32(float* theta, float* a, const float* g, size_t n, float lr, float momentum, int nesterov, void* stream);
/* tf.keras.optimizers.RMSprop: r = rho*r + (1-rho)*g^2 ; centered: mg = rho*mg + (1-rho)*g, d = r - mg^2 (else d = r);
 * momentum 0 (Keras' Python path): theta -= lr*g / (sqrt(d) + eps) ; momentum > 0 (ResourceApplyRMSProp /
 * ResourceApplyCenteredRMSProp): p = momentum*p + lr*g / sqrt(d + eps), theta -= p.  p may be NULL when momentum == 0, mg when
 * centered == 0. */
int bg_rmsprop_f32(float* theta, float* r, float* p, float* mg, const float* g, size_t n, float lr, float rho, float momentum,
                   float eps, int centered, void* stream);
/* tf.keras.optimizers.Adam(amsgrad=True): ResourceApplyAdamWithAmsgrad -- bg_adam_f32's m / v, vhat = max(vhat, v),
 * theta -= lr_t*m / (sqrt(vhat) + eps).  Adam without amsgrad (any beta / epsilon) is bg_adam_f32. */
int bg_adam_amsgrad_f32(float* theta, float* m, float* v, float* vhat, const float* g, size_t n, float lr_t, float b1, float b2,
                        float eps, void* stream);

/* ---- weight averaging: tf.train.ExponentialMovingAverage over a network (the averaged generator GANs sample from) ----
 * TF's assign_moving_average, per element in fp32 and in this order: avg = avg - w * (avg - theta), with w = 1 - decay formed by
 * the host in double and rounded once (1 - 0.999f in fp32 is 1.00004673e-3).  Two segments in ONE launch: a network's flat
 * trainable buffer (avg, theta, n) and its non-trainable state buffer, the BatchNorm moving statistics (avg2, theta2, n2;
 * n2 == 0: both may be NULL).  16-byte aligned pointers (BG_ERR_BAD_ALIGNMENT otherwise), any n > 0 and n2 (scalar tails cover
 * n % 4), w in [0, 1].  The average is plain fp32, as TF's: for w below about 1e-4 an update can fall under one ulp of the
 * average and is then lost to rounding.  Under a step program w is bound with BG_BIND_EMA_W. */
int bg_ema_f32(float* avg, const float* theta, size_t n, float* avg2, const float* theta2, size_t n2, float w, void* stream);

/* ---- RNG: tf.random.uniform (wgan.py:118,237) and Dropout masks; counter-based, own stream ---- */
int bg_uniform_f32(float* out, size_t n, uint64_t seed, uint64_t offset, void* stream);
int bg_keep_mask_u8(uint8_t* out, size_t n, float keep_prob, uint64_t seed, uint64_t offset, void* stream);
/* N(0, 1) draws (the per-pixel noise inputs of a StyleGAN synthesis layer, and latents drawn from N(0, I)).  The layout contract of
 * the two draws above: element e comes from the Philox4x32-10 block with counter offset + e / 4, and a draw consumes (n + 3) / 4
 * blocks; the third counter word is 2 (0: the uniforms, 1: the keep masks).  Box-Muller inside a block: words (0, 1) give elements
 * (0, 1), words (2, 3) give elements (2, 3); u1 = ((w_a >> 8) + 1) * 2^-24 in (0, 1], u2 = (w_b >> 8) * 2^-24 in [0, 1),
 * r = sqrtf(-2 logf(u1)), and the two elements are r * cospi(2 u2) and r * sinpi(2 u2) by the accurate library functions.
 * |z| <= 5.77 by construction; u1 = 1 gives an exact 0.  Any n > 0 and any 4-byte aligned out; nothing is written outside
 * [0, n).  Takes BG_BIND_RNG_OFFSET as bg_uniform_f32 does. */
int bg_normal_f32(float* out, size_t n, uint64_t seed, uint64_t offset, void* stream);

/* ---- step programs: the step-level entry points of SURVEY.md 8b (bg_dstep / bg_gstep) -----------------------------------
 * The reference runs one Python pass over its TF ops per batch (wgan.py:86-114: discriminator_step :132-151, generator_step
 * :159-172).  With static shapes and caller-owned persistent buffers the launch list of such a step is the same every batch, so
 * it is recorded ONCE and replayed with ONE call:
 *   bg_program_record_begin(p); ...the entry points above, exactly as the eager step calls them...; bg_program_record_end(p);
 * While recording, every kernel launch of the calling thread is executed AND appended to `p` as (kernel, grid, block, LDS bytes,
 * a by-value copy of every kernel argument).  bg_program_replay(p, first, last, stream) issues nodes [first, last) (last < 0 =
 * all) on `stream` -- no geometry checks, tap tables, grid planning or host language in between.  What changes per step:
 *   - the optimisers' learning rates, the weight average's w and the RNG counter offsets: announce bg_program_bind_next(what, slot)
 *     right before the call that owns the argument; the recorded launch then re-reads slots_f64[slot] (BG_BIND_ADAM_LR,
 *     BG_BIND_OPT_LR, BG_BIND_EMA_W) / slots_u64[slot] (BG_BIND_RNG_OFFSET) before every replay.  The slot arrays belong to the program and are written directly by the host.
 *   - the blur taps' VALUES live in a caller-owned device buffer the host refreshes in stream order; a changed tap COUNT selects
 *     other kernels and needs a newly recorded program (the host keeps one per count).
 *   - collectives (data parallel) are the host's: it splits the replay at the node indices bg_program_size() returned when the
 *     collective was issued during recording.
 * Every device pointer seen while recording must stay valid for the life of the program (the host keeps the tensors alive).
 * bg_dstep / bg_gstep replay a whole program: one call per discriminator_step / generator_step.
 * bg_program_graph_launch: the same node range as one hipGraph (kernel nodes in a linear chain, bound arguments refreshed with
 * hipGraphExecKernelNodeSetParams); with bg_prof_enable(1) it falls back to the node-by-node replay.
 * Profiling brackets travel with the program: a replay under bg_prof_enable(1) yields the same records as the eager step.
 * Synchronisation: no call of this section waits for the device, with ONE exception -- destroying, evicting or re-recording a
 * program that has been launched in graph form (bg_program_destroy, bg_program_record_begin) waits for the STREAM of its last
 * bg_program_graph_launch (hipStreamSynchronize, never hipDeviceSynchronize) before the executable graphs are freed.  The
 * node-by-node replay (the default) never synchronises.
 * A binding that does not fit the launch it was announced for (wrong argument size, no launch at all) fails
 * bg_program_record_end: a silently dropped one would replay the recording step's value for ever. */
typedef struct bg_program bg_program;
#define BG_BIND_ADAM_LR 1     /* bg_adam_f32: lr_t <- (float) slots_f64[slot]                         */
#define BG_BIND_RNG_OFFSET 2  /* bg_uniform_f32, bg_keep_mask_u8, bg_normal_f32: offset <- slots_u64[slot] */
#define BG_BIND_OPT_LR 3      /* bg_sgd_f32, bg_rmsprop_f32: lr, bg_adam_amsgrad_f32: lr_t <- (float) slots_f64[slot] */
#define BG_BIND_EMA_W 4       /* bg_ema_f32: w <- (float) slots_f64[slot]                              */
int bg_program_create(bg_program** out, int n_slots);
int bg_program_destroy(bg_program* p);
int bg_program_record_begin(bg_program* p);
int bg_program_record_end(bg_program* p);
int bg_program_size(const bg_program* p);       /* nodes so far (launches + profiling brackets): replay range boundaries */
int bg_program_launches(const bg_program* p);   /* kernel launches recorded                                               */
int bg_program_binds(const bg_program* p);      /* bound arguments recorded                                               */
int bg_program_bind_next(int what, int slot);
double* bg_program_slots_f64(bg_program* p);
uint64_t* bg_program_slots_u64(bg_program* p);
int bg_program_replay(bg_program* p, int first, int last, void* stream);
int bg_program_graph_launch(bg_program* p, int first, int last, void* stream);
int bg_dstep(bg_program* p, void* stream);      /* wgan.py:132-151 as recorded */
int bg_gstep(bg_program* p, void* stream);      /* wgan.py:159-172 as recorded */

/* ---- data-parallel exchange step (the reference never ran multi-GPU, demo_mnist.py:116) --------
 * One process per GPU.  Rank 0 makes an id and hands its BG_COMM_ID_BYTES bytes to the other ranks over the host's
 * own channel (env, file, torch.distributed store ...); every rank then calls bg_comm_init with the HIP device it
 * trains on current.  bg_allreduce_sum_f32 is the step's only collective: in-place SUM of a flat fp32 gradient range
 * over RCCL (xGMI inside a node), asynchronous on `stream`.  RCCL is loaded on first use (BGAN_RCCL_LIB overrides
 * the library name); BG_ERR_RCCL when it is absent or a call fails. */
#define BG_COMM_ID_BYTES 128
typedef struct bg_comm bg_comm;
int bg_comm_unique_id(unsigned char* id_out);
int bg_comm_init(bg_comm** out, int rank, int nranks, const unsigned char* id_bytes);
/* One communicator may be driven from TWO streams (the step issues its bucketed gradient reductions on a private stream and the
 * SyncBN statistics exchanges in line on the compute stream): the calls are then ordered by RCCL in ISSUE order on the host, so
 * every rank must issue them in the same order (the step program guarantees it); a host that cannot should keep to one stream. */
int bg_allreduce_sum_f32(bg_comm* comm, float* buf_d, size_t n, void* stream);
/* ranks and own rank as the communicator itself reports them (ncclCommCount / ncclCommUserRank): evidence for a bench line
   that the collective really ran over N peers (bench.py --gpus N "rccl_nranks"). */
int bg_comm_query(bg_comm* comm, int* nranks, int* rank);
int bg_comm_destroy(bg_comm* comm);

#ifdef __cplusplus
}
#endif
#endif /* BGAN_H */
