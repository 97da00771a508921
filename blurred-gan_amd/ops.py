"""Tensor-level wrappers over the C ABI (include/bgan.h).  torch is only the container: every call
hands raw device pointers + torch's current HIP stream to libbgan_hip.so.  Nothing here computes
with torch ops, and nothing falls back to the CPU."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, program
from ._lib import Epilogue, EPI_NONE, EPI_BIAS_LRELU, EPI_MUL_GRAD, EPI_TANH, EPI_AFFINE_LRELU, check

LRELU_ALPHA = 0.3


_dev_index = None          # device the last launch's tensors were verified against (refreshed whenever a tensor disagrees)
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_get_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """Raw handle of torch's CURRENT stream on the CURRENT device (one process per GPU; `_ptr` has checked that every
    operand lives there).  The raw-stream query is a single C call; ``torch.cuda.current_stream()`` builds a Python object
    per call and was a third of the host time of a step."""
    if _raw_stream is None or _get_device is None:
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cur = _get_device()
    if _dev_index is not None and cur != _dev_index:
        raise BgDeviceError(f"operands live on cuda:{_dev_index} but the current device is cuda:{cur}")
    return _raw_stream(cur)            # a plain int: the bindings declare the parameter as c_void_p and ctypes converts


def _ptr(t):
    """Raw device address of a contiguous tensor that lives on the process's current device.  A CPU tensor or a tensor of
    another GPU raises: the kernels are launched on the current device's stream and must never see foreign pointers."""
    global _dev_index
    if t is None:
        return None
    d = t.get_device()
    if d != _dev_index:
        if d < 0:
            raise BgDeviceError("tensor must live on the GPU (cuda/ROCm device); the HIP path has no CPU fallback")
        cur = torch.cuda.current_device()
        if d != cur:
            raise BgDeviceError(f"tensor lives on cuda:{d} but the current device is cuda:{cur}: call "
                                "torch.cuda.set_device(local_rank) before building the model (one process per GPU)")
        _dev_index = cur
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous")
    if program.active() is not None:
        program.active().keep.append(t)      # a step program holds this address: the tensor lives as long as the program
    return t.data_ptr()                # a plain int (c_void_p parameter): one Python object less per operand and launch


class BgDeviceError(RuntimeError):
    pass


def _f32(*ts):
    for t in ts:
        if t is not None and t.dtype != torch.float32:
            raise ValueError(f"expected float32, got {t.dtype}")


def same_out(n, s):
    return -(-n // s)


def conv2d_splitk_workspace_bytes(bwd_data, B, H, W, Cin, Cout, ksize, stride):
    return _lib.load().bg_conv2d_splitk_workspace_bytes(int(bwd_data), B, H, W, Cin, Cout, ksize, stride)


def epilogue(mode=EPI_NONE, bias=None, ref=None, keep=None, alpha=LRELU_ALPHA, scale=1.0, ws=None, keep_elems=0, stats=None):
    e = Epilogue()
    e.keep_elems = int(keep_elems)
    e.stats = stats.data_ptr() if stats is not None else None
    e.stats_capacity = stats.numel() if stats is not None else 0
    e._rows = C.c_int(0)                    # out: rows of `stats` the conv call wrote (conv2d_stats_rows(e))
    e.stats_rows = C.pointer(e._rows) if stats is not None else None
    e.splitk_ws = ws.data_ptr() if ws is not None else None
    e.splitk_ws_bytes = ws.numel() * ws.element_size() if ws is not None else 0
    e.mode = mode
    e.bias = bias.data_ptr() if bias is not None else None
    e.ref = ref.data_ptr() if ref is not None else None
    e.keep = keep.data_ptr() if keep is not None else None
    e.alpha, e.scale = alpha, scale
    e._hold = (bias, ref, keep, ws, stats)  # keep the tensors alive for the duration of the launch call
    return e


# ------------------------------------------------------------------ blur
def blur_policy(sigma, H, W):
    ks, se, nt = C.c_float(), C.c_float(), C.c_int()
    check(_lib.load().bg_blur_policy(float(sigma), H, W, C.byref(ks), C.byref(se), C.byref(nt)), "bg_blur_policy")
    return ks.value, se.value, nt.value


def gauss_kernel_1d(sigma_eff, kernel_size):
    buf = (C.c_float * 1024)()
    n = C.c_int()
    check(_lib.load().bg_gauss_kernel_1d(float(sigma_eff), float(kernel_size), buf, 1024, C.byref(n)), "bg_gauss_kernel_1d")
    return [buf[i] for i in range(n.value)]


def blur_workspace_bytes(B, H, W, Cc, T):
    return _lib.load().bg_blur_workspace_bytes(B, H, W, Cc, T)


def blur_nhwc(x, y, taps_d, n_taps, tmp=None):
    _f32(x, y, taps_d)
    B, H, W, Cc = x.shape
    assert y.shape == x.shape and taps_d.numel() >= n_taps
    check(_lib.load().bg_blur_nhwc_f32(_ptr(x), _ptr(y), B, H, W, Cc, _ptr(taps_d), n_taps, _ptr(tmp), _stream()), "bg_blur_nhwc_f32")
    return y


def blur3_lerp_supported(B, H, W, Cc, n_taps):
    return bool(_lib.load().bg_blur3_lerp_supported(B, H, W, Cc, n_taps))


def blur3_lerp(f, r, alpha_b, y3, taps_d, n_taps):
    """y3 = [blur(f); blur(r); blur(r + alpha (f - r))] in one launch (include/bgan.h bg_blur3_lerp_nhwc_f32)."""
    _f32(f, r, alpha_b, y3, taps_d)
    B, H, W, Cc = f.shape
    assert r.shape == f.shape and tuple(y3.shape) == (3 * B, H, W, Cc) and alpha_b.numel() == B
    check(_lib.load().bg_blur3_lerp_nhwc_f32(_ptr(f), _ptr(r), _ptr(alpha_b), _ptr(y3), B, H, W, Cc, _ptr(taps_d), n_taps, _stream()),
          "bg_blur3_lerp_nhwc_f32")
    return y3


# ------------------------------------------------------------------ conv family
# conv math modes of the forward / data gradient (include/bgan.h bg_conv_math): "fp32" is the plain entry point, exactly;
# "bf16x6" the opt-in split-bf16 kernel on the geometries of its dispatch table (the rest of such a call runs fp32)
CONV_MATH = {"fp32": 0, "bf16x6": 1}


def conv_math_code(math):
    """The bg_conv_math code of a mode name; ValueError for anything else."""
    if not isinstance(math, str) or math not in CONV_MATH:
        raise ValueError(f"conv math {math!r}: expected one of {sorted(CONV_MATH)}")
    return CONV_MATH[math]


def conv2d_math_taken(bwd_data, B, H, W, Cin, Cout, ksize, stride, math):
    """True when a call of that geometry in mode ``math`` runs the split-bf16 kernel (bg_conv2d_math_taken)."""
    return bool(_lib.load().bg_conv2d_math_taken(int(bwd_data), B, H, W, Cin, Cout, ksize, stride, conv_math_code(math)))


def conv2d_fwd(x, wT, y, ksize, stride, epi=None, math="fp32"):
    """x [B,H,W,Cin], wT [k*k,Cout,Cin] -> y [B,Ho,Wo,Cout]."""
    code = conv_math_code(math)
    _f32(x, wT, y)
    B, H, W, Cin = x.shape
    Cout = y.shape[3]
    assert wT.numel() == ksize * ksize * Cin * Cout, (wT.shape, Cin, Cout)
    assert tuple(y.shape) == (B, same_out(H, stride), same_out(W, stride), Cout), (x.shape, y.shape)
    e = C.byref(epi) if epi is not None else None
    if code == 0:
        check(_lib.load().bg_conv2d_fwd(_ptr(x), _ptr(wT), _ptr(y), B, H, W, Cin, Cout, ksize, stride, e, _stream()), "bg_conv2d_fwd")
    else:
        check(_lib.load().bg_conv2d_fwd_math(_ptr(x), _ptr(wT), _ptr(y), B, H, W, Cin, Cout, ksize, stride, e, _stream(), code),
              "bg_conv2d_fwd_math")
    return y


def conv2d_bwd_data(dy, w, dx, ksize, stride, epi=None, math="fp32"):
    """dy [B,Ho,Wo,Cout], w [k*k,Cin,Cout] -> dx [B,H,W,Cin]."""
    code = conv_math_code(math)
    _f32(dy, w, dx)
    B, H, W, Cin = dx.shape
    Cout = dy.shape[3]
    assert w.numel() == ksize * ksize * Cin * Cout
    assert tuple(dy.shape) == (B, same_out(H, stride), same_out(W, stride), Cout), (dy.shape, dx.shape)
    e = C.byref(epi) if epi is not None else None
    if code == 0:
        check(_lib.load().bg_conv2d_bwd_data(_ptr(dy), _ptr(w), _ptr(dx), B, H, W, Cin, Cout, ksize, stride, e, _stream()),
              "bg_conv2d_bwd_data")
    else:
        check(_lib.load().bg_conv2d_bwd_data_math(_ptr(dy), _ptr(w), _ptr(dx), B, H, W, Cin, Cout, ksize, stride, e, _stream(), code),
              "bg_conv2d_bwd_data_math")
    return dx


def conv2d_bwd_filter_workspace_bytes(B, H, W, Cin, Cout, ksize, stride):
    return _lib.load().bg_conv2d_bwd_filter_workspace_bytes(B, H, W, Cin, Cout, ksize, stride)


def conv2d_bwd_filter(x, dy, dw, ksize, stride, beta=0.0, scale=1.0, ws=None):
    """x [B,H,W,Cin], dy [B,Ho,Wo,Cout] -> dw [k,k,Cin,Cout] = beta*dw + scale*grad."""
    _f32(x, dy, dw)
    B, H, W, Cin = x.shape
    Cout = dy.shape[3]
    assert dw.numel() == ksize * ksize * Cin * Cout
    assert tuple(dy.shape[:3]) == (B, same_out(H, stride), same_out(W, stride))
    wsb = ws.numel() * ws.element_size() if ws is not None else 0
    check(_lib.load().bg_conv2d_bwd_filter(_ptr(x), _ptr(dy), _ptr(dw), B, H, W, Cin, Cout, ksize, stride, beta, scale,
                                           _ptr(ws), wsb, _stream()), "bg_conv2d_bwd_filter")
    return dw


def transpose_last2(src, dst, T, R, Cc):
    _f32(src, dst)
    assert src.numel() == T * R * Cc == dst.numel()
    check(_lib.load().bg_transpose_last2(_ptr(src), _ptr(dst), T, R, Cc, _stream()), "bg_transpose_last2")
    return dst


def transpose_last2_batched(src_base, dst_base, desc, n, total_tiles):
    """desc: int32 device tensor [n, 6] = (src_off, dst_off, T, R, C, first_tile); see include/bgan.h."""
    _f32(src_base, dst_base)
    assert desc.dtype == torch.int32 and desc.is_contiguous() and desc.numel() == 6 * n
    check(_lib.load().bg_transpose_last2_batched(_ptr(src_base), _ptr(dst_base), _ptr(desc), n, total_tiles, _stream()),
          "bg_transpose_last2_batched")
    return dst_base


# ------------------------------------------------------------------ dense / reductions / BN
def gemm(A, Bm, Cm, M, N, K, transA=False, transB=False, bias=None, beta=0.0, scale=1.0):
    _f32(A, Bm, Cm, bias)
    assert A.numel() == M * K and Bm.numel() == K * N and Cm.numel() == M * N
    check(_lib.load().bg_gemm_f32(_ptr(A), _ptr(Bm), _ptr(Cm), M, N, K, int(transA), int(transB), _ptr(bias), beta, scale,
                                  _stream()), "bg_gemm_f32")
    return Cm


def colsum_workspace_bytes(M, N):
    return _lib.load().bg_colsum_workspace_bytes(M, N)


def colsum(x, out, M, N, ws, square=False, beta=0.0, scale=1.0):
    _f32(x, out)
    assert x.numel() == M * N and out.numel() == N
    check(_lib.load().bg_colsum_f32(_ptr(x), _ptr(out), M, N, int(square), beta, scale, _ptr(ws),
                                    ws.numel() * ws.element_size(), _stream()), "bg_colsum_f32")
    return out


def bn_workspace_bytes(M, Cc):
    return _lib.load().bg_bn_workspace_bytes(M, Cc)


def bn_train_fwd(x, y, M, Cc, gamma, beta, moving_mean, moving_var, save_mean, save_inv, ws, eps=1e-3, momentum=0.99,
                 unbiased=True, lrelu_alpha=LRELU_ALPHA):
    _f32(x, y, gamma, beta, save_mean, save_inv)
    assert x.numel() == M * Cc == y.numel()
    check(_lib.load().bg_bn_train_fwd(_ptr(x), _ptr(y), M, Cc, _ptr(gamma), _ptr(beta), _ptr(moving_mean), _ptr(moving_var),
                                      _ptr(save_mean), _ptr(save_inv), eps, momentum, int(unbiased), lrelu_alpha, _ptr(ws),
                                      ws.numel() * ws.element_size(), _stream()), "bg_bn_train_fwd")
    return y


def conv2d_stats_rows(epi):
    """Rows of epilogue(stats=...) that the conv2d_fwd / conv2d_bwd_data call given ``epi`` wrote (0: that geometry took a
    kernel without the statistics epilogue -- run the normal statistics pass).  Returned through the call's own epilogue."""
    return epi._rows.value if epi is not None and epi.stats else 0


def bn_train_fwd_partials(partial, nrows, x, y, M, Cc, gamma, beta, moving_mean, moving_var, save_mean, save_inv, eps=1e-3, momentum=0.99,
                          unbiased=True, lrelu_alpha=LRELU_ALPHA):
    _f32(x, y, partial)
    assert x.numel() == M * Cc == y.numel() and partial.numel() >= nrows * 2 * Cc
    check(_lib.load().bg_bn_train_fwd_partials(_ptr(partial), nrows, _ptr(x), _ptr(y), M, Cc, _ptr(gamma), _ptr(beta), _ptr(moving_mean),
                                               _ptr(moving_var), _ptr(save_mean), _ptr(save_inv), eps, momentum, int(unbiased), lrelu_alpha,
                                               _stream()), "bg_bn_train_fwd_partials")
    return y


def bn_sums_from_partials(partial, nrows, Cc, sums):
    check(_lib.load().bg_bn_sums_from_partials(_ptr(partial), nrows, Cc, _ptr(sums), _stream()), "bg_bn_sums_from_partials")
    return sums


def bn_infer_fwd(x, y, M, Cc, gamma, beta, moving_mean, moving_var, eps=1e-3, lrelu_alpha=LRELU_ALPHA):
    _f32(x, y)
    assert x.numel() == M * Cc == y.numel()
    check(_lib.load().bg_bn_infer_fwd(_ptr(x), _ptr(y), M, Cc, _ptr(gamma), _ptr(beta), _ptr(moving_mean), _ptr(moving_var),
                                      eps, lrelu_alpha, _stream()), "bg_bn_infer_fwd")
    return y


def bn_train_bwd(dy, y, x, dx, M, Cc, gamma, save_mean, save_inv, dgamma, dbeta, ws, lrelu_alpha=LRELU_ALPHA, beta=None):
    """``y`` may be None when ``beta`` is given: the activation's sign is re-derived from ``x`` (bit-identical, one tensor less per
    pass; include/bgan.h at bg_bn_train_bwd).  The same holds for bn_bwd_stats / bn_bwd_apply."""
    _f32(dy, x, dx) if y is None else _f32(dy, y, x, dx)
    assert dy.numel() == M * Cc == dx.numel()
    check(_lib.load().bg_bn_train_bwd(_ptr(dy), _ptr(y), _ptr(x), _ptr(dx), M, Cc, _ptr(gamma), _ptr(beta), _ptr(save_mean), _ptr(save_inv),
                                      _ptr(dgamma), _ptr(dbeta), lrelu_alpha, _ptr(ws), ws.numel() * ws.element_size(),
                                      _stream()), "bg_bn_train_bwd")
    return dx


def bn_fold(gamma, beta, moving_mean, moving_var, eps, scale_out, shift_out):
    check(_lib.load().bg_bn_fold_f32(_ptr(gamma), _ptr(beta), _ptr(moving_mean), _ptr(moving_var), eps, gamma.numel(), _ptr(scale_out),
                                     _ptr(shift_out), _stream()), "bg_bn_fold_f32")


FOLD_MAX = 8


def bn_fold_many(layers):
    """``layers``: up to FOLD_MAX tuples (gamma, beta, moving_mean, moving_var, eps, scale_out, shift_out) folded in ONE launch."""
    import ctypes as C
    n = len(layers)
    assert 0 < n <= FOLD_MAX
    P = C.c_void_p * n
    cols = [P(*[_ptr(l[j]) for l in layers]) for j in (0, 1, 2, 3, 5, 6)]
    eps = (C.c_float * n)(*[float(l[4]) for l in layers])
    cs = (C.c_int * n)(*[int(l[0].numel()) for l in layers])
    check(_lib.load().bg_bn_fold_many_f32(n, cols[0], cols[1], cols[2], cols[3], eps, cs, cols[4], cols[5], _stream()),
          "bg_bn_fold_many_f32")


def bn_stats(x, M, Cc, sums, ws):
    check(_lib.load().bg_bn_stats_f32(_ptr(x), M, Cc, _ptr(sums), _ptr(ws), ws.numel() * ws.element_size(), _stream()), "bg_bn_stats_f32")
    return sums


def bn_finalize(sums, M_total, Cc, save_mean, save_inv, moving_mean, moving_var, eps=1e-3, momentum=0.99, unbiased=True):
    check(_lib.load().bg_bn_finalize_f32(_ptr(sums), M_total, Cc, _ptr(save_mean), _ptr(save_inv), _ptr(moving_mean), _ptr(moving_var),
                                         eps, momentum, int(unbiased), _stream()), "bg_bn_finalize_f32")


def bn_apply(x, y, M, Cc, gamma, beta, mean, inv, lrelu_alpha=LRELU_ALPHA):
    check(_lib.load().bg_bn_apply_f32(_ptr(x), _ptr(y), M, Cc, _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(inv), lrelu_alpha, _stream()),
          "bg_bn_apply_f32")
    return y


def bn_finalize_apply(sums, M_total, x, y, M, Cc, gamma, beta, save_mean, save_inv, moving_mean, moving_var, eps=1e-3, momentum=0.99,
                      unbiased=True, lrelu_alpha=LRELU_ALPHA):
    check(_lib.load().bg_bn_finalize_apply_f32(_ptr(sums), M_total, _ptr(x), _ptr(y), M, Cc, _ptr(gamma), _ptr(beta), _ptr(save_mean),
                                               _ptr(save_inv), _ptr(moving_mean), _ptr(moving_var), eps, momentum, int(unbiased), lrelu_alpha,
                                               _stream()), "bg_bn_finalize_apply_f32")
    return y


def bn_bwd_stats(dy, y, x, M, Cc, save_mean, save_inv, sums, ws, lrelu_alpha=LRELU_ALPHA, gamma=None, beta=None):
    check(_lib.load().bg_bn_bwd_stats_f32(_ptr(dy), _ptr(y), _ptr(x), M, Cc, _ptr(gamma), _ptr(beta), _ptr(save_mean), _ptr(save_inv), lrelu_alpha, _ptr(sums),
                                          _ptr(ws), ws.numel() * ws.element_size(), _stream()), "bg_bn_bwd_stats_f32")
    return sums


def bn_bwd_apply(dy, y, x, dx, M, M_total, Cc, gamma, save_mean, save_inv, sums, lrelu_alpha=LRELU_ALPHA, beta=None):
    check(_lib.load().bg_bn_bwd_apply_f32(_ptr(dy), _ptr(y), _ptr(x), _ptr(dx), M, M_total, Cc, _ptr(gamma), _ptr(beta), _ptr(save_mean),
                                          _ptr(save_inv), _ptr(sums), lrelu_alpha, _stream()), "bg_bn_bwd_apply_f32")
    return dx


def bn_param_grads(sums, Cc, scale, dgamma, dbeta):
    check(_lib.load().bg_bn_param_grads_f32(_ptr(sums), Cc, scale, _ptr(dgamma), _ptr(dbeta), _stream()), "bg_bn_param_grads_f32")


# ------------------------------------------------------------------ layer normalisation (include/bgan.h "layer normalisation")
class layernorm:
    """The LayerNormalization kernels.  A namespace, not module-level functions: the engine-trace maker (tests/golden) replaces
    every public FUNCTION of this module by a recorder from a list it holds and refuses one it does not know; these calls are
    recorded by the layer normalisation tests' own recorder instead."""

    @staticmethod
    def route(Cc):
        """How the kernels lay a row of ``Cc`` channels over a wave: dict(vec, lanes, regs, chunks, rows_per_workgroup)."""
        v = [C.c_int() for _ in range(4)]
        check(_lib.load().bg_ln_route(int(Cc), *[C.byref(x) for x in v]), "bg_ln_route")
        vec, lanes, regs, chunks = (x.value for x in v)
        return dict(vec=vec, lanes=lanes, regs=regs, chunks=chunks, rows_per_workgroup=4 * (64 // lanes))

    @staticmethod
    def workspace_bytes(R, Cc):
        return _lib.load().bg_ln_workspace_bytes(R, Cc)

    @staticmethod
    def _ws_bytes(ws):
        return 0 if ws is None else ws.numel() * ws.element_size()

    @staticmethod
    def fwd(z, a, R, Cc, gamma, beta, mu, r, eps=1e-3, lrelu_alpha=LRELU_ALPHA, keep=None, scale=1.0, keep_elems=0):
        """a = Dropout(LeakyReLU(LayerNorm(z))) over the rows of z [R, Cc]; saves the rows' mean and 1 / sqrt(var + eps)."""
        _f32(z, a, gamma, beta, mu, r)
        assert z.numel() == R * Cc == a.numel() and gamma.numel() == Cc == beta.numel() and mu.numel() >= R and r.numel() >= R
        assert keep is None or (keep.dtype == torch.uint8 and keep.numel() >= (keep_elems or R * Cc))
        check(_lib.load().bg_ln_fwd_f32(_ptr(z), _ptr(a), R, Cc, _ptr(gamma), _ptr(beta), eps, lrelu_alpha, _ptr(keep), scale, int(keep_elems),
                                        _ptr(mu), _ptr(r), _stream()), "bg_ln_fwd_f32")
        return a

    @staticmethod
    def bwd(g, z, dz, R, Cc, gamma, beta, mu, r, lrelu_alpha=LRELU_ALPHA, keep=None, scale=1.0, keep_elems=0, addend=None, u_out=None,
            u_rows=None, dgamma=None, dbeta=None, dw_rows=0, acc_beta=0.0, acc_scale=1.0, ws=None):
        """dz = M(gamma * u) [+ addend] with u = g * LeakyReLU' * Dropout'; ``u_out`` keeps u of rows ``u_rows`` = (lo, hi); dgamma /
        dbeta (both or neither) = acc_beta * old + acc_scale * sums over the first ``dw_rows`` rows (0: all)."""
        _f32(g, z, dz, gamma, beta, mu, r, addend, u_out, dgamma, dbeta)
        assert g.numel() == R * Cc == z.numel() == dz.numel() and (addend is None or addend.numel() == R * Cc)
        assert keep is None or (keep.dtype == torch.uint8 and keep.numel() >= (keep_elems or R * Cc))
        lo, hi = (0, R) if u_rows is None else u_rows
        assert u_out is None or u_out.numel() == (hi - lo) * Cc
        assert dgamma is None or (dgamma.numel() == Cc == dbeta.numel())
        check(_lib.load().bg_ln_bwd_f32(_ptr(g), _ptr(z), _ptr(dz), R, Cc, _ptr(gamma), _ptr(beta), _ptr(mu), _ptr(r), lrelu_alpha, _ptr(keep),
                                        scale, int(keep_elems), _ptr(addend), _ptr(u_out), lo, hi - lo, _ptr(dgamma), _ptr(dbeta), int(dw_rows),
                                        acc_beta, acc_scale, _ptr(ws), layernorm._ws_bytes(ws), _stream()), "bg_ln_bwd_f32")
        return dz

    @staticmethod
    def tangent(zdot, z, vout, R, Cc, gamma, beta, mu, r, lrelu_alpha=LRELU_ALPHA):
        """vout = LeakyReLU' * gamma * M(zdot): the gradient penalty's linearised forward through a LayerNorm stage."""
        _f32(zdot, z, vout, gamma, beta, mu, r)
        assert zdot.numel() == R * Cc == z.numel() == vout.numel()
        check(_lib.load().bg_ln_tangent_f32(_ptr(zdot), _ptr(z), _ptr(vout), R, Cc, _ptr(gamma), _ptr(beta), _ptr(mu), _ptr(r), lrelu_alpha,
                                            _stream()), "bg_ln_tangent_f32")
        return vout

    @staticmethod
    def gp_source(u, zdot, z, s, R, Cc, gamma, mu, r, dgamma, ws, acc_beta=1.0, acc_scale=1.0):
        """s = dT/dz and dgamma = acc_beta * dgamma + acc_scale * dT/dgamma of T = <u, gamma * M(zdot)> (bg_ln_gp_source_f32)."""
        _f32(u, zdot, z, s, gamma, mu, r, dgamma)
        assert u.numel() == R * Cc == zdot.numel() == z.numel() == s.numel() and dgamma.numel() == Cc
        check(_lib.load().bg_ln_gp_source_f32(_ptr(u), _ptr(zdot), _ptr(z), _ptr(s), R, Cc, _ptr(gamma), _ptr(mu), _ptr(r), _ptr(dgamma),
                                              acc_beta, acc_scale, _ptr(ws), layernorm._ws_bytes(ws), _stream()), "bg_ln_gp_source_f32")
        return s


# ------------------------------------------------------------------ pixel normalisation (include/bgan.h "pixel normalisation")
class pixelnorm:
    """The PixelNormalization kernels.  A namespace for the reason ``layernorm`` is one: the engine-trace maker knows the module's
    public functions by name; these calls are recorded by the pixel normalisation tests' own recorder."""

    @staticmethod
    def route(Cc, aligned=True):
        """How the kernels lay a row of ``Cc`` channels over a wave: dict(vec, lanes, regs, chunks, rows_per_workgroup) of a call
        whose matrices are all 16-byte aligned (``aligned=False``: of one with a misaligned view)."""
        v = (C.c_int * _lib.PIXELNORM_ROUTE_INTS)()
        check(_lib.load().bg_pixelnorm_route(int(Cc), v), "bg_pixelnorm_route")
        vec, lanes, regs, chunks = v[0:4] if aligned else v[4:8]
        return dict(vec=vec, lanes=lanes, regs=regs, chunks=chunks, rows_per_workgroup=4 * (64 // lanes))

    @staticmethod
    def fwd(x, y, R, Cc, r=None, eps=1e-8, lrelu_alpha=1.0):
        """y = a / sqrt(mean(a^2) + eps) over the rows of a = LeakyReLU(x) [R, Cc]; ``r`` keeps the rows' 1 / sqrt(...) for bwd."""
        _f32(x, y, r)
        assert x.numel() == R * Cc == y.numel() and (r is None or r.numel() >= R)
        check(_lib.load().bg_pixelnorm_fwd_f32(_ptr(x), _ptr(y), _ptr(r), R, Cc, eps, lrelu_alpha, _stream()), "bg_pixelnorm_fwd_f32")
        return y

    @staticmethod
    def bwd(g, y, r, dz, R, Cc, lrelu_alpha=1.0):
        """dz = LeakyReLU' * r * (g - y * mean(g * y)): through the normalisation and the LeakyReLU in front of it; may run in place
        (dz is g) where the route has one chunk."""
        _f32(g, y, r, dz)
        assert g.numel() == R * Cc == y.numel() == dz.numel() and r.numel() >= R
        check(_lib.load().bg_pixelnorm_bwd_f32(_ptr(g), _ptr(y), _ptr(r), _ptr(dz), R, Cc, lrelu_alpha, _stream()), "bg_pixelnorm_bwd_f32")
        return dz


# ------------------------------------------------------------------ noise inputs (include/bgan.h "noise inputs")
class noise:
    """The NoiseInjection kernels.  A namespace for the reason ``layernorm`` is one: the engine-trace maker knows the module's
    public functions by name; these calls are recorded by the noise tests' own recorder."""

    @staticmethod
    def route(Cc, aligned=True):
        """How the kernels lay a row of ``Cc`` channels over a wave: ``pixelnorm.route``'s dict, for these kernels."""
        v = (C.c_int * _lib.NOISE_ROUTE_INTS)()
        check(_lib.load().bg_noise_route(int(Cc), v), "bg_noise_route")
        vec, lanes, regs, chunks = v[0:4] if aligned else v[4:8]
        return dict(vec=vec, lanes=lanes, regs=regs, chunks=chunks, rows_per_workgroup=4 * (64 // lanes))

    @staticmethod
    def workspace_bytes(R, Cc):
        return int(_lib.load().bg_noise_grad_workspace_bytes(R, Cc))

    @staticmethod
    def add(x, noise, strength, y, R, Cc, lrelu_alpha=1.0):
        """y = LeakyReLU(x + strength[0] * noise[r]) over the rows of x [R, Cc]; ``strength`` is a device scalar; y may be x."""
        _f32(x, noise, strength, y)
        assert x.numel() == R * Cc == y.numel() and noise.numel() == R and strength.numel() == 1
        check(_lib.load().bg_noise_add_f32(_ptr(x), _ptr(noise), _ptr(strength), _ptr(y), R, Cc, lrelu_alpha, _stream()), "bg_noise_add_f32")
        return y

    @staticmethod
    def grad(dz, noise, dstrength, R, Cc, ws, beta=0.0, scale=1.0):
        """dstrength[0] = beta * old + scale * sum_r noise[r] * sum_c dz[r, c]: two launches, a fixed order, the same bits every run."""
        _f32(dz, noise, dstrength)
        assert dz.numel() == R * Cc and noise.numel() == R and dstrength.numel() == 1
        assert ws is not None and ws.numel() * ws.element_size() >= _lib.load().bg_noise_grad_workspace_bytes(R, Cc), "noise.grad: workspace too small"
        check(_lib.load().bg_noise_grad_f32(_ptr(dz), _ptr(noise), _ptr(dstrength), R, Cc, _ptr(ws), beta, scale, _stream()), "bg_noise_grad_f32")
        return dstrength


# ------------------------------------------------------------------ mapping network (include/bgan.h "mapping network")
class mapping:
    """The MappingNetwork kernels.  A namespace for the reason ``layernorm`` is one: the engine-trace maker knows the module's
    public functions by name; these calls are recorded by the mapping tests' own recorder."""

    @staticmethod
    def plan(M, N, K):
        """The tile of ``dense_lrelu`` and the workgroups of a call: dict(tile_m, tile_n, tile_k, workgroups)."""
        v = (C.c_int * _lib.DENSE_LRELU_PLAN_INTS)()
        check(_lib.load().bg_dense_lrelu_plan(int(M), int(N), int(K), v), "bg_dense_lrelu_plan")
        return dict(tile_m=v[0], tile_n=v[1], tile_k=v[2], workgroups=v[3])

    @staticmethod
    def dense_lrelu(x, W, bias, y, M, N, K, c=1.0, bias_mul=1.0, alpha=1.0):
        """y = LeakyReLU_alpha(c * (x . W) + bias_mul * bias); ``bias`` may be None; alpha = 1 is the linear case."""
        _f32(x, W, bias, y)
        assert x.numel() == M * K and W.numel() == K * N and y.numel() == M * N and (bias is None or bias.numel() == N)
        check(_lib.load().bg_dense_lrelu_f32(_ptr(x), _ptr(W), _ptr(bias), _ptr(y), M, N, K, c, bias_mul, alpha, _stream()), "bg_dense_lrelu_f32")
        return y

    @staticmethod
    def workspace_bytes(M, N):
        return int(_lib.load().bg_lrelu_bias_bwd_workspace_bytes(M, N))

    @staticmethod
    def lrelu_bias_bwd(g, y, gp, dbias, M, N, ws, alpha=LRELU_ALPHA, beta=0.0, scale=1.0):
        """gp = g * (y > 0 ? 1 : alpha) (gp may be g) and dbias = beta * old + scale * the column sums of gp, in a fixed order."""
        _f32(g, y, gp, dbias)
        assert g.numel() == M * N == y.numel() == gp.numel() and dbias.numel() == N
        check(_lib.load().bg_lrelu_bias_bwd_f32(_ptr(g), _ptr(y), _ptr(gp), _ptr(dbias), M, N, alpha, beta, scale, _ptr(ws),
                                                0 if ws is None else ws.numel() * ws.element_size(), _stream()), "bg_lrelu_bias_bwd_f32")
        return gp

    @staticmethod
    def truncate(w, w_avg, out, psi, B, U):
        """out = w_avg + psi * (w - w_avg) with the device-resident ``w_avg`` [U]; out may be w."""
        _f32(w, w_avg, out)
        assert w.numel() == B * U == out.numel() and w_avg.numel() == U
        check(_lib.load().bg_truncate_f32(_ptr(w), _ptr(w_avg), _ptr(out), psi, B, U, _stream()), "bg_truncate_f32")
        return out


# ------------------------------------------------------------------ style modulation (include/bgan.h "style modulation")
class modconv:
    """The StyleModulation kernels.  A namespace for the reason ``layernorm`` is one: the engine-trace maker knows the module's
    public functions by name; these calls are recorded by the modconv tests' own recorder."""

    @staticmethod
    def dot_plan(B, P, Cc, aligned=True):
        """How ``dot`` cuts a [B, P, Cc] call: float4 or single-float units, channel lanes per workgroup, chunks of the channel axis
        and slabs of pixels (more than one: the two-launch route with scratch)."""
        v = (C.c_int * _lib.MOD_DOT_PLAN_INTS)()
        check(_lib.load().bg_mod_dot_plan(int(B), int(P), int(Cc), v), "bg_mod_dot_plan")
        vec, lanes, chunks, slabs = v[0:4] if aligned else v[4:8]
        return dict(vec=vec, lanes=lanes, chunks=chunks, slabs=slabs)

    @staticmethod
    def dot_workspace_bytes(B, P, Cc):
        return int(_lib.load().bg_mod_dot_workspace_bytes(B, P, Cc))

    @staticmethod
    def scale(x, v, out, B, P, Cc, bias=None, lrelu_alpha=1.0):
        """out[n, p, c] = LeakyReLU(x[n, p, c] * v[n, c] (+ bias[c])); out may be x."""
        _f32(x, v, out, bias)
        assert x.numel() == B * P * Cc == out.numel() and v.numel() == B * Cc and (bias is None or bias.numel() == Cc)
        check(_lib.load().bg_mod_scale_f32(_ptr(x), _ptr(v), _ptr(bias), _ptr(out), B, P, Cc, lrelu_alpha, _stream()), "bg_mod_scale_f32")
        return out

    @staticmethod
    def dot(a, b, out, B, P, Cc, ws=None, beta=0.0, scale=1.0):
        """out[n, c] = beta * out + scale * sum_p a[n, p, c] * b[n, p, c]: a fixed order, the same bits every run."""
        _f32(a, b, out)
        assert a.numel() == B * P * Cc == b.numel() and out.numel() == B * Cc
        nb = 0 if ws is None else ws.numel() * ws.element_size()
        check(_lib.load().bg_mod_dot_f32(_ptr(a), _ptr(b), _ptr(out), B, P, Cc, _ptr(ws), nb, beta, scale, _stream()), "bg_mod_dot_f32")
        return out

    @staticmethod
    def wsq(w, q, taps, I, O, transposed=False):
        """q[i, o] = sum over the taps of w^2; w is [taps, I, O], or [taps, O, I] with ``transposed`` (a Conv2DTranspose kernel)."""
        _f32(w, q)
        assert w.numel() == taps * I * O and q.numel() == I * O
        check(_lib.load().bg_mod_wsq_f32(_ptr(w), _ptr(q), taps, I, O, int(transposed), _stream()), "bg_mod_wsq_f32")
        return q

    @staticmethod
    def wsq_grad(w, dq, dw, taps, I, O, transposed=False, scale=1.0):
        """dw += scale * 2 * w * dq, dq [I, O] broadcast over the taps of either kernel layout."""
        _f32(w, dq, dw)
        assert w.numel() == taps * I * O == dw.numel() and dq.numel() == I * O
        check(_lib.load().bg_mod_wsq_grad_f32(_ptr(w), _ptr(dq), _ptr(dw), taps, I, O, int(transposed), scale, _stream()), "bg_mod_wsq_grad_f32")
        return dw

    @staticmethod
    def demod(s, q, d, B, I, O, eps=1e-8):
        """d[n, o] = 1 / sqrt(sum_i s[n, i]^2 * q[i, o] + eps)."""
        _f32(s, q, d)
        assert s.numel() == B * I and q.numel() == I * O and d.numel() == B * O
        check(_lib.load().bg_mod_demod_f32(_ptr(s), _ptr(q), _ptr(d), B, I, O, eps, _stream()), "bg_mod_demod_f32")
        return d

    @staticmethod
    def demod_bwd(d, dd, s, q, dq, ds, B, I, O):
        """dq = -1/2 * d^3 * dd; ds[n, i] += 2 * s[n, i] * sum_o dq[n, o] * q[i, o]."""
        _f32(d, dd, s, q, dq, ds)
        assert d.numel() == dd.numel() == dq.numel() == B * O and s.numel() == ds.numel() == B * I and q.numel() == I * O
        check(_lib.load().bg_mod_demod_bwd_f32(_ptr(d), _ptr(dd), _ptr(s), _ptr(q), _ptr(dq), _ptr(ds), B, I, O, _stream()), "bg_mod_demod_bwd_f32")
        return dq, ds


# ------------------------------------------------------------------ differentiable augmentation (include/bgan.h)
class diffaug:
    """The DiffAugment kernels.  A namespace for the reason ``layernorm`` is one: the engine-trace maker knows the module's public
    functions by name; these calls are recorded by the augmentation tests' own recorder."""

    @staticmethod
    def route(H, W, Cc):
        """dict(resident, resident_floats): whether a sample of this geometry waits in LDS between its mean and its use."""
        r, f = C.c_int(), C.c_int()
        check(_lib.load().bg_diffaug_route(int(H), int(W), int(Cc), C.byref(r), C.byref(f)), "bg_diffaug_route")
        return dict(resident=bool(r.value), resident_floats=f.value)

    @staticmethod
    def plan(n, H, W, Cc, ops_mask=7):
        """What fwd / adjoint launch for this batch and mask: dict(resident, threads, grid_x, grid_y, lds_bytes) (host only)."""
        names = ("resident", "threads", "grid_x", "grid_y", "lds_bytes")
        v = [C.c_int() for _ in names]
        check(_lib.load().bg_diffaug_plan(int(n), int(H), int(W), int(Cc), int(ops_mask), *[C.byref(x) for x in v]), "bg_diffaug_plan")
        return dict(zip(names, [bool(v[0].value)] + [x.value for x in v[1:]]))

    @staticmethod
    def decode(u, H, W, ops_mask=7, translation_ratio=0.125, cutout_ratio=0.5):
        """The library's own decode of one row of eight uniforms, on the host: dict(b, s, c, ty, tx, y0, x0, cy, cx, Sy, Sx)."""
        row = (C.c_float * 8)(*[float(v) for v in u])
        bsc, geo = (C.c_float * 3)(), (C.c_int * 8)()
        check(_lib.load().bg_diffaug_decode(row, int(H), int(W), int(ops_mask), translation_ratio, cutout_ratio, bsc, geo), "bg_diffaug_decode")
        return dict(zip(("b", "s", "c", "ty", "tx", "y0", "x0", "cy", "cx", "Sy", "Sx"), [*bsc, *geo]))

    @staticmethod
    def _check(x, y, params):
        _f32(x, y, params)
        assert x.dim() == 4 and x.shape == y.shape and params.numel() == 8 * x.size(0)
        return tuple(int(v) for v in x.shape)

    @staticmethod
    def fwd(x, y, params, ops_mask, translation_ratio, cutout_ratio, linear=False):
        """y = T(x) per sample of x [n, H, W, C] from params [n, 8] (``linear``: the linear part L, without the brightness offset)."""
        n, H, W, Cc = diffaug._check(x, y, params)
        check(_lib.load().bg_diffaug_f32(_ptr(x), _ptr(y), _ptr(params), n, H, W, Cc, int(ops_mask), translation_ratio, cutout_ratio,
                                         int(bool(linear)), _stream()), "bg_diffaug_f32")
        return y

    @staticmethod
    def adjoint(dy, dx, params, ops_mask, translation_ratio, cutout_ratio):
        """dx = L^T dy per sample."""
        n, H, W, Cc = diffaug._check(dy, dx, params)
        check(_lib.load().bg_diffaug_adjoint_f32(_ptr(dy), _ptr(dx), _ptr(params), n, H, W, Cc, int(ops_mask), translation_ratio,
                                                 cutout_ratio, _stream()), "bg_diffaug_adjoint_f32")
        return dx

    # ---- the gated calls of adaptive augmentation: params [n, 12], p one float in device memory, read by the kernel itself
    @staticmethod
    def decode_gated(u, p, H, W, ops_mask=7, translation_ratio=0.125, cutout_ratio=0.5):
        """The library's decode of one row of twelve uniforms at probability ``p``, on the host: decode()'s dict (cy, cx: the box's
        extent, 0 where the cutout did not fire) plus ``fired`` = ops_mask & the gates that fired."""
        row = (C.c_float * 12)(*[float(v) for v in u])
        bsc, geo, fired = (C.c_float * 3)(), (C.c_int * 8)(), C.c_int()
        check(_lib.load().bg_diffaug_decode_gated(row, float(p), int(H), int(W), int(ops_mask), translation_ratio, cutout_ratio, bsc, geo,
                                                  C.byref(fired)), "bg_diffaug_decode_gated")
        return dict(zip(("b", "s", "c", "ty", "tx", "y0", "x0", "cy", "cx", "Sy", "Sx", "fired"), [*bsc, *geo, fired.value]))

    @staticmethod
    def _check_gated(x, y, params, p):
        _f32(x, y, params, p)
        assert x.dim() == 4 and x.shape == y.shape and params.numel() == 12 * x.size(0) and p.numel() >= 1
        return tuple(int(v) for v in x.shape)

    @staticmethod
    def fwd_gated(x, y, params, p, ops_mask, translation_ratio, cutout_ratio, linear=False):
        """y = T(x) per sample with every operation of the policy gated by params[:, 8:11] < p[0]."""
        n, H, W, Cc = diffaug._check_gated(x, y, params, p)
        check(_lib.load().bg_diffaug_gated_f32(_ptr(x), _ptr(y), _ptr(params), _ptr(p), n, H, W, Cc, int(ops_mask), translation_ratio,
                                               cutout_ratio, int(bool(linear)), _stream()), "bg_diffaug_gated_f32")
        return y

    @staticmethod
    def adjoint_gated(dy, dx, params, p, ops_mask, translation_ratio, cutout_ratio):
        """dx = L^T dy per sample, gated likewise."""
        n, H, W, Cc = diffaug._check_gated(dy, dx, params, p)
        check(_lib.load().bg_diffaug_gated_adjoint_f32(_ptr(dy), _ptr(dx), _ptr(params), _ptr(p), n, H, W, Cc, int(ops_mask), translation_ratio,
                                                       cutout_ratio, _stream()), "bg_diffaug_gated_adjoint_f32")
        return dx


# ------------------------------------------------------------------ adaptive augmentation's controller (include/bgan.h)
class ada:
    """The two controller kernels of adaptive augmentation.  A namespace for the reason ``layernorm`` is one."""
    STATS_FLOATS, STATE_FLOATS = 4, 8

    @staticmethod
    def stats(scores, stats):
        """stats[4] = {sum of sign(scores), count, 0, 0}; sign(0) = sign(NaN) = 0."""
        _f32(scores, stats)
        assert stats.numel() >= ada.STATS_FLOATS
        check(_lib.load().bg_ada_stats_f32(_ptr(scores), int(scores.numel()), _ptr(stats), _stream()), "bg_ada_stats_f32")
        return stats

    @staticmethod
    def update(stats, state, metrics_out, target, interval, inv_speed_images):
        """One step of the controller on state[8] = {p, acc_sign, acc_count, k, r_last, ...}; ``metrics_out`` (2 floats or None)
        receives {p, r_last}."""
        _f32(stats, state, metrics_out)
        assert stats.numel() >= ada.STATS_FLOATS and state.numel() >= ada.STATE_FLOATS and (metrics_out is None or metrics_out.numel() >= 2)
        check(_lib.load().bg_ada_update_f32(_ptr(stats), _ptr(state), _ptr(metrics_out), float(target), int(interval), float(inv_speed_images),
                                            _stream()), "bg_ada_update_f32")
        return state


# ------------------------------------------------------------------ minibatch standard deviation (include/bgan.h)
class mbstd:
    """The MinibatchStdDev kernels.  A namespace for the reason ``layernorm`` is one: the engine-trace maker knows the module's public
    functions by name; these calls are recorded by the minibatch standard deviation tests' own recorder."""
    CALLS = {"fwd": 0, "bwd": 1, "gp": 2}
    PLAN = ("resident", "threads", "grid_x", "grid_y", "grid_y_emit", "lds_bytes", "launches", "vecs", "trips_min", "trips_max", "head", "tail")

    @staticmethod
    def plan(N, G, P, Cc, call="fwd", offset_floats=0):
        """What ``call`` ('fwd', 'bwd', 'gp') launches for N samples in groups of G (host only): dict over mbstd.PLAN."""
        out = (C.c_int * _lib.MBSTD_PLAN_INTS)()
        check(_lib.load().bg_mbstd_plan(int(N), int(G), int(P), int(Cc), mbstd.CALLS[call], int(offset_floats), out), "bg_mbstd_plan")
        return dict(zip(mbstd.PLAN, [bool(out[0])] + list(out)[1:]))

    @staticmethod
    def workspace_bytes(N, G, P, Cc):
        return _lib.load().bg_mbstd_workspace_bytes(int(N), int(G), int(P), int(Cc))

    @staticmethod
    def _ws_bytes(ws):
        return 0 if ws is None else ws.numel() * ws.element_size()

    @staticmethod
    def _geo(x, y, G, *stats):
        """(N, P, C) of x [N, ..., C] against y [N, ..., C + 1] and the per-group buffers."""
        N, Cc = int(x.shape[0]), int(x.shape[-1])
        P = x.numel() // max(N * Cc, 1)
        assert y.numel() == N * P * (Cc + 1), (tuple(x.shape), tuple(y.shape))
        for t in stats:
            assert t.numel() >= (N // G) * P * Cc
        return N, P, Cc

    @staticmethod
    def fwd(x, y, mu, rs, f, G, eps=1e-8, ws=None):
        """y [N, ..., C + 1] = x with the group's mean standard deviation as channel C; keeps mu, rs = 1 / s per group and column, f
        per group (bg_mbstd_fwd_f32)."""
        _f32(x, y, mu, rs, f, ws)
        N, P, Cc = mbstd._geo(x, y, G, mu, rs)
        check(_lib.load().bg_mbstd_fwd_f32(_ptr(x), _ptr(y), _ptr(mu), _ptr(rs), _ptr(f), N, int(G), P, Cc, eps, _ptr(ws), mbstd._ws_bytes(ws),
                                           _stream()), "bg_mbstd_fwd_f32")
        return y

    @staticmethod
    def bwd(u, x, mu, rs, dx, q, G):
        """dx = u[..., :C] + q * k * (x - mu) * rs with q = the group's sum of u[..., C], kept in ``q`` (bg_mbstd_bwd_f32)."""
        _f32(u, x, mu, rs, dx, q)
        N, P, Cc = mbstd._geo(x, u, G, mu, rs)
        assert dx.numel() == x.numel() and q.numel() >= N // G
        check(_lib.load().bg_mbstd_bwd_f32(_ptr(u), _ptr(x), _ptr(mu), _ptr(rs), _ptr(dx), _ptr(q), N, int(G), P, Cc, _stream()), "bg_mbstd_bwd_f32")
        return dx

    @staticmethod
    def gp(d, x, mu, rs, q, vout, src, fdot, G, eps=1e-8, ws=None):
        """The penalty's tangent vout (d with fdot as channel C) and source src at the layer's primal input (bg_mbstd_gp_f32)."""
        _f32(d, x, mu, rs, q, vout, src, fdot, ws)
        N, P, Cc = mbstd._geo(x, vout, G, mu, rs)
        assert d.numel() == x.numel() == src.numel() and q.numel() >= N // G and fdot.numel() >= N // G
        check(_lib.load().bg_mbstd_gp_f32(_ptr(d), _ptr(x), _ptr(mu), _ptr(rs), _ptr(q), _ptr(vout), _ptr(src), _ptr(fdot), N, int(G), P, Cc, eps,
                                          _ptr(ws), mbstd._ws_bytes(ws), _stream()), "bg_mbstd_gp_f32")
        return vout


# ------------------------------------------------------------------ spectral normalisation (include/bgan.h "spectral normalisation")
class SpectralTable:
    """The descriptor table of one batch of wrapped layers: the rows in host memory (the calls check them before anything touches
    the device), their device copy (the kernels read it) and the workspace the table asks for."""

    def __init__(self, rows, device):
        import numpy as np
        self.host = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, _lib.SPECTRAL_DESC_INTS)
        self.n = int(self.host.shape[0])
        self.dev = torch.from_numpy(self.host.copy()).to(device)
        self.ws_bytes = spectral.workspace_bytes(self.host)
        self.ws = torch.empty(max(self.ws_bytes // 4, 4), dtype=torch.float32, device=device)


class spectral:
    """The SpectralNormalization kernels, batched over a SpectralTable.  A namespace for the reason ``layernorm`` is one: the
    engine-trace maker refuses module-level functions it does not know."""

    @staticmethod
    def route(K, N, taps=1):
        """How the kernels cut a [K, N] matrix: dict(vec, lanes, chunks, strip_rows, pass_units, ew_units, tiles, ws_floats)."""
        names = ("vec", "lanes", "chunks", "strip_rows", "pass_units", "ew_units", "tiles", "ws_floats")
        v = [C.c_int() for _ in names]
        check(_lib.load().bg_spectral_route(int(K), int(N), int(taps), *[C.byref(x) for x in v]), "bg_spectral_route")
        return {k: x.value for k, x in zip(names, v)}

    @staticmethod
    def rows(layers):
        """Table rows for ``layers`` = [dict(w_off, u_off, v_off, sigma_off, eff_off, tr_off, K, N, taps)]: the first units and the
        workspace offsets are running sums of what ``route`` gives."""
        out, pf, ef, tf, ws = [], 0, 0, 0, 0
        for l in layers:
            r = spectral.route(l["K"], l["N"], l["taps"])
            out.append([l["w_off"], l["u_off"], l["v_off"], l["sigma_off"], l["eff_off"], l["tr_off"], l["K"], l["N"], l["taps"], pf, ef, tf, ws, 0, 0, 0])
            pf, ef, tf, ws = pf + r["pass_units"], ef + r["ew_units"], tf + r["tiles"], ws + r["ws_floats"]
        return out

    @staticmethod
    def _host(rows):
        assert rows.dtype.name == "int32" and rows.flags["C_CONTIGUOUS"] and rows.shape[1] == _lib.SPECTRAL_DESC_INTS
        return rows.ctypes.data, int(rows.shape[0])

    @staticmethod
    def workspace_bytes(host_rows):
        return _lib.load().bg_spectral_workspace_bytes(*spectral._host(host_rows))

    @staticmethod
    def power(theta, state, table, sigma_only=False):
        """One power round over every layer of ``table`` (u, v, sigma in ``state``), or sigma = v^T W u alone."""
        _f32(theta, state)
        check(_lib.load().bg_spectral_power_f32(_ptr(theta), _ptr(state), _ptr(table.dev), *spectral._host(table.host), int(bool(sigma_only)),
                                                _ptr(table.ws), table.ws.numel() * 4, _stream()), "bg_spectral_power_f32")

    @staticmethod
    def scale(theta, state, eff, table):
        """eff = W / sigma, with the transposed copies of the conv kernels."""
        _f32(theta, state, eff)
        check(_lib.load().bg_spectral_scale_f32(_ptr(theta), _ptr(state), _ptr(eff), _ptr(table.dev), *spectral._host(table.host), _stream()),
              "bg_spectral_scale_f32")
        return eff

    @staticmethod
    def grad(grad, eff, state, table):
        """In place on the flat gradient buffer: dL/dW-bar -> dL/dW = (g - <g, W-bar> v u^T) / sigma."""
        _f32(grad, eff, state)
        check(_lib.load().bg_spectral_grad_f32(_ptr(grad), _ptr(eff), _ptr(state), _ptr(table.dev), *spectral._host(table.host), _ptr(table.ws),
                                               table.ws.numel() * 4, _stream()), "bg_spectral_grad_f32")
        return grad


# ------------------------------------------------------------------ equalised learning rate (include/bgan.h "equalised learning rate")
class EqlrTable:
    """The descriptor table of one batch of wrapped layers: the rows in host memory (the calls check them before anything touches
    the device) and their device copy (the kernels read it)."""

    def __init__(self, rows, device):
        import numpy as np
        self.host = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, _lib.EQLR_DESC_INTS)
        self.n = int(self.host.shape[0])
        self.dev = torch.from_numpy(self.host.copy()).to(device)


class eqlr:
    """The EqualizedLearningRate kernels, batched over an EqlrTable.  A namespace for the reason ``spectral`` is one."""

    @staticmethod
    def plan(K, N, taps=1):
        """How the kernels cut a [K, N] matrix: dict(tiles, vec, grad_units, unit_elems)."""
        names = ("tiles", "vec", "grad_units", "unit_elems")
        v = [C.c_int() for _ in names]
        check(_lib.load().bg_eqlr_plan(int(K), int(N), int(taps), *[C.byref(x) for x in v]), "bg_eqlr_plan")
        return {k: x.value for k, x in zip(names, v)}

    @staticmethod
    def rows(layers):
        """Table rows for ``layers`` = [dict(w_off, eff_off, tr_off, K, N, taps, c)]: the first units are running sums of what ``plan``
        gives, ``c`` goes in as the bits of its fp32 value."""
        import numpy as np
        out, tf, uf = [], 0, 0
        for l in layers:
            p = eqlr.plan(l["K"], l["N"], l["taps"])
            bits = int(np.array([l["c"]], dtype=np.float32).view(np.int32)[0])
            out.append([l["w_off"], l["eff_off"], l["tr_off"], l["K"], l["N"], l["taps"], tf, uf, bits, 0, 0, 0])
            tf, uf = tf + p["tiles"], uf + p["grad_units"]
        return out

    @staticmethod
    def _host(rows):
        assert rows.dtype.name == "int32" and rows.flags["C_CONTIGUOUS"] and rows.shape[1] == _lib.EQLR_DESC_INTS
        return rows.ctypes.data, int(rows.shape[0])

    @staticmethod
    def check_table(host_rows, theta_floats, eff_floats):
        """Raises what ``scale`` / ``grad`` would raise for this host table and these buffer sizes; touches no device."""
        check(_lib.load().bg_eqlr_check_table(*eqlr._host(host_rows), int(theta_floats), int(eff_floats)), "bg_eqlr_check_table")

    @staticmethod
    def scale(theta, eff, table):
        """eff = c * W per layer, with the transposed copies of the conv kernels."""
        _f32(theta, eff)
        check(_lib.load().bg_eqlr_scale_f32(_ptr(theta), theta.numel(), _ptr(eff), eff.numel(), _ptr(table.dev), *eqlr._host(table.host), _stream()),
              "bg_eqlr_scale_f32")
        return eff

    @staticmethod
    def grad(grad, table):
        """In place on the flat gradient buffer: dL/dW_eff -> dL/dW = c * dL/dW_eff over each wrapped kernel's segment."""
        _f32(grad)
        check(_lib.load().bg_eqlr_grad_f32(_ptr(grad), grad.numel(), _ptr(table.dev), *eqlr._host(table.host), _stream()), "bg_eqlr_grad_f32")
        return grad


# ------------------------------------------------------------------ pointwise / losses / optimisers / rng
def lerp(r, f, alpha_b, out):
    B = r.shape[0]
    n_per = r.numel() // B
    check(_lib.load().bg_lerp_f32(_ptr(r), _ptr(f), _ptr(alpha_b), _ptr(out), B, n_per, _stream()), "bg_lerp_f32")
    return out


def row_norm(g, out_b):
    B = g.shape[0]
    check(_lib.load().bg_row_norm_f32(_ptr(g), _ptr(out_b), B, g.numel() // B, _stream()), "bg_row_norm_f32")
    return out_b


def gp_seed(g, norm_b, coef, out, zero_norm_guard=False):
    B = g.shape[0]
    fn = _lib.load().bg_gp_seed_guarded_f32 if zero_norm_guard else _lib.load().bg_gp_seed_f32
    check(fn(_ptr(g), _ptr(norm_b), coef, _ptr(out), B, g.numel() // B, _stream()), "bg_gp_seed_f32")
    return out


def mul_grad(d, ref, out, keep=None, alpha=LRELU_ALPHA, scale=1.0):
    assert d.numel() == ref.numel() == out.numel()
    check(_lib.load().bg_mul_grad_f32(_ptr(d), _ptr(ref), _ptr(keep), alpha, scale, _ptr(out), d.numel(), _stream()), "bg_mul_grad_f32")
    return out


def tanh_bwd(dy, y, out):
    check(_lib.load().bg_tanh_bwd_f32(_ptr(dy), _ptr(y), _ptr(out), dy.numel(), _stream()), "bg_tanh_bwd_f32")
    return out


def outer(s_b, w_k, out):
    B, K = s_b.numel(), w_k.numel()
    assert out.numel() == B * K
    check(_lib.load().bg_outer_f32(_ptr(s_b), _ptr(w_k), _ptr(out), B, K, _stream()), "bg_outer_f32")
    return out


def fill(x, v):
    check(_lib.load().bg_fill_f32(_ptr(x), float(v), x.numel(), _stream()), "bg_fill_f32")
    return x


def scale_(x, v):
    check(_lib.load().bg_scale_f32(_ptr(x), float(v), x.numel(), _stream()), "bg_scale_f32")
    return x


def copy_(dst, src):
    """dst <- src through a kernel of the library (recordable into a step program)."""
    _f32(dst, src)
    assert dst.numel() == src.numel()
    check(_lib.load().bg_copy_f32(_ptr(dst), _ptr(src), dst.numel(), _stream()), "bg_copy_f32")
    return dst


def upsample2x(x, y, scale=1.0, ref=None, keep=None, alpha=LRELU_ALPHA, grad_scale=1.0):
    """y[B,2H,2W,C] = scale * nearest-neighbour 2x upsample of x[B,H,W,C]; with ``ref`` (and ``keep``) what is written is further
    multiplied by ``mul_grad``'s factor, as ``mul_grad(y, ref, y, keep, alpha, grad_scale)`` after the plain call would."""
    _f32(x, y, ref)
    B, H, W, Cc = x.shape
    assert tuple(y.shape) == (B, 2 * H, 2 * W, Cc), (tuple(x.shape), tuple(y.shape))
    assert ref is None or ref.numel() == y.numel()
    assert keep is None or (ref is not None and keep.dtype == torch.uint8 and keep.numel() == y.numel())
    check(_lib.load().bg_upsample2x_nhwc_f32(_ptr(x), _ptr(y), B, H, W, Cc, scale, _ptr(ref), _ptr(keep), alpha, grad_scale, _stream()),
          "bg_upsample2x_nhwc_f32")
    return y


def pool2x_sum(x, y, scale=1.0):
    """y[B,H,W,C] = scale * ((x00 + x01) + (x10 + x11)) over the 2x2 blocks of x[B,2H,2W,C]."""
    _f32(x, y)
    B, H, W, Cc = y.shape
    assert tuple(x.shape) == (B, 2 * H, 2 * W, Cc), (tuple(x.shape), tuple(y.shape))
    check(_lib.load().bg_pool2x_sum_nhwc_f32(_ptr(x), _ptr(y), B, H, W, Cc, scale, _stream()), "bg_pool2x_sum_nhwc_f32")
    return y


def wgangp_d_loss(fs, rs, norm_b, inv_gbs, gp_coef, e_drift, vec_scale, dfs, drs, metrics):
    B = fs.numel()
    check(_lib.load().bg_wgangp_d_loss(_ptr(fs), _ptr(rs), _ptr(norm_b), B, inv_gbs, gp_coef, e_drift, vec_scale, _ptr(dfs),
                                       _ptr(drs), _ptr(metrics), _stream()), "bg_wgangp_d_loss")


def wgan_g_loss(s, inv_gbs, ds, metrics):
    check(_lib.load().bg_wgan_g_loss(_ptr(s), s.numel(), inv_gbs, _ptr(ds), _ptr(metrics), _stream()), "bg_wgan_g_loss")


class objective:
    """The GAN-objective kernels (include/bgan.h bg_gan_loss).  A namespace for the reason ``layernorm`` is one: the engine-trace
    maker knows the module's public functions by name, and the default objective launches none of these."""

    LOSS = {"wasserstein": _lib.LOSS_WASSERSTEIN, "hinge": _lib.LOSS_HINGE, "nonsaturating": _lib.LOSS_NONSATURATING}

    @staticmethod
    def d_loss(fs, rs, norm_b, loss, inv_gbs, gp_coef, gp_target, e_drift, vec_scale, dfs, drs, metrics):
        """``wgangp_d_loss`` for the loss code ``loss`` and the penalty target ``gp_target``."""
        _f32(fs, rs, norm_b, dfs, drs, metrics)
        B = fs.numel()
        assert rs.numel() == B == dfs.numel() == drs.numel() and metrics.numel() >= 6 and (norm_b is None or norm_b.numel() == B)
        check(_lib.load().bg_gan_d_loss(_ptr(fs), _ptr(rs), _ptr(norm_b), B, int(loss), inv_gbs, gp_coef, gp_target, e_drift, vec_scale,
                                        _ptr(dfs), _ptr(drs), _ptr(metrics), _stream()), "bg_gan_d_loss")

    @staticmethod
    def g_loss(s, loss, inv_gbs, ds, metrics):
        _f32(s, ds, metrics)
        assert ds.numel() == s.numel() and metrics.numel() >= 2
        check(_lib.load().bg_gan_g_loss(_ptr(s), s.numel(), int(loss), inv_gbs, _ptr(ds), _ptr(metrics), _stream()), "bg_gan_g_loss")

    @staticmethod
    def gp_seed(g, norm_b, coef, target, out, zero_norm_guard=False):
        """out = coef * (n - target) / n * g per sample; ``out`` may be ``g``."""
        _f32(g, norm_b, out)
        B = g.shape[0]
        assert out.numel() == g.numel() and norm_b.numel() == B
        check(_lib.load().bg_gp_seed_target_f32(_ptr(g), _ptr(norm_b), coef, target, int(bool(zero_norm_guard)), _ptr(out), B,
                                                g.numel() // B, _stream()), "bg_gp_seed_target_f32")
        return out


def u8_normalize_resize(src_u8, dst):
    """uint8 NHWC -> float32 NHWC in [-1, 1], bilinear-resized to dst's spatial size (demo_celeba.py:22-35)."""
    assert src_u8.dtype == torch.uint8 and dst.dtype == torch.float32
    B, Hs, Ws, Cc = src_u8.shape
    assert dst.shape[0] == B and dst.shape[3] == Cc
    check(_lib.load().bg_u8_normalize_resize_f32(_ptr(src_u8), _ptr(dst), B, Hs, Ws, Cc, dst.shape[1], dst.shape[2], _stream()),
          "bg_u8_normalize_resize_f32")
    return dst


def u8_gather_normalize_resize(src_u8, idx, dst, flip=None):
    """dst[b] = resize(normalise(src_u8[idx[b]])), mirrored left-right where flip[b] != 0, in ONE launch: src_u8 is the
    device-resident uint8 [N,Hs,Ws,C] dataset, idx an int32 device vector of dst.shape[0] entries (repeats / any order), flip an
    optional uint8 one.  The kernel cannot check idx: the caller guarantees every entry lies in [0, N)."""
    assert src_u8.dtype == torch.uint8 and dst.dtype == torch.float32 and idx.dtype == torch.int32
    assert flip is None or flip.dtype == torch.uint8
    N, Hs, Ws, Cc = src_u8.shape
    B = dst.shape[0]
    assert dst.dim() == 4 and dst.shape[3] == Cc and idx.numel() == B and (flip is None or flip.numel() == B)
    check(_lib.load().bg_u8_gather_normalize_resize_f32(_ptr(src_u8), N, _ptr(idx), _ptr(flip), _ptr(dst), B, Hs, Ws, Cc, dst.shape[1],
                                                        dst.shape[2], _stream()), "bg_u8_gather_normalize_resize_f32")
    return dst


# ------------------------------------------------------------------ SWD metric (include/bgan.h "SWD metric")
def swd_ingest(src, dst, nhwc, scale=1.0, shift=0.0):
    """dst[B,3,H,W] = src * scale + shift from an NHWC (``nhwc``) or NCHW float32 batch of 1 or 3 channels; one channel is
    replicated three times."""
    _f32(src, dst)
    assert src.dim() == 4 and dst.dim() == 4
    B, H, W, Cc = src.shape if nhwc else (src.shape[0], src.shape[2], src.shape[3], src.shape[1])
    assert tuple(dst.shape) == (B, 3, H, W)
    check(_lib.load().bg_swd_ingest_f32(_ptr(src), _ptr(dst), B, H, W, Cc, int(bool(nhwc)), scale, shift, _stream()), "bg_swd_ingest_f32")
    return dst


def pyr_down(x, y):
    """y[..., ceil(H/2), ceil(W/2)] = pyr_down(x[..., H, W]): the host sliced_wasserstein.pyr_down bit for bit."""
    _f32(x, y)
    H, W = x.shape[-2:]
    planes = x.numel() // (H * W)
    assert y.numel() == planes * ((H + 1) // 2) * ((W + 1) // 2)
    check(_lib.load().bg_pyr_down_f32(_ptr(x), _ptr(y), planes, H, W, _stream()), "bg_pyr_down_f32")
    return y


def pyr_up(low, out, minuend=None):
    """out[..., 2h, 2w] = pyr_up(low[..., h, w]), or minuend - pyr_up(low) (``minuend`` may be ``out``)."""
    _f32(low, out, minuend)
    h, w = low.shape[-2:]
    planes = low.numel() // (h * w)
    assert out.numel() == 4 * low.numel() and (minuend is None or minuend.numel() == out.numel())
    check(_lib.load().bg_pyr_up_f32(_ptr(low), _ptr(minuend), _ptr(out), planes, h, w, _stream()), "bg_pyr_up_f32")
    return out


def swd_gather(level, cx, cy, desc, nhood, per_image):
    """desc[t, c, a, b] = level[t // per_image, c, cy[t] + b - half, cx[t] + a - half]; cx, cy: int32 device vectors whose
    entries the caller has checked to lie in [half, size - half)."""
    _f32(level, desc)
    assert cx.dtype == torch.int32 and cy.dtype == torch.int32
    B, Cc, H, W = level.shape
    total = B * per_image
    assert Cc == 3 and cx.numel() == total == cy.numel() and desc.numel() == total * 3 * nhood * nhood
    check(_lib.load().bg_swd_gather_f32(_ptr(level), _ptr(cx), _ptr(cy), _ptr(desc), B, H, W, nhood, per_image, _stream()),
          "bg_swd_gather_f32")
    return desc


def swd_standardize_workspace_bytes(rows, nhood):
    return _lib.load().bg_swd_standardize_workspace_bytes(rows, nhood)


def swd_standardize(desc, rows, nhood, ws, stats=None):
    """desc[rows, 3, nhood, nhood] <- (desc - mean) / std per channel, in place; float64 statistics (``stats``: 6 doubles)."""
    _f32(desc)
    assert desc.numel() == rows * 3 * nhood * nhood and (stats is None or (stats.dtype == torch.float64 and stats.numel() == 6))
    check(_lib.load().bg_swd_standardize_f32(_ptr(desc), rows, nhood, _ptr(stats), _ptr(ws), ws.numel() * ws.element_size(), _stream()),
          "bg_swd_standardize_f32")
    return desc


def sort_rows(x, rows, n):
    """Sorts each of the ``rows`` contiguous rows of ``n`` floats ascending, in place."""
    _f32(x)
    assert x.numel() == rows * n
    check(_lib.load().bg_sort_rows_f32(_ptr(x), rows, n, _stream()), "bg_sort_rows_f32")
    return x


def abs_diff_mean_workspace_bytes(seg, nseg):
    return _lib.load().bg_abs_diff_mean_workspace_bytes(seg, nseg)


def abs_diff_mean(a, b, seg, nseg, out, ws):
    """out[s] (float64) = mean |a - b| over segment s of ``seg`` elements."""
    _f32(a, b)
    assert a.numel() == seg * nseg == b.numel() and out.dtype == torch.float64 and out.numel() == nseg
    check(_lib.load().bg_abs_diff_mean_f32(_ptr(a), _ptr(b), seg, nseg, _ptr(out), _ptr(ws), ws.numel() * ws.element_size(), _stream()),
          "bg_abs_diff_mean_f32")
    return out


def adam(theta, m, v, g, lr_t, b1=0.9, b2=0.999, eps=1e-7):
    assert theta.numel() == m.numel() == v.numel() == g.numel()
    check(_lib.load().bg_adam_f32(_ptr(theta), _ptr(m), _ptr(v), _ptr(g), theta.numel(), lr_t, b1, b2, eps, _stream()), "bg_adam_f32")


def sgd(theta, a, g, lr, momentum=0.0, nesterov=False):
    """tf.keras.optimizers.SGD's update; ``a`` (the momentum slot) may be None when momentum == 0."""
    assert theta.numel() == g.numel() and (a is None or a.numel() == theta.numel())
    check(_lib.load().bg_sgd_f32(_ptr(theta), _ptr(a), _ptr(g), theta.numel(), lr, momentum, int(bool(nesterov)), _stream()), "bg_sgd_f32")


def rmsprop(theta, r, p, mg, g, lr, rho=0.9, momentum=0.0, eps=1e-7, centered=False):
    """tf.keras.optimizers.RMSprop's update; ``p`` (momentum) / ``mg`` (centered) may be None when unused."""
    assert theta.numel() == r.numel() == g.numel() and all(x is None or x.numel() == theta.numel() for x in (p, mg))
    check(_lib.load().bg_rmsprop_f32(_ptr(theta), _ptr(r), _ptr(p), _ptr(mg), _ptr(g), theta.numel(), lr, rho, momentum, eps,
                                     int(bool(centered)), _stream()), "bg_rmsprop_f32")


def adam_amsgrad(theta, m, v, vhat, g, lr_t, b1=0.9, b2=0.999, eps=1e-7):
    assert theta.numel() == m.numel() == v.numel() == vhat.numel() == g.numel()
    check(_lib.load().bg_adam_amsgrad_f32(_ptr(theta), _ptr(m), _ptr(v), _ptr(vhat), _ptr(g), theta.numel(), lr_t, b1, b2, eps, _stream()),
          "bg_adam_amsgrad_f32")


def ema(avg, theta, avg2, theta2, w):
    """Weight averaging (tf.train.ExponentialMovingAverage): avg -= w * (avg - theta) over a network's trainable buffer and, in
    the same launch, avg2 -= w * (avg2 - theta2) over its state buffer (both None: no second segment).  w = 1 - decay."""
    assert avg.numel() == theta.numel() and (avg2 is None) == (theta2 is None)
    n2 = 0 if avg2 is None else avg2.numel()
    assert n2 == 0 or theta2.numel() == n2
    check(_lib.load().bg_ema_f32(_ptr(avg), _ptr(theta), avg.numel(), _ptr(avg2) if n2 else None, _ptr(theta2) if n2 else None, n2, w,
                                 _stream()), "bg_ema_f32")


def _draw_offset(out, offset, counter):
    """Offset of a counter-based draw.  ``counter`` = (obj, attr): the draw starts at that host counter, which then advances by the
    Philox blocks the draw consumes; while a step program is being recorded the launch's offset is bound to the counter."""
    if counter is None:
        return offset
    obj, attr = counter
    inc = (out.numel() + 3) // 4
    offset = getattr(obj, attr)
    if program.active() is not None:
        program.active().bind_rng(obj, attr, inc)        # the recorded launch re-reads the counter before every replay
    setattr(obj, attr, offset + inc)
    return offset


def uniform(out, seed, offset=0, counter=None):
    offset = _draw_offset(out, offset, counter)
    check(_lib.load().bg_uniform_f32(_ptr(out), out.numel(), seed, offset, _stream()), "bg_uniform_f32")
    return out


class rng:
    """Draws beyond the reference's two.  A namespace for the reason ``layernorm`` is one: the engine-trace maker knows the module's
    public functions by name; these calls are recorded by the noise tests' own recorder."""

    @staticmethod
    def normal(out, seed, offset=0, counter=None):
        """N(0, 1) draws (bg_normal_f32): the layout contract, offset and counter of ``uniform``; Box-Muller inside a Philox block."""
        _f32(out)
        offset = _draw_offset(out, offset, counter)
        check(_lib.load().bg_normal_f32(_ptr(out), out.numel(), seed, offset, _stream()), "bg_normal_f32")
        return out


def keep_mask(out, keep_prob, seed, offset=0, counter=None):
    assert out.dtype == torch.uint8
    offset = _draw_offset(out, offset, counter)
    check(_lib.load().bg_keep_mask_u8(_ptr(out), out.numel(), keep_prob, seed, offset, _stream()), "bg_keep_mask_u8")
    return out


# ------------------------------------------------------------------ profiling
_ranges_on = None


class trace_range:
    """Named range on the rocprofv3 marker timeline (roctx through the C ABI).  Off unless BGAN_ROCTX=1: then the first use binds
    roctx; with the switch off (the default) entering and leaving cost one attribute test."""
    __slots__ = ("name",)

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        global _ranges_on
        if _ranges_on is None:
            import os
            _ranges_on = bool(os.environ.get("BGAN_ROCTX") == "1" and _lib.load().bg_range_enable(1))
        if _ranges_on:
            _lib.load().bg_range_push(self.name.encode())
        return self

    def __exit__(self, *exc):
        if _ranges_on:
            _lib.load().bg_range_pop()
        return False


def prof_enable(on):
    _lib.load().bg_prof_enable(int(on))


def prof_reset():
    _lib.load().bg_prof_reset()


def conv2d_useful_flops(B, H, W, Cin, Cout, k=5, stride=2):
    """Flops of a k x k SAME convolution that multiply real data (no zero-padding taps): bg_conv2d_useful_flops."""
    return float(_lib.load().bg_conv2d_useful_flops(B, H, W, Cin, Cout, k, stride))


def prof_records(with_exec=False, with_useful=False):
    """[(name, ms, algorithmic flops, algorithmic bytes)] per recorded launch; with_exec appends the flops the launch issued
    on the matrix pipe (bg_prof_get_exec), with_useful the flops that multiply real data (bg_prof_get_useful)."""
    lib = _lib.load()
    n = lib.bg_prof_count()
    out = []
    name = C.create_string_buffer(128)
    ms, fl, by, ex = C.c_float(), C.c_double(), C.c_double(), C.c_double()
    for i in range(n):
        check(lib.bg_prof_get(i, name, 128, C.byref(ms), C.byref(fl), C.byref(by)), "bg_prof_get")
        rec = (name.value.decode(), ms.value, fl.value, by.value)
        if with_exec:
            check(lib.bg_prof_get_exec(i, C.byref(ex)), "bg_prof_get_exec")
            rec = rec + (ex.value,)
        if with_useful:
            check(lib.bg_prof_get_useful(i, C.byref(ex)), "bg_prof_get_useful")
            rec = rec + (ex.value,)
        out.append(rec)
    return out


# The FIR-filtered resampling pair (fir_ops.py), under the names the rest of the package calls it by
from .fir_ops import fir_downsample2x, fir_upsample2x  # noqa: E402,F401
