"""Tensor-level wrappers of the FIR-filtered resampling pair (include/bgan.h "resampling": bg_fir_upsample2x_nhwc_f32 /
bg_fir_downsample2x_nhwc_f32), re-exported as ``ops.fir_upsample2x`` / ``ops.fir_downsample2x``.

They live in a module of their own because tests/golden/make_engine_trace.py lists every launch function DEFINED in ``ops`` by name
and its fixture's configurations have no filtered stage; tests/test_firsample_cpu.py records what the engine enqueues through these
two."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, ops
from ._lib import check


def _host_taps(taps):
    """(host float array, count) of a tap sequence: the library copies the values into the kernel's arguments."""
    n = len(taps)
    return (C.c_float * n)(*[float(t) for t in taps]), n


def fir_upsample2x(x, y, taps, scale=1.0, ref=None, keep=None, alpha=ops.LRELU_ALPHA, grad_scale=1.0):
    """y[B,2H,2W,C] = scale * UP_taps(x[B,H,W,C]) over H and W (``taps``: 2, 4, 6 or 8 floats); with ``ref`` (and ``keep``) what is
    written is further multiplied by ``mul_grad``'s factor, as in ``ops.upsample2x``."""
    ops._f32(x, y, ref)
    B, H, W, Cc = x.shape
    assert tuple(y.shape) == (B, 2 * H, 2 * W, Cc), (tuple(x.shape), tuple(y.shape))
    assert ref is None or ref.numel() == y.numel()
    assert keep is None or (ref is not None and keep.dtype == torch.uint8 and keep.numel() == y.numel())
    t, n = _host_taps(taps)
    check(_lib.load().bg_fir_upsample2x_nhwc_f32(ops._ptr(x), ops._ptr(y), B, H, W, Cc, t, n, scale, ops._ptr(ref), ops._ptr(keep), alpha,
                                                 grad_scale, ops._stream()), "bg_fir_upsample2x_nhwc_f32")
    return y


def fir_downsample2x(x, y, taps, scale=1.0):
    """y[B,H,W,C] = scale * DOWN_taps(x[B,2H,2W,C]) over H and W (``taps``: 2, 4, 6 or 8 floats)."""
    ops._f32(x, y)
    B, H, W, Cc = y.shape
    assert tuple(x.shape) == (B, 2 * H, 2 * W, Cc), (tuple(x.shape), tuple(y.shape))
    t, n = _host_taps(taps)
    check(_lib.load().bg_fir_downsample2x_nhwc_f32(ops._ptr(x), ops._ptr(y), B, H, W, Cc, t, n, scale, ops._stream()),
          "bg_fir_downsample2x_nhwc_f32")
    return y
