"""GPU parity of the opt-in split-bf16 conv math (BG_CONV_MATH_BF16X6): forward and data gradient against the float64 oracle
with the same bounds as the fp32 kernels (tests/test_conv_gpu.py), on every geometry of that file and on the C2 layer shapes;
the epilogue modes of the step, Inf / NaN inputs, run-to-run reproducibility, and that the geometries the dispatch table names
really run the split kernel."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import np_ops as O
from helpers import dev, conv_tol
from test_conv_gpu import CASES, _data

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# celeba64 layer shapes (tools/bench_conv.py): conv input side H, W, Cin -> Cout, stride 2
C2_LAYERS = [(32, 32, 32, 64), (16, 16, 64, 128), (8, 8, 128, 256), (4, 4, 256, 512), (16, 16, 128, 256), (32, 32, 64, 128),
             (64, 64, 32, 64)]
C2_B = 256
ROWS = [0, 1, 2, 127, 128, 253, 254, 255]       # images checked against the oracle at B 256 (first / last tiles, a tile seam)


def _kernels(fn):
    from blurred_gan_amd import ops
    torch.cuda.synchronize()
    ops.prof_reset()
    ops.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        names = [r[0] for r in ops.prof_records()]
    finally:
        ops.prof_enable(False)
        ops.prof_reset()
    return out, names


def _fwd(x, w, s, epi=None, math="bf16x6"):
    from blurred_gan_amd import ops
    B, H, W, Ci = x.shape
    Co = w.shape[-1]
    wT = dev(np.transpose(w, (0, 1, 3, 2)))
    return ops.conv2d_fwd(dev(x), wT, torch.empty((B, -(-H // s), -(-W // s), Co), device="cuda"), 5, s, epi, math=math)


def _bwd(dy, w, s, hw, epi=None, math="bf16x6", out=None):
    from blurred_gan_amd import ops
    B = dy.shape[0]
    dx = out if out is not None else torch.empty((B, hw[0], hw[1], w.shape[2]), device="cuda")
    return ops.conv2d_bwd_data(dev(dy), dev(w), dx, 5, s, epi, math=math)


def _check_ran(bwd, x_shape, Co, s, names):
    from blurred_gan_amd import ops
    B, H, W, Ci = x_shape
    taken = ops.conv2d_math_taken(bwd, B, H, W, Ci, Co, 5, s, "bf16x6")
    ran = any("x6" in n for n in names)
    assert ran == taken, (names, taken)
    assert not ops.conv2d_math_taken(bwd, B, H, W, Ci, Co, 5, s, "fp32")
    return taken


@pytest.mark.parametrize("B,H,W,Ci,Co,s", CASES)
def test_conv_fwd_x6(B, H, W, Ci, Co, s):
    x, w, dy = _data(B, H, W, Ci, Co, s)
    ref = O.conv2d_fwd(x, w, s)
    y, names = _kernels(lambda: _fwd(x, w, s))
    _check_ran(0, x.shape, Co, s, names)
    np.testing.assert_allclose(y.cpu().numpy(), ref, rtol=1e-4, atol=conv_tol(25 * Ci, np.abs(ref).max()))


@pytest.mark.parametrize("B,H,W,Ci,Co,s", CASES)
def test_conv_bwd_data_x6(B, H, W, Ci, Co, s):
    x, w, dy = _data(B, H, W, Ci, Co, s, seed=1)
    ref = O.conv2d_bwd_data(dy, w, s, (H, W))
    dx, names = _kernels(lambda: _bwd(dy, w, s, (H, W)))
    _check_ran(1, x.shape, Co, s, names)
    np.testing.assert_allclose(dx.cpu().numpy(), ref, rtol=1e-4, atol=conv_tol(25 * Co, np.abs(ref).max()))


@pytest.mark.parametrize("H,W,Ci,Co", C2_LAYERS)
def test_c2_layers_x6(H, W, Ci, Co):
    """The C2 layer shapes at B 256, both directions; the oracle on a sample of the images (each image is independent)."""
    x, w, dy = _data(C2_B, H, W, Ci, Co, 2, seed=3)
    y, names = _kernels(lambda: _fwd(x, w, 2))
    taken_f = _check_ran(0, x.shape, Co, 2, names)
    ref = O.conv2d_fwd(x[ROWS], w, 2)
    np.testing.assert_allclose(y.cpu().numpy()[ROWS], ref, rtol=1e-4, atol=conv_tol(25 * Ci, np.abs(ref).max()))
    dx, names = _kernels(lambda: _bwd(dy, w, 2, (H, W)))
    taken_b = _check_ran(1, x.shape, Co, 2, names)
    ref = O.conv2d_bwd_data(dy[ROWS], w, 2, (H, W))
    np.testing.assert_allclose(dx.cpu().numpy()[ROWS], ref, rtol=1e-4, atol=conv_tol(25 * Co, np.abs(ref).max()))


def test_kernel_on_every_geometry_it_runs():
    """BG_CONV_X6_FORCE=1 (tuning aid): the split kernel on every geometry of test_conv_gpu.CASES it can run, table or not --
    M and N tails, odd maps, sub-pixel phases of different extents, stride 1 and 2, all three tile widths; and the data-gradient
    direction through the epilogue, Inf / NaN and reproducibility tests below."""
    code = r"""
import sys, numpy as np, torch
sys.path[:0] = [%r, %r]
from oracle import np_ops as O
from helpers import dev, conv_tol
from test_conv_gpu import CASES, _data
from test_conv_math_gpu import _kernels, _fwd, _bwd
n = 0
for (B, H, W, Ci, Co, s) in CASES:
    x, w, dy = _data(B, H, W, Ci, Co, s)
    y, names = _kernels(lambda: _fwd(x, w, s))
    ref = O.conv2d_fwd(x, w, s)
    np.testing.assert_allclose(y.cpu().numpy(), ref, rtol=1e-4, atol=conv_tol(25 * Ci, np.abs(ref).max()))
    n += any("x6" in k for k in names)
    dx, names = _kernels(lambda: _bwd(dy, w, s, (H, W)))
    ref = O.conv2d_bwd_data(dy, w, s, (H, W))
    np.testing.assert_allclose(dx.cpu().numpy(), ref, rtol=1e-4, atol=conv_tol(25 * Co, np.abs(ref).max()))
    n += any("x6" in k for k in names)
# the data-gradient direction (no geometry of it is in the table) through the epilogue, Inf / NaN and reproducibility checks
import test_conv_math_gpu as M
for mode in ("none_bias", "bias_lrelu_keep", "mul_grad_alias", "tanh", "affine_lrelu", "stats"):
    M.test_epilogues_x6(1, mode)
M.test_inf_nan_inputs_x6(1)
M.test_x6_is_bit_reproducible(1)
print("X6_RUNS", n)
""" % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, BG_CONV_X6_FORCE="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    n = int(r.stdout.split("X6_RUNS")[1].split()[0])
    assert n >= 12, r.stdout


# ---- epilogues, on a table geometry at a small batch (bias, LeakyReLU, dropout mask, LeakyReLU gradient, tanh, statistics)
G_EPI = (4, 32, 32, 64, 128)     # B, H, W, Cin, Cout (stride 2): the C2 G4 geometry (a table entry); forward N = 128, data gradient N = 64


def _lrelu(v, a=0.3):
    return np.where(v > 0, v, a * v)


@pytest.mark.parametrize("bwd", [0])          # bwd = 1: test_kernel_on_every_geometry_it_runs
@pytest.mark.parametrize("mode", ["none_bias", "bias_lrelu_keep", "mul_grad_alias", "tanh", "affine_lrelu", "stats"])
def test_epilogues_x6(bwd, mode):
    from blurred_gan_amd import ops
    B, H, W, Ci, Co = G_EPI
    x, w, dy = _data(B, H, W, Ci, Co, 2, seed=4)
    rng = np.random.default_rng(5)
    acc = O.conv2d_bwd_data(dy, w, 2, (H, W)) if bwd else O.conv2d_fwd(x, w, 2)
    N = acc.shape[-1]
    K = 25 * (Co if bwd else Ci)
    bias = rng.uniform(-0.5, 0.5, N).astype(np.float32)
    out = torch.full(acc.shape, 7.0, device="cuda")
    stats = None
    if mode == "none_bias":
        epi, ref = ops.epilogue(ops.EPI_NONE, bias=dev(bias)), acc + bias
    elif mode == "bias_lrelu_keep":
        keep = (rng.uniform(size=acc.shape) < 0.7).astype(np.uint8)
        ke = (acc.size // 2) // 4 * 4                 # the mask covers the leading samples only
        kflat = keep.reshape(-1).copy()
        kflat[ke:] = 1
        ref = (_lrelu(acc + bias).reshape(-1) * np.where(kflat == 1, 1 / 0.7, 0.0))
        ref[ke:] = _lrelu(acc + bias).reshape(-1)[ke:]
        ref = ref.reshape(acc.shape)
        epi = ops.epilogue(ops.EPI_BIAS_LRELU, bias=dev(bias), keep=torch.from_numpy(keep).cuda(), scale=1 / 0.7, keep_elems=ke)
    elif mode == "mul_grad_alias":
        r = rng.uniform(-1, 1, acc.shape).astype(np.float32)
        out = dev(r)                                   # ref aliases the output
        epi, ref = ops.epilogue(ops.EPI_MUL_GRAD, ref=out), acc * np.where(r > 0, 1.0, 0.3)
    elif mode == "tanh":
        epi, ref = ops.epilogue(ops.EPI_TANH, bias=dev(bias)), np.tanh(acc + bias)
    elif mode == "affine_lrelu":                       # folded inference BatchNorm: per-channel multiplier, then bias, then LeakyReLU
        mul = rng.uniform(0.5, 1.5, N).astype(np.float32)
        epi, ref = ops.epilogue(ops.EPI_AFFINE_LRELU, bias=dev(bias), ref=dev(mul)), _lrelu(acc * mul + bias)
    else:
        stats = torch.full((4096 * 2 * N,), 3.0, device="cuda")
        epi, ref = ops.epilogue(ops.EPI_NONE, stats=stats), acc
    if bwd:
        (y, names) = _kernels(lambda: _bwd(dy, w, 2, (H, W), epi, out=out))
    else:
        wT = dev(np.transpose(w, (0, 1, 3, 2)))
        (y, names) = _kernels(lambda: ops.conv2d_fwd(dev(x), wT, out, 5, 2, epi, math="bf16x6"))
    assert any("x6" in n for n in names), names
    tol = conv_tol(K, np.abs(acc).max())
    np.testing.assert_allclose(y.cpu().numpy(), ref, rtol=1e-4, atol=tol)
    if stats is not None:
        rows = ops.conv2d_stats_rows(epi)
        assert rows > 0
        part = stats[: rows * 2 * N].view(rows, 2, N).double().sum(0).cpu().numpy()
        a2 = acc.reshape(-1, N)
        np.testing.assert_allclose(part[0], a2.sum(0), rtol=1e-4, atol=tol * a2.shape[0] ** 0.5)
        np.testing.assert_allclose(part[1], (a2 ** 2).sum(0), rtol=1e-4, atol=tol * np.abs(a2).max() * a2.shape[0] ** 0.5 * 2)


@pytest.mark.parametrize("bwd", [0])
def test_inf_nan_inputs_x6(bwd):
    """Inf / NaN in the data operand: the same non-finite outputs as the fp32 kernel (no NaN made by inf - inf or inf x 0 inside
    the split), the finite outputs within the usual bound of it."""
    B, H, W, Ci, Co = G_EPI
    x, w, dy = _data(B, H, W, Ci, Co, 2, seed=6)
    w[0, 0, 0, :] = 0.5                               # weights with zero mid / lo pieces meet the Inf
    w[2, 2, :, 0] = 0.25
    if bwd:
        a = dy.copy()
        a[0, 3, 4, :] = np.inf
        a[1, 5, 5, 7] = -np.inf
        a[2, 2, 6, 9] = np.nan
        run = lambda m: _bwd(a, w, 2, (H, W), math=m)
    else:
        a = x.copy()
        a[0, 7, 8, :] = np.inf
        a[1, 10, 10, 5] = -np.inf
        a[2, 4, 12, 3] = np.nan
        run = lambda m: _fwd(a, w, 2, math=m)
    f32 = run("fp32").cpu().numpy()
    y, names = _kernels(lambda: run("bf16x6"))
    assert any("x6" in n for n in names), names
    y = y.cpu().numpy()
    assert np.isinf(f32).any() and np.isnan(f32).any()
    np.testing.assert_array_equal(np.isnan(y), np.isnan(f32))
    np.testing.assert_array_equal(np.isposinf(y), np.isposinf(f32))
    np.testing.assert_array_equal(np.isneginf(y), np.isneginf(f32))
    fin = np.isfinite(f32)
    np.testing.assert_allclose(y[fin], f32[fin], rtol=1e-4, atol=2 * conv_tol(25 * (Co if bwd else Ci), np.abs(f32[fin]).max()))


@pytest.mark.parametrize("bwd", [0])
def test_x6_is_bit_reproducible(bwd):
    H, W, Ci, Co = 32, 32, 64, 128
    x, w, dy = _data(64, H, W, Ci, Co, 2, seed=7)
    run = (lambda: _bwd(dy, w, 2, (H, W))) if bwd else (lambda: _fwd(x, w, 2))
    a, names = _kernels(run)
    assert any("x6" in n for n in names), names
    b = run()
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_fp32_mode_is_the_plain_entry_point():
    """math="fp32" is bit-identical to the call without a mode (same kernels), also through the C entry with the mode."""
    from blurred_gan_amd import ops, _lib
    import ctypes as C
    x, w, dy = _data(8, 16, 16, 64, 128, 2, seed=8)
    wT = dev(np.transpose(w, (0, 1, 3, 2)))
    xd = dev(x)
    y0 = ops.conv2d_fwd(xd, wT, torch.empty((8, 8, 8, 128), device="cuda"), 5, 2)
    y1 = torch.empty_like(y0)
    rc = _lib.load().bg_conv2d_fwd_math(xd.data_ptr(), wT.data_ptr(), y1.data_ptr(), 8, 16, 16, 64, 128, 5, 2, None,
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream), 0)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(y0, y1)
