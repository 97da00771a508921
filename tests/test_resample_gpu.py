"""GPU tests of the resampling kernels (include/bgan.h "resampling": bg_upsample2x_nhwc_f32, bg_pool2x_sum_nhwc_f32; ops.upsample2x,
ops.pool2x_sum): both routes bit for bit against numpy evaluated in the same order, guard regions, adjointness, the fused
LeakyReLU' / Dropout' factor against the two-launch form, misaligned views."""
import numpy as np
import pytest
import torch

from blurred_gan_amd import ops

pytestmark = pytest.mark.gpu

# low-resolution (B, H, W, C): float4 route (C % 4 == 0), scalar route, and one case of 181 * 183 * 16 = 529 968 channel quads --
# more threads than the launch's 2048 x 256, ragged last block: the grid-stride loop takes a second trip
SHAPES = [(1, 1, 1, 4), (3, 3, 5, 4), (2, 3, 5, 20), (2, 4, 4, 16), (2, 5, 3, 3), (1, 2, 2, 1), (3, 2, 3, 6), (1, 181, 183, 64)]
SCALES = [1.0, 0.25, 0.5]
POISON = -7777.0
GUARD = 64          # floats on either side of a tensor (keeps the tensor 16-byte aligned)


def _data(kind, shape, seed):
    rng = np.random.default_rng(seed)
    if kind == "int":
        return rng.integers(-64, 65, size=shape).astype(np.float32)
    return rng.uniform(-1, 1, size=shape).astype(np.float32)


def _hi(shape):
    B, H, W, C = shape
    return (B, 2 * H, 2 * W, C)


class Guarded:
    """A device tensor of ``shape`` inside a poisoned buffer: what a kernel writes beyond the tensor shows."""

    def __init__(self, shape, dtype=torch.float32, fill=None):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), POISON if dtype == torch.float32 else 77, dtype=dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        if fill is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(fill)).to(dtype))
        self.n = n

    def guards_intact(self):
        v = POISON if self.buf.dtype == torch.float32 else 77
        return bool((self.buf[:GUARD] == v).all()) and bool((self.buf[GUARD + self.n:] == v).all())

    def np(self):
        return self.t.cpu().numpy()


def np_upsample(x, scale):
    return (np.float32(scale) * x).repeat(2, 1).repeat(2, 2)


def np_pool_sum(x, scale):
    return np.float32(scale) * ((x[:, 0::2, 0::2] + x[:, 0::2, 1::2]) + (x[:, 1::2, 0::2] + x[:, 1::2, 1::2]))


@pytest.mark.parametrize("kind", ["int", "uniform"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_both_kernels_equal_numpy_bit_for_bit(shape, kind):
    lo, hi = _data(kind, shape, 1), _data(kind, _hi(shape), 2)
    xl, xh = Guarded(shape, fill=lo), Guarded(_hi(shape), fill=hi)
    for scale in SCALES:
        yh, yl = Guarded(_hi(shape)), Guarded(shape)
        assert ops.upsample2x(xl.t, yh.t, scale) is yh.t
        assert ops.pool2x_sum(xh.t, yl.t, scale) is yl.t
        torch.cuda.synchronize()
        want_up, want_pool = np_upsample(lo, scale), np_pool_sum(hi, scale)
        assert want_up.dtype == want_pool.dtype == np.float32
        assert np.array_equal(yh.np(), want_up), (shape, kind, scale)
        assert np.array_equal(yl.np(), want_pool), (shape, kind, scale)
        assert yh.guards_intact() and yl.guards_intact()
    assert np.array_equal(xl.np(), lo) and np.array_equal(xh.np(), hi) and xl.guards_intact() and xh.guards_intact()


@pytest.mark.parametrize("shape", SHAPES[:-1], ids=lambda s: "x".join(map(str, s)))
def test_adjointness_is_exact_on_integer_data(shape):
    """<up(x), y> == <x, poolsum(y)>: every product and sum is an integer below 2^53."""
    x, y = _data("int", shape, 3), _data("int", _hi(shape), 4)
    ux, py = torch.empty(_hi(shape), device="cuda"), torch.empty(shape, device="cuda")
    ops.upsample2x(torch.from_numpy(x).cuda(), ux, 1.0)
    ops.pool2x_sum(torch.from_numpy(y).cuda(), py, 1.0)
    lhs = (ux.cpu().numpy().astype(np.float64) * y).sum()
    rhs = (x.astype(np.float64) * py.cpu().numpy()).sum()
    assert lhs == rhs and lhs == (np_upsample(x, 1.0).astype(np.float64) * y).sum()


def _ref_with_zeros(shape, seed):
    rng = np.random.default_rng(seed)
    r = rng.uniform(-1, 1, size=shape).astype(np.float32)
    z = rng.uniform(size=shape)
    r[z < 0.2] = 0.0
    r[(z >= 0.2) & (z < 0.25)] = -0.0
    assert (r == 0).any() and (r > 0).any() and (r < 0).any()
    return r


@pytest.mark.parametrize("alpha", [0.3, 0.25])
@pytest.mark.parametrize("with_keep", [False, True], ids=["nokeep", "keep"])
@pytest.mark.parametrize("shape", [(3, 3, 5, 4), (2, 3, 5, 20), (2, 4, 4, 16), (2, 5, 3, 3), (3, 2, 3, 6), (1, 181, 183, 64)],
                         ids=lambda s: "x".join(map(str, s)))
def test_fused_backward_equals_upsample_then_mul_grad(shape, with_keep, alpha):
    rng = np.random.default_rng(5)
    x = Guarded(shape, fill=_data("uniform", shape, 6))
    ref = Guarded(_hi(shape), fill=_ref_with_zeros(_hi(shape), 7))
    keep = None
    if with_keep:
        k = (rng.uniform(size=_hi(shape)) >= 0.3).astype(np.uint8)
        k[(rng.uniform(size=_hi(shape)) < 0.05) & (k == 1)] = 255            # any non-zero byte keeps
        keep = Guarded(_hi(shape), dtype=torch.uint8, fill=k)
    gs = 1.0 / 0.7
    for scale in (0.25, 1.0):
        fused, two = Guarded(_hi(shape)), Guarded(_hi(shape))
        ops.upsample2x(x.t, fused.t, scale, ref=ref.t, keep=None if keep is None else keep.t, alpha=alpha, grad_scale=gs)
        ops.upsample2x(x.t, two.t, scale)
        ops.mul_grad(two.t, ref.t, two.t, keep=None if keep is None else keep.t, alpha=alpha, scale=gs)
        torch.cuda.synchronize()
        assert torch.equal(fused.t, two.t), (shape, with_keep, alpha, scale)
        assert fused.guards_intact() and two.guards_intact()
        # and the factor itself, spelled out: (scale * x) * f, f = (ref > 0 ? 1 : alpha) [* keep ? gs : 0]
        f = np.where(ref.np() > 0, np.float32(1.0), np.float32(alpha))
        if keep is not None:
            f = np.where(keep.np() != 0, f * np.float32(gs), np.float32(0.0))
        assert np.array_equal(fused.np(), np_upsample(x.np(), scale) * f)


@pytest.mark.parametrize("shape", [(3, 3, 5, 4), (3, 2, 3, 6), (4, 2, 2, 16)], ids=lambda s: "x".join(map(str, s)))
def test_fused_backward_on_a_row_sub_range(shape):
    """The merged critic pass: rows [0, DR) with the Dropout mask (whose buffer covers those rows only), the rest without."""
    B, DR = shape[0], shape[0] - 1
    x = torch.from_numpy(_data("uniform", shape, 8)).cuda()
    ref = torch.from_numpy(_ref_with_zeros(_hi(shape), 9)).cuda()
    keep = torch.from_numpy((np.random.default_rng(10).uniform(size=(DR,) + _hi(shape)[1:]) >= 0.3).astype(np.uint8)).cuda()
    out = Guarded(_hi(shape))
    ops.upsample2x(x[:DR], out.t[:DR], 0.25, ref=ref[:DR], keep=keep, alpha=0.3, grad_scale=1.0 / 0.7)
    torch.cuda.synchronize()
    assert bool((out.t[DR:] == POISON).all())                                  # the other rows are not this launch's
    ops.upsample2x(x[DR:], out.t[DR:], 0.25, ref=ref[DR:], alpha=0.3)
    two = torch.empty(_hi(shape), device="cuda")
    ops.upsample2x(x, two, 0.25)
    ops.mul_grad(two[:DR], ref[:DR], two[:DR], keep=keep, alpha=0.3, scale=1.0 / 0.7)
    ops.mul_grad(two[DR:], ref[DR:], two[DR:], alpha=0.3)
    torch.cuda.synchronize()
    assert torch.equal(out.t, two) and out.guards_intact()


def test_misaligned_views_are_an_error_status_and_launch_nothing():
    lo, hi = (2, 3, 3, 4), (2, 6, 6, 4)
    nl, nh = int(np.prod(lo)), int(np.prod(hi))
    a, b, r = (torch.ones(nh + 8, device="cuda") for _ in range(3))
    k = torch.ones(nh + 8, dtype=torch.uint8, device="cuda")
    v = lambda t, off, n, s: t[off:off + n].view(s)
    for call in (lambda: ops.upsample2x(v(a, 1, nl, lo), v(b, 0, nh, hi)),
                 lambda: ops.upsample2x(v(a, 0, nl, lo), v(b, 2, nh, hi)),
                 lambda: ops.upsample2x(v(a, 0, nl, lo), v(b, 0, nh, hi), ref=v(r, 3, nh, hi)),
                 lambda: ops.upsample2x(v(a, 0, nl, lo), v(b, 0, nh, hi), ref=v(r, 0, nh, hi), keep=v(k, 4, nh, hi)),
                 lambda: ops.pool2x_sum(v(a, 1, nh, hi), v(b, 0, nl, lo)),
                 lambda: ops.pool2x_sum(v(a, 0, nh, hi), v(b, 3, nl, lo))):
        with pytest.raises(ValueError, match="aligned"):
            call()
    torch.cuda.synchronize()
    assert float(a.min()) == float(a.max()) == 1.0 and float(b.min()) == float(b.max()) == 1.0
