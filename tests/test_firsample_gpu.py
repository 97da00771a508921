"""GPU tests of the FIR-filtered resampling kernels (include/bgan.h "resampling": bg_fir_upsample2x_nhwc_f32,
bg_fir_downsample2x_nhwc_f32; ops.fir_upsample2x, ops.fir_downsample2x): both routes and every tap count bit for bit against numpy on
exact data, against float64 within the rounding bound on uniform data, guard regions, adjointness, the nearest pair at (1, 1), the
fused LeakyReLU' / Dropout' factor against the two-launch form, misaligned views.

The kernels do not tile (one thread per low-resolution unit, neighbours through the caches), so there are no tile-edge sizes; the
shapes cover H or W below the filter's reach, both routes, odd sizes, grids below, at and above the 8 workgroups from which the block
index is permuted, and one map of more units than one grid trip covers."""
import numpy as np
import pytest
import torch

from blurred_gan_amd import ops
import firsample_reference as FR

pytestmark = pytest.mark.gpu

# low-resolution (B, H, W, C).  (2, 17, 19, 16) and (1, 13, 17, 10): 2584 float4 / 2210 scalar units = 11 / 9 workgroups, which the
# launch rounds up to 16 and permutes over the XCDs (csrc/firsample.hip xcd_chunked_block): surplus workgroups, a ragged last one.
# The last: 181 * 183 * 16 = 529 968 channel quads, more threads than the launch's 2048 x 256 with a ragged last block: the
# grid-stride loop takes a second trip, permuted too
SHAPES = [(1, 1, 1, 4), (1, 1, 3, 4), (2, 2, 1, 3), (3, 3, 5, 4), (2, 3, 5, 20), (2, 4, 4, 16), (2, 5, 3, 3), (1, 2, 2, 1), (3, 2, 3, 6),
          (2, 17, 19, 16), (1, 13, 17, 10), (1, 181, 183, 64)]
# sums that are powers of two: every weight, product and partial sum on integer data is exact in float32 in any order
EXACT_KERNELS = [(1, 1), (1, 3, 3, 1), (1, 2, 4, 1), (1, 3, 2, 2), (1, 5, 10, 10, 5, 1), (1, 2, 3, 4, 2, 2, 1, 1)]
ROUNDED_KERNELS = [(1, 3, 3, 1), (1, 2, 5, 3)]
SCALES = [1.0, 4.0, 0.25]
POISON = -7777.0
GUARD = 64          # floats on either side of a tensor (keeps the tensor 16-byte aligned)
U = 2.0 ** -24
ids = lambda s: "x".join(map(str, s))


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


@pytest.fixture(scope="module")
def exact_inputs():
    """The integer inputs of every shape, made once and left unchanged."""
    return {s: (_data("int", s, 1), _data("int", _hi(s), 2)) for s in SHAPES}


@pytest.mark.parametrize("kernel", EXACT_KERNELS, ids=ids)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_both_kernels_equal_numpy_bit_for_bit_on_exact_data(exact_inputs, shape, kernel):
    lo, hi = exact_inputs[shape]
    taps = FR.normalized(kernel)
    assert sum(kernel) & (sum(kernel) - 1) == 0 and np.array_equal(np.float64(taps), np.asarray(kernel) / sum(kernel))
    xl, xh = Guarded(shape, fill=lo), Guarded(_hi(shape), fill=hi)
    want_up, want_down = FR.np_up(lo, taps, 1.0, np.float32), FR.np_down(hi, taps, 1.0, np.float32)
    assert want_up.dtype == want_down.dtype == np.float32
    assert np.array_equal(want_up, FR.np_up(lo, taps).astype(np.float32)) and np.array_equal(want_down, FR.np_down(hi, taps).astype(np.float32))
    for scale in SCALES:
        yh, yl = Guarded(_hi(shape)), Guarded(shape)
        assert ops.fir_upsample2x(xl.t, yh.t, taps, scale) is yh.t
        assert ops.fir_downsample2x(xh.t, yl.t, taps, scale) is yl.t
        torch.cuda.synchronize()
        assert np.array_equal(yh.np(), np.float32(scale) * want_up), (shape, kernel, scale)
        assert np.array_equal(yl.np(), np.float32(scale) * want_down), (shape, kernel, scale)
        assert yh.guards_intact() and yl.guards_intact()
    assert np.array_equal(xl.np(), lo) and np.array_equal(xh.np(), hi) and xl.guards_intact() and xh.guards_intact()


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_the_box_kernel_equals_the_nearest_pair_bit_for_bit(exact_inputs, shape):
    lo, hi = exact_inputs[shape]
    xl, xh = torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda()
    for scale in SCALES:
        a, b = torch.empty(_hi(shape), device="cuda"), torch.empty(_hi(shape), device="cuda")
        c, d = torch.empty(shape, device="cuda"), torch.empty(shape, device="cuda")
        ops.fir_upsample2x(xl, a, (0.5, 0.5), 4.0 * scale)
        ops.upsample2x(xl, b, scale)
        ops.fir_downsample2x(xh, c, (0.5, 0.5), 4.0 * scale)
        ops.pool2x_sum(xh, d, scale)
        assert torch.equal(a, b) and torch.equal(c, d), (shape, scale)


@pytest.mark.parametrize("kernel", ROUNDED_KERNELS, ids=ids)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_both_kernels_match_float64_within_the_rounding_bound(shape, kernel):
    """|y - y64| <= (n_terms + 3) * 2^-24 * scale * sum|w| * max|x| per output, n_terms = T^2 (up) or (2T)^2 (down), sum|w| over the
    2-D weights of that output's terms: the first-order bound of any-order float32 summation (a rounding per product, per addition and
    for the scale).  The float64 reference takes the float32 taps the kernels take."""
    B, H, W, C = shape
    taps = FR.normalized(kernel)
    T = len(taps) // 2
    lo, hi = _data("uniform", shape, 3), _data("uniform", _hi(shape), 4)
    xl, xh = Guarded(shape, fill=lo), Guarded(_hi(shape), fill=hi)
    ref_up, ref_down = FR.np_up(lo, taps), FR.np_down(hi, taps)
    sw_up, sw_down = FR.abs_weight_sums(taps, H, W, True), FR.abs_weight_sums(taps, H, W, False)
    for scale in SCALES:
        yh, yl = Guarded(_hi(shape)), Guarded(shape)
        ops.fir_upsample2x(xl.t, yh.t, taps, scale)
        ops.fir_downsample2x(xh.t, yl.t, taps, scale)
        torch.cuda.synchronize()
        for name, got, ref, sw, n_terms, xmax in (("up", yh.np(), ref_up, sw_up, T * T, np.abs(lo).max()),
                                                  ("down", yl.np(), ref_down, sw_down, 4 * T * T, np.abs(hi).max())):
            err = np.abs(got.astype(np.float64) - scale * ref)
            bound = (n_terms + 3) * U * scale * sw[None, :, :, None] * float(xmax)
            worst = float((err / np.maximum(bound, 1e-300)).max())
            print(f"[{name} {ids(shape)} {ids(kernel)} scale {scale}] max err {err.max():.3e}, max err / bound {worst:.3f}")
            assert (err <= bound).all(), (name, shape, kernel, scale, worst)
        assert yh.guards_intact() and yl.guards_intact()
    assert np.array_equal(xl.np(), lo) and np.array_equal(xh.np(), hi)


@pytest.mark.parametrize("kernel", EXACT_KERNELS, ids=ids)
@pytest.mark.parametrize("shape", SHAPES[:-1], ids=ids)
def test_adjointness_is_exact_on_integer_data(shape, kernel):
    """<up_t(x), g> == <x, down_flip(t)(g)>: every product and sum is a multiple of 2^-12 below 2^40, exact in float64."""
    taps = FR.normalized(kernel)
    x, g = _data("int", shape, 5), _data("int", _hi(shape), 6)
    ux, dg = torch.empty(_hi(shape), device="cuda"), torch.empty(shape, device="cuda")
    ops.fir_upsample2x(torch.from_numpy(x).cuda(), ux, taps, 1.0)
    ops.fir_downsample2x(torch.from_numpy(g).cuda(), dg, taps[::-1], 1.0)
    lhs = (ux.cpu().numpy().astype(np.float64) * g).sum()
    rhs = (x.astype(np.float64) * dg.cpu().numpy()).sum()
    assert lhs == rhs and lhs == (FR.np_up(x, taps) * g).sum()


def _ref_with_zeros(shape, seed):
    rng = np.random.default_rng(seed)
    r = rng.uniform(-1, 1, size=shape).astype(np.float32)
    z = rng.uniform(size=shape)
    r[z < 0.2] = 0.0
    r[(z >= 0.2) & (z < 0.25)] = -0.0
    assert (r == 0).any() and (r > 0).any() and (r < 0).any()
    return r


@pytest.mark.parametrize("kernel", [(1, 3, 3, 1), (1, 3, 2, 2), (1, 1), (1, 2, 3, 4, 2, 2, 1, 1)], ids=ids)
@pytest.mark.parametrize("with_keep", [False, True], ids=["nokeep", "keep"])
@pytest.mark.parametrize("shape", [(1, 1, 3, 4), (3, 3, 5, 4), (2, 3, 5, 20), (2, 4, 4, 16), (2, 5, 3, 3), (3, 2, 3, 6), (2, 17, 19, 16),
                                   (1, 13, 17, 10), (1, 181, 183, 64)], ids=ids)
def test_fused_backward_equals_upsample_then_mul_grad(shape, with_keep, kernel):
    rng = np.random.default_rng(7)
    taps = FR.normalized(kernel)
    x = Guarded(shape, fill=_data("uniform", shape, 8))
    ref = Guarded(_hi(shape), fill=_ref_with_zeros(_hi(shape), 9))
    keep = None
    if with_keep:
        k = (rng.uniform(size=_hi(shape)) >= 0.3).astype(np.uint8)
        k[(rng.uniform(size=_hi(shape)) < 0.05) & (k == 1)] = 255            # any non-zero byte keeps
        keep = Guarded(_hi(shape), dtype=torch.uint8, fill=k)
    gs = 1.0 / 0.7
    for scale, alpha in ((1.0, 0.3), (0.25, 0.25)):
        fused, two = Guarded(_hi(shape)), Guarded(_hi(shape))
        ops.fir_upsample2x(x.t, fused.t, taps, scale, ref=ref.t, keep=None if keep is None else keep.t, alpha=alpha, grad_scale=gs)
        ops.fir_upsample2x(x.t, two.t, taps, scale)
        plain = two.t.clone()
        ops.mul_grad(two.t, ref.t, two.t, keep=None if keep is None else keep.t, alpha=alpha, scale=gs)
        torch.cuda.synchronize()
        assert torch.equal(fused.t, two.t), (shape, with_keep, alpha, scale)
        assert fused.guards_intact() and two.guards_intact()
        # and the factor itself, spelled out: y * f, f = (ref > 0 ? 1 : alpha) [* keep ? gs : 0]
        f = np.where(ref.np() > 0, np.float32(1.0), np.float32(alpha))
        if keep is not None:
            f = np.where(keep.np() != 0, f * np.float32(gs), np.float32(0.0))
        assert np.array_equal(fused.np(), plain.cpu().numpy() * f)
    assert x.guards_intact() and ref.guards_intact() and (keep is None or keep.guards_intact())


@pytest.mark.parametrize("shape", [(3, 3, 5, 4), (3, 2, 3, 6), (4, 2, 2, 16)], ids=ids)
def test_fused_backward_on_a_row_sub_range(shape):
    """The merged critic pass: rows [0, DR) with the Dropout mask (whose buffer covers those rows only), the rest without."""
    B, DR = shape[0], shape[0] - 1
    taps = FR.normalized((1, 3, 2, 2))
    x = torch.from_numpy(_data("uniform", shape, 10)).cuda()
    ref = torch.from_numpy(_ref_with_zeros(_hi(shape), 11)).cuda()
    keep = torch.from_numpy((np.random.default_rng(12).uniform(size=(DR,) + _hi(shape)[1:]) >= 0.3).astype(np.uint8)).cuda()
    out = Guarded(_hi(shape))
    ops.fir_upsample2x(x[:DR], out.t[:DR], taps, 1.0, ref=ref[:DR], keep=keep, alpha=0.3, grad_scale=1.0 / 0.7)
    torch.cuda.synchronize()
    assert bool((out.t[DR:] == POISON).all())                                  # the other rows are not this launch's
    ops.fir_upsample2x(x[DR:], out.t[DR:], taps, 1.0, ref=ref[DR:], alpha=0.3)
    two = torch.empty(_hi(shape), device="cuda")
    ops.fir_upsample2x(x, two, taps, 1.0)
    ops.mul_grad(two[:DR], ref[:DR], two[:DR], keep=keep, alpha=0.3, scale=1.0 / 0.7)
    ops.mul_grad(two[DR:], ref[DR:], two[DR:], alpha=0.3)
    torch.cuda.synchronize()
    assert torch.equal(out.t, two) and out.guards_intact()


@pytest.mark.parametrize("shape", [(2, 2, 1, 3), (2, 5, 3, 3), (1, 2, 2, 1), (3, 2, 3, 6)], ids=ids)
def test_misaligned_views_take_the_scalar_route_and_still_match(shape):
    """C % 4 != 0 makes no alignment demand: every operand one float (one byte for the mask) off a 16-byte boundary."""
    taps = FR.normalized((1, 3, 2, 2))
    lo, hi = _data("int", shape, 13), _data("int", _hi(shape), 14)
    nl, nh = lo.size, hi.size
    off = lambda a: torch.cat([torch.full((1,), POISON, device="cuda"), torch.from_numpy(a).cuda().flatten(),
                               torch.full((3,), POISON, device="cuda")])[1:1 + a.size].view(a.shape)
    xl, xh = off(lo), off(hi)
    assert xl.data_ptr() % 16 == 4 and xh.data_ptr() % 16 == 4
    yh, yl = off(np.zeros_like(hi)), off(np.zeros_like(lo))
    ops.fir_upsample2x(xl, yh, taps, 4.0)
    ops.fir_downsample2x(xh, yl, taps, 1.0)
    assert np.array_equal(yh.cpu().numpy(), FR.np_up(lo, taps, 4.0, np.float32))
    assert np.array_equal(yl.cpu().numpy(), FR.np_down(hi, taps, 1.0, np.float32))
    ref = off(_ref_with_zeros(_hi(shape), 15))
    kbuf = torch.from_numpy((np.random.default_rng(16).uniform(size=nh + 1) >= 0.3).astype(np.uint8)).cuda()
    keep = kbuf[1:].view(_hi(shape))
    fused, two = off(np.zeros_like(hi)), off(np.zeros_like(hi))
    ops.fir_upsample2x(xl, fused, taps, 1.0, ref=ref, keep=keep, alpha=0.3, grad_scale=1.0 / 0.7)
    ops.fir_upsample2x(xl, two, taps, 1.0)
    ops.mul_grad(two, ref, two, keep=keep, alpha=0.3, scale=1.0 / 0.7)
    assert torch.equal(fused, two)
    assert nl and nh


def test_misaligned_views_on_the_float4_route_are_an_error_status_and_launch_nothing():
    lo, hi = (2, 3, 3, 4), (2, 6, 6, 4)
    nl, nh = int(np.prod(lo)), int(np.prod(hi))
    a, b, r = (torch.ones(nh + 8, device="cuda") for _ in range(3))
    k = torch.ones(nh + 8, dtype=torch.uint8, device="cuda")
    v = lambda t, off, n, s: t[off:off + n].view(s)
    t = (0.125, 0.375, 0.375, 0.125)
    for call in (lambda: ops.fir_upsample2x(v(a, 1, nl, lo), v(b, 0, nh, hi), t),
                 lambda: ops.fir_upsample2x(v(a, 0, nl, lo), v(b, 2, nh, hi), t),
                 lambda: ops.fir_upsample2x(v(a, 0, nl, lo), v(b, 0, nh, hi), t, ref=v(r, 3, nh, hi)),
                 lambda: ops.fir_upsample2x(v(a, 0, nl, lo), v(b, 0, nh, hi), t, ref=v(r, 0, nh, hi), keep=v(k, 4, nh, hi)),
                 lambda: ops.fir_downsample2x(v(a, 1, nh, hi), v(b, 0, nl, lo), t),
                 lambda: ops.fir_downsample2x(v(a, 0, nh, hi), v(b, 3, nl, lo), t)):
        with pytest.raises(ValueError, match="aligned"):
            call()
    with pytest.raises(ValueError, match="n_taps"):
        ops.fir_upsample2x(v(a, 0, nl, lo), v(b, 0, nh, hi), (0.25, 0.5, 0.25))
    torch.cuda.synchronize()
    assert float(a.min()) == float(a.max()) == 1.0 and float(b.min()) == float(b.max()) == 1.0
