"""The uint8 input pipeline's kernels (csrc/input.hip bg_u8_gather_normalize_resize_f32, csrc/misc.hip u8_normalize_resize_kernel) on
every case of tests/input_cases.py (tests/test_input_cases_cpu.py proves what the list reaches): against the float64 oracle
oracle.np_ops.normalize_resize_bilinear of the gathered images, mirrored with np.flip where flagged, and bit for bit against
themselves.

Tolerance (the rule of tests/test_mbstd_gpu.py): per element POINT_RTOL * |reference| + POINT_ATOL * max|reference|; where the same oracle
in float32 does not meet that itself, YARDSTICK x its own largest deviation instead (never above input_cases.YARDSTICK_CAP: the CPU test).
The destination is NaN-filled between sentinel bands: every element must be written, nothing outside, and the source, the indices and
the flags stay as they were.  Each (image, flag) pair has one reference; every output sample is compared with its pair's."""
import math

import numpy as np
import pytest
import torch

from blurred_gan_amd import ops
from helpers import Guarded
import input_cases as IC

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class _Run:
    """One launch on guarded buffers.  ``off`` = 1 hands over the views data.py does: the indices one element past a 16-byte
    boundary, the flags and the source one byte past."""

    def __init__(self, src, idx, shape, flip=None, off=0):
        self.shape = tuple(shape)
        self.src = Guarded(src.size, src, torch.uint8, offset=off)
        self.idx = Guarded(len(idx), idx, torch.int32, offset=off)
        self.flip = None if flip is None else Guarded(len(flip), flip, torch.uint8, offset=off)
        self.dst = Guarded(math.prod(shape))
        for b, size in ((self.src, 1), (self.idx, 4)) + (((self.flip, 1),) if flip is not None else ()):
            assert b.view.data_ptr() % 16 == off * size
        ops.u8_gather_normalize_resize(self.src.t(*src.shape), self.idx.view, self.out, None if flip is None else self.flip.view)
        torch.cuda.synchronize()

    @property
    def out(self):
        return self.dst.t(*self.shape)

    def check_buffers(self):
        bufs = dict(src=self.src, idx=self.idx, dst=self.dst, **({} if self.flip is None else {"flip": self.flip}))
        for name, b in bufs.items():
            assert b.guards_intact(), f"{name}: written outside"
            assert name == "dst" or b.unchanged(), f"{name}: input changed"
        unwritten = int(torch.isnan(self.dst.view).sum())
        assert unwritten == 0, f"dst: {unwritten} elements left unwritten"
        return self


def _dense(batch, shape):
    """The dense kernel on a batch of images, into a guarded destination."""
    dst = Guarded(math.prod(shape))
    ops.u8_normalize_resize(torch.from_numpy(np.ascontiguousarray(batch)).cuda(), dst.t(*shape))
    torch.cuda.synchronize()
    assert dst.guards_intact() and not bool(torch.isnan(dst.view).any())
    return dst


def _check_against(got, rows, ref, tol):
    err = np.abs(got[rows].astype(np.float64) - ref[None])
    assert np.isfinite(got[rows]).all()
    assert (err <= tol[None]).all(), f"samples {rows}: max|err| {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}"
    return float(err.max())


@pytest.mark.parametrize("name", [c[0] for c in IC.CASES])
def test_every_case_matches_the_oracle_and_itself(name):
    _, N, B, src_hw, dst_hw, C, idx, flip = IC.case(name)
    src, ref, tol, rule, dev32 = IC.case_references(name)
    shape = (B, *dst_hw, C)
    run = _Run(src, idx, shape, flip).check_buffers()
    # 1. the float64 oracle: each output sample against its (image, flag) pair's reference
    got, worst = run.dst.get(*shape), 0.0
    for n in sorted(set(idx)):
        for fl in (0, 1):
            rows = [b for b in range(B) if idx[b] == n and bool(flip[b]) == bool(fl)]
            if rows:
                worst = max(worst, _check_against(got, rows, np.flip(ref[n], 1) if fl else ref[n], np.flip(tol[n], 1) if fl else tol[n]))
    print(f"[{name}] max|err| {worst:.3e}, rule {rule}, float32 oracle max|dev| {dev32:.3e}")
    # 2. the mirror is exact: a flagged sample is torch.flip of the same sample run without flags; no flags = all-zero flags
    plain = _Run(src, idx, shape).check_buffers().out
    flags = torch.tensor(flip, dtype=torch.bool, device="cuda")[:, None, None, None]
    assert _same_bits(run.out, torch.where(flags, torch.flip(plain, dims=[2]), plain))
    assert _same_bits(_Run(src, idx, shape, [0] * B).check_buffers().out, plain)
    # 3. the gather is exact: the same call on the pre-gathered batch with idx = range(B), and the dense kernel on that batch
    gathered = np.ascontiguousarray(src[idx])
    assert _same_bits(_Run(gathered, list(range(B)), shape).check_buffers().out, plain)
    assert _same_bits(_dense(gathered, shape).t(*shape), plain)
    # 4. a second run into fresh buffers: the same bits; and the misaligned views data.py passes: the same bits
    assert _same_bits(_Run(src, idx, shape, flip).check_buffers().out, run.out)
    assert _same_bits(_Run(src, idx, shape, flip, off=1).check_buffers().out, run.out)
    assert _same_bits(_Run(src, idx, shape, off=1).check_buffers().out, plain)


@pytest.mark.parametrize("name", [c[0] for c in IC.CASES])
def test_constant_images_come_out_as_their_own_value_exactly(name):
    """Image n holds the byte v_n everywhere: the interpolation adds 0 * l, so every float of output sample b is
    float32((v - 127.5) / 127.5) of its own image, at every geometry.  A pixel read through a neighbouring sample's pointer (or past
    the image) is an exact mismatch."""
    _, N, B, src_hw, dst_hw, C, idx, flip = IC.case(name)
    src, v = IC.constant_images(N, *src_hw, C)
    shape = (B, *dst_hw, C)
    value = (v.astype(np.float32) - np.float32(127.5)) / np.float32(127.5)
    want = torch.from_numpy(value[np.asarray(idx)]).cuda()[:, None, None, None].expand(shape)
    for off in (0, 1):
        got = _Run(src, idx, shape, flip, off=off).check_buffers().out
        wrong = _bits(got) != _bits(want)
        assert not bool(wrong.any()), f"{int(wrong.sum())} of {wrong.numel()} floats, first at {torch.nonzero(wrong)[0].tolist()}"


def test_the_dense_kernel_past_its_grids_capacity():
    name, B, src_hw, dst_hw, C = IC.DENSE_CASE
    src = IC.data(name, B, *src_hw, C)
    shape = (B, *dst_hw, C)
    assert math.prod(shape) > IC.CAPACITY
    dst = _dense(src, shape)
    ref, ref32 = IC.references(src, dst_hw)
    rule, tol, dev32 = IC.tolerance(ref, ref32)
    got = dst.get(*shape)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"[{name}] max|err| {err.max():.3e}, rule {rule}, float32 oracle max|dev| {dev32:.3e}")
    assert np.isfinite(got).all() and (err <= tol).all(), f"max|err| {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}"
    # the gather kernel on the same batch, and a second run: the same bits
    assert _same_bits(_Run(src, list(range(B)), shape).check_buffers().out, dst.t(*shape))
    assert _same_bits(_dense(src, shape).t(*shape), dst.t(*shape))
    # constant images: exact
    const, v = IC.constant_images(B, *src_hw, C)
    value = torch.from_numpy((v.astype(np.float32) - np.float32(127.5)) / np.float32(127.5)).cuda()
    assert _same_bits(_dense(const, shape).t(*shape), value[:, None, None, None].expand(shape))


def test_a_destination_one_float_off_is_refused_and_nothing_is_written():
    _, N, B, src_hw, dst_hw, C, idx, flip = IC.case("c3_down")
    src = torch.from_numpy(IC.data("c3_down", N, *src_hw, C)).cuda()
    dst = Guarded(B * math.prod(dst_hw) * C, offset=1)
    assert dst.view.data_ptr() % 16 == 4
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.u8_gather_normalize_resize(src, torch.tensor(idx, dtype=torch.int32, device="cuda"), dst.t(B, *dst_hw, C),
                                       torch.tensor(flip, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    assert dst.guards_intact() and bool(torch.isnan(dst.view).all())
