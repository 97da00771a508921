"""The PixelNormalization kernels (csrc/pixelnorm.hip) against the float64 formulas of tests/pixelnorm_reference.py, on every case
of tests/pixelnorm_cases.py, once with all views 16-byte aligned and once with all of them one float off.

Tolerance (the rule of tests/helpers.py, as tests/test_mbstd_gpu.py applies it): per element POINT_RTOL * |reference| + POINT_ATOL *
max|reference|; where a float32 numpy evaluation of the same formulas does not meet that itself, YARDSTICK x its own largest
deviation instead.  Every buffer is guarded: nothing is written outside, every element inside is written, inputs stay as they
were.  Each run is repeated into fresh buffers: the same bits."""
import numpy as np
import pytest
import torch

from blurred_gan_amd import ops
from helpers import POINT_ATOL, POINT_RTOL, YARDSTICK, Guarded
import pixelnorm_cases as PC
import pixelnorm_reference as PR

pytestmark = pytest.mark.gpu
EPS = PC.EPS


def _close(got, ref, ref32, what):
    ref, ref32 = np.asarray(ref, np.float64).reshape(got.shape), np.asarray(ref32, np.float64).reshape(got.shape)
    tol = POINT_RTOL * np.abs(ref) + POINT_ATOL * float(np.abs(ref).max())
    err, dev32 = np.abs(got.astype(np.float64) - ref), np.abs(ref32 - ref)
    rule = "point"
    if not (dev32 <= tol).all():
        rule, tol = "yardstick", np.full_like(tol, YARDSTICK * float(dev32.max()))
    print(f"[{what}] max|err| {err.max():.3e}, max|ref| {np.abs(ref).max():.3e}, float32 numpy max|dev| {dev32.max():.3e}, rule {rule}")
    assert np.isfinite(got).all(), what
    assert (err <= tol).all(), f"{what}: max|err| {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)} ({rule})"


class _Run:
    """Forward and backward of one case on guarded buffers at ``off`` floats past a 16-byte boundary.  ``keep_r`` False: a forward
    with r = NULL first (its y must be the same bits), then the one that keeps r for the backward.  ``in_place``: the backward
    writes dz over g."""

    def __init__(self, x, g, alpha, off, keep_r=True, in_place=False, eps=EPS):
        R, C = x.shape
        G = lambda size, init=None: Guarded(size, init=init, offset=off)
        self.R, self.C = R, C
        self.inputs = dict(x=G(x.size, x), g=G(g.size, g))
        self.out = dict(y=G(x.size), r=G(R), dz=G(x.size))
        I, O = self.inputs, self.out
        self.y_without_r = None
        if not keep_r:
            y0 = G(x.size)
            ops.pixelnorm.fwd(I["x"].t(R, C), y0.t(R, C), R, C, r=None, eps=eps, lrelu_alpha=alpha)
            assert y0.guards_intact()
            self.y_without_r = y0.get(R, C)
        ops.pixelnorm.fwd(I["x"].t(R, C), O["y"].t(R, C), R, C, r=O["r"].view, eps=eps, lrelu_alpha=alpha)
        if in_place:
            O["dz"] = I.pop("g")
        ops.pixelnorm.bwd(O["dz"].t(R, C) if in_place else I["g"].t(R, C), O["y"].t(R, C), O["r"].view, O["dz"].t(R, C), R, C, lrelu_alpha=alpha)
        torch.cuda.synchronize()

    def check_buffers(self):
        for name, b in {**self.inputs, **self.out}.items():
            assert b.guards_intact(), f"{name}: written outside"
        for name, b in self.inputs.items():
            assert b.unchanged(), f"{name}: input changed"
        for name, b in self.out.items():
            assert not np.isnan(b.get()).any(), f"{name}: elements left unwritten"

    def get(self, name):
        return self.out[name].get(*((self.R,) if name == "r" else (self.R, self.C)))


def _references(x, g, alpha, eps=EPS):
    out = {}
    for dt in (np.float64, np.float32):
        y, r = PR.np_fwd(x.astype(dt), eps, alpha)
        out[dt] = dict(y=y, r=r, dz=PR.np_bwd(g.astype(dt), y, r, alpha))
    return out[np.float64], out[np.float32]


@pytest.mark.parametrize("off", PC.OFFSETS)
@pytest.mark.parametrize("name", [c[0] for c in PC.CASES])
def test_kernels_match_the_formulas(name, off):
    _, R, C, alpha = PC.case(name)
    x, g = PC.data(R, C, seed=len(name) * 7 + C)
    ref, ref32 = _references(x, g, alpha)
    run = _Run(x, g, alpha, off)
    run.check_buffers()
    for key in ("y", "r", "dz"):
        _close(run.get(key), ref[key], ref32[key], f"{name} off={off} {key}")
    # the sign of the output is the input's, whatever alpha: what lets the backward read LeakyReLU's branch from y
    assert np.array_equal(run.get("y") > 0, x > 0)
    # determinism: a second run into fresh buffers gives the same bits
    again = _Run(x, g, alpha, off)
    for key in run.out:
        assert np.array_equal(run.get(key).view(np.uint32), again.get(key).view(np.uint32)), key


@pytest.mark.parametrize("off", PC.OFFSETS)
@pytest.mark.parametrize("name", ["latent_100", "latent_6", "c5", "c512", "c1028", "c911", "r257"])
def test_forward_without_r_and_backward_in_place(name, off):
    """r = NULL keeps nothing and changes no bit of y; where the call's route holds a row in registers the backward may overwrite
    the incoming gradient, with the bits of the out-of-place call; on the chunked route that is refused and nothing is launched."""
    _, R, C, alpha = PC.case(name)
    x, g = PC.data(R, C, seed=C)
    plain = _Run(x, g, alpha, off, keep_r=False)
    plain.check_buffers()
    assert np.array_equal(plain.y_without_r.view(np.uint32), plain.get("y").view(np.uint32))
    if ops.pixelnorm.route(C, aligned=off == 0)["chunks"] == 1:
        inp = _Run(x, g, alpha, off, in_place=True)
        inp.check_buffers()
        assert np.array_equal(inp.get("dz").view(np.uint32), plain.get("dz").view(np.uint32))
    else:
        buf = Guarded(R * C, g, offset=off)
        with pytest.raises(ValueError, match="register routes only"):
            ops.pixelnorm.bwd(buf.t(R, C), plain.out["y"].t(R, C), plain.out["r"].view, buf.t(R, C), R, C, lrelu_alpha=alpha)
        torch.cuda.synchronize()
        assert buf.unchanged() and buf.guards_intact()


@pytest.mark.parametrize("off", PC.OFFSETS)
def test_zeros_take_mul_grads_branch_exactly(off):
    """Rows with zeros of either sign, every value exact: y == 0 takes the alpha branch (bg_mul_grad's ``ref > 0 ? 1 : alpha``)."""
    alpha = 0.25
    x, g, y, r, dz = PC.zero_rows(alpha)
    run = _Run(x, g, alpha, off)
    run.check_buffers()
    assert np.array_equal(run.get("r"), r.astype(np.float32))
    assert np.array_equal(run.get("y"), y.astype(np.float32)) and np.array_equal(run.get("dz"), dz.astype(np.float32))
    assert (dz[y == 0] == alpha * 0.5 * g[y == 0]).all() and (y == 0).sum() >= 6
    # the same rows through bg_mul_grad: the factor it applies at y == 0 is the one in dz
    ones = torch.ones(x.size, device="cuda")
    f = ops.mul_grad(ones, run.out["y"].view.clone(), torch.empty_like(ones), alpha=alpha).cpu().numpy().reshape(x.shape)
    assert np.array_equal(f, np.where(y > 0, 1.0, alpha).astype(np.float32))


def test_a_row_of_zeros_is_finite():
    """mean(a^2) == 0: r = 1 / sqrt(epsilon), y = 0 and dz = alpha * r * g, nothing NaN or Inf."""
    x, g = np.zeros((3, 8)), PC.data(3, 8, 1)[1]
    run = _Run(x, g, 0.2, 0)
    run.check_buffers()
    r = np.float32(1) / np.sqrt(np.float32(EPS))
    assert not run.get("y").any() and np.array_equal(run.get("r"), np.full(3, r, np.float32))
    np.testing.assert_allclose(run.get("dz"), 0.2 * float(r) * g, rtol=1e-6)
