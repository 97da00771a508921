"""The MinibatchStdDev kernels (csrc/mbstd.hip) against the float64 formulas of tests/mbstd_reference.py, on every case of
tests/mbstd_cases.py, once with all views 16-byte aligned and once with all of them one float off.

Tolerance (the rule of tests/helpers.py): per element POINT_RTOL * |reference| + POINT_ATOL * max|reference|; where a float32 numpy
evaluation of the same formulas does not meet that itself, YARDSTICK x its own largest deviation instead.  Every output and the
kept statistics live in guarded buffers: nothing is written outside, every element inside is written, inputs stay as they were.
Each run is repeated into fresh buffers: the same bits."""
import numpy as np
import pytest
import torch

from blurred_gan_amd import ops
from helpers import POINT_ATOL, POINT_RTOL, YARDSTICK, Guarded
import mbstd_cases as MC
import mbstd_reference as MR

pytestmark = pytest.mark.gpu
EPS = MC.EPS


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
    """One run of the three calls on guarded buffers at ``off`` floats past a 16-byte boundary."""

    def __init__(self, x, u, d, G, off, eps=EPS):
        N, P, C = x.shape
        n = N // G
        g = lambda size, init=None: Guarded(size, init=init, offset=off)
        self.inputs = dict(x=g(x.size, x), u=g(u.size, u), d=g(d.size, d))
        self.out = dict(y=g(N * P * (C + 1)), mu=g(n * P * C), rs=g(n * P * C), f=g(n), dx=g(x.size), q=g(n), vout=g(N * P * (C + 1)),
                        src=g(x.size), fdot=g(n))
        nb = ops.mbstd.workspace_bytes(N, G, P, C)
        self.ws = g(nb // 4) if nb else None
        I, O = self.inputs, self.out
        ws = None if self.ws is None else self.ws.view
        ops.mbstd.fwd(I["x"].t(N, P, C), O["y"].t(N, P, C + 1), O["mu"].view, O["rs"].view, O["f"].view, G, eps, ws)
        ops.mbstd.bwd(I["u"].t(N, P, C + 1), I["x"].t(N, P, C), O["mu"].view, O["rs"].view, O["dx"].t(N, P, C), O["q"].view, G)
        ops.mbstd.gp(I["d"].t(N, P, C), I["x"].t(N, P, C), O["mu"].view, O["rs"].view, O["q"].view, O["vout"].t(N, P, C + 1),
                     O["src"].t(N, P, C), O["fdot"].view, G, eps, ws)
        torch.cuda.synchronize()
        self.shapes = dict(y=(N, P, C + 1), mu=(n, P, C), rs=(n, P, C), f=(n,), dx=(N, P, C), q=(n,), vout=(N, P, C + 1), src=(N, P, C), fdot=(n,))

    def check_buffers(self):
        for name, b in {**self.inputs, **self.out, **({"ws": self.ws} if self.ws is not None else {})}.items():
            assert b.guards_intact(), f"{name}: written outside"
        for name, b in self.inputs.items():
            assert b.unchanged(), f"{name}: input changed"
        for name, b in self.out.items():
            assert not np.isnan(b.get()).any(), f"{name}: elements left unwritten"

    def get(self, name):
        return self.out[name].get(*self.shapes[name])


def _references(x, u, d, G, eps=EPS):
    out = {}
    for dt in (np.float64, np.float32):
        xx, uu, dd = x.astype(dt), u.astype(dt), d.astype(dt)
        y, mu, rs, f = MR.np_fwd(xx, G, eps)
        dx, q = MR.np_bwd(uu, xx, G, eps)
        vout, src, fdot = MR.np_gp(dd, xx, q, G, eps)
        out[dt] = dict(y=y, mu=mu, rs=rs, f=f, dx=dx, q=q, vout=vout, src=src, fdot=fdot)
    return out[np.float64], out[np.float32]


@pytest.mark.parametrize("off", MC.OFFSETS)
@pytest.mark.parametrize("name", [c[0] for c in MC.CASES])
def test_kernels_match_the_formulas(name, off):
    _, G, groups, P, C = MC.case(name)
    x, u, d = MC.data(G, groups, P, C, seed=len(name) * 7 + G)
    ref, ref32 = _references(x, u, d, G)
    s = 1 / ref["rs"]
    assert 0.49 < s.min() and s.max() < 2.01, (s.min(), s.max())
    run = _Run(x, u, d, G, off)
    run.check_buffers()
    for key in ("y", "mu", "rs", "f", "dx", "q", "vout", "src", "fdot"):
        _close(run.get(key), ref[key], ref32[key], f"{name} off={off} {key}")
    # the passed-through channels are copies
    assert np.array_equal(run.get("y")[..., :C], x.astype(np.float32)) and np.array_equal(run.get("vout")[..., :C], d.astype(np.float32))
    # every pixel of every member carries its group's scalar
    assert np.array_equal(run.get("y")[..., C], np.broadcast_to(np.repeat(run.get("f"), G)[:, None], (G * groups, P)))
    assert np.array_equal(run.get("vout")[..., C], np.broadcast_to(np.repeat(run.get("fdot"), G)[:, None], (G * groups, P)))
    # determinism: a second run into fresh buffers gives the same bits
    again = _Run(x, u, d, G, off)
    for key in run.out:
        assert np.array_equal(run.get(key).view(np.uint32), again.get(key).view(np.uint32)), key


@pytest.mark.parametrize("off", MC.OFFSETS)
@pytest.mark.parametrize("groups,P,C", [(1, 1, 1), (3, 4, 8), (2, 4, 512)])
def test_exact_integer_data(groups, P, C, off):
    """G = 2, x = a +- k: mu == a, s == k and f_g are exact; the passed-through channels are the input's bits."""
    x, k = MC.exact_data(groups, P, C, seed=groups + C)
    rng = np.random.default_rng(5)
    u, d = rng.normal(size=(2 * groups, P, C + 1)), rng.normal(size=(2 * groups, P, C))
    run = _Run(x, u, d, 2, off)
    run.check_buffers()
    assert np.array_equal(run.get("mu"), x.reshape(groups, 2, P, C).mean(1).astype(np.float32))
    assert np.array_equal(run.get("rs"), (np.float32(1) / k.astype(np.float32)))
    f = k.reshape(groups, -1).sum(1) / (P * C)
    assert np.array_equal(run.get("f"), f.astype(np.float32)) and np.array_equal(f.astype(np.float32).astype(np.float64), f)
    y = run.get("y")
    assert np.array_equal(y[..., :C].view(np.uint32), x.astype(np.float32).view(np.uint32))
    assert np.array_equal(y[..., C], np.broadcast_to(np.repeat(f.astype(np.float32), 2)[:, None], (2 * groups, P)))


@pytest.mark.parametrize("off", MC.OFFSETS)
@pytest.mark.parametrize("G", [2, 3, 4])
def test_zero_variance_columns_and_a_zero_variance_group(G, off):
    """Columns whose members are all equal (as all dropped by Dropout: x and the tangent d both) add exactly zero to dx, fdot and
    src; a group that consists of such columns has f_g == sqrt(epsilon); nothing is NaN or Inf.  (Where d differs between the
    members of such a column the source is q k (d - dbar) / sqrt(epsilon), as autograd has it: the comparison with the formulas
    below covers that.)"""
    groups, P, C = 3, 4, 8
    x, u, d = MC.data(G, groups, P, C, seed=G)
    xg, dg = x.reshape(groups, G, P, C), d.reshape(groups, G, P, C)
    xg[0, :, :, 2] = 0.0                    # dropped units
    dg[0, :, :, 2] = 0.0
    xg[0, :, 1, 5] = xg[0, 0, 1, 5]         # an equal non-zero value
    dg[0, :, 1, 5] = dg[0, 0, 1, 5]
    xg[1] = xg[1, :1] * 0 + np.float32(0.7)         # a whole group without variance, d equal too
    dg[1] = dg[1, :1]
    run = _Run(x, u, d, G, off)
    run.check_buffers()
    for key in run.out:
        assert np.isfinite(run.get(key)).all(), key
    sq = np.sqrt(np.float32(EPS), dtype=np.float32)
    assert run.get("f")[1] == sq, (run.get("f")[1], sq)
    dx, src, uu = (run.get("dx").reshape(groups, G, P, C), run.get("src").reshape(groups, G, P, C),
                   u.astype(np.float32).reshape(groups, G, P, C + 1))
    assert np.array_equal(dx[0, :, :, 2], uu[0, :, :, 2]) and np.array_equal(dx[0, :, 1, 5], uu[0, :, 1, 5]) and np.array_equal(dx[1], uu[1, ..., :C])
    assert not src[0, :, :, 2].any() and not src[0, :, 1, 5].any() and not src[1].any()
    assert run.get("fdot")[1] == 0.0
    # fdot of group 0 is the sum over its other columns alone: the same bits as with those columns' tangent set to anything else
    d2 = d.copy().reshape(groups, G, P, C)
    d2[0, :, :, 2] = 3.0
    assert run.get("fdot")[0] == _Run(x, u, d2.reshape(d.shape), G, off).get("fdot")[0]
    # a constant column whose tangent differs: the formulas (autograd's value), finite
    d3 = d.copy().reshape(groups, G, P, C)
    d3[0, :, :, 2] = np.random.default_rng(1).normal(size=(G, P)).astype(np.float32)
    ref, ref32 = _references(x, u, d3.reshape(d.shape), G)
    got = _Run(x, u, d3.reshape(d.shape), G, off)
    _close(got.get("src"), ref["src"], ref32["src"], f"G={G} off={off} src with an unequal tangent on a constant column")
