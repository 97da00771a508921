"""The MinibatchStdDev kernels (csrc/mbstd.hip) against the float64 formulas of tests/mbstd_reference.py, on every case of
tests/mbstd_cases.py, once with all views 16-byte aligned and once with all of them one float off.

Tolerance (the rule of tests/helpers.py): per element POINT_RTOL * |reference| + POINT_ATOL * max|reference|; where a float32 numpy
evaluation of the same formulas does not meet that itself, YARDSTICK x its own largest deviation instead.  Every output and the
kept statistics live in guarded buffers: nothing is written outside, every element inside is written, inputs stay as they were.
Each run is repeated into fresh buffers: the same bits.  A second group per workgroup on the two-launch route is held by bit identity
with a small run of the same groups (the last test)."""
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


def tile_groups(flat, per_group, groups):
    """[groups, per_group] on the device: the groups of ``flat`` (whole groups of per_group floats), repeated in order."""
    small = flat.view(-1, per_group)
    return small.repeat(-(-groups // small.shape[0]), 1)[:groups]


class _Run:
    """One run of the three calls on guarded buffers at ``off`` floats past a 16-byte boundary."""

    def __init__(self, x, u, d, G, off, eps=EPS):
        N, P, C = x.shape
        g = lambda size, init=None: Guarded(size, init=init, offset=off)
        self.inputs = dict(x=g(x.size, x), u=g(u.size, u), d=g(d.size, d))
        self._launch(N, P, C, G, off, eps)

    @classmethod
    def tiled(cls, small, groups, P, C, G, eps=EPS):
        """``groups`` groups that repeat the groups of the run ``small`` in order (its inputs tiled on the device), 16-byte aligned."""
        self = cls.__new__(cls)
        self.inputs = {}
        for key, per_group in (("x", G * P * C), ("u", G * P * (C + 1)), ("d", G * P * C)):
            self.inputs[key] = Guarded(groups * per_group)
            self.inputs[key].view.view(groups, per_group).copy_(tile_groups(small.inputs[key].view, per_group, groups))
        self._launch(G * groups, P, C, G, 0, eps)
        return self

    def _launch(self, N, P, C, G, off, eps):
        n = N // G
        g = lambda size, init=None: Guarded(size, init=init, offset=off)
        self.out = dict(y=g(N * P * (C + 1)), mu=g(n * P * C), rs=g(n * P * C), f=g(n), dx=g(N * P * C), q=g(n), vout=g(N * P * (C + 1)),
                        src=g(N * P * C), fdot=g(n))
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


def test_a_second_group_per_workgroup_on_the_two_launch_route_repeats_the_first():
    """1027 groups of 15360 floats (the resident_first_out geometry: two launches, two cuts) for 1024 workgroup columns: three of them
    take a second group.  The float64 formulas at that size would cost too much on the host, so: six groups are run on their own and
    checked against the formulas as usual; the large run repeats those six in order, and every output of its group g must equal the
    small run's group g % 6 bit for bit.  That rests on the kernels' contract: a group's bits depend on its data, its alignment (all
    group bases 16-byte aligned here: 15360 floats apart) and its cut count, which depends on the group's size alone -- not on which
    workgroup or which trip handles it.  Where the small run passes and this fails, the fault is in the second trip."""
    _, G, _, P, C = MC.case("resident_first_out")
    few, many = 6, MC.MAX_BLOCKS + 3
    x, u, d = MC.data(G, few, P, C, seed=23)
    ref, ref32 = _references(x, u, d, G)
    small = _Run(x, u, d, G, 0)
    small.check_buffers()
    for key in small.out:
        _close(small.get(key), ref[key], ref32[key], f"{few} groups {key}")
    plan = {n: ops.mbstd.plan(G * n, G, P, C, "fwd") for n in (few, many)}
    assert not plan[many]["resident"] and plan[many]["grid_x"] == MC.MAX_BLOCKS < many and plan[many]["launches"] == 2
    assert plan[many]["grid_y"] == plan[few]["grid_y"] > 1 and plan[many]["grid_y_emit"] == plan[few]["grid_y_emit"]
    big = _Run.tiled(small, many, P, C, G)
    for name, b in {**big.inputs, **big.out, "ws": big.ws}.items():
        assert b.guards_intact(), f"{name}: written outside"
    per_group = dict(x=G * P * C, u=G * P * (C + 1), d=G * P * C, y=G * P * (C + 1), mu=P * C, rs=P * C, f=1, dx=G * P * C, q=1,
                     vout=G * P * (C + 1), src=G * P * C, fdot=1)
    bits = lambda t: t.contiguous().view(torch.int32)
    for key, b in big.inputs.items():
        assert torch.equal(bits(b.view.view(many, -1)), bits(tile_groups(small.inputs[key].view, per_group[key], many))), f"{key}: input changed"
    for key, b in big.out.items():
        assert not bool(torch.isnan(b.view).any()), f"{key}: elements left unwritten"
        got, want = bits(b.view.view(many, per_group[key])), bits(tile_groups(small.out[key].view, per_group[key], many))
        wrong = (got != want).any(1)
        assert not bool(wrong.any()), f"{key}: groups {torch.nonzero(wrong).flatten().tolist()[:8]} differ from the small run's"
