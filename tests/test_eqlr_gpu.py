"""GPU tests of the equalised-learning-rate kernels (csrc/eqlr.hip) on their own: bg_eqlr_scale_f32 and bg_eqlr_grad_f32 bit for bit
against numpy float32 (each element gets one fp32 multiply), every case alone and all cases in one table, with guard floats around
every segment.  Unit sizes and routes are read from bg_eqlr_plan, never from a literal."""
import numpy as np
import pytest
import torch

from blurred_gan_amd import ops

pytestmark = pytest.mark.gpu

GUARD = 8                     # floats in front of and behind every segment
SENTINEL = np.float32(3.0)    # what the source buffers hold outside the segments: a stray read or write shows as a finite number
pad4 = lambda n: -(-n // 4) * 4

# (taps, R, N) -> the route bg_eqlr_plan must report, transposed copy or not
CASES = {
    "dense_scalar_no_copy": ((1, 130, 1), 1, False),
    "dense_float4": ((1, 12, 68), 4, False),
    "conv_float4_ragged_tiles": ((9, 68, 132), 4, True),
    "conv_exactly_one_tile": ((1, 64, 64), 4, True),
    "conv_below_one_tile": ((4, 4, 8), 4, True),
    "conv_scalar": ((25, 3, 5), 1, True),
    "conv_scalar_single_input_channel": ((25, 1, 4), 1, True),
}


def _coefficient(i):
    return float(np.float32(np.sqrt(2.0) / np.sqrt(3.0 + 7.0 * i)))      # a different, inexact multiplier per layer


class Batch:
    """Segments of theta and of the effective-weight buffer for a list of (name, (taps, R, N), transposed copy) layers."""

    def __init__(self, layers, seed=0):
        self.layers, rows, self.W = layers, [], {}
        off_t = off_e = GUARD
        for i, (name, (taps, R, N), copy) in enumerate(layers):
            n = taps * R * N
            rows.append(dict(w_off=off_t, eff_off=off_e, tr_off=off_e + pad4(n) + GUARD if copy else -1, K=taps * R, N=N, taps=taps, c=_coefficient(CASE_INDEX[name])))
            self.W[name] = np.random.default_rng([seed, CASE_INDEX[name]]).standard_normal(n).astype(np.float32)      # the same data alone and batched
            off_t += pad4(n) + GUARD
            off_e += (2 if copy else 1) * (pad4(n) + GUARD)
        self.rows = rows
        theta = np.full(off_t, SENTINEL, np.float32)
        for r, (name, _, _) in zip(rows, layers):
            theta[r["w_off"]:r["w_off"] + r["K"] * r["N"]] = self.W[name]
        self.theta_h = theta
        self.theta = torch.from_numpy(theta).cuda()
        self.eff = torch.full((off_e,), float("nan"), dtype=torch.float32, device="cuda")
        self.table = ops.EqlrTable(ops.eqlr.rows(rows), "cuda")

    def scale(self):
        ops.eqlr.scale(self.theta, self.eff, self.table)
        torch.cuda.synchronize()
        eff = self.eff.cpu().numpy()
        assert np.array_equal(self.theta.cpu().numpy(), self.theta_h)                  # the source is read only
        out, written = {}, np.zeros(eff.size, bool)
        for r, (name, _, _) in zip(self.rows, self.layers):
            n = r["K"] * r["N"]
            e = eff[r["eff_off"]:r["eff_off"] + n].copy()
            written[r["eff_off"]:r["eff_off"] + n] = True
            t = None
            if r["tr_off"] >= 0:
                t = eff[r["tr_off"]:r["tr_off"] + n].copy()
                written[r["tr_off"]:r["tr_off"] + n] = True
            out[name] = (e, t)
        assert np.isnan(eff[~written]).all(), "a write outside the segments (guards and padding were NaN)"
        return out


CASE_INDEX = {name: i for i, name in enumerate(CASES)}


def _want(name):
    (taps, R, N), _, copy = CASES[name]
    W = np.random.default_rng([0, CASE_INDEX[name]]).standard_normal(taps * R * N).astype(np.float32)
    eff = np.float32(_coefficient(CASE_INDEX[name])) * W
    assert eff.dtype == np.float32
    return eff, (np.ascontiguousarray(eff.reshape(taps, R, N).transpose(0, 2, 1)).ravel() if copy else None)


@pytest.fixture(scope="module")
def batched():
    return Batch([(name, shape, copy) for name, (shape, _, copy) in CASES.items()]).scale()


def test_cases_take_the_routes_they_are_named_for():
    for name, ((taps, R, N), vec, _) in CASES.items():
        p = ops.eqlr.plan(taps * R, N, taps)
        assert p["vec"] == vec and p["tiles"] == taps * -(-R // 64) * -(-N // 64), name
    assert ops.eqlr.plan(9 * 68, 132, 9)["tiles"] == 9 * 2 * 3 and ops.eqlr.plan(64, 64, 1)["tiles"] == 1


@pytest.mark.parametrize("name", sorted(CASES))
def test_scale_alone_batched_and_numpy_agree_bit_for_bit(name, batched):
    shape, _, copy = CASES[name]
    alone = Batch([(name, shape, copy)]).scale()[name]
    want = _want(name)
    for got in (alone, batched[name]):
        assert np.array_equal(got[0].view(np.int32), want[0].view(np.int32)), "eff != float32(c) * W"
        assert (got[1] is None) == (not copy)
        if copy:
            assert np.array_equal(got[1].view(np.int32), want[1].view(np.int32)), "transposed copy != eff.reshape(taps, R, N).transpose(0, 2, 1)"


def test_scale_in_another_order_of_the_layers_gives_the_same_bits(batched):
    rev = Batch([(name, shape, copy) for name, (shape, _, copy) in reversed(list(CASES.items()))]).scale()
    for name in CASES:
        assert np.array_equal(rev[name][0].view(np.int32), batched[name][0].view(np.int32))
        assert rev[name][1] is None or np.array_equal(rev[name][1].view(np.int32), batched[name][1].view(np.int32))


# ------------------------------------------------------------------ the gradient kernel
def _grad_sizes():
    unit = ops.eqlr.plan(1, 1)["unit_elems"]
    return unit, [1, 3, 4, 5, unit - 1, unit, unit + 1, 2 * unit + 7]


def _grad_run(sizes, index):
    """g *= c over segments of ``sizes`` floats (layer j's data and multiplier depend on index[j] alone); returns the segments and checks
    that nothing else of the buffer changed."""
    rows, off, off_e = [], GUARD, 0
    for n in sizes:
        rows.append(dict(w_off=off, eff_off=off_e, tr_off=-1, K=n, N=1, taps=1, c=_coefficient(index[n])))
        off += pad4(n) + GUARD
        off_e += pad4(n)
    g0 = np.full(off, SENTINEL, np.float32)
    for r in rows:
        g0[r["w_off"]:r["w_off"] + r["K"]] = np.random.default_rng([5, index[r["K"]]]).standard_normal(r["K"]).astype(np.float32)
    g = torch.from_numpy(g0).cuda()
    table = ops.EqlrTable(ops.eqlr.rows(rows), "cuda")
    assert [int(x) for x in table.host[:, 7]] == list(np.cumsum([0] + [ops.eqlr.plan(n, 1)["grad_units"] for n in sizes[:-1]]))
    ops.eqlr.grad(g, table)
    torch.cuda.synchronize()
    got = g.cpu().numpy()
    out, inside = {}, np.zeros(off, bool)
    for r in rows:
        out[r["K"]] = got[r["w_off"]:r["w_off"] + r["K"]].copy()
        inside[r["w_off"]:r["w_off"] + r["K"]] = True
    assert np.array_equal(got[~inside].view(np.int32), g0[~inside].view(np.int32)), "guards or padding changed"
    return out, {r["K"]: g0[r["w_off"]:r["w_off"] + r["K"]] for r in rows}


def test_grad_scales_each_segment_and_nothing_else():
    unit, sizes = _grad_sizes()
    assert [ops.eqlr.plan(n, 1)["grad_units"] for n in sizes] == [1, 1, 1, 1, 1, 1, 2, 3]
    index = {n: i for i, n in enumerate(sizes)}
    got, g0 = _grad_run(sizes, index)
    for n in sizes:
        want = np.float32(_coefficient(index[n])) * g0[n]
        assert np.array_equal(got[n].view(np.int32), want.view(np.int32)), n
        alone, _ = _grad_run([n], index)
        assert np.array_equal(alone[n].view(np.int32), got[n].view(np.int32)), n
